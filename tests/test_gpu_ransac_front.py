"""Front half of a RANSAC round: the hypothesis kernel (k_ransac_hyp, unrolled and generic sampling paths) and the
per-call pair-image set-up (packed pairs, per-problem means, the K = 16 and K = 32 f16 images and their statistics).
One small ragged batch whose sizes sit around one 192-row LDS stage of the prefilter; every result is compared bit for
bit with the CPU oracle, with the exact-only path, and (survivor totals) with what the parent commit produced."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# pairs per problem: ransac_n itself, one 192-row stage minus / exactly / plus one row, several stages, none
SIZES = [10, 191, 192, 193, 700, 0]
INLIERS = [0.5, 0.3, 0.2, 0.4, 0.25, 0.0]
MAX_CORR = 0.2

# cs_ransac_prefilter_stats (survivors, hypotheses generated) of _batch() with ransac_n 10, 2 048 iterations, seed 7 and
# CS_RANSAC_CHECK=1, recorded from a run of the parent commit d7c6e7a ("Estimate normals on a GPU cell grid"), per
# CS_RANSAC_PF_K.  A wrong image byte, row constant or per-problem statistic moves the survivor total.
PARENT_STATS = {16: (46, 9331), 32: (43, 9331)}


def _batch():
    from corsair_amd import synth

    rng = np.random.default_rng(2024)
    probs = []
    for i, (m, f) in enumerate(zip(SIZES, INLIERS)):
        src = rng.uniform(-0.8, 0.8, (m, 3)).astype(np.float32)
        tgt = synth.apply_pose(src, synth.random_pose(40 + i, max_trans=0.5)) + rng.normal(0, 0.01, (m, 3)).astype(np.float32)
        bad = rng.random(m) > f
        tgt[bad] = rng.uniform(-1.2, 1.2, (int(bad.sum()), 3)).astype(np.float32)
        probs.append((src, tgt.astype(np.float32)))
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    return np.concatenate([p[0] for p in probs]), np.concatenate([p[1] for p in probs]), off


@pytest.fixture(scope="module")
def batch(gpu):
    src, tgt, off = _batch()
    return src, tgt, off, torch.from_numpy(src).to(gpu), torch.from_numpy(tgt).to(gpu)


def _run(batch, ransac_n, max_iter, seed):
    from corsair_amd import backend as B

    _, _, off, S, D = batch
    return [t.cpu().numpy() for t in B.ransac_batch(S, D, off.tolist(), MAX_CORR, ransac_n, max_iter, 0.999, seed)]


def _stats(reset=False):
    from corsair_amd import _lib

    out = (ctypes.c_uint64 * 5)()
    _lib.load().cs_ransac_prefilter_stats(out, int(reset))
    return [int(v) for v in out]


def _assert_oracle(got, want, what):
    T, inl, rmse, iters = got
    wT, winl, wrmse, wit = want
    assert np.array_equal(inl, winl) and np.array_equal(iters, wit), (what, inl, winl, iters, wit)
    assert np.array_equal(T, wT), what
    print("front", what, "max |rmse - oracle|", float(np.abs(rmse - wrmse).max()))
    assert np.array_equal(rmse, wrmse), (what, rmse, wrmse)


@pytest.mark.parametrize("ransac_n", [10, 4])
def test_front_half_bit_identical_to_oracle(batch, oracle_native, ransac_n):
    """Test A: T, inliers, rmse and iterations equal the oracle's for the unrolled (ransac_n = 10) and the generic (4)
    sampling path, two seeds, a call that ends inside a prefiltered chunk (600) and one of several rounds (2 048)."""
    src, tgt, off = batch[:3]
    for seed in (0, 7):
        for max_iter in (600, 2048):
            want = oracle_native.ransac_batch(src, tgt, off, MAX_CORR, ransac_n, max_iter, 0.999, seed)
            _assert_oracle(_run(batch, ransac_n, max_iter, seed), want, (ransac_n, seed, max_iter))
    # m < ransac_n and m = 0: Open3D's default result
    got = _run(batch, ransac_n, 600, 0)
    assert np.array_equal(got[0][5], np.eye(4, dtype=np.float32)) and got[1][5] == 0


def test_front_half_jacobi_bit_identical_to_oracle(batch, oracle_native, monkeypatch):
    """Test A with every hypothesis through the Jacobi eigen-solver (CS_RANSAC_JACOBI=1)."""
    src, tgt, off = batch[:3]
    monkeypatch.setenv("CS_RANSAC_JACOBI", "1")
    lib = oracle_native.load()
    lib.oc_rigid_fit_force_jacobi(1)
    try:
        want = oracle_native.ransac_batch(src, tgt, off, MAX_CORR, 10, 2048, 0.999, 7)
    finally:
        lib.oc_rigid_fit_force_jacobi(0)
    _assert_oracle(_run(batch, 10, 2048, 7), want, "jacobi")


@pytest.mark.parametrize("pf_k", [16, 32])
def test_setup_images_and_statistics(batch, monkeypatch, pf_k):
    """Test B: with CS_RANSAC_CHECK=1 no bound is violated, the results equal the exact-only path, and the survivor and
    hypothesis totals are the parent commit's."""
    monkeypatch.setenv("CS_RANSAC_PF_K", str(pf_k))
    monkeypatch.setenv("CS_RANSAC_PREFILTER", "0")
    exact = _run(batch, 10, 2048, 7)
    monkeypatch.setenv("CS_RANSAC_PREFILTER", "1")
    monkeypatch.setenv("CS_RANSAC_CHECK", "1")
    _stats(reset=True)
    checked = _run(batch, 10, 2048, 7)      # raises CorsairHipError on a bound violation
    viol, n_checked, _, surv, gen = _stats()
    monkeypatch.delenv("CS_RANSAC_CHECK")
    plain = _run(batch, 10, 2048, 7)
    print("front K=%d: violations %d of %d checked, survivors %d, hypotheses %d" % (pf_k, viol, n_checked, surv, gen))
    assert viol == 0 and n_checked > 0
    for a, b, c in zip(exact, checked, plain):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert (surv, gen) == PARENT_STATS[pf_k]


@pytest.mark.parametrize("pf_k", [16, 32])
def test_out_of_range_problem_bypasses_the_prefilter(gpu, oracle_native, monkeypatch, pf_k):
    """A problem with one pair beyond the f16 range (point norm above 128) beside an ordinary problem: its rows are written
    by the bypass branch of the K = 16 image kernel (in-range pairs keep their rows, the out-of-range pair gets a zero row),
    every one of its hypotheses is counted exactly, and both problems equal the exact-only path and the oracle."""
    from corsair_amd import backend as B

    src, tgt, off = _batch()
    lo, hi = int(off[4]), int(off[5])                  # the 700-pair problem
    src, tgt = src.copy(), tgt.copy()
    src[lo + 5] = np.float32([150.0, -20.0, 3.0])
    tgt[lo + 5] = np.float32([-0.3, 140.0, 9.0])
    S, D = torch.from_numpy(src).to(gpu), torch.from_numpy(tgt).to(gpu)
    monkeypatch.setenv("CS_RANSAC_PF_K", str(pf_k))

    def run():
        return [t.cpu().numpy() for t in B.ransac_batch(S, D, off.tolist(), MAX_CORR, 10, 2048, 0.999, 7)]

    monkeypatch.setenv("CS_RANSAC_PREFILTER", "0")
    exact = run()
    monkeypatch.setenv("CS_RANSAC_PREFILTER", "1")
    monkeypatch.setenv("CS_RANSAC_CHECK", "1")
    _stats(reset=True)
    checked = run()
    assert _stats()[0] == 0
    for a, b in zip(exact, checked):
        assert np.array_equal(a, b)
    _assert_oracle(checked, oracle_native.ransac_batch(src, tgt, off, MAX_CORR, 10, 2048, 0.999, 7), ("bypass", pf_k))
