"""The references of tests/test_gpu_nonfinite.py against the CPU oracle, on inputs the oracle is defined on: a reference
that cleans a problem must be the oracle itself on a clean problem, and must equal the oracle run on the input with the
dirty rows deleted by hand."""
import numpy as np
import pytest

from tests import nonfinite_ref as NF


def _feat(rng, n, d=16):
    f = rng.standard_normal((n, d)).astype(np.float32)
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def test_knn_and_topk_references_delete_rows_and_map_indices_back(oracle_native):
    rng = np.random.default_rng(1)
    qf, tf = _feat(rng, 30), _feat(rng, 50)
    wi, wd = oracle_native.knn(qf, tf, 5, return_distance=True)
    gi, gd = NF.knn_clean(oracle_native, qf, tf, 5)
    assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    gone = [int(wi[0, 0]), 7, 49]
    dirty_t = tf.copy()
    for r, kind in zip(gone, ("nan_row", "pos_inf", "neg_inf")):
        dirty_t[r] = NF.dirty(dirty_t[r], kind, 4)
    dirty_q = qf.copy()
    dirty_q[29] = NF.dirty(dirty_q[29], "nan_elem", 0)
    keep = np.setdiff1d(np.arange(50), gone)
    wi, wd = oracle_native.knn(qf[:29], tf[keep], 5, return_distance=True)
    gi, gd = NF.knn_clean(oracle_native, dirty_q, dirty_t, 5)
    assert np.array_equal(gi[:29], keep[wi]) and np.array_equal(gd[:29], wd)
    assert (gi[29] == -1).all() and np.isinf(gd[29]).all()
    # fewer finite rows than k: real rows, then (-1, +inf)
    few = tf.copy()
    few[3:] = np.nan
    gi, gd = NF.knn_clean(oracle_native, qf, few, 5)
    assert (np.sort(gi[:, :3], axis=1) == [0, 1, 2]).all() and (gi[:, 3:] == -1).all() and np.isinf(gd[:, 3:]).all()

    q, x = _feat(rng, 12, 64), _feat(rng, 40, 64)
    d2 = oracle_native.dist2_matrix(q, x)
    gi, gd2 = NF.topk_clean(oracle_native, q, x, 6)
    want = np.argsort(d2, axis=1, kind="stable")[:, :6]
    assert np.array_equal(gi, want) and np.array_equal(gd2, np.take_along_axis(d2, want, 1))
    x[want[0, 0]] = np.nan
    x[5, 9] = 1e30                                   # finite: stays in, last
    gi, gd2 = NF.topk_clean(oracle_native, q, x, 39)
    assert want[0, 0] not in gi and (gi[:, 38] == 5).all() and np.isfinite(gd2).all()
    gi, gd2 = NF.topk_clean(oracle_native, q, x, 40)
    assert (gi[:, 39] == -1).all() and np.isinf(gd2[:, 39]).all()


def test_ransac_reference_loop_is_the_oracle_on_clean_problems(oracle_native):
    from corsair_amd import synth

    rng = np.random.default_rng(2)
    for m, frac, max_iter in ((300, 0.8, 400), (257, 0.45, 300), (10, 0.9, 50), (7, 0.9, 50)):
        src = rng.uniform(-0.8, 0.8, (m, 3)).astype(np.float32)
        tgt = (synth.apply_pose(src, synth.random_pose(m, max_trans=0.5)) + rng.normal(0, 0.01, (m, 3))).astype(np.float32)
        out = rng.random(m) > frac
        tgt[out] = rng.uniform(-1.2, 1.2, (int(out.sum()), 3)).astype(np.float32)
        wT, winl, wrmse, wit = oracle_native.ransac(src, tgt, 0.2, 10, max_iter, 0.999, 3)
        gT, gT64, ginl, grmse, git = NF.ransac_clean(oracle_native, src, tgt, 0.2, 10, max_iter, 0.999, 3)
        assert np.array_equal(gT, wT) and ginl == winl and git == wit, (m, ginl, winl, git, wit)
        assert grmse == pytest.approx(wrmse, rel=1e-12)


def test_voxelize_and_nearest_references(oracle_native):
    from corsair_amd import synth
    from oracle import sparse

    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        clouds = [rng.uniform(-1, 1, (150, 3)).astype(dtype) for _ in range(2)]
        keep, grid, off = NF.voxelize_clean(clouds, 0.5)
        parts = [sparse.quantize_cloud(c, 0.5) for c in clouds]
        assert np.array_equal(keep, np.concatenate([parts[0][2], parts[1][2] + 150]))
        assert np.array_equal(grid, sparse.sparse_collate([p[1] for p in parts])) and off == [0, len(parts[0][2]), len(keep)]
    src = rng.uniform(-1, 1, (40, 3)).astype(np.float32)
    tgt = rng.uniform(-1, 1, (60, 3)).astype(np.float32)
    T = synth.random_pose(4, max_trans=0.3).astype(np.float32)
    want = oracle_native.chamfer_1dir(src, tgt, T)
    assert NF.nearest_clean(src, tgt, T).mean() == pytest.approx(want, rel=1e-12)
    assert NF.chamfer_clean(oracle_native, src, tgt, T) == want
    tgt2 = np.concatenate([tgt, [[np.nan, 0, 0]], [[0, np.inf, 0]]]).astype(np.float32)
    assert NF.chamfer_clean(oracle_native, src, tgt2, T) == want
    src[3, 2] = np.nan
    assert NF.chamfer_clean(oracle_native, src, tgt, T) == np.inf and NF.nearest_clean(src, tgt, T)[3] == np.inf
