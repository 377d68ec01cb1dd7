"""GPU parity of the post-processing kernels (top-k, k-NN, Chamfer, RANSAC, part cut, sym_pose)
against the CPU oracle.  Indices / inlier counts / iteration counts: bit-exact.  f64 sums whose
association differs (Chamfer mean): 1e-12 relative.  RRE / Chamfer of the full sym_pose: 1e-4
(north-star tolerance), in practice identical transforms."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _feat(rng, n, d=16):
    f = rng.standard_normal((n, d)).astype(np.float32)
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def test_l2_topk_matches_reference_fixture(gpu):
    from corsair_amd.utils import retrieval

    z = np.load(os.path.join(GOLD, "retrieval_kat.npz"))
    pos_n = int(z["pos_n"])
    rank = retrieval.predicted_rank(z["scan"], z["lib"], pos_n)
    assert np.array_equal(rank, z["rank_top"])  # ids of scipy cdist + argsort (reference run)
    stat = retrieval.scan2cad_retrieval_eval(z["scan"], z["lib"], z["best_match"], z["table"], pos_n)
    assert stat["precision"] == pytest.approx(float(z["precision"]), abs=1e-12)
    assert stat["top1_error"] == pytest.approx(float(z["top1_error"]), abs=1e-12)
    assert stat["top1_predict"] == z["top1_predict"].tolist()
    assert stat["gt"] == z["gt"].tolist()


@pytest.mark.parametrize("nq,nx,d,k", [(37, 5000, 256, 10), (300, 700, 256, 65), (5, 3, 256, 3),
                                       (64, 4100, 512, 1024)])
def test_l2_topk_bit_exact_vs_oracle(gpu, oracle_native, nq, nx, d, k):
    from corsair_amd import backend as B, synth

    q = synth.make_descriptors(nq, d, seed=1)
    x = synth.make_descriptors(nx, d, seed=2)
    x[1] = x[0]  # an exact tie: the smaller index must win
    idx, dist = B.l2_topk(torch.from_numpy(q).to(gpu), torch.from_numpy(x).to(gpu), k, True)
    d2 = oracle_native.dist2_matrix(q, x)
    want = np.argsort(d2, axis=1, kind="stable")[:, :k]
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(dist.cpu().numpy(), np.sqrt(np.take_along_axis(d2, want, 1)))


@pytest.mark.parametrize("mfma", ["1", "0"])
def test_knn_feat_bit_exact(gpu, oracle_native, monkeypatch, mfma):
    """Both code paths return the oracle's indices and distances: the f16 matrix-core shortlist with
    canonical rescore + verification (default for 16-d features) and the exhaustive all-VALU kernel
    (CS_KNN_MFMA=0)."""
    from corsair_amd import backend as B

    monkeypatch.setenv("CS_KNN_MFMA", mfma)
    rng = np.random.default_rng(0)
    sizes = [(700, 900), (1, 40), (513, 7), (0, 10), (300, 256)]
    qf = [_feat(rng, a) for a, _ in sizes]
    tf = [_feat(rng, b) for _, b in sizes]
    tf[0][5] = tf[0][3]  # exact duplicate target rows: tie -> smaller index
    qoff = np.concatenate([[0], np.cumsum([a for a, _ in sizes])]).tolist()
    toff = np.concatenate([[0], np.cumsum([b for _, b in sizes])]).tolist()
    Q = torch.from_numpy(np.concatenate(qf)).to(gpu)
    T = torch.from_numpy(np.concatenate(tf)).to(gpu)
    idx, dist = B.knn_feat(Q, qoff, T, toff, 5, return_distance=True)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    for p, (a, b) in enumerate(sizes):
        wi, wd = oracle_native.knn(qf[p], tf[p], 5, return_distance=True)
        assert np.array_equal(idx[qoff[p]:qoff[p + 1]], wi), p
        assert np.array_equal(dist[qoff[p]:qoff[p + 1]], wd), p
    # labelled search, segments reused by several problems, problem-major output rows
    lab_q_h = rng.integers(0, 4, qoff[-1]).astype(np.int32)
    lab_t_h = rng.integers(0, 4, toff[-1]).astype(np.int32)
    lab_q_h[10:20] = -1          # queries without a part: no neighbours
    lab_t_h[30:60] = 9           # targets without a part: never matched
    lab_t_h[toff[4]:toff[5]] = 1
    lab_t_h[toff[4]:toff[4] + 3] = 0   # segment 4: part 0 has 3 targets < k -> -1 padding
    lab_q = torch.from_numpy(lab_q_h).to(gpu)
    lab_t = torch.from_numpy(lab_t_h).to(gpu)
    perms = [[1, 2, 3, 0], [0, 3, 2, 1], [2, 2, 0, 0]]
    qseg, tseg = [0, 0, 4], [0, 0, 4]
    perm_t = torch.tensor([p + [-3] * 4 for p in perms], dtype=torch.int32, device=gpu)
    got = B.knn_feat(Q, qoff, T, toff, 5, qseg=qseg, tseg=tseg, qlabel=lab_q, tlabel=lab_t,
                     perm=perm_t).cpu().numpy()
    row = 0
    for j, s in enumerate(qseg):
        a = qoff[s + 1] - qoff[s]
        want = oracle_native.knn(qf[s], tf[s], 5, lab_q.cpu().numpy()[qoff[s]:qoff[s + 1]],
                                 lab_t.cpu().numpy()[toff[s]:toff[s + 1]], perms[j])
        assert np.array_equal(got[row:row + a], want), j
        row += a


def test_knn_f16_shortlist_falls_back_on_ties(gpu, oracle_native, monkeypatch):
    """40 identical target rows tie for every query's nearest neighbours: the shortlist cannot be verified
    (the dropped copies are as close as the kept ones), the flagged queries are recomputed exhaustively and
    the (distance, smaller row) rule of the oracle holds."""
    import ctypes

    from corsair_amd import _lib, backend as B

    rng = np.random.default_rng(12)
    nq, nt = 700, 3000
    qf = _feat(rng, nq)
    tf = _feat(rng, nt)
    dup = rng.choice(nt, 40, replace=False)
    tf[dup] = qf[3] * np.float32(0.999)          # 40 copies of a vector next to query 3
    monkeypatch.setenv("CS_KNN_STATS", "1")
    st = (ctypes.c_uint64 * 2)()
    _lib.load().cs_knn_shortlist_stats(st, 1)
    idx, dist = B.knn_feat(torch.from_numpy(qf).to(gpu), [0, nq], torch.from_numpy(tf).to(gpu), [0, nt], 5,
                           return_distance=True)
    _lib.load().cs_knn_shortlist_stats(st, 0)
    wi, wd = oracle_native.knn(qf, tf, 5, return_distance=True)
    assert np.array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(dist.cpu().numpy(), wd)
    assert np.array_equal(wi[3], np.sort(dup)[:5])           # the tie rule is what decides query 3
    assert int(st[0]) == nq and 1 <= int(st[1]) < nq // 4    # some, not most, went through the fallback


def test_knn_mfma_64_is_the_f16_path(gpu, monkeypatch):
    """CS_KNN_MFMA has two meanings: a value that begins with 0 is the exhaustive kernel, anything else -- 64, once a path of
    its own, included -- the default f16 shortlist.  65 queries x 193 targets: one row past a 64-lane wave and one past the
    192-row LDS stage."""
    import ctypes

    from corsair_amd import _lib, backend as B

    rng = np.random.default_rng(65193)
    nq, nt = 65, 193
    Q = torch.from_numpy(_feat(rng, nq)).to(gpu)
    T = torch.from_numpy(_feat(rng, nt)).to(gpu)
    monkeypatch.setenv("CS_KNN_STATS", "1")
    st = (ctypes.c_uint64 * 2)()
    monkeypatch.setenv("CS_KNN_MFMA", "64")
    _lib.load().cs_knn_shortlist_stats(st, 1)
    idx, dist = B.knn_feat(Q, [0, nq], T, [0, nt], 5, return_distance=True)
    _lib.load().cs_knn_shortlist_stats(st, 1)
    assert int(st[0]) == nq                                  # every query was answered by the f16 path
    monkeypatch.setenv("CS_KNN_MFMA", "0")
    widx, wdist = B.knn_feat(Q, [0, nq], T, [0, nt], 5, return_distance=True)
    _lib.load().cs_knn_shortlist_stats(st, 0)
    assert int(st[0]) == 0                                   # ... and none of them under CS_KNN_MFMA=0
    assert np.array_equal(idx.cpu().numpy(), widx.cpu().numpy())
    assert np.array_equal(dist.cpu().numpy().view(np.int64), wdist.cpu().numpy().view(np.int64))


@pytest.mark.parametrize("path", ["f16", "f64", "valu"])
def test_chamfer_matches_oracle(gpu, oracle_native, monkeypatch, path):
    """The three kernels behind cs_chamfer_1dir: f16 matrix-core ranking + canonical re-evaluation of the two best tiles per
    lane + verification (default, round 5), the f64 matrix-pipe arg-min (CS_CHAMFER_F16=0, also the fallback of the first)
    and the exhaustive VALU chain (CS_CHAMFER_MFMA=0)."""
    from corsair_amd import backend as B, synth

    if path == "f64":
        monkeypatch.setenv("CS_CHAMFER_F16", "0")
    elif path == "valu":
        monkeypatch.setenv("CS_CHAMFER_MFMA", "0")

    rng = np.random.default_rng(3)
    clouds = [rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (1500, 777, 1, 300)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    X = torch.from_numpy(np.concatenate(clouds)).to(gpu)
    Ts = np.stack([synth.random_pose(i, max_trans=0.3).astype(np.float32) for i in range(5)])
    src_seg, tgt_seg = [0, 1, 2, 3, 0], [1, 0, 3, 3, 0]
    got = B.chamfer_1dir(X, off, X, off, src_seg, tgt_seg, torch.from_numpy(Ts).to(gpu)).cpu().numpy()
    for p in range(5):
        want = oracle_native.chamfer_1dir(clouds[src_seg[p]], clouds[tgt_seg[p]], Ts[p])
        assert got[p] == pytest.approx(want, rel=1e-12), p


def test_chamfer_f16_ranking_vouches_or_falls_back(gpu, oracle_native, monkeypatch):
    """The f16 ranking only ANSWERS where its error budget proves the evaluated rows hold the nearest target.  (1) Voxelised
    real-shaped clouds (the bench's use): the default path equals the f64 kernel bit for bit, and few tiles fall back.
    (2) Adversarial: every target exists four times within 1e-8 of itself, scattered over the array (so the copies sit in
    different 32-row tiles): best, second and third candidate tie far inside the budget, every tile must be flagged and
    recomputed -- and the result is still the oracle's.  (3) Coordinates beyond the f16 range of the scaled image (|x| >= 60)
    take the f64 kernel as well."""
    import ctypes

    from corsair_amd import _lib, backend as B, synth

    monkeypatch.setenv("CS_CHAMFER_STATS", "1")
    st = (ctypes.c_uint64 * 2)()
    lib = _lib.load()

    def run(src, tgt, Ts):
        off_s = [0, len(src)]
        off_t = [0, len(tgt)]
        n = len(Ts)
        return B.chamfer_1dir(torch.from_numpy(src).to(gpu), off_s, torch.from_numpy(tgt).to(gpu), off_t, [0] * n, [0] * n,
                              torch.from_numpy(Ts).to(gpu)).cpu().numpy()

    # (1) two re-samplings of one shape, voxelised like the bench's clouds, 6 poses near the aligning one
    full = synth.make_cloud(5, 15000)
    keep = lambda pc: pc[np.unique(np.floor(pc / 0.03).astype(np.int64), axis=0, return_index=True)[1]]
    src, tgt = keep(full[:10000]).astype(np.float32), keep(full[5000:]).astype(np.float32)
    Ts = np.stack([synth.random_pose(40 + i, max_trans=0.02 * i).astype(np.float32) for i in range(6)])
    Ts[0] = np.eye(4, dtype=np.float32)
    lib.cs_chamfer_f16_stats(st, 1)
    got = run(src, tgt, Ts)
    lib.cs_chamfer_f16_stats(st, 0)
    tiles, flagged = int(st[0]), int(st[1])
    monkeypatch.setenv("CS_CHAMFER_F16", "0")
    ref = run(src, tgt, Ts)
    monkeypatch.delenv("CS_CHAMFER_F16")
    assert np.array_equal(got, ref)
    assert tiles == 6 * -(-len(src) // 256) and flagged <= tiles // 4, (tiles, flagged)
    want = oracle_native.chamfer_1dir(src, tgt, Ts[3])
    assert got[3] == pytest.approx(want, rel=1e-12)
    # (2) four near-copies of every target, shuffled
    rng = np.random.default_rng(8)
    base = rng.uniform(-0.8, 0.8, (1200, 3))
    tgt4 = np.concatenate([base + rng.normal(0, 1e-8, base.shape) for _ in range(4)])
    tgt4 = tgt4[rng.permutation(len(tgt4))].astype(np.float32)
    src2 = rng.uniform(-0.8, 0.8, (700, 3)).astype(np.float32)
    T2 = np.stack([synth.random_pose(7, max_trans=0.1).astype(np.float32)])
    lib.cs_chamfer_f16_stats(st, 1)
    got2 = run(src2, tgt4, T2)
    lib.cs_chamfer_f16_stats(st, 0)
    assert int(st[0]) == 3 and int(st[1]) == 3            # every tile fell back
    assert got2[0] == pytest.approx(oracle_native.chamfer_1dir(src2, tgt4, T2[0]), rel=1e-12)
    # (3) out of the scaled f16 range
    far = (src2 * 100.0).astype(np.float32)
    lib.cs_chamfer_f16_stats(st, 1)
    got3 = run(far, (tgt4[:900] * 100.0).astype(np.float32), np.eye(4, dtype=np.float32)[None])
    lib.cs_chamfer_f16_stats(st, 0)
    assert int(st[1]) == int(st[0]) == 3
    assert got3[0] == pytest.approx(oracle_native.chamfer_1dir(far, (tgt4[:900] * 100.0).astype(np.float32), np.eye(4, dtype=np.float32)), rel=1e-12)


def _corr_problem(rng, m, inlier_frac, noise=0.01, pose_id=0):
    from corsair_amd import synth

    src = rng.uniform(-0.8, 0.8, (m, 3)).astype(np.float32)
    T = synth.random_pose(pose_id, max_trans=0.5)
    tgt = synth.apply_pose(src, T) + rng.normal(0, noise, (m, 3)).astype(np.float32)
    bad = rng.random(m) > inlier_frac
    tgt[bad] = rng.uniform(-1.2, 1.2, (int(bad.sum()), 3)).astype(np.float32)
    return src, tgt.astype(np.float32), T


def test_ransac_bit_exact_vs_oracle(gpu, oracle_native):
    from corsair_amd import backend as B

    rng = np.random.default_rng(11)
    specs = [(4000, 0.35, 0), (2500, 0.7, 1), (900, 0.15, 2), (5, 0.5, 3), (3000, 0.05, 4)]
    probs = [_corr_problem(rng, m, f, pose_id=i) for m, f, i in specs]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])]).tolist()
    S = torch.from_numpy(np.concatenate([p[0] for p in probs])).to(gpu)
    D = torch.from_numpy(np.concatenate([p[1] for p in probs])).to(gpu)
    max_iter = 6000
    T, inl, rmse, iters = B.ransac_batch(S, D, off, 0.2, 10, max_iter, 0.999, 0)
    T, inl, rmse, iters = T.cpu().numpy(), inl.cpu().numpy(), rmse.cpu().numpy(), iters.cpu().numpy()
    for p, (src, tgt, Tgt) in enumerate(probs):
        wT, winl, wrmse, wit = oracle_native.ransac(src, tgt, 0.2, 10, max_iter, 0.999, 0)
        assert inl[p] == winl and iters[p] == wit, (p, inl[p], winl, iters[p], wit)
        assert np.array_equal(T[p], wT), p
        assert rmse[p] == pytest.approx(wrmse, rel=1e-12)
    # the 70 % inlier problem must exit early and recover the pose
    assert iters[1] < max_iter
    assert np.abs(T[1][:3, :3] - probs[1][2][:3, :3]).max() < 0.15  # no refinement step, like Open3D
    # fewer pairs than ransac_n: identity, like Open3D's default RegistrationResult
    assert np.array_equal(T[3], np.eye(4, dtype=np.float32)) and inl[3] == 0


def test_ransac_hypothesis_eigen_solver_paths_bit_exact(gpu, oracle_native, monkeypatch):
    """k_ransac_hyp takes the largest eigenpair of the Horn matrix from its characteristic polynomial (horn_qcp) and
    falls back to the Jacobi solver per lane when the eigenvalue is not well separated.  Both paths equal the oracle's
    (oc_horn_qcp / oc_jacobi4) bit for bit: (a) problems whose samples are degenerate -- sources on a line, all sources
    equal, half of the sources on a line (a few hypotheses per wave diverge into the fallback) -- under the default
    switch; (b) every hypothesis through the fallback (CS_RANSAC_JACOBI=1 / force_jacobi)."""
    from corsair_amd import backend as B

    rng = np.random.default_rng(23)
    probs = [_corr_problem(rng, m, f, pose_id=30 + i) for i, (m, f) in enumerate([(2000, 0.3), (1200, 0.1), (800, 0.5), (1500, 0.2)])]
    line = (np.outer(rng.uniform(-1, 1, 1200), [0.3, -0.5, 0.8]) + [0.1, 0.0, -0.2]).astype(np.float32)
    probs[1] = (line, probs[1][1], None)
    probs[2] = (np.tile(np.float32([[0.2, 0.1, -0.4]]), (800, 1)), probs[2][1], None)
    half = probs[3][0].copy()
    half[::2] = (np.outer(rng.uniform(-1, 1, 750), [0.6, 0.2, -0.7])).astype(np.float32)
    probs[3] = (half, probs[3][1], None)
    for src, tgt, _ in probs[1:3]:                       # these samples do take the fallback
        idx = oracle_native.rng_indices(0, 5, 10, len(src))
        assert oracle_native.rigid_fit(src[idx], tgt[idx], return_path=True)[2] == 1
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])]).tolist()
    S = torch.from_numpy(np.concatenate([p[0] for p in probs])).to(gpu)
    D = torch.from_numpy(np.concatenate([p[1] for p in probs])).to(gpu)
    for force in (False, True):
        if force:
            monkeypatch.setenv("CS_RANSAC_JACOBI", "1")
        T, inl, rmse, iters = (t.cpu().numpy() for t in B.ransac_batch(S, D, off, 0.2, 10, 3000, 0.999, 0))
        for p, (src, tgt, _) in enumerate(probs):
            wT, winl, wrmse, wit = oracle_native.ransac(src, tgt, 0.2, 10, 3000, 0.999, 0, force_jacobi=force)
            assert inl[p] == winl and iters[p] == wit, (force, p, inl[p], winl, iters[p], wit)
            assert np.array_equal(T[p], wT), (force, p)
            assert rmse[p] == pytest.approx(wrmse, rel=1e-12)


@pytest.mark.parametrize("ransac_n", [3, 6, 17])
def test_ransac_other_sample_sizes_bit_exact(gpu, oracle_native, ransac_n):
    """ransac_n other than the reference's 10 (Open3D's default is 6) goes through the run-time-sized
    sampling loop of the hypothesis kernel."""
    from corsair_amd import backend as B

    rng = np.random.default_rng(40 + ransac_n)
    probs = [_corr_problem(rng, m, f, pose_id=20 + i) for i, (m, f) in enumerate([(1500, 0.4), (700, 0.2), (ransac_n - 1, 0.5)])]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])]).tolist()
    S = torch.from_numpy(np.concatenate([p[0] for p in probs])).to(gpu)
    D = torch.from_numpy(np.concatenate([p[1] for p in probs])).to(gpu)
    T, inl, rmse, iters = (t.cpu().numpy() for t in B.ransac_batch(S, D, off, 0.2, ransac_n, 3000, 0.999, 5))
    for p, (src, tgt, _) in enumerate(probs):
        wT, winl, wrmse, wit = oracle_native.ransac(src, tgt, 0.2, ransac_n, 3000, 0.999, 5)
        assert inl[p] == winl and iters[p] == wit, (p, inl[p], winl, iters[p], wit)
        assert np.array_equal(T[p], wT), p


def test_ransac_seed_changes_samples_but_not_quality(gpu):
    from corsair_amd import backend as B

    rng = np.random.default_rng(5)
    src, tgt, Tgt = _corr_problem(rng, 3000, 0.5)
    S, D = torch.from_numpy(src).to(gpu), torch.from_numpy(tgt).to(gpu)
    outs = [B.ransac_batch(S, D, [0, 3000], 0.1, 10, 20000, 0.999, seed)[0].cpu().numpy()[0]
            for seed in (0, 1, 0)]
    assert np.array_equal(outs[0], outs[2])        # deterministic
    assert not np.array_equal(outs[0], outs[1])    # seed-dependent
    for T in outs:
        assert np.abs(T[:3, :3] - Tgt[:3, :3]).max() < 0.1


def _prefilter_stats(reset=False):
    import ctypes

    from corsair_amd import _lib

    out = (ctypes.c_uint64 * 5)()
    _lib.load().cs_ransac_prefilter_stats(out, int(reset))
    return [int(v) for v in out]


@pytest.mark.parametrize("pf_k", [16, 32])
@pytest.mark.parametrize("scale,max_corr", [(1.0, 0.2), (1.0, 0.03), (6.0, 0.5), (11.0, 1.5), (40.0, 4.0), (100.0, 10.0)])
def test_ransac_prefilter_bound_and_identity(gpu, oracle_native, monkeypatch, scale, max_corr, pf_k):
    """The f16 matrix-core prefilter must (a) never under-estimate an inlier count (CS_RANSAC_CHECK
    recomputes every hypothesis exactly) and (b) leave the result bit-identical to the exact-only
    path and to the oracle, at every coordinate scale (100: beyond the f16 range -> bypass; 40: bound valid but loose).
    Both forms: K = 16 (default since round 4: one MFMA per tile, the dropped a_hi . b_lo bounded per pair) and K = 32."""
    from corsair_amd import backend as B

    monkeypatch.setenv("CS_RANSAC_PF_K", str(pf_k))

    rng = np.random.default_rng(int(scale * 10) + 3)
    specs = [(3500, 0.04, 0), (2200, 0.08, 1), (1300, 0.03, 2), (4100, 0.02, 3), (700, 0.12, 4), (2900, 0.0, 5)]
    probs = []
    for m, f, i in specs:
        src, tgt, _ = _corr_problem(rng, m, f, noise=0.02, pose_id=i)
        probs.append(((src * scale).astype(np.float32), (tgt * scale).astype(np.float32)))
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])]).tolist()
    S = torch.from_numpy(np.concatenate([p[0] for p in probs])).to(gpu)
    D = torch.from_numpy(np.concatenate([p[1] for p in probs])).to(gpu)
    max_iter = 40000

    def run():
        return [t.cpu().numpy() for t in B.ransac_batch(S, D, off, max_corr, 10, max_iter, 0.999, 7)]

    monkeypatch.setenv("CS_RANSAC_PREFILTER", "0")
    exact = run()
    monkeypatch.setenv("CS_RANSAC_PREFILTER", "1")
    monkeypatch.setenv("CS_RANSAC_CHECK", "1")
    _prefilter_stats(reset=True)
    checked = run()                      # raises CorsairHipError on a bound violation
    viol, n_checked, slack, surv, gen = _prefilter_stats()
    assert viol == 0 and n_checked > 0
    monkeypatch.delenv("CS_RANSAC_CHECK")
    plain = run()
    for a, b, c in zip(exact, checked, plain):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    if scale <= 6.0 and not (pf_k == 16 and max_corr < 0.1):
        # the bound has to be useful, not just valid: most hypotheses are pruned (the per-pair bound of the K = 16 form is
        # ~1e-3 in squared distance for unit-sized objects: as large as thr^2 itself at max_corr 0.03, still valid)
        assert surv < 0.25 * n_checked, (surv, n_checked)
    print("prefilter K=%d scale %g max_corr %g: survivors %d of %d, mean slack %.1f" % (pf_k, scale, max_corr, surv, gen, slack / max(n_checked, 1)))
    for p in (1, 4):
        wT, winl, wrmse, wit = oracle_native.ransac(probs[p][0], probs[p][1], max_corr, 10, max_iter, 0.999, 7)
        assert exact[1][p] == winl and exact[3][p] == wit
        assert np.array_equal(exact[0][p], wT)


@pytest.mark.parametrize("max_iter", [40, 64, 100, 600, 60000])
def test_ransac_first_chunk_size_leaves_the_results_unchanged(gpu, monkeypatch, max_iter):
    """Round 5: the first (unfiltered, exactly counted) chunk of a call is 64 iterations -- lane = hypothesis + 64 x quarter of
    the pairs in k_ransac_count<false, 64> -- and the second chunk, [64, 512), is prefiltered against the best of those 64.
    Results equal the 256- and 512-iteration first chunks of rounds 1-4 and the prefilter-free run, also when the iteration
    budget ends inside the first or the second chunk, and with inlier ratios from none to early-exit territory."""
    from corsair_amd import backend as B

    rng = np.random.default_rng(78)
    specs = [(int(rng.integers(40, 9000)), float(rng.choice([0.0, 0.05, 0.3, 0.8])), i) for i in range(30)]
    probs = [_corr_problem(rng, m, f, noise=0.02, pose_id=300 + i)[:2] for m, f, i in specs]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])]).tolist()
    S = torch.from_numpy(np.concatenate([p[0] for p in probs])).to(gpu)
    D = torch.from_numpy(np.concatenate([p[1] for p in probs])).to(gpu)
    out = {}
    for first in ("64", "256", "512", "exact"):
        if first == "exact":
            monkeypatch.delenv("CS_RANSAC_FIRST")
            monkeypatch.setenv("CS_RANSAC_PREFILTER", "0")
        else:
            monkeypatch.setenv("CS_RANSAC_FIRST", first)
        out[first] = [t.cpu().numpy() for t in B.ransac_batch(S, D, off, 0.06, 10, max_iter, 0.999, 5)]
    for first in ("256", "512", "exact"):
        for a, b in zip(out["64"], out[first]):
            assert np.array_equal(a, b), (max_iter, first)


def test_ransac_second_stage_leaves_the_trajectory_unchanged(gpu, monkeypatch):
    """Round 4: the survivors of the K = 16 prefilter go through the K = 32 bound (a compact list per problem, one small
    launch) before they are counted exactly.  With and without it (CS_RANSAC_STAGE2) the results AND the number of
    first-stage survivors of the whole run are identical -- the survivor count is a fingerprint of every problem's best
    count in every round: a hypothesis the second stage dropped wrongly would leave the best count lower and let more
    through later.  Many problems of very different sizes, thresholds from tight to loose, so that the number of
    survivors per problem and round swings from 0 to beyond the list capacity (a round's counts are not known on the host:
    the launch must cover the whole capacity and pass what exceeds it)."""
    from corsair_amd import backend as B

    rng = np.random.default_rng(77)
    specs = [(int(rng.integers(300, 9000)), float(rng.choice([0.0, 0.02, 0.05, 0.15])), i) for i in range(40)]
    probs = [_corr_problem(rng, m, f, noise=0.02, pose_id=200 + i)[:2] for m, f, i in specs]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in probs])]).tolist()
    S = torch.from_numpy(np.concatenate([p[0] for p in probs])).to(gpu)
    D = torch.from_numpy(np.concatenate([p[1] for p in probs])).to(gpu)
    for max_corr in (0.2, 0.06, 0.02):
        out = {}
        for stage2 in ("0", "1"):
            monkeypatch.setenv("CS_RANSAC_STAGE2", stage2)
            _prefilter_stats(reset=True)
            out[stage2] = [t.cpu().numpy() for t in B.ransac_batch(S, D, off, max_corr, 10, 60000, 0.999, 3)]
            out[stage2].append(_prefilter_stats()[3])
        for a, b in zip(out["0"][:4], out["1"][:4]):
            assert np.array_equal(a, b), max_corr
        assert out["0"][4] == out["1"][4] and out["0"][4] > 0, (max_corr, out["0"][4], out["1"][4])
    monkeypatch.setenv("CS_RANSAC_PREFILTER", "0")
    exact = [t.cpu().numpy() for t in B.ransac_batch(S, D, off, 0.02, 10, 60000, 0.999, 3)]
    for a, b in zip(exact, out["1"][:4]):
        assert np.array_equal(a, b)


def _ball(rng, n, centre, radius):
    v = rng.standard_normal((n, 3))
    v *= (radius * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    return (v + np.asarray(centre)).astype(np.float32)


def test_ransac_long_survivor_list_bit_exact(gpu, oracle_native):
    """The list path of a prefiltered round: k_ransac_count<true> -> k_ransac_err -> k_ransac_scan2.  Source and target are
    two balls of radius 0.01: every finite hypothesis maps its sample centroid onto the target's, so every residual is at
    most 0.04 < max_corr, every hypothesis counts all 300 pairs and every bound reaches the carried best -- whole chunks
    survive.  The round [2048, 4096) leaves 2 048 survivors (> FEW_MAX = 1024) and the round [4096, 8192) has b = 4096
    (> 1024), so that round counts its survivors with the list kernel.  confidence = 1: no early exit."""
    from corsair_amd import backend as B

    rng = np.random.default_rng(61)
    src = _ball(rng, 300, (0.0, 0.0, 0.0), 0.01)
    tgt = _ball(rng, 300, (0.3, -0.2, 0.1), 0.01)
    S, D = torch.from_numpy(src).to(gpu), torch.from_numpy(tgt).to(gpu)
    _prefilter_stats(reset=True)
    T, inl, rmse, iters = (t.cpu().numpy() for t in B.ransac_batch(S, D, [0, 300], 0.2, 10, 8192, 1.0, 0))
    surv = _prefilter_stats()[3]
    wT, winl, wrmse, wit = oracle_native.ransac(src, tgt, 0.2, 10, 8192, 1.0, 0)
    assert inl[0] == winl and iters[0] == wit, (inl[0], winl, iters[0], wit)
    assert np.array_equal(T[0], wT)
    assert rmse[0] == pytest.approx(wrmse, rel=1e-12)
    assert winl == 300 and wit == 8192
    assert surv >= 4096 + 2048, surv       # the last two rounds passed whole: the list path ran


def test_ransac_device_placement_table_bit_exact(gpu, oracle_native):
    """More than 64 problems on an XCD: the placement table of a round no longer fits the kernel argument and is read
    from device memory by k_ransac_hyp and k_ransac_prefilter (xcd_ptr != nullptr).  520 live problems of 12 pairs (65 per
    XCD) and two that are done at the start (0 and 3 pairs < ransac_n); the round [64, 128) is prefiltered."""
    from corsair_amd import backend as B

    rng = np.random.default_rng(62)
    sizes = [12] * 520
    sizes.insert(100, 0)
    sizes.insert(400, 3)
    probs = [_corr_problem(rng, m, float(rng.choice([0.3, 0.5, 0.8, 1.0])), pose_id=400 + i)[:2] for i, m in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    src, tgt = np.concatenate([p[0] for p in probs]), np.concatenate([p[1] for p in probs])
    _prefilter_stats(reset=True)
    T, inl, rmse, iters = (t.cpu().numpy() for t in B.ransac_batch(torch.from_numpy(src).to(gpu), torch.from_numpy(tgt).to(gpu),
                                                                   off, 0.2, 4, 128, 0.999, 3))
    assert _prefilter_stats()[4] > 64 * 520    # hypotheses were evaluated beyond the first chunk
    wT, winl, wrmse, wit = oracle_native.ransac_batch(src, tgt, off, 0.2, 4, 128, 0.999, 3)
    assert np.array_equal(inl, winl) and np.array_equal(iters, wit)
    assert np.array_equal(T, wT)
    assert rmse == pytest.approx(wrmse, rel=1e-12)
    for p in (100, 400):
        assert np.array_equal(T[p], np.eye(4, dtype=np.float32)) and inl[p] == 0 and iters[p] == 0


def _engine_features(gpu, cloud_ids, pose_ids):
    from corsair_amd import engine, synth
    from tests.helpers import make_batch

    coords, feats, origins, offsets = make_batch(cloud_ids, n_points=6000, pose_ids=pose_ids)
    sd, emb = synth.make_state_dicts(31)
    eng = engine.ResUNetEngine(sd, emb, device=gpu)
    out, _, _ = eng.forward(torch.from_numpy(coords).to(gpu), torch.from_numpy(feats).to(gpu))
    return out, torch.from_numpy(origins).to(gpu), offsets


def test_symcut_fit_bit_exact(gpu, oracle_native):
    from corsair_amd import backend as B, registration as R

    F, X, off = _engine_features(gpu, [20, 21], [None, None])
    Ks = [2, 4]
    anchors = np.stack([R.draw_anchors(off[c + 1] - off[c], 24, c) for c in range(2)])
    c, cnt, mcd, mer = B.symcut_fit(F, X, off, torch.from_numpy(anchors).to(gpu), Ks, 50, 10, 300)
    Fh, Xh = F.cpu().numpy(), X.cpu().numpy()
    for i in range(2):
        f, x = Fh[off[i]:off[i + 1]], Xh[off[i]:off[i + 1]]
        wc, wcnt, wmcd, wmer = oracle_native.symcut_fit(f, x, anchors[i], Ks[i], 50, 10, 300, 0)
        assert np.array_equal(cnt[i].cpu().numpy(), wcnt)
        assert np.array_equal(c[i].cpu().numpy(), wc)
        assert np.array_equal(mcd[i].cpu().numpy(), wmcd)
        assert np.array_equal(mer[i].cpu().numpy(), wmer)
        sel = np.zeros((1, 4, 3))
        sel[0, :Ks[i]] = wc[0, :Ks[i]]
        lab = B.symcut_labels(X[off[i]:off[i + 1]].contiguous(), [0, len(x)], [Ks[i]],
                              torch.from_numpy(sel).to(gpu)).cpu().numpy()
        assert np.array_equal(lab, oracle_native.symcut_labels(x, Ks[i], wc[0]))


@pytest.mark.parametrize("n", [37, 2048, 8190, 8192, 8193, 9500])
def test_symcut_selection_paths_bit_exact(gpu, oracle_native, n):
    """The 50-nearest selection of the part cut keeps a cloud's distance keys in registers up to 8 192 rows and re-reads
    them from memory beyond that: both paths, ragged sizes around the boundary, and a cloud with many DUPLICATE features
    (ties at the selection threshold go to the smaller row) against the oracle."""
    from corsair_amd import backend as B, registration as R

    rng = np.random.default_rng(n)
    f = rng.standard_normal((n, 16)).astype(np.float32)
    f[n // 3:n // 3 + min(200, n // 4)] = f[0]              # 200 copies of row 0: a tie block across the threshold
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    x = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    anchors = R.draw_anchors(n, 12, 7)
    anchors[0] = 0                                           # an anchor inside the tie block
    c, cnt, mcd, mer = B.symcut_fit(torch.from_numpy(f).to(gpu), torch.from_numpy(x).to(gpu), [0, n],
                                    torch.from_numpy(anchors[None]).to(gpu), [4], 50, 10, 300)
    wc, wcnt, wmcd, wmer = oracle_native.symcut_fit(f, x, anchors, 4, 50, 10, 300, 0)
    assert np.array_equal(cnt[0].cpu().numpy(), wcnt)
    assert np.array_equal(c[0].cpu().numpy(), wc)
    assert np.array_equal(mcd[0].cpu().numpy(), wmcd)
    assert np.array_equal(mer[0].cpu().numpy(), wmer)


def test_sym_pose_matches_oracle(gpu, oracle_native):
    """Whole sym_pose (utils/symmetry.py:262-358) on ResUNet features of posed copies of two clouds."""
    from corsair_amd import registration as R
    from oracle import post

    # queries = clouds 30, 31 under seeded rotations; CAD side = the unposed clouds
    F, X, off = _engine_features(gpu, [30, 31, 30, 31], [7, 8, None, None])
    off0, off1 = off[:3], [o - off[2] for o in off[2:]]
    bF, x0 = F[:off[2]].contiguous(), X[:off[2]].contiguous()
    pF, x1 = F[off[2]:].contiguous(), X[off[2]:].contiguous()
    syms = [1, 2]
    max_iter = 3000
    res = R.sym_pose_batch(bF, x0, off0, pF, x1, off1, syms, 5, 0.2, 0, [(0, 1), (2, 3)], 100,
                           max_iter, 0.999)
    for p in range(2):
        a = (bF[off0[p]:off0[p + 1]].cpu().numpy(), x0[off0[p]:off0[p + 1]].cpu().numpy(),
             pF[off1[p]:off1[p + 1]].cpu().numpy(), x1[off1[p]:off1[p + 1]].cpu().numpy())
        anc0 = R.draw_anchors(len(a[0]), 100, 2 * p)
        anc1 = R.draw_anchors(len(a[2]), 100, 2 * p + 1)
        Tb, cdb, Tr, cdr, ok = post.sym_pose(a[0], a[1], a[2], a[3], syms[p], 5, 0.2, 0, anc0, anc1,
                                             max_iter, 0.999)
        assert bool(res.ok[p]) == ok
        assert np.array_equal(res.T_ransac[p].cpu().numpy(), Tr)
        assert np.array_equal(res.T_best[p].cpu().numpy(), Tb)
        assert float(res.cd_ransac[p]) == pytest.approx(cdr, rel=1e-12)
        assert float(res.cd_best[p]) == pytest.approx(cdb, rel=1e-12)
        assert float(res.cd_best[p]) <= float(res.cd_ransac[p])  # invariant of the caches


def test_sym_pose_is_independent_of_the_overlap_switches(gpu, monkeypatch):
    """The vanilla / symmetric split of the RANSAC call (helper thread + stream) and the pipelined RANSAC
    rounds (second stream inside cs_ransac_batch) only change WHEN work runs: every output is identical
    to the single-call, single-stream path.  force_gate keeps the symmetric hypotheses in play and
    max_iter spans prefiltered, pipelined rounds."""
    from corsair_amd import registration as R

    F, X, off = _engine_features(gpu, [30, 31, 32, 30, 31, 32], [7, 8, 9, None, None, None])
    off0, off1 = off[:4], [o - off[3] for o in off[3:]]
    bF, x0 = F[:off[3]].contiguous(), X[:off[3]].contiguous()
    pF, x1 = F[off[3]:].contiguous(), X[off[3]:].contiguous()

    def run():
        r = R.sym_pose_batch(bF, x0, off0, pF, x1, off1, [1, 2, 4], 5, 0.2, 0, None, 100, 40000, 0.999,
                             force_gate=True)
        return [t.cpu().numpy() for t in (r.T_best, r.cd_best, r.T_ransac, r.cd_ransac, r.iters)] + [r.ok]

    monkeypatch.setenv("CORSAIR_SPLIT_RANSAC", "0")
    monkeypatch.setenv("CS_RANSAC_OVERLAP", "0")
    want = run()
    assert want[4].max() > 16384                         # several prefiltered rounds were run
    for split, overlap in (("1", "0"), ("0", "1"), ("1", "1")):
        monkeypatch.setenv("CORSAIR_SPLIT_RANSAC", split)
        monkeypatch.setenv("CS_RANSAC_OVERLAP", overlap)
        for _ in range(2):                               # timing-dependent paths: twice each
            got = run()
            for a, b in zip(want, got):
                assert np.array_equal(a, b), (split, overlap)


@pytest.mark.parametrize("nq,nx,d,k", [(37, 5000, 256, 10), (5, 70, 256, 3), (300, 9000, 512, 1),
                                       (130, 20000, 100, 10)])
def test_l2_topk_mfma_shortlist_path_bit_exact(gpu, oracle_native, monkeypatch, nq, nx, d, k):
    """The f64-MFMA shortlist + exact re-score path (config C5 sizes) returns exactly the ids and
    distances of the canonical chain, duplicates (exact ties) included."""
    from corsair_amd import backend as B, synth

    monkeypatch.setenv("CS_TOPK_MFMA", "1")
    q = synth.make_descriptors(nq, d, seed=11)
    x = synth.make_descriptors(nx, d, seed=12)
    x[7] = x[3]
    x[nx - 1] = x[3]
    idx, dist = B.l2_topk(torch.from_numpy(q).to(gpu), torch.from_numpy(x).to(gpu), k, True)
    d2 = oracle_native.dist2_matrix(q, x)
    want = np.argsort(d2, axis=1, kind="stable")[:, :k]
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(dist.cpu().numpy(), np.sqrt(np.take_along_axis(d2, want, 1)))


def _topk_stats(reset=False):
    import ctypes

    from corsair_amd import _lib

    out = (ctypes.c_uint64 * 2)()
    _lib.load().cs_l2_topk_stats(out, int(reset))
    return int(out[0]), int(out[1])


@pytest.mark.parametrize("nq,nx,d,k", [(37, 5000, 256, 10), (300, 9000, 128, 1), (130, 20000, 64, 10),
                                       (5, 64, 256, 3), (700, 777, 256, 10), (290, 6000, 512, 10),
                                       (33, 97, 512, 4)])
def test_l2_topk_f16_shortlist_path_bit_exact(gpu, oracle_native, monkeypatch, nq, nx, d, k):
    """The f16 matrix-core shortlist + exact re-score + verification path returns exactly the ids and
    distances of the canonical chain; exact ties at the k-th neighbour (duplicated catalog rows) make the
    verification fail and those queries are recomputed by the f64 path."""
    from corsair_amd import backend as B, synth

    monkeypatch.setenv("CS_TOPK_MFMA", "16")
    q = synth.make_descriptors(nq, d, seed=21)
    x = synth.make_descriptors(nx, d, seed=22)
    x[7] = x[3]
    x[nx - 1] = x[3]
    q[0] = x[3]                                   # query 0: three catalog rows at distance 0
    _topk_stats(reset=True)
    idx, dist = B.l2_topk(torch.from_numpy(q).to(gpu), torch.from_numpy(x).to(gpu), k, True)
    took, fell_back = _topk_stats()
    assert took == nq and fell_back <= max(2, nq // 20)
    d2 = oracle_native.dist2_matrix(q, x)
    want = np.argsort(d2, axis=1, kind="stable")[:, :k]
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(dist.cpu().numpy(), np.sqrt(np.take_along_axis(d2, want, 1)))


@pytest.mark.parametrize("nq,nx,d,k,force", [(37, 5000, 256, 10, "16"), (130, 20000, 64, 10, "16"), (290, 6000, 512, 10, "16"),
                                             (50, 652, 256, 1, None), (5, 40, 256, 3, "16"), (20, 3000, 48, 5, "16")])
def test_l2_topk_catalog_handle_equals_plain_calls(gpu, oracle_native, monkeypatch, nq, nx, d, k, force):
    """cs_topk_catalog (image and norms of a fixed library made once) gives the ids and distances of cs_l2_topk /
    cs_l2_topk_sq on the same arrays -- on the f16 path that uses the prepared pieces, on shapes that path does not take
    (slab path, d not a multiple of 64, fewer rows than one stage) and for two different query sets against one handle --
    and those are the oracle's."""
    from corsair_amd import backend as B, synth

    if force:
        monkeypatch.setenv("CS_TOPK_MFMA", force)
    x = synth.make_descriptors(nx, d, seed=32)
    xd = torch.from_numpy(x).to(gpu)
    cat = B.TopkCatalog(xd)
    for seed in (31, 33):
        q = synth.make_descriptors(nq, d, seed=seed)
        qd = torch.from_numpy(q).to(gpu)
        i0, d0 = B.l2_topk(qd, xd, k, True)
        i1, d1 = B.l2_topk(qd, cat, k, True)
        assert torch.equal(i0, i1) and torch.equal(d0, d1)
        i2, s2 = B.l2_topk(qd, cat, k, True, squared=True)
        i3, s3 = B.l2_topk(qd, xd, k, True, squared=True)
        assert torch.equal(i2, i3) and torch.equal(s2, s3) and torch.equal(i2, i0)
        assert torch.equal(B.l2_topk(qd, cat, k), i0)
        d2 = oracle_native.dist2_matrix(q, x)
        want = np.argsort(d2, axis=1, kind="stable")[:, :k]
        assert np.array_equal(i1.cpu().numpy(), want)
        assert np.array_equal(d1.cpu().numpy(), np.sqrt(np.take_along_axis(d2, want, 1)))
    with pytest.raises(ValueError):
        B.l2_topk(torch.zeros((2, d + 1), device=gpu), cat, 1)


def test_l2_topk_f16_falls_back_on_ties_and_scales(gpu, oracle_native, monkeypatch):
    """600 copies of one catalog row: for the query next to it more rows tie at the k-th neighbour than
    the shortlist holds, the verification cannot succeed and the query is recomputed by the f64 path --
    same ids (smallest indices first) as the canonical chain.  Un-normalised descriptors (norms 0.1 .. 40)
    keep the bound valid for everybody else."""
    from corsair_amd import backend as B, synth

    monkeypatch.setenv("CS_TOPK_MFMA", "16")
    q = (synth.make_descriptors(50, 128, seed=31) * np.linspace(0.1, 40, 50)[:, None]).astype(np.float32)
    base = (synth.make_descriptors(1500, 128, seed=32) * np.linspace(0.5, 30, 1500)[:, None]).astype(np.float32)
    x = np.concatenate([base, np.repeat(base[17:18], 600, axis=0)])
    q[0] = base[17] * np.float32(1.001)
    _topk_stats(reset=True)
    idx, dist = B.l2_topk(torch.from_numpy(q).to(gpu), torch.from_numpy(x).to(gpu), 5, True)
    took, fell_back = _topk_stats()
    assert took == 50 and 1 <= fell_back <= 5
    d2 = oracle_native.dist2_matrix(q, x)
    want = np.argsort(d2, axis=1, kind="stable")[:, :5]
    assert want[0].tolist() == [17, 1500, 1501, 1502, 1503]
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(dist.cpu().numpy(), np.sqrt(np.take_along_axis(d2, want, 1)))
    # descriptors beyond the f16 range: nothing is trusted, everything is recomputed
    big = (base * np.float32(3000.0)).astype(np.float32)
    _topk_stats(reset=True)
    idx, _ = B.l2_topk(torch.from_numpy(q).to(gpu), torch.from_numpy(big).to(gpu), 5, True)
    assert _topk_stats() == (50, 50)
    assert np.array_equal(idx.cpu().numpy(), np.argsort(oracle_native.dist2_matrix(q, big), axis=1, kind="stable")[:, :5])
    # without the copies everything verifies
    _topk_stats(reset=True)
    idx, _ = B.l2_topk(torch.from_numpy(q).to(gpu), torch.from_numpy(base).to(gpu), 5, True)
    took, fell_back = _topk_stats()
    assert took == 50 and fell_back == 0
    assert np.array_equal(idx.cpu().numpy(), np.argsort(oracle_native.dist2_matrix(q, base), axis=1, kind="stable")[:, :5])


@pytest.mark.parametrize("d", [256, 512])
def test_l2_topk_f16_tiny_norms_take_the_absolute_error_term(gpu, oracle_native, monkeypatch, d):
    """descriptors scaled by 1e-4 put the hi / lo halves of the f16 split into the subnormal
    range, where the split error is absolute (2^-25 per element), not relative.  With the absolute term in
    the verification bound the result is still exactly the canonical chain's -- through the shortlist or,
    where the bound no longer separates, through the f64 recomputation."""
    from corsair_amd import backend as B, synth

    monkeypatch.setenv("CS_TOPK_MFMA", "16")
    for scale_q, scale_x in ((1e-4, 1e-4), (1.0, 1e-4), (3e-3, 2.0)):
        q = (synth.make_descriptors(64, d, seed=41) * np.float32(scale_q)).astype(np.float32)
        x = (synth.make_descriptors(4096, d, seed=42) * np.float32(scale_x)).astype(np.float32)
        _topk_stats(reset=True)
        idx, dist = B.l2_topk(torch.from_numpy(q).to(gpu), torch.from_numpy(x).to(gpu), 10, True)
        took, _ = _topk_stats()
        assert took == 64
        d2 = oracle_native.dist2_matrix(q, x)
        want = np.argsort(d2, axis=1, kind="stable")[:, :10]
        assert np.array_equal(idx.cpu().numpy(), want), (scale_q, scale_x)
        assert np.array_equal(dist.cpu().numpy(), np.sqrt(np.take_along_axis(d2, want, 1)))


def test_l2_topk_large_matches_exact_slab_path(gpu, monkeypatch):
    """Stress-shaped run (65 536 x 262 144 x 256, top-10): MFMA path == exact slab path on a sample of
    queries, and the size-independent properties hold (sorted distances, unique ids, idempotent)."""
    from corsair_amd import backend as B, synth

    nq, nx = 65536, 262144
    q = torch.from_numpy(synth.make_descriptors(nq, 256, seed=1234)).to(gpu)
    x = torch.from_numpy(synth.make_descriptors(nx, 256, seed=4321)).to(gpu)
    idx, dist = B.l2_topk(q, x, 10, True)
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    assert bool((idx >= 0).all()) and bool((idx < nx).all())
    srt = torch.sort(idx, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    sample = torch.arange(0, nq, 1021, device=gpu)
    monkeypatch.setenv("CS_TOPK_MFMA", "0")
    idx_ref, dist_ref = B.l2_topk(q[sample].contiguous(), x, 10, True)
    assert torch.equal(idx[sample], idx_ref) and torch.equal(dist[sample], dist_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5])
def test_find_kcorr_subsample_follows_the_reference_expression(gpu, k):
    """utils/eval_pose.py:48-79 with subsample_size > 0 (off the evaluated path, VERDICT r4 missing #3): two draws without
    replacement from NumPy's global generator, F0's first; neighbours searched among the drawn rows only; indices refer to
    the full sets.  Written out here with SciPy's KDTree (the reference's call) on the same seed; below the size the
    reference does not sub-sample either."""
    from scipy.spatial import KDTree

    from corsair_amd.utils import eval_pose as EP

    rng = np.random.default_rng(3)
    F0 = rng.standard_normal((700, 16)).astype(np.float32)
    F1 = rng.standard_normal((900, 16)).astype(np.float32)
    np.random.seed(31)
    i0, i1 = EP.find_kcorr(F0, F1, k=k, subsample_size=256)
    np.random.seed(31)
    s0 = np.random.choice(700, 256, replace=False)
    s1 = np.random.choice(900, 256, replace=False)
    nn = KDTree(F1[s1]).query(F0[s0], k=k)[1].reshape(-1)
    assert np.array_equal(i0, np.repeat(s0, k)) and np.array_equal(i1, s1[nn])
    j0, j1 = EP.find_kcorr(F0, F1, k=k, subsample_size=700)      # len(F0) > subsample_size is false: everything
    assert np.array_equal(j0, np.repeat(np.arange(700), k))
    assert np.array_equal(j1, KDTree(F1).query(F0, k=k)[1].reshape(-1))
