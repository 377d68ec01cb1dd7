"""Non-finite rows in the nearest-neighbour family (cs_knn_feat, cs_l2_topk*, cs_chamfer_1dir / cs_hausdorff_1dir,
cs_ransac_batch, cs_voxelize*) and in sym_pose_batch, on every kernel path of each.  The contract is the "Non-finite"
paragraph of each entry in include/corsair_hip.h: a candidate whose canonical f64 squared distance is NaN or +inf is
never a neighbour, and a non-finite row changes nothing outside itself.  The references (tests/nonfinite_ref.py) are the CPU
oracle or NumPy f64 on the CLEANED problem; a finite 1e30 element is an ordinary, very distant row that exercises the
range fallbacks of the f16 and f64 shortlists."""
import numpy as np
import pytest
import torch

from tests import nonfinite_ref as NF

pytestmark = pytest.mark.gpu


def _feat(rng, n, d=16):
    f = rng.standard_normal((n, d)).astype(np.float32)
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()


# ---- cs_knn_feat -----------------------------------------------------------------------------------------------------
KNN_SIZES = [(70, 200), (40, 64), (33, 40), (257, 193)]
KNN_FINITE_TARGETS_OF_2 = (3, 17, 39)


def _knn_problems(oracle):
    rng = np.random.default_rng(101)
    qf = [_feat(rng, a) for a, _ in KNN_SIZES]
    tf = [_feat(rng, b) for _, b in KNN_SIZES]
    # dirty queries in problems 0 and 3: one at a row that is a multiple of 64, one at the last row, every kind once
    for p, rows in ((0, {64: "nan_elem", 69: "pos_inf", 7: "huge"}),
                    (3, {128: "nan_row", 256: "neg_inf", 192: "huge", 3: "nan_elem"})):
        for r, kind in rows.items():
            qf[p][r] = NF.dirty(qf[p][r], kind, (r + 5) % 16)
    # dirty targets in problem 0: the true nearest neighbour of query 0 becomes a NaN row, the others sit elsewhere
    nn0 = int(oracle.knn(qf[0][:1], tf[0], 1)[0, 0])
    dirty_t0 = {nn0: "nan_row", (nn0 + 50) % 200: "pos_inf", (nn0 + 91) % 200: "neg_inf", (nn0 + 130) % 200: "nan_elem",
                (nn0 + 161) % 200: "huge"}
    for r, kind in dirty_t0.items():
        tf[0][r] = NF.dirty(tf[0][r], kind, (r + 2) % 16)
    # problem 2: 37 of its 40 targets are NaN (whole rows and single elements): three neighbours, then two -1
    for r in range(40):
        if r not in KNN_FINITE_TARGETS_OF_2:
            tf[2][r] = NF.dirty(tf[2][r], "nan_row" if r % 2 else "nan_elem", r % 16)
    tf[3][100] = NF.dirty(tf[3][100], "huge", 9)     # finite: stays a (distant) candidate
    return qf, tf, nn0, sorted(dirty_t0)


def test_knn_feat_nonfinite_rows_all_paths(gpu, oracle_native, monkeypatch):
    from corsair_amd import backend as B

    qf, tf, nn0, dirty_t0 = _knn_problems(oracle_native)
    qoff, toff = _offsets(qf), _offsets(tf)
    Q = torch.from_numpy(np.concatenate(qf)).to(gpu)
    T = torch.from_numpy(np.concatenate(tf)).to(gpu)
    k = 5
    want = [NF.knn_clean(oracle_native, qf[p], tf[p], k) for p in range(4)]
    # the reference itself says what the case is about
    assert nn0 not in want[0][0][0] and (want[0][0][[64, 69]] == -1).all() and (want[0][0][7] >= 0).all()
    assert sorted(want[2][0][0, :3].tolist()) == list(KNN_FINITE_TARGETS_OF_2) and (want[2][0][:, 3:] == -1).all()
    assert np.isinf(want[2][1][:, 3:]).all() and (want[3][0][[128, 256, 3]] == -1).all()

    # labelled search: segments reused by several problems; the dirty target rows of segment 0 sit in ONE part
    rng = np.random.default_rng(102)
    lab_q_h = rng.integers(0, 4, qoff[-1]).astype(np.int32)
    lab_t_h = rng.integers(0, 4, toff[-1]).astype(np.int32)
    lab_q_h[10:20] = -1
    lab_t_h[30:60] = 9
    lab_t_h[dirty_t0] = 2
    perms = [[1, 2, 3, 0], [0, 3, 2, 1], [2, 2, 0, 0], [3, 0, 1, 2]]
    qseg = tseg = [0, 0, 3, 2]
    want_lab = [NF.knn_clean(oracle_native, qf[s], tf[s], k, lab_q_h[qoff[s]:qoff[s + 1]], lab_t_h[toff[s]:toff[s + 1]],
                             perms[j]) for j, s in enumerate(qseg)]
    lab_q, lab_t = torch.from_numpy(lab_q_h).to(gpu), torch.from_numpy(lab_t_h).to(gpu)
    perm_t = torch.tensor([p + [-3] * 4 for p in perms], dtype=torch.int32, device=gpu)

    by_path = {}
    for mfma in ("1", "0"):
        monkeypatch.setenv("CS_KNN_MFMA", mfma)
        idx, dist = (t.cpu().numpy() for t in B.knn_feat(Q, qoff, T, toff, k, return_distance=True))
        for p in range(4):
            assert np.array_equal(idx[qoff[p]:qoff[p + 1]], want[p][0]), (mfma, p)
            assert np.array_equal(dist[qoff[p]:qoff[p + 1]], want[p][1]), (mfma, p)
        # the clean problem is what it is alone
        solo_i, solo_d = (t.cpu().numpy() for t in B.knn_feat(Q[qoff[1]:qoff[2]], [0, 40], T[toff[1]:toff[2]], [0, 64], k,
                                                               return_distance=True))
        assert np.array_equal(idx[qoff[1]:qoff[2]], solo_i) and np.array_equal(dist[qoff[1]:qoff[2]], solo_d), mfma
        li, ld = (t.cpu().numpy() for t in B.knn_feat(Q, qoff, T, toff, k, qseg=qseg, tseg=tseg, qlabel=lab_q, tlabel=lab_t,
                                                       perm=perm_t, return_distance=True))
        row = 0
        for j, s in enumerate(qseg):
            n = qoff[s + 1] - qoff[s]
            assert np.array_equal(li[row:row + n], want_lab[j][0]), (mfma, "labelled", j)
            assert np.array_equal(ld[row:row + n], want_lab[j][1]), (mfma, "labelled", j)
            row += n
        by_path[mfma] = (idx, dist, li, ld)
    for mfma in ("0",):
        for a, b in zip(by_path["1"], by_path[mfma]):
            assert np.array_equal(a, b), mfma


# ---- cs_l2_topk / _sq / _catalog -------------------------------------------------------------------------------------
def _topk_stats(reset=False):
    import ctypes

    from corsair_amd import _lib

    out = (ctypes.c_uint64 * 2)()
    _lib.load().cs_l2_topk_stats(out, int(reset))
    return [int(v) for v in out]


@pytest.mark.parametrize("nq,nx,d,k,catalog", [(40, 200, 64, 10, "all"), (40, 200, 64, 10, "nan"), (33, 130, 512, 10, "all"),
                                               (33, 130, 512, 10, "nan"), (20, 300, 100, 5, "all"), (5, 70, 256, 12, "all"),
                                               (9, 70, 64, 10, "few")])
def test_l2_topk_nonfinite_rows_all_paths(gpu, oracle_native, monkeypatch, nq, nx, d, k, catalog):
    """Shapes: the three-term f16 kernel, the two-term one (d = 512), an f64-only shape (d = 100), an exact-only one
    (k > 10).  Catalog rows: "all" five dirty kinds (an infinite or 1e30 row puts max |x|^2 out of the f16 range, so the
    f16 path hands every query to the f64 one), "nan" NaN rows alone (the f16 shortlist and its verification stay in
    charge), "few": 5 of the 70 rows are finite and k = 10 -- 5 real rows, then 5 x (-1, +inf), on every path (before
    this test the exact slab path returned the infinite rows there and the shortlists did not)."""
    few = catalog == "few"
    from corsair_amd import backend as B, synth

    q = synth.make_descriptors(nq, d, seed=11 + nx)
    x = synth.make_descriptors(nx, d, seed=12 + nx)
    clean_first = int(np.argmin(oracle_native.dist2_matrix(q[:1], x)[0]))     # query 0's nearest row of the clean catalog
    for i, r in enumerate([1, 2, nq // 2, nq - 2, nq - 1]):                   # (query 0 stays clean)
        q[r] = NF.dirty(q[r], NF.DIRTY_KINDS[i], 3)
    if few:
        finite = (0, 13, 38, 64, 69)
        for r in range(nx):
            if r not in finite:
                x[r] = NF.dirty(x[r], NF.DIRTY_KINDS[r % 4], 7)               # NaN / inf kinds only
    else:
        # a NaN row in the place of query 0's nearest neighbour must remove exactly that row; the other kinds elsewhere
        rows = [clean_first] + [(clean_first + s) % nx for s in (17, 40, 63, 101)]
        kinds = ("nan_row", "nan_elem", "pos_inf", "neg_inf", "huge") if catalog == "all" else ("nan_row", "nan_elem") * 3
        for r, kind in zip(rows, kinds):
            x[r] = NF.dirty(x[r], kind, 7)
    want_i, want_d2 = NF.topk_clean(oracle_native, q, x, k)
    if few:
        assert sorted(want_i[0, :5].tolist()) == list(finite) and (want_i[0, 5:] == -1).all()
    else:
        assert clean_first not in want_i and (want_i[0] >= 0).all()
    assert (want_i[[1, 2, nq // 2, nq - 2]] == -1).all() and want_i[nq - 1, 0] >= 0        # the 1e30 query is finite
    Q, X = torch.from_numpy(q).to(gpu), torch.from_numpy(x).to(gpu)
    _topk_stats(reset=True)
    for mfma in ("0", "64", "16"):
        monkeypatch.setenv("CS_TOPK_MFMA", mfma)
        cat = B.TopkCatalog(X)
        calls = {"plain": (B.l2_topk(Q, X, k, True), False), "sq": (B.l2_topk(Q, X, k, True, squared=True), True),
                 "catalog": (B.l2_topk(Q, cat, k, True), False), "catalog_sq": (B.l2_topk(Q, cat, k, True, squared=True), True)}
        for name, ((idx, dist), squared) in calls.items():
            assert np.array_equal(idx.cpu().numpy(), want_i), (mfma, name)
            assert np.array_equal(dist.cpu().numpy(), want_d2 if squared else np.sqrt(want_d2)), (mfma, name)
        assert np.array_equal(B.l2_topk(Q, X, k).cpu().numpy(), want_i), (mfma, "indices only")
    took, recomputed = _topk_stats()
    print("top-k %s catalog: f16 path {queries, recomputed by the f64 path} = %s" % (catalog, [took, recomputed]))
    if catalog == "nan":
        # the lists compared above under "16" are the f16 shortlist's own: only some queries (the dirty ones are among
        # them) were handed to the f64 path
        assert took == 5 * nq and 5 * 4 <= recomputed < took, (took, recomputed)


# ---- cs_chamfer_1dir / cs_hausdorff_1dir -----------------------------------------------------------------------------
CH_PATHS = {"f16": {}, "f64": {"CS_CHAMFER_F16": "0"}, "valu": {"CS_CHAMFER_MFMA": "0"}}
CH_SRC_SEG, CH_TGT_SEG = [0, 1, 0, 1, 0, 1], [0, 0, 1, 1, 0, 1]


def _chamfer_clouds():
    from corsair_amd import synth

    rng = np.random.default_rng(7)
    src = [rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (300, 257)]
    tgt = [rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (600, 33)]
    Ts = np.stack([synth.random_pose(40 + i, max_trans=0.3).astype(np.float32) for i in range(6)])
    return src, tgt, Ts


def _chamfer_run(gpu, monkeypatch, path, src, tgt, Ts):
    from corsair_amd import backend as B

    for name in ("CS_CHAMFER_F16", "CS_CHAMFER_MFMA"):
        monkeypatch.delenv(name, raising=False)
    for name, value in CH_PATHS[path].items():
        monkeypatch.setenv(name, value)
    S, soff = torch.from_numpy(np.concatenate(src)).to(gpu), _offsets(src)
    G, toff = torch.from_numpy(np.concatenate(tgt)).to(gpu), _offsets(tgt)
    T = torch.from_numpy(Ts).to(gpu)
    return (B.chamfer_1dir(S, soff, G, toff, CH_SRC_SEG, CH_TGT_SEG, T).cpu().numpy(),
            B.hausdorff_1dir(S, soff, G, toff, CH_SRC_SEG, CH_TGT_SEG, T).cpu().numpy())


def _chamfer_cases():
    src, tgt, Ts = _chamfer_clouds()
    # the target of segment 0 that is nearest to source row 0 of segment 0 under pose 0: taking it out changes the answer
    p0 = src[0][0].astype(np.float64) @ Ts[0][:3, :3].astype(np.float64).T + Ts[0][:3, 3]
    near = int(np.argmin(((p0 - tgt[0].astype(np.float64)) ** 2).sum(axis=1)))
    cases = {}
    for kind in NF.DIRTY_KINDS:                      # a dirty target row (NaN, inf: never the nearest; 1e30: just far)
        t = [c.copy() for c in tgt]
        t[0][near] = NF.dirty(t[0][near], kind, 1)
        cases["target_" + kind] = (src, t, Ts)
    for kind in ("nan_row", "pos_inf"):              # the same in the 33-row segment, at its last row
        t = [c.copy() for c in tgt]
        t[1][32] = NF.dirty(t[1][32], kind, 2)
        cases["small_target_" + kind] = (src, t, Ts)
    s = [c.copy() for c in src]
    s[0][299] = NF.dirty(s[0][299], "nan_elem", 0)   # one NaN source row: +inf for the problems of segment 0
    cases["source_nan"] = (s, tgt, Ts)
    s = [c.copy() for c in src]
    s[1][64] = NF.dirty(s[1][64], "neg_inf", 2)
    cases["source_inf"] = (s, tgt, Ts)
    Tn = Ts.copy()
    Tn[2, 1, 2] = np.nan                             # a NaN in d_T of problem 2
    cases["pose_nan"] = (src, tgt, Tn)
    t = [c.copy() for c in tgt]
    t[1][:] = np.nan                                 # no finite target in segment 1
    cases["target_all_nan"] = (src, t, Ts)
    return (src, tgt, Ts), cases


def test_chamfer_hausdorff_nonfinite_rows_all_paths(gpu, oracle_native, monkeypatch):
    clean, cases = _chamfer_cases()
    clean_out = {path: _chamfer_run(gpu, monkeypatch, path, *clean) for path in CH_PATHS}
    for name, (src, tgt, Ts) in cases.items():
        want_cd = np.array([NF.chamfer_clean(oracle_native, src[CH_SRC_SEG[p]], tgt[CH_TGT_SEG[p]], Ts[p]) for p in range(6)])
        want_hd = np.array([NF.nearest_clean(src[CH_SRC_SEG[p]], tgt[CH_TGT_SEG[p]], Ts[p]).max() for p in range(6)])
        # problems that hold no dirty value at all: bit-identical to the clean batch on the same path
        untouched = [p for p in range(6) if np.isfinite(src[CH_SRC_SEG[p]]).all() and np.isfinite(Ts[p]).all() and
                     np.array_equal(tgt[CH_TGT_SEG[p]], clean[1][CH_TGT_SEG[p]])]
        if name == "pose_nan":
            assert untouched == [0, 1, 3, 4, 5] and np.isinf(want_cd[2]) and np.isinf(want_hd[2])
        if name == "source_nan":
            assert np.isinf(want_cd[[0, 2, 4]]).all() and np.isfinite(want_cd[[1, 3, 5]]).all()
        if name == "target_all_nan":
            assert np.isinf(want_cd[[2, 3, 5]]).all() and np.isinf(want_hd[[2, 3, 5]]).all()
        hd_by_path = {}
        for path in CH_PATHS:
            cd, hd = _chamfer_run(gpu, monkeypatch, path, src, tgt, Ts)
            for p in range(6):
                if np.isinf(want_cd[p]):
                    assert cd[p] == np.inf and hd[p] == np.inf, (name, path, p, cd[p], hd[p])
                else:
                    assert cd[p] == pytest.approx(want_cd[p], rel=1e-12), (name, path, p)
                    assert hd[p] == pytest.approx(want_hd[p], rel=1e-12), (name, path, p)
            for p in untouched:
                assert cd[p] == clean_out[path][0][p] and hd[p] == clean_out[path][1][p], (name, path, p)
            hd_by_path[path] = hd
        assert np.array_equal(hd_by_path["f16"], hd_by_path["f64"]) and np.array_equal(hd_by_path["f16"], hd_by_path["valu"]), name


# ---- cs_ransac_batch -------------------------------------------------------------------------------------------------
def _corr_problem(rng, m, inlier_frac, noise=0.01, pose_id=0):
    from corsair_amd import synth

    src = rng.uniform(-0.8, 0.8, (m, 3)).astype(np.float32)
    T = synth.random_pose(pose_id, max_trans=0.5)
    tgt = synth.apply_pose(src, T) + rng.normal(0, noise, (m, 3)).astype(np.float32)
    bad = rng.random(m) > inlier_frac
    tgt[bad] = rng.uniform(-1.2, 1.2, (int(bad.sum()), 3)).astype(np.float32)
    return src, tgt.astype(np.float32)


def _ransac_problems():
    """Problems 0 (193 pairs, 85 % inliers: stops early) and 1 (400, 55 %: runs all iterations): 5 % of the pairs dirty, on
    either side, every kind; 2 (10 pairs), 3 (none) and 5 (257 pairs, 45 % inliers: a clean problem that keeps the prefilter
    busy to the last iteration) are clean; 4 has a NaN in every pair."""
    rng = np.random.default_rng(77)
    probs = [list(_corr_problem(rng, m, f, pose_id=60 + i)) for i, (m, f) in
             enumerate([(193, 0.85), (400, 0.55), (10, 0.9), (0, 0.5), (50, 0.5), (257, 0.45)])]
    for p in (0, 1):
        m = len(probs[p][0])
        for i, r in enumerate(rng.choice(m, max(1, m // 20), replace=False)):
            side = probs[p][i % 2]
            side[r] = NF.dirty(side[r], NF.DIRTY_KINDS[i % 5], i % 3)
    probs[4][0][:, 1] = np.nan
    probs[4][1][::2] = np.nan
    return probs


def _prefilter_stats(reset=False):
    import ctypes

    from corsair_amd import _lib

    out = (ctypes.c_uint64 * 5)()
    _lib.load().cs_ransac_prefilter_stats(out, int(reset))
    return [int(v) for v in out]


@pytest.mark.parametrize("pf_k", [16, 32])
def test_ransac_nonfinite_pairs(gpu, oracle_native, monkeypatch, pf_k):
    """rmse and inliers are those of the best f64 transform, which the entry point returns only as its f32 cast: the
    reference loop (nonfinite_ref.ransac_clean: the header's loop with the oracle's sampling and rigid fit on finite
    samples, a NumPy f64 recount over the finite pairs) supplies the f64 transform, its cast must BE the returned matrix,
    and its recount must give the returned inliers and rmse (1e-12).  A recount of the RETURNED matrix widened to f64
    gives the same inlier counts (asserted) but cannot give the rmse to 1e-12: the f32 rounding of the transform moves it
    by 9.6e-8 (problem 0: 0.054360701314723446 against 0.05436069612406648) and 7.4e-8 (problem 1) relative."""
    from corsair_amd import backend as B

    monkeypatch.setenv("CS_RANSAC_PF_K", str(pf_k))
    probs = _ransac_problems()
    max_corr, max_iter, seed = 0.2, 700, 3

    def run(sel):
        off = _offsets([probs[p][0] for p in sel])
        S = torch.from_numpy(np.concatenate([probs[p][0] for p in sel])).to(gpu)
        D = torch.from_numpy(np.concatenate([probs[p][1] for p in sel])).to(gpu)
        return [t.cpu().numpy() for t in B.ransac_batch(S, D, off, max_corr, 10, max_iter, 0.999, seed)]

    everything = list(range(6))
    monkeypatch.setenv("CS_RANSAC_PREFILTER", "0")
    exact = run(everything)
    monkeypatch.setenv("CS_RANSAC_PREFILTER", "1")
    monkeypatch.setenv("CS_RANSAC_CHECK", "1")
    _prefilter_stats(reset=True)
    checked = run(everything)                # CorsairHipError on a bound violation
    assert _prefilter_stats()[0] == 0
    monkeypatch.delenv("CS_RANSAC_CHECK")
    plain = run(everything)
    for a, b, c in zip(exact, checked, plain):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    T, inl, rmse, iters = plain
    # no finite pair: identity, 0 inliers, rmse 0
    assert np.array_equal(T[4], np.eye(4, dtype=np.float32)) and inl[4] == 0 and rmse[4] == 0.0
    # the clean problems are what they are in a batch without the others
    clean = [2, 3, 5]
    alone = run(clean)
    for got, want in zip(plain, alone):
        assert np.array_equal(got[clean], want)
    for p in (0, 1, 2, 5):
        wT, wT64, winl, wrmse, wit = NF.ransac_clean(oracle_native, probs[p][0], probs[p][1], max_corr, 10, max_iter, 0.999, seed)
        print("ransac problem %d: inliers %d (ref %d) rmse %.17g (ref %.17g) iters %d (ref %d)" %
              (p, inl[p], winl, rmse[p], wrmse, iters[p], wit))
        assert np.array_equal(T[p], wT), p
        assert inl[p] == winl and iters[p] == wit, (p, inl[p], winl, iters[p], wit)
        assert rmse[p] == pytest.approx(wrmse, rel=1e-12), p
        if p in (0, 1):
            assert winl >= (20 if p == 0 else 1), (p, winl)     # the dirty problems are registration problems, not empty ones
            cnt, err, scale = NF.ransac_count(wT64[:, :3], wT64[:, 3], probs[p][0], probs[p][1], max_corr)
            assert cnt == inl[p] and np.sqrt(err / scale / cnt) == pytest.approx(rmse[p], rel=1e-12)
            T64c = T[p].astype(np.float64)
            assert NF.ransac_count(T64c[:3, :3], T64c[:3, 3], probs[p][0], probs[p][1], max_corr)[0] == inl[p]


# ---- cs_voxelize / cs_voxelize_f64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxelize_refuses_nonfinite_and_far_coordinates(gpu, dtype):
    """voxel = 0.5 makes x / voxel exact in both types: 16383.5 is index 32767, the last one coord_in_range accepts, 16384.0 is
    32768, the first it refuses; likewise -16383.5 / -16384.0."""
    from corsair_amd import _lib, backend as B

    rng = np.random.default_rng(5)
    voxel = 0.5
    clouds = [rng.uniform(-1, 1, (150, 3)).astype(dtype) for _ in range(2)]
    off = [0, 150, 300]

    def check_valid(cl):
        keep, grid, out_off = B.voxelize(torch.from_numpy(np.concatenate(cl)).to(gpu), off, voxel)
        wk, wg, wo = NF.voxelize_clean(cl, voxel)
        assert np.array_equal(keep.cpu().numpy(), wk) and np.array_equal(grid.cpu().numpy(), wg) and out_off == wo
        return grid.cpu().numpy()

    check_valid(clouds)
    for bad in (np.nan, np.inf, -np.inf, 1e30, 16384.0, -16384.0):
        cl = [c.copy() for c in clouds]
        cl[1][77, 1] = bad
        with pytest.raises(_lib.CorsairHipError, match="cs_voxelize"):
            B.voxelize(torch.from_numpy(np.concatenate(cl)).to(gpu), off, voxel)
        check_valid(clouds)                  # the next valid call on the thread is right
    for last, index in ((16383.5, 32767), (-16383.5, -32767)):
        cl = [c.copy() for c in clouds]
        cl[1][77, 1] = last
        grid = check_valid(cl)
        assert ((grid[:, 0] == 1) & (grid[:, 2] == index)).sum() == 1


# ---- sym_pose_batch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("use_symmetry", [True, False])
@pytest.mark.parametrize("registration", ["ransac", "fgr"])
def test_sym_pose_refuses_nonfinite_descriptors(gpu, monkeypatch, registration, use_symmetry, split):
    """SciPy's KD-tree raises ValueError on non-finite data (build: the CAD side) and queries; so does sym_pose_batch,
    naming the pair and the side, and the calls around the refused one are unaffected."""
    from corsair_amd import registration as R

    monkeypatch.setenv("CORSAIR_SPLIT_RANSAC", split)
    rng = np.random.default_rng(21)
    n0, n1 = [300, 290], [200, 210]
    F0, F1 = _feat(rng, sum(n0)), _feat(rng, sum(n1))
    X0 = rng.uniform(-1, 1, (sum(n0), 3)).astype(np.float32)
    X1 = rng.uniform(-1, 1, (sum(n1), 3)).astype(np.float32)
    off0, off1 = [0, 300, 590], [0, 200, 410]

    def call(f0, f1):
        dev = [torch.from_numpy(a).to(gpu) for a in (f0, X0, f1, X1)]
        return R.sym_pose_batch(dev[0], dev[1], off0, dev[2], dev[3], off1, [1, 2], 5, 0.2, 0, None, 100, 400, 0.999,
                                use_symmetry, True, registration=registration)

    def same(a, b):
        return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("T_best", "cd_best", "T_all", "cd_all", "inliers",
                                                                      "iters")) and a.prob_pair == b.prob_pair

    before = call(F0, F1)
    bad_q = F0.copy()
    bad_q[300 + 64, 3] = np.nan                        # pair 1, query side
    with pytest.raises(ValueError, match=r"query descriptors of pair 1\b"):
        call(bad_q, F1)
    assert same(call(F0, F1), before)
    bad_c = F1.copy()
    bad_c[17] = np.nan                                 # pair 0, CAD side
    with pytest.raises(ValueError, match=r"CAD descriptors of pair 0\b"):
        call(F0, bad_c)
    assert same(call(F0, F1), before)
    both = bad_q.copy()
    both[5, 0] = np.inf                                # pair 0 too: the first pair is the one named
    with pytest.raises(ValueError, match=r"query descriptors of pair 0\b"):
        call(both, F1)
