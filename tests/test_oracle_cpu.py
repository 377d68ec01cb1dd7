"""CPU suite (-m "not gpu"): pins the oracle against the reference's own golden vectors and against
independent cross-oracles (dense conv3d, SciPy cKDTree/cdist, NumPy SVD), checks the host logic and
that the C-ABI library loads and exports every declared symbol.  No GPU compute is called."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- golden vectors from the reference's shipped caches ---------------------------------------------
def test_eval_pose_known_answers():
    """eval_pose (utils/eval_pose.py:103-128) vs (t, r) pairs cached by the reference
    (data/cache_*/{r,t}_losses_*; T0 = configs/fix_trans.npy[i,0], T1 = I)."""
    from corsair_amd.utils.eval_pose import eval_pose
    from oracle import post

    z = np.load(os.path.join(GOLD, "eval_pose_kat.npz"))
    assert z["reproduced"][0] >= z["reproduced"][1] - 2  # 20542 / 20544 at generation time
    assert len(z["sym"]) >= 200
    for i in range(len(z["sym"])):
        for fn in (post.eval_pose, eval_pose):
            t, r = fn(z["T_est"][i], z["T0"][i], np.eye(4), int(z["sym"][i]))
            assert abs(r - z["r"][i]) < 1e-4 and abs(t - z["t"][i]) < 1e-4, (i, str(z["src"][i]))


def test_aggregate_reproduces_readme_tables():
    """evaluation.py:334-358 aggregation on the cached per-query losses -> README.md:175-176,215-216."""
    from corsair_amd.harness import aggregate

    z = np.load(os.path.join(GOLD, "aggregate_kat.npz"))
    for tag, rk, tk in (("nosym", "r_losses_ransac", "t_losses_ransac"), ("sym", "r_losses_sym", "t_losses_sym")):
        a = aggregate(z[rk], z[tk], z["chamfer_dist_" + ("ransac" if tag == "nosym" else "sym")])
        rre = np.array([a["rre_mean_deg"], 100 * a["rre_5"], 100 * a["rre_15"], 100 * a["rre_45"]])
        rte = np.array([a["rte_mean"], 100 * a["rte_002"], 100 * a["rte_005"], 100 * a["rte_010"], 100 * a["rte_015"]])
        assert np.allclose(rre, z["readme_rre_" + tag], atol=0.011), (tag, rre)
        assert np.allclose(rte, z["readme_rte_" + tag], atol=0.011), (tag, rte)
    # "keep the best by Chamfer" invariant of sym_pose (utils/symmetry.py:322-324,354-356)
    assert (z["chamfer_dist_sym"] <= z["chamfer_dist_ransac"] + 1e-12).all()


def test_retrieval_oracle_matches_reference_run():
    """oracle retrieval vs the outputs of the reference's own utils/retrieval.py (fixture made by
    importing it in the build container, tests/golden/make_fixtures.py)."""
    from oracle import post

    z = np.load(os.path.join(GOLD, "retrieval_kat.npz"))
    pos_n = int(z["pos_n"])
    rank, dist = post.retrieval_rank(z["scan"], z["lib"])
    assert np.array_equal(rank[:, :pos_n], z["rank_top"])
    assert np.allclose(np.take_along_axis(dist, rank[:, :pos_n], 1), z["dist_top"], rtol=0, atol=1e-12)
    stat = post.scan2cad_retrieval_eval(z["scan"], z["lib"], z["best_match"], z["table"], pos_n)
    assert stat["precision"] == pytest.approx(float(z["precision"]), abs=1e-12)
    assert stat["top1_error"] == pytest.approx(float(z["top1_error"]), abs=1e-12)
    assert stat["top1_predict"] == z["top1_predict"].tolist() and stat["gt"] == z["gt"].tolist()
    # the host-side metric of the product (rank -> stats) on the same ranks
    from corsair_amd.utils import retrieval

    stat2 = retrieval.scan2cad_retrieval_eval_rank(rank[:, :pos_n], z["table"], z["best_match"], pos_n)
    assert stat2["precision"] == pytest.approx(float(z["precision"]), abs=1e-12)


# ---- C ABI ------------------------------------------------------------------------------------------
def test_library_exports_every_declared_symbol():
    from corsair_amd import _lib

    lib = _lib.load()
    names = _lib.header_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), n
    assert lib.cs_version() >= 100
    assert isinstance(lib.cs_last_error(), bytes)


def test_product_fails_loudly_without_gpu():
    import torch

    from corsair_amd import _lib, backend

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.CorsairHipError):
        _lib.require_gpu()
    with pytest.raises(_lib.CorsairHipError):
        backend.CoordMap.create(torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(_lib.CorsairHipError):
        backend.l2_topk(torch.zeros((2, 8)), torch.zeros((3, 8)), 1)


# ---- sparse-side semantics --------------------------------------------------------------------------
def _coords(seed, n=500, span=8, batch=2):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(batch):
        g = rng.integers(-span, span, (n, 3))
        _, first = np.unique(g, axis=0, return_index=True)
        g = g[np.sort(first)]
        out.append(np.concatenate([np.full((len(g), 1), b), g], 1))
    return np.concatenate(out).astype(np.int32)


def test_shim_sparse_quantize_inverse_map_pairs_with_the_kept_rows():
    """ME.utils.sparse_quantize(return_index=True, return_inverse=True): coords[index][inverse] == coords
    (VERDICT r1 hygiene: the inverse used to follow np.unique's lexicographic numbering)."""
    import corsair_amd.minkowski as ME

    rng = np.random.default_rng(1)
    g = rng.integers(-4, 4, (3000, 3))
    idx, inv = ME.utils.sparse_quantize(g, return_index=True, return_inverse=True, return_maps_only=True)
    assert (np.diff(idx) > 0).all() and np.array_equal(g[idx][inv], g)
    q, idx2, inv2 = ME.utils.sparse_quantize(g, return_index=True, return_inverse=True)
    assert np.array_equal(idx2, idx) and np.array_equal(inv2, inv) and np.array_equal(q, g[idx])


def test_sparse_quantize_keeps_first_point_per_voxel():
    from oracle import sparse

    rng = np.random.default_rng(0)
    pts = rng.uniform(-1, 1, (4000, 3)).astype(np.float32)
    xyz, grid, keep = sparse.quantize_cloud(pts, 0.1)
    assert (np.diff(keep) > 0).all()
    g = np.floor(pts / np.float32(0.1)).astype(np.int64)
    seen = {}
    for i, v in enumerate(map(tuple, g)):
        seen.setdefault(v, i)
    assert sorted(seen.values()) == keep.tolist()
    assert np.array_equal(grid, g[keep]) and np.array_equal(xyz, pts[keep])
    # collate prepends the batch index, int32
    c = sparse.sparse_collate([grid, grid[:10]])
    assert c.dtype == np.int32 and c.shape == (len(grid) + 10, 4) and (c[-10:, 0] == 1).all()


def test_quantize_cloud_floors_in_the_clouds_own_type():
    """The reference floors `rot_coords / voxel_size` in whatever type the cloud has: f32 for the catalog
    (utils/Info/CADLib.py:106-121), f64 for posed queries (datasets/CategoryDataset.py:179-197 on apply_transform's
    output, evaluation-shapenet.py:97-119).  The oracle preserves the type; narrowing first changes voxels."""
    from corsair_amd import synth
    from oracle import sparse

    moved = 0
    for c in (63, 110, 186, 197, 5):
        p64 = synth.apply_pose(synth.make_cloud(c, 15000)[:10000], synth.random_pose(c), np.float64)
        xyz, grid, keep = sparse.quantize_cloud(p64, 0.03)
        assert xyz.dtype == np.float64
        g = np.floor(p64 / 0.03)
        seen = {}
        for i, v in enumerate(map(tuple, g.astype(np.int64))):
            seen.setdefault(v, i)
        assert sorted(seen.values()) == keep.tolist() and np.array_equal(grid, g[keep].astype(np.int32))
        p32 = p64.astype(np.float32)
        x32, g32, k32 = sparse.quantize_cloud(p32, 0.03)
        assert x32.dtype == np.float32
        assert np.array_equal(g32, np.floor(p32 / np.float32(0.03))[k32].astype(np.int32))
        moved += int(not np.array_equal(np.floor(p32 / np.float32(0.03)).astype(np.float64), g))
    assert moved >= 3
    with pytest.raises(TypeError):
        sparse.quantize_cloud(np.zeros((4, 3), np.int32), 0.03)


def test_strided_map_first_occurrence_order_and_kernel_map_properties():
    from oracle import sparse

    c1 = _coords(1)
    c2, ts2 = sparse.coordmap_stride(c1, 1)
    assert ts2 == 2 and (c2[:, 1:] % 2 == 0).all()
    # first-occurrence order: walking c1, new coarse cells appear in exactly c2's order
    seen, order = set(), []
    for r in c1:
        k = (r[0], r[1] // 2 * 2, r[2] // 2 * 2, r[3] // 2 * 2)
        if k not in seen:
            seen.add(k)
            order.append(k)
    assert [tuple(r) for r in c2] == order
    # same-stride map: pair (k, i, o) exists iff (26-k, o, i) exists; centre offset is the identity
    nbr = sparse.kernel_map(c1, 1, c1, 1)
    assert np.array_equal(nbr[:, 13], np.arange(len(c1)))
    k, i, o = sparse.kernel_map_triples(nbr)
    fwd = set(zip(k.tolist(), i.tolist(), o.tolist()))
    assert fwd == {(26 - kk, oo, ii) for kk, ii, oo in fwd}
    # transposed map = strided map with in/out swapped and the same k
    down = sparse.kernel_map(c1, 1, c2, 2)
    up = sparse.kernel_map(c2, 2, c1, 1, transposed=True)
    kd, idn, od = sparse.kernel_map_triples(down)
    ku, iu, ou = sparse.kernel_map_triples(up)
    assert set(zip(kd.tolist(), idn.tolist(), od.tolist())) == set(zip(ku.tolist(), ou.tolist(), iu.tolist()))
    # every fine voxel has its parent cell among its transposed neighbours
    assert ((up >= 0).sum(1) >= 1).all()


@pytest.mark.parametrize("mode", ["same", "down", "up"])
def test_sparse_conv_equals_dense_conv3d(oracle_native, mode):
    """Independent cross-oracle: densify, run torch conv3d / conv_transpose3d on the
    CPU, sample at the sparse output coordinates."""
    import torch
    import torch.nn.functional as F

    from oracle import sparse

    rng = np.random.default_rng(5)
    g = rng.integers(0, 12, (300, 3))
    _, first = np.unique(g, axis=0, return_index=True)
    g = g[np.sort(first)]
    c1 = np.concatenate([np.zeros((len(g), 1), np.int64), g], 1).astype(np.int32)
    c2, _ = sparse.coordmap_stride(c1, 1)
    cin, cout, G = 5, 7, 14
    w = rng.standard_normal((27, cin, cout)).astype(np.float32)
    # dense kernel Wd[co, ci, dz+1, dy+1, dx+1] = kernel[k(dx,dy,dz), ci, co]
    wd = np.zeros((cout, cin, 3, 3, 3), np.float32)
    for k in range(27):
        dx, dy, dz = k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1
        wd[:, :, dz + 1, dy + 1, dx + 1] = w[k].T

    def densify(coords, feats, scale):
        X = np.zeros((1, feats.shape[1], G, G, G), np.float32)
        X[0, :, coords[:, 3] // scale, coords[:, 2] // scale, coords[:, 1] // scale] = feats
        return torch.from_numpy(X)

    if mode == "same":
        x = rng.standard_normal((len(c1), cin)).astype(np.float32)
        got = oracle_native.conv_fwd(sparse.kernel_map(c1, 1, c1, 1), x, w)
        Y = F.conv3d(densify(c1, x, 1), torch.from_numpy(wd), padding=1)[0].numpy()
        want = Y[:, c1[:, 3], c1[:, 2], c1[:, 1]].T
    elif mode == "down":
        x = rng.standard_normal((len(c1), cin)).astype(np.float32)
        got = oracle_native.conv_fwd(sparse.kernel_map(c1, 1, c2, 2), x, w)
        Y = F.conv3d(densify(c1, x, 1), torch.from_numpy(wd), stride=2, padding=1)[0].numpy()
        want = Y[:, c2[:, 3] // 2, c2[:, 2] // 2, c2[:, 1] // 2].T
    else:
        x = rng.standard_normal((len(c2), cin)).astype(np.float32)
        got = oracle_native.conv_fwd(sparse.kernel_map(c2, 2, c1, 1, transposed=True), x, w)
        # out[o] = sum_k W[k] in[(o - delta_k)/2]  ==  conv_transpose3d with the spatially flipped
        # kernel; torch's layout is [cin, cout, kz, ky, kx]
        wt = np.ascontiguousarray(np.transpose(wd, (1, 0, 2, 3, 4)))
        Xc = np.zeros((1, cin, G // 2, G // 2, G // 2), np.float32)
        Xc[0, :, c2[:, 3] // 2, c2[:, 2] // 2, c2[:, 1] // 2] = x
        Y = F.conv_transpose3d(torch.from_numpy(Xc), torch.from_numpy(wt), stride=2, padding=1,
                               output_padding=1)[0].numpy()
        want = Y[:, c1[:, 3], c1[:, 2], c1[:, 1]].T
    assert np.allclose(got, want, rtol=1e-4, atol=1e-4), np.abs(got - want).max()


def test_real_cloud_statistics_and_forward(oracle_native):
    """Bundled ShapeNet clouds through the oracle network: occupancy statistics match SURVEY
    Appendix B, outputs are unit rows, skip features non-negative."""
    from corsair_amd import synth
    from oracle import resunet, sparse

    z = np.load(os.path.join(GOLD, "real_clouds.npz"))
    pc = z["chair"].copy()
    pc -= pc.mean(0)
    pc = pc / np.max(np.linalg.norm(pc, 2, 1))
    xyz, grid, _ = sparse.quantize_cloud(pc, 0.03)
    assert 1500 < len(grid) < 11000
    coords = sparse.sparse_collate([grid])
    maps, km = resunet.build_maps(coords)
    pairs_per_point = (km["s1"] >= 0).sum() / len(grid)
    assert 5.0 < pairs_per_point < 16.0
    assert (km["s1_s2"] >= 0).sum() == (km["s2_s1_T"] >= 0).sum()
    sd, emb = synth.make_state_dicts(31)
    out, feat, _ = resunet.resunet_forward(sd, coords, np.ones((len(grid), 1), np.float32))
    assert out.shape == (len(grid), 16) and feat.shape[1] == 256
    assert np.allclose(np.linalg.norm(out, axis=1), 1.0, atol=1e-5) and (feat >= 0).all()
    g = resunet.embedding_forward(emb, feat, maps["c8"][:, 0], 1)
    assert g.shape == (1, 256) and abs(np.linalg.norm(g) - 1) < 1e-5


# ---- post-processing cross-oracles ----------------------------------------------------------------------
def test_knn_and_chamfer_match_scipy_kdtree(oracle_native):
    """find_knn_cpu is scipy KDTree(feat1).query(feat0, k) (utils/find_nn.py:43-49);
    chamfer_kdtree_1direction is KDTree(pc1).query(pc0).mean() (utils/preprocess.py:67-70)."""
    from scipy.spatial import KDTree

    rng = np.random.default_rng(2)
    f0 = rng.standard_normal((400, 16)).astype(np.float32)
    f1 = rng.standard_normal((700, 16)).astype(np.float32)
    idx, dist = oracle_native.knn(f0, f1, 5, return_distance=True)
    dd, ii = KDTree(f1).query(f0, k=5)
    assert np.array_equal(idx, ii) and np.allclose(dist, dd, rtol=1e-12)
    a = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    b = rng.uniform(-1, 1, (800, 3)).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.1, -0.2, 0.05]
    want = KDTree(b).query(a.astype(np.float64) + T[:3, 3].astype(np.float64))[0].mean()
    assert oracle_native.chamfer_1dir(a, b, T) == pytest.approx(want, rel=1e-12)


def test_rigid_fit_matches_svd_umeyama(oracle_native):
    """Horn-quaternion fit == Eigen::umeyama(with_scaling=false) (SVD form) on random point sets."""
    from corsair_amd import synth

    rng = np.random.default_rng(3)
    for trial in range(20):
        n = int(rng.integers(3, 12))
        ps = rng.uniform(-1, 1, (n, 3))
        T = synth.random_pose(trial, max_trans=0.7)
        pt = ps @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.02, (n, 3))
        R, t = oracle_native.rigid_fit(ps, pt)
        cs, ct = ps.mean(0), pt.mean(0)
        H = (pt - ct).T @ (ps - cs)
        U, S, Vt = np.linalg.svd(H)
        D = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
        Rw = U @ D @ Vt
        assert np.allclose(R, Rw, atol=1e-9) and np.allclose(t, ct - Rw @ cs, atol=1e-9)
        assert abs(np.linalg.det(R) - 1) < 1e-12


def test_rigid_fit_characteristic_polynomial_path_and_its_fallback(oracle_native):
    """Round 4: the largest eigenpair of the Horn matrix comes from its characteristic polynomial (Halley from
    sqrt(3)|S|_F, adjugate row) -- path 0 -- with the Jacobi solver as the fallback when the largest eigenvalue is
    not well separated -- path 1.  Both agree with the SVD optimum where that is unique and with each other."""
    rng = np.random.default_rng(17)
    paths = []
    for trial in range(3000):
        n = 10 if trial % 3 else int(rng.integers(3, 12))
        ps = rng.uniform(-1, 1, (n, 3))
        pt = rng.uniform(-1, 1, (n, 3)) if trial % 2 else ps @ _rot(rng).T + rng.normal(0, 0.05, (n, 3)) + rng.uniform(-1, 1, 3)
        R, t, path = oracle_native.rigid_fit(ps, pt, return_path=True)
        paths.append(path)
        Rj, tj = oracle_native.rigid_fit(ps, pt, force_jacobi=True)
        cs, ct = ps.mean(0), pt.mean(0)
        U, S, Vt = np.linalg.svd((pt - ct).T @ (ps - cs))
        d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
        sep = (S[1] + d * S[2]) / S[0]                    # (l1 - l2) / 2 sigma1: how unique the optimum is
        if sep > 1e-3:
            Rw = U @ np.diag([1, 1, d]) @ Vt
            tol = 1e-11 / sep
            assert np.abs(R - Rw).max() < tol and np.abs(Rj - Rw).max() < tol, (trial, path, sep)
            assert np.abs(t - (ct - Rw @ cs)).max() < 4 * tol
        assert abs(np.linalg.det(R) - 1) < 1e-12
    assert np.mean(paths) < 0.01                          # the fallback is rare on generic samples
    # degenerate samples take the fallback and give what the Jacobi solver gives, bit for bit
    line = np.outer(np.linspace(-1, 1, 10), [0.3, -0.5, 0.8])
    same = np.tile([[0.2, 0.1, -0.4]], (10, 1))
    tgt = rng.uniform(-1, 1, (10, 3))
    for ps in (line, same):
        R, t, path = oracle_native.rigid_fit(ps, tgt, return_path=True)
        Rj, tj = oracle_native.rigid_fit(ps, tgt, force_jacobi=True)
        assert path == 1 and np.array_equal(R, Rj) and np.array_equal(t, tj)


def _rot(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_ransac_oracle_recovers_pose_and_exits_early(oracle_native):
    from corsair_amd import synth

    rng = np.random.default_rng(4)
    src = rng.uniform(-0.8, 0.8, (1500, 3)).astype(np.float32)
    T = synth.random_pose(9, max_trans=0.4)
    tgt = synth.apply_pose(src, T) + rng.normal(0, 0.005, (1500, 3)).astype(np.float32)
    bad = rng.random(1500) > 0.6
    tgt[bad] = rng.uniform(-1.2, 1.2, (int(bad.sum()), 3)).astype(np.float32)
    Te, inl, rmse, iters = oracle_native.ransac(src, tgt.astype(np.float32), 0.05, 10, 20000, 0.999, 0)
    assert iters < 20000 and inl > 0.5 * 1500
    assert np.abs(Te[:3, :3] - T[:3, :3]).max() < 0.05 and np.abs(Te[:3, 3] - T[:3, 3]).max() < 0.05
    # expected early-exit bound from the final inlier ratio (Open3D formula)
    k = np.log(1 - 0.999) / np.log(1 - (inl / 1500) ** 10)
    assert iters <= int(np.ceil(k)) + 1 or iters == 20000
    # confidence 1.0 never exits early; fewer pairs than ransac_n -> identity
    assert oracle_native.ransac(src[:200], tgt[:200].astype(np.float32), 0.05, 10, 300, 1.0, 0)[3] == 300
    Ti, inl0, _, it0 = oracle_native.ransac(src[:5], tgt[:5].astype(np.float32), 0.05, 10, 300, 0.999, 0)
    assert np.array_equal(Ti, np.eye(4, dtype=np.float32)) and inl0 == 0 and it0 == 0


def test_ransac_oracle_equals_an_independent_f64_replay(oracle_native):
    """Independent check of oc_ransac (it lands with every edit of that function):
    a plain NumPy replay of Open3D's single-thread loop in float64 -- samples from the counter RNG,
    SVD (Umeyama, no scaling) fit instead of the Horn quaternion, `(R @ s.T).T + t - q` with ordinary
    matmul instead of the fma chain, the comparison with the DOUBLE max_corr ** 2, better = more inliers
    or equal inliers and smaller rmse, est_k from Open3D's formula -- must select the same iteration,
    count, iteration total and (to 1e-6) transform.  The number of (hypothesis, pair) decisions an f32
    evaluation (the oracle's arithmetic before round 2) would flip is printed (-s)."""
    from corsair_amd import synth

    rng = np.random.default_rng(21)
    for trial, (m, frac, max_corr, max_iter) in enumerate([(700, 0.5, 0.2, 1500), (1200, 0.25, 0.05, 2500),
                                                           (400, 0.8, 0.1, 1000)]):
        src = rng.uniform(-0.8, 0.8, (m, 3)).astype(np.float32)
        T = synth.random_pose(60 + trial, max_trans=0.4)
        tgt = (synth.apply_pose(src, T) + rng.normal(0, 0.02, (m, 3))).astype(np.float32)
        bad = rng.random(m) > frac
        tgt[bad] = rng.uniform(-1.2, 1.2, (int(bad.sum()), 3)).astype(np.float32)
        Te, inl, rmse, iters = oracle_native.ransac(src, tgt, max_corr, 10, max_iter, 0.999, 3)

        S, Q = src.astype(np.float64), tgt.astype(np.float64)
        thr2 = max_corr * max_corr
        best = (0, np.inf, None, -1)
        est_k, itr, n_diff32 = max_iter, 0, 0
        while itr < max_iter and itr < est_k:
            idx = oracle_native.rng_indices(3, itr, 10, m)
            ps, pt = S[idx], Q[idx]
            cs, ct = ps.mean(0), pt.mean(0)
            U, _, Vt = np.linalg.svd((pt - ct).T @ (ps - cs))
            D = np.diag([1, 1, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
            R = U @ D @ Vt
            t = ct - R @ cs
            d2 = (((R @ S.T).T + t - Q) ** 2).sum(1)
            ok = d2 < thr2
            cnt = int(ok.sum())
            R32, t32 = R.astype(np.float32), t.astype(np.float32)
            d2_32 = (((src @ R32.T) + t32 - tgt) ** 2).sum(1, dtype=np.float32)
            n_diff32 += int(((d2_32 < np.float32(max_corr) ** 2) != ok).sum())
            err = float(d2[ok].sum())
            if cnt > best[0] or (cnt == best[0] and cnt > 0 and err < best[1]):
                best = (cnt, err, np.concatenate([R, t[:, None]], 1), itr)
                ratio = min(1.0, cnt / m)
                den = np.log(1.0 - ratio ** 10) if ratio < 1 else -np.inf
                if den < 0:
                    k = np.log(1 - 0.999) / den
                    if k < est_k:
                        est_k = int(np.ceil(k))
            itr += 1
        assert inl == best[0] and iters == itr, (trial, inl, best[0], iters, itr)
        assert np.abs(Te[:3, :4].astype(np.float64) - best[2]).max() < 1e-6
        assert rmse == pytest.approx(np.sqrt(best[1] / best[0]), rel=1e-9)
        print("trial", trial, "iterations", itr, "(hypothesis, pair) decisions an f32 evaluation flips:", n_diff32)


def test_symmetric_cut_on_four_legged_object(oracle_native):
    """Part cut on a synthetic 4-fold object whose features encode the height: the 50 feature-NN of
    a leg anchor are the four leg tips -> K=4 k-means finds the four legs, the gate accepts, the
    centres come out in cyclic order [0, nearest, farthest, middle] (utils/symmetry.py:244-257)."""
    from oracle import post

    rng = np.random.default_rng(6)
    legs = np.array([[0.3, 0, 0.3], [-0.3, 0, 0.3], [-0.3, 0, -0.3], [0.3, 0, -0.3]])
    pts, feat = [], []
    for l in legs:
        n = 300
        h = rng.uniform(-0.5, 0.5, n)
        p = l + np.stack([rng.normal(0, 0.01, n), h, rng.normal(0, 0.01, n)], 1)
        pts.append(p)
        f = np.zeros((n, 16))
        f[:, 0] = h
        f[:, 1] = rng.normal(0, 1e-3, n)
        feat.append(f)
    xyz = np.concatenate(pts).astype(np.float32)
    F = np.concatenate(feat).astype(np.float32)
    perm = rng.permutation(len(xyz))
    xyz, F = xyz[perm], F[perm]
    anchors = post.draw_anchors(len(xyz), 100, 77, 0)
    labels = post.symmetric_cut4(F, xyz, 4, anchors)
    # every part is one leg
    leg_of = np.argmin(np.linalg.norm(xyz[:, None, :] - legs[None], axis=2), axis=1)
    for p in range(4):
        assert len(np.unique(leg_of[labels == p])) == 1
    centres = np.stack([xyz[labels == p].mean(0) for p in range(4)])
    d = np.linalg.norm(centres[0] - centres[1:], axis=1)
    assert d[1] > d[0] and d[1] > d[2]  # part 2 is the diagonal (farthest) leg
    # K = 2 on the same object also passes the gate here (two groups of two legs)? not guaranteed;
    # a degenerate cloud must fail like the reference (exception -> sym failed)
    with pytest.raises(AttributeError):
        post.symmetric_cut4(F[:150] * 0, xyz[:150] * 0, 4, post.draw_anchors(150, 100, 77, 1))
    with pytest.raises(ValueError):
        post.draw_anchors(50, 100, 77, 2)


def test_sym_pose_host_logic_part_configs():
    from corsair_amd import registration as R

    assert R.part_configs(2, 1) == [[0, 1], [1, 0]]
    c = R.part_configs(4, 2)
    assert len(c) == 8 and c[0] == [0, 1, 2, 3] and c[1] == [1, 2, 3, 0]
    assert c[4] == [0, 3, 2, 1] and c[5] == [3, 2, 1, 0]
    # gate: matches the oracle's on random statistics
    from oracle import post

    rng = np.random.default_rng(8)
    centers = rng.uniform(-1, 1, (30, 4, 3))
    counts = rng.integers(1, 100, (30, 4)).astype(np.int32)
    mcd = rng.uniform(0.05, 0.4, 30)
    mer = rng.uniform(0.05, 0.3, 30)
    for K in (2, 4):
        n = int(counts[:, :K].sum(1).max())
        got = R.gate_and_order(centers, counts, mcd, mer, n, K)
        want = post.gate_and_order(centers, counts, mcd, mer, n, K)
        assert np.array_equal(got[:K], want)
    assert R.gate_and_order(centers, counts, mcd * 0, mer, 100, 4) is None
    # the batched gate is the per-pair gate applied to every candidate pair (bit for bit)
    P = 9
    C = rng.uniform(-1, 1, (P, 30, 4, 3))
    N = rng.integers(1, 100, (P, 30, 4)).astype(np.int32)
    MCD = rng.uniform(0.05, 0.4, (P, 30))
    MER = rng.uniform(0.05, 0.3, (P, 30))
    MCD[4] = 0.0                                     # pair 4: no anchor passes
    Ks = [2, 4, 4, 2, 4, 2, 4, 4, 2]
    n = [int(N[p].sum(1).max()) for p in range(P)]
    cand = [0, 1, 2, 4, 5, 6, 8]
    for gate in (R.GATE_REFERENCE, R.GATE_ANY, (0.1, 0.3)):
        sel, ok = R.gate_and_order_batch(C, N, MCD, MER, n, Ks, cand, gate)
        for p in range(P):
            one = R.gate_and_order(C[p], N[p], MCD[p], MER[p], n[p], Ks[p], gate) if p in cand else None
            assert ok[p] == (one is not None)
            if one is not None:
                assert np.array_equal(sel[p], one)
            else:
                assert not sel[p].any()
    assert R.draw_anchors(50, 100, 0) is None
    a = R.draw_anchors(500, 100, 3)
    assert len(np.unique(a)) == 100 and np.array_equal(a, R.draw_anchors(500, 100, 3))


def test_instance_norm_oracle_matches_plain_definition():
    """oracle.sparse.instance_norm (chunked f64 sums, f32 roundings) against the textbook formula in f64."""
    from oracle import sparse

    rng = np.random.default_rng(3)
    seg = [0, 700, 700, 1213, 1214]                 # ragged, one empty sample, one single-row sample
    x = (rng.normal(size=(seg[-1], 24)) * rng.uniform(0.1, 5, 24) + rng.normal(size=24)).astype(np.float32)
    w = rng.normal(size=(1, 24)).astype(np.float32)
    b = rng.normal(size=(1, 24)).astype(np.float32)
    got = sparse.instance_norm(x, seg, w, b)
    for i in range(len(seg) - 1):
        xs = x[seg[i]:seg[i + 1]].astype(np.float64)
        if len(xs) == 0:
            continue
        want = (xs - xs.mean(0)) / np.sqrt(xs.var(0) + 1e-8) * w.astype(np.float64) + b.astype(np.float64)
        assert np.allclose(got[seg[i]:seg[i + 1]], want, rtol=2e-5, atol=2e-5)
    # no affine part
    assert np.allclose(sparse.instance_norm(x, seg)[:700].mean(0), 0, atol=1e-5)


def test_checkpoint_round_trip(tmp_path):
    """utils/ckpts.py:21-63 format: save_checkpoint -> load_checkpoint / load_state_dicts."""
    import torch

    from corsair_amd.utils import ckpts

    model, head = torch.nn.Linear(3, 2), torch.nn.Linear(2, 2)
    opt = torch.optim.SGD(list(model.parameters()) + list(head.parameters()), lr=0.1)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.9)
    ckpts.save_checkpoint(model, head, opt, sched, 7, str(tmp_path / "out"), "ckpt.pth")
    path = str(tmp_path / "out" / "ckpt.pth")
    raw = torch.load(path, weights_only=False)
    assert set(raw) == {"state_dict", "embedding_state_dict", "optimizer", "scheduler", "epoch"}
    m2, h2 = torch.nn.Linear(3, 2), torch.nn.Linear(2, 2)
    o2 = torch.optim.SGD(list(m2.parameters()) + list(h2.parameters()), lr=0.5)
    s2 = torch.optim.lr_scheduler.ExponentialLR(o2, 0.9)
    _, _, _, epoch = ckpts.load_checkpoint(m2, h2, o2, s2, path)
    assert epoch == 7 and torch.equal(m2.weight, model.weight) and torch.equal(h2.bias, head.bias)
    sd, esd = ckpts.load_state_dicts(path)
    assert set(sd) == {"weight", "bias"} and esd is not None
    ckpts.save_checkpoint(model, None, opt, sched, 8, str(tmp_path / "out"), "net_only.pth")
    assert "embedding_state_dict" not in torch.load(str(tmp_path / "out" / "net_only.pth"), weights_only=False)


def test_tiling_mask_bit_order_is_centre_faces_edges_corners():
    """kernelmap.hip's KORDER (bit j of a row's tiling mask = kernel offset KORDER[j]): the 27 offsets k = (dx+1) + 3 (dy+1) +
    9 (dz+1) sorted by |d|_1 (centre, six faces, twelve edges, eight corners), then by k -- a permutation, and the table
    tools/exec_ratio_cpu.py evaluates is the same one."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "corsair_amd", "csrc", "kernelmap.hip")).read()
    body = re.search(r"KORDER\[32\]\s*=\s*\{([^}]*)\}", src).group(1)
    table = [int(v) for v in body.split(",")]
    assert len(table) == 32 and table[27:] == [0] * 5
    offs = [(k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1) for k in range(27)]
    want = sorted(range(27), key=lambda k: (sum(abs(v) for v in offs[k]), k))
    assert table[:27] == want and sorted(want) == list(range(27))
    assert want[0] == 13 and [sum(abs(v) for v in offs[k]) for k in want] == [0] + [1] * 6 + [2] * 12 + [3] * 8
