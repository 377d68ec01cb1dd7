"""The symmetry part cut (csrc/symcut.hip) off its default path, bit-exact against the oracle on the inputs of
tests/symcut_cases.py: every accepted (dim, n_nn, n_init, max_iter), the Lloyd branches ordinary clouds never take
(tests/test_symcut_cpu.py states on the oracle's branch census that these inputs take them), the packing of (cloud,
anchor) pairs into k-means workgroups, a batch of very different clouds, selection ties laid out against the wave
quarters, cs_symcut_labels, and the drop-in modules corsair_amd.utils.{symmetry, find_nn, eval_pose} on top."""
import numpy as np
import pytest
import torch

from tests import symcut_cases as C
from tests.helpers import legged_object, rot_y_pose

pytestmark = pytest.mark.gpu

DEFAULT = (50, 10, 300)
CONFIGS = [DEFAULT, (64, 10, 300), (4, 10, 300), (7, 3, 300), (50, 1, 300), (50, 7, 300), (50, 10, 1), (50, 10, 2),
           (50, 10, 3)]
NAMES = ("centres", "counts", "min centre distance", "max error")


def _fit(gpu, f, x, off, anchors, Ks, cfg=DEFAULT):
    """B.symcut_fit on host arrays; anchors int32 [n_cloud, n_anchor].  Returns the four outputs as NumPy arrays."""
    from corsair_amd import backend as B

    out = B.symcut_fit(torch.from_numpy(f).to(gpu), torch.from_numpy(x).to(gpu), off,
                       torch.from_numpy(np.ascontiguousarray(anchors, dtype=np.int32)).to(gpu), Ks, *cfg)
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name)      # (+inf == +inf; no NaN is ever expected)
        assert not np.isnan(g).any(), (tag, name)


def _check_one_cloud(gpu, native, f, x, anchors, K, cfg=DEFAULT, tag=None):
    got = _fit(gpu, f, x, [0, len(x)], anchors[None], [K], cfg)
    want = native.symcut_fit(f, x, anchors, K, *cfg)
    _assert_same([g[0] for g in got], want, (tag, K, cfg))
    return want


# ---- 1. every accepted parameter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("dim", [16, 32])
def test_every_accepted_parameter(gpu, oracle_native, dim, K):
    f, x, a = C.uniform(dim=dim)
    for cfg in CONFIGS:
        _check_one_cloud(gpu, oracle_native, f, x, a, K, cfg, "uniform dim %d" % dim)


def test_refusals_leave_the_library_usable(gpu, oracle_native):
    from corsair_amd import _lib

    f, x, a = C.uniform()
    for bad in ((3, 10, 300), (65, 10, 300), (50, 0, 300), (50, 10, 0)):
        with pytest.raises(_lib.CorsairHipError):
            _fit(gpu, f, x, [0, len(x)], a[None], [4], bad)
        _check_one_cloud(gpu, oracle_native, f, x, a, 4, DEFAULT, ("after refusal", bad))
    with pytest.raises(_lib.CorsairHipError):
        _fit(gpu, np.ascontiguousarray(f[:, :8]), x, [0, len(x)], a[None], [4])
    _check_one_cloud(gpu, oracle_native, f, x, a, 2, DEFAULT, "after refusal of dim 8")


# ---- 2. Lloyd's rare branches -----------------------------------------------------------------------------------------------
RARE = [("three_positions", 2), ("three_positions", 4), ("identical", 2), ("identical", 4), ("blobs", 4),
        ("blobs_tight", 4), ("exactly_K", 2), ("exactly_K", 4)]


@pytest.mark.parametrize("name,K", RARE)
def test_lloyd_rare_branches(gpu, oracle_native, name, K):
    """Relocated empty clusters (three_positions K = 4, identical), the shift <= tol stop with the re-assignment before
    the inertia (those, blobs, exactly_K), and clusters without a member at the final assignment (identical)."""
    f, x, a = {"three_positions": C.three_positions, "identical": C.identical, "blobs": C.blobs,
               "blobs_tight": lambda: C.blobs(sd=3e-4), "exactly_K": lambda: C.exactly_K(K)}[name]()
    got = _fit(gpu, f, x, [0, len(x)], a[None], [K])
    _assert_same([g[0] for g in got], oracle_native.symcut_fit(f, x, a, K), (name, K))
    cen, cnt, mcd, mer = (g[0] for g in got)
    assert np.isfinite(cen).all()
    if len(np.unique(x, axis=0)) < K:
        # what the caller relies on: two centres coincide, the reference's gate `dist.min() > 0.15` refuses the model
        assert (mcd == 0.0).all() and (cnt.sum(1) == len(x)).all()
    if name == "identical":
        assert np.isposinf(mer).all() and (cnt[:, 0] == len(x)).all()
    if name == "exactly_K":
        assert (np.sort(cnt[:, :K], axis=1) == 1).all() and (mer == 0.0).all()


@pytest.mark.parametrize("cfg", [(50, 1, 300), (24, 1, 300), (64, 1, 300), DEFAULT])
def test_relocation_between_distinct_points(gpu, oracle_native, cfg):
    """The one input on which the relocation is visible in the outputs: an emptied cluster takes a point that is no
    duplicate of a centre (tests/symcut_cases.py ring_and_core; the census condition is in tests/test_symcut_cpu.py)."""
    f, x, a = C.ring_and_core()
    cen, cnt, mcd, mer = _check_one_cloud(gpu, oracle_native, f, x, a, 4, cfg, "ring_and_core")
    assert (cnt[0] > 0).all() and mcd[0] > 0.15 and np.isfinite(mer[0])


# ---- 3. workgroup packing ---------------------------------------------------------------------------------------------------
def _per(n_nn, n_init):
    """(cloud, anchor) pairs per k_symcut_kmeans workgroup: the host arithmetic of cs_symcut_fit (csrc/symcut.hip, "per"),
    restated: as many as the 256 lanes have restarts for and as fit into the 156 KiB of dynamic LDS next to the
    [n_nn][256] f64 table of closest distances, 64 x 3 f64 points each."""
    closest_bytes = 8 * 256 * n_nn
    per_fit = (156 * 1024 - closest_bytes) // (8 * 64 * 3)
    return max(1, min(256 // n_init, per_fit))


@pytest.mark.parametrize("n_nn,n_init", [(50, 1), (50, 7), (50, 10), (64, 10)])
def test_workgroup_packing(gpu, oracle_native, n_nn, n_init):
    """1, per, per + 1 and 2 per + 3 anchors of one cloud: a single pair, a full workgroup, a second workgroup with one
    pair, a third that is partial.  Every result is the oracle's and the one the anchor gets when it runs alone."""
    per = _per(n_nn, n_init)
    assert per == {(50, 1): 37, (50, 7): 36, (50, 10): 25, (64, 10): 18}[(n_nn, n_init)]
    f, x, _ = C.uniform(n=300)
    cfg = (n_nn, n_init, 300)
    anchors = np.random.default_rng(per).integers(0, 300, 2 * per + 3).astype(np.int32)
    want = oracle_native.symcut_fit(f, x, anchors, 4, *cfg)
    alone = [_fit(gpu, f, x, [0, 300], anchors[i:i + 1][None], [4], cfg) for i in range(len(anchors))]
    alone = [np.concatenate([r[k][0] for r in alone]) for k in range(4)]
    _assert_same(alone, want, ("alone", cfg))
    for na in (1, per, per + 1, 2 * per + 3):
        got = _fit(gpu, f, x, [0, 300], anchors[:na][None], [4], cfg)
        _assert_same([g[0] for g in got], [w[:na] for w in want], (na, cfg))
        _assert_same([g[0] for g in got], [w[:na] for w in alone], ("vs alone", na, cfg))


# ---- 4. mixed batch -----------------------------------------------------------------------------------------------------------
def test_mixed_batch_overwrites_every_output(gpu, oracle_native):
    """Clouds of 0, 3, 4, 37, 300 and 8193 rows with K = 4, 4, 4, 2, 4, 2 and 130 anchors each (two chunks of
    k_symcut_keys' anchor loop) in ONE call, through the C ABI on sentinel-filled outputs."""
    from corsair_amd import _lib
    from corsair_amd._lib import i32_array, i64_array, ptr, stream_ptr

    sizes, Ks, na = [0, 3, 4, 37, 300, 8193], [4, 4, 4, 2, 4, 2], 130
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    rng = np.random.default_rng(41)
    clouds = [C.uniform(n=n, n_anchor=0, seed=40 + i)[:2] for i, n in enumerate(sizes)]
    # the anchors of the empty cloud are never read: any value does, 0 is what a caller would pass
    anchors = np.stack([rng.integers(0, n, na) if n else np.zeros(na, np.int64) for n in sizes]).astype(np.int32)
    F = torch.from_numpy(np.concatenate([c[0] for c in clouds])).to(gpu)
    X = torch.from_numpy(np.concatenate([c[1] for c in clouds])).to(gpu)
    A = torch.from_numpy(anchors).to(gpu)
    nc = len(sizes)
    sent32, sent64 = 0x7FC5A5A5, (0x7FC5A5A5 << 32) | 0x7FC5A5A5
    cen = torch.full((nc, na, 4, 3), sent64, dtype=torch.int64, device=gpu).view(torch.float64)
    cnt = torch.full((nc, na, 4), sent32, dtype=torch.int32, device=gpu)
    mcd = torch.full((nc, na), sent64, dtype=torch.int64, device=gpu).view(torch.float64)
    mer = torch.full((nc, na), sent64, dtype=torch.int64, device=gpu).view(torch.float64)
    _lib.check(_lib.load().cs_symcut_fit(ptr(F), 16, ptr(X), i64_array(off), nc, ptr(A), na, i32_array(Ks), 50, 10, 300,
                                         ptr(cen), ptr(cnt), ptr(mcd), ptr(mer), stream_ptr()))
    torch.cuda.synchronize()
    for t in (cen, mcd, mer):
        assert not (t.view(torch.int64) == sent64).any()
    assert not (cnt == sent32).any()
    got = [t.cpu().numpy() for t in (cen, cnt, mcd, mer)]
    for c in (0, 1):                                     # fewer rows than K: a model the gate always rejects
        assert not got[0][c].any() and not got[1][c].any()
        assert (got[2][c] == 0.0).all() and np.isposinf(got[3][c]).all()
        assert not np.signbit(got[0][c]).any() and not np.signbit(got[2][c]).any()
    for c in range(nc):
        want = oracle_native.symcut_fit(clouds[c][0], clouds[c][1], anchors[c], Ks[c])
        _assert_same([g[c] for g in got], want, ("cloud", c, sizes[c]))
    # and the same clouds one per call
    for c in (2, 3, 5):
        _check_one_cloud(gpu, oracle_native, clouds[c][0], clouds[c][1], anchors[c], Ks[c], DEFAULT, ("single", c))


# ---- 5. selection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["q2", "q1"])
@pytest.mark.parametrize("n_nn", [50, 20])
@pytest.mark.parametrize("n", [256, 8193])
def test_selection_tie_blocks(gpu, oracle_native, n, n_nn, variant):
    """Ties at the selection threshold across the wave quarters of the ordered compaction, keys in registers (n = 256)
    and re-read from memory (n = 8193): the block straddles quarters 0 | 1, continues in 2, and the budget of ties is
    spent in quarter 2 ("q2") or 1 ("q1") -- the later quarters hold ties that must not be taken.  One wrong row moves
    a centre.  (tests/test_symcut_cpu.py checks that the oracle selects the rows the builder intends.)"""
    t = C.tie_blocks(n, n_nn, variant)
    _check_one_cloud(gpu, oracle_native, t.feat, t.xyz, t.anchors, 4, (n_nn, 10, 300), ("tie_blocks", n, variant))


def test_selection_wide_keys(gpu, oracle_native):
    f, x, a = C.wide_keys()
    for K in (2, 4):
        _check_one_cloud(gpu, oracle_native, f, x, a, K, DEFAULT, "wide_keys")


# ---- 6. labels --------------------------------------------------------------------------------------------------------------------
def _labels(gpu, x, off, Ks, centres):
    from corsair_amd import backend as B

    return B.symcut_labels(torch.from_numpy(x).to(gpu), off, Ks, torch.from_numpy(centres).to(gpu)).cpu().numpy()


def test_labels_batch_and_ignored_centre_rows(gpu, oracle_native):
    sizes, Ks = [300, 0, 37, 2048], [4, 2, 2, 4]
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    rng = np.random.default_rng(61)
    x = rng.uniform(-0.5, 0.5, (off[-1], 3)).astype(np.float32)
    cen = rng.uniform(-0.5, 0.5, (4, 4, 3))
    cen[3, 2] = cen[3, 0]                                      # duplicated centres: the smaller index wins
    cen[3, 3] = cen[3, 1]
    want = np.concatenate([oracle_native.symcut_labels(x[off[c]:off[c + 1]], Ks[c], cen[c, :Ks[c]]) for c in range(4)])
    lab = _labels(gpu, x, off, Ks, cen)
    assert lab.dtype == np.int32 and np.array_equal(lab, want)
    assert set(np.unique(lab[off[3]:])) == {0, 1} and set(np.unique(lab[:300])) == {0, 1, 2, 3}
    # rows >= K of the centres are ignored: NaN, or a point nearer to every voxel than centres 0 and 1
    for filler in (np.nan, 0.0):
        c2 = cen.copy()
        c2[2, :2] = [[10.0, 0.0, 0.0], [-10.0, 0.5, 0.0]]
        base = _labels(gpu, x, off, Ks, c2)
        c2[1, 2:] = filler
        c2[2, 2:] = filler
        got = _labels(gpu, x, off, Ks, c2)
        assert np.array_equal(got, base) and set(np.unique(got[off[2]:off[3]])) == {0, 1}
        assert np.array_equal(got[off[2]:off[3]], oracle_native.symcut_labels(x[off[2]:off[3]], 2, c2[2, :2]))


def test_labels_equidistant_points_take_the_smaller_index(gpu, oracle_native):
    rng = np.random.default_rng(62)
    x = rng.uniform(-0.5, 0.5, (500, 3)).astype(np.float32)
    x[::2, 0] = 0.0                                            # every other point is exactly between the centres
    for K, cen in ((2, [[1, 0, 0], [-1, 0, 0], [0, 0, 0], [0, 0, 0]]), (2, [[-1, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]]),
                   (4, [[5, 5, 5], [1, 0, 0], [5, 5, 5], [-1, 0, 0]])):
        cen = np.asarray(cen, np.float64)[None]
        lab = _labels(gpu, x, [0, 500], [K], cen)
        assert np.array_equal(lab, oracle_native.symcut_labels(x, K, cen[0, :K]))
        assert (lab[::2] == (0 if K == 2 else 1)).all() and len(np.unique(lab[1::2])) == 2


def test_counts_are_the_histogram_of_the_labels(gpu, oracle_native):
    """Cross-check between kernels: the counts of k_symcut_finish are the histogram of k_symcut_labels under the same centres."""
    for dim, K, cfg in ((16, 4, DEFAULT), (32, 2, (7, 3, 300)), (16, 4, (50, 10, 1))):
        f, x, a = C.uniform(dim=dim)
        cen, cnt, _, _ = (g[0] for g in _fit(gpu, f, x, [0, len(x)], a[None], [K], cfg))
        for i in (0, 5, 23):
            lab = _labels(gpu, x, [0, len(x)], [K], np.ascontiguousarray(cen[i][None]))
            assert np.array_equal(np.bincount(lab, minlength=4), cnt[i]), (dim, K, cfg, i)


# ---- 7. drop-in layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,seed", [(4, 10), (2, 29)])
def test_symmetric_cut4_matches_oracle(gpu, oracle_native, K, seed):
    from corsair_amd import registration as R
    from corsair_amd.utils.symmetry import symmetric_cut4
    from oracle import post

    xyz, F = legged_object(seed, K)
    for counter in (0, 3):
        masks = symmetric_cut4(F, xyz, K, 100, counter)
        assert len(masks) == K and all(m.dtype == np.bool_ and m.shape == (len(xyz),) for m in masks)
        want = post.symmetric_cut4(F, xyz, K, R.draw_anchors(len(xyz), 100, counter))
        for i in range(K):
            assert np.array_equal(masks[i], want == i), (K, counter, i)
        assert np.array_equal(np.sum(masks, axis=0), np.ones(len(xyz), int))      # a partition
        assert min(m.sum() for m in masks) > 0.2 * len(xyz) / K                     # the legs, not slivers
    # torch inputs are accepted like NumPy ones
    again = symmetric_cut4(torch.from_numpy(F), torch.from_numpy(xyz).to(gpu), K, 100, 3)
    assert all(np.array_equal(u, v) for u, v in zip(again, masks))


def test_symmetric_cut4_exceptions(gpu, oracle_native):
    """The two exceptions sym_pose catches in the reference: fewer voxels than anchors, and no anchor through the gate."""
    from corsair_amd.utils.symmetry import symmetric_cut4

    f, x, _ = C.uniform()
    with pytest.raises(ValueError):
        symmetric_cut4(f[:99], x[:99], 4, 100, 0)
    with pytest.raises(AttributeError):
        symmetric_cut4(f, x, 4, 100, 0)
    with pytest.raises(AttributeError):
        symmetric_cut4(f, x, 2, 100, 0)


def test_split_corr_gathers_per_part(gpu, oracle_native):
    from corsair_amd.utils.eval_pose import find_kcorr
    from corsair_amd.utils.symmetry import split_corr, symmetric_cut4
    from oracle import post

    xa, Fa = legged_object(10, 4)
    xb, Fb = legged_object(110, 4)
    ma, mb = symmetric_cut4(Fa, xa, 4, 100, 0), symmetric_cut4(Fb, xb, 4, 100, 1)
    empty = np.zeros(len(xa), bool)
    pa = [xa[m] for m in ma[:2]] + [xa[empty]] + [xa[m] for m in ma[2:]]
    fa = [Fa[m] for m in ma[:2]] + [Fa[empty]] + [Fa[m] for m in ma[2:]]
    pb = [xb[m] for m in mb[:2]] + [xb[mb[0]]] + [xb[m] for m in mb[2:]]
    fb = [Fb[m] for m in mb[:2]] + [Fb[mb[0]]] + [Fb[m] for m in mb[2:]]
    got_a, got_b = split_corr(pa, pb, fa, fb, 5)
    want_a, want_b = [], []
    for i in (0, 1, 3, 4):                               # part 2 is empty and skipped
        i0, i1 = find_kcorr(fa[i], fb[i], k=5)
        o0, o1 = post.find_kcorr(fa[i], fb[i], k=5)
        assert np.array_equal(i0, o0) and np.array_equal(i1, o1)
        want_a.append(pa[i][i0])
        want_b.append(pb[i][i1])
    assert np.array_equal(got_a, np.concatenate(want_a)) and np.array_equal(got_b, np.concatenate(want_b))
    assert got_a.shape == (5 * len(xa), 3) and got_a.dtype == np.float32


def test_sym_pose_single_pair(gpu, oracle_native):
    from corsair_amd import registration as R
    from corsair_amd.utils.symmetry import sym_pose

    x1, F1 = legged_object(10, 4)
    xq, Fq = legged_object(110, 4)
    T0 = rot_y_pose(100.0)
    xq = (xq.astype(np.float64) @ T0[:3, :3].T + T0[:3, 3]).astype(np.float32)
    max_iter = 5000
    Tb, cdb, Tr, cdr, ok = sym_pose(Fq, xq, F1, x1, 4, 5, 0.2, 0, (20, 21), max_iter, 0.999)
    dev = lambda a: torch.from_numpy(a).to(gpu)
    res = R.sym_pose_batch(dev(Fq), dev(xq), [0, len(xq)], dev(F1), dev(x1), [0, len(x1)], [4], 5, 0.2, 0, [(20, 21)],
                           100, max_iter, 0.999)
    for T in (Tb, Tr):
        assert isinstance(T, torch.Tensor) and T.dtype == torch.float32 and T.shape == (4, 4) and not T.is_cuda
    assert type(cdb) is float and type(cdr) is float and type(ok) is bool
    assert torch.equal(Tb, res.T_best[0].cpu()) and torch.equal(Tr, res.T_ransac[0].cpu())
    assert cdb == float(res.cd_best[0]) and cdr == float(res.cd_ransac[0]) and ok == bool(res.ok[0])
    assert ok and cdb < cdr                               # the gate opened and a symmetric hypothesis won


def test_find_nn_wrappers(gpu, oracle_native):
    from corsair_amd import backend as B
    from corsair_amd.utils.find_nn import find_knn, find_knn_cpu, find_nn_cpu

    f0, _, _ = C.uniform(n=333, seed=71)
    f1, _, _ = C.uniform(n=600, seed=72)
    idx, dist = B.knn_feat(torch.from_numpy(f0).to(gpu), [0, 333], torch.from_numpy(f1).to(gpu), [0, 600], 5,
                           return_distance=True)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(idx, oracle_native.knn(f0, f1, 5))
    for fn in (find_knn, find_knn_cpu):
        got = fn(f0, f1, 5)
        assert got.dtype == np.int64 and got.shape == (333, 5) and np.array_equal(got, idx)
        gi, gd = fn(torch.from_numpy(f0), f1, 5, return_distance=True)
        assert gi.dtype == np.int64 and np.array_equal(gi, idx)
        assert gd.dtype == np.float64 and np.array_equal(gd, dist)
    one = find_nn_cpu(f0, f1)
    assert one.dtype == np.int64 and one.shape == (333,) and np.array_equal(one, idx[:, 0])
    oi, od = find_nn_cpu(f0, f1, return_distance=True)
    assert oi.shape == od.shape == (333,) and np.array_equal(oi, idx[:, 0]) and np.array_equal(od, dist[:, 0])


def test_registration_based_on_corr(gpu, oracle_native):
    from corsair_amd import backend as B
    from corsair_amd.utils.eval_pose import registration_based_on_corr

    rng = np.random.default_rng(81)
    tgt = rng.uniform(-0.5, 0.5, (400, 3)).astype(np.float32)
    T0 = rot_y_pose(35.0)
    src = ((tgt.astype(np.float64) - T0[:3, 3]) @ T0[:3, :3]).astype(np.float32)      # tgt = R src + t
    src[::3] = rng.uniform(-0.5, 0.5, (len(src[::3]), 3)).astype(np.float32)         # a third are outliers
    T = registration_based_on_corr(src, tgt, 0.05, 3, 4000, 0.999)
    assert T.dtype == np.float64 and T.shape == (4, 4)
    want = B.ransac_batch(torch.from_numpy(src).to(gpu), torch.from_numpy(tgt).to(gpu), [0, 400], 0.05, 10, 4000, 0.999, 3)
    assert np.array_equal(T, want[0][0].cpu().numpy().astype(np.float64))
    assert np.array_equal(T.astype(np.float32), oracle_native.ransac(src, tgt, 0.05, 10, 4000, 0.999, 3)[0])
    assert np.abs(T - T0).max() < 1e-3
