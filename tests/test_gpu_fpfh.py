"""cs_fpfh, cs_orient_normals and the 33-d cs_knn_feat on the GPU: every descriptor is BIT-EQUAL to tests/fpfh_ref.py on the
cell-grid path (segments of more than 512 rows) and on the exhaustive path (smaller segments, and everything under
CS_FPFH_GRID=0); then the descriptors register real clouds without a checkpoint."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fpfh_ref as FR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_MIN = 513     # the smallest segment that takes the grid path (FP_GRID_MIN, fpfh.hip)
LIST_CAP = 256     # entries of the on-chip list (FP_CAP); a ball of more than 192 candidates is ranked in parts


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _assert_bits(got, want, what=""):
    assert got.shape == want.shape
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(1))[0]
    assert not len(bad), (what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]])


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _run(dev, xyz, nrm, off, radius, max_nn):
    from corsair_amd import backend as B

    return B.fpfh(_t(dev, xyz).reshape(-1, 3), off, _t(dev, nrm).reshape(-1, 3), radius, max_nn).cpu().numpy()


def _sphere(n, seed=3, radius=0.5):
    rng = np.random.default_rng(seed)
    sph = rng.standard_normal((n, 3))
    return (radius * sph / np.linalg.norm(sph, axis=1, keepdims=True)).astype(np.float32)


def _rough_normals(pc, seed):
    """unit vectors near the radial direction: any oriented normals serve a bit-for-bit comparison"""
    rng = np.random.default_rng(seed)
    n = pc.astype(np.float64) - pc.astype(np.float64).mean(0) + 0.2 * rng.standard_normal(pc.shape)
    return (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-9)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _mixed():
    """0, 1, 3, 300 (exhaustive path), 700 and 1500 rows (grid path) of one cloud in one call, an empty segment at the end"""
    from corsair_amd import synth

    rng = np.random.default_rng(21)
    cloud = synth.make_cloud(9, 6000)
    sizes = [0, 1, 3, 300, 700, 1500, 0]
    xyz = np.concatenate([cloud[rng.choice(len(cloud), n, replace=False)] for n in sizes]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    nrm = _rough_normals(xyz, 22)
    return xyz, nrm, off, FR.fpfh(xyz, nrm, off, 0.15, 100)


def test_mixed_segments_match_reference(gpu):
    xyz, nrm, off, want = _mixed()
    got = _run(gpu, xyz, nrm, off, 0.15, 100)
    _assert_bits(got, want)
    m = np.asarray([len(FR.neighbours(xyz[off[5]:off[6]], i, 0.15, 100)) for i in range(0, 1500, 50)])
    print("1500-row segment: neighbours per row min / mean / max: %d / %.1f / %d" % (m.min(), m.mean(), m.max()))
    assert (got[off[1]] == 0).all()                               # the single row: no neighbour
    assert _bits_equal(_run(gpu, xyz, nrm, off, 0.15, 100), got)   # two runs: identical bits
    # a row's descriptor depends on its segment alone
    for s in (3, 4):
        a, b = off[s], off[s + 1]
        assert _bits_equal(_run(gpu, xyz[a:b], nrm[a:b], [0, b - a], 0.15, 100), want[a:b]), s


@functools.lru_cache(maxsize=None)
def _ball():
    """about 40 rows inside the radius of every row, below and above the grid threshold"""
    a, b = _sphere(400, 5), _sphere(900, 6, 0.75)
    xyz = np.concatenate([a, b])
    return xyz, _rough_normals(xyz, 7), [0, 400, 1300]


@pytest.mark.parametrize("max_nn", (4, 16))
def test_truncation(gpu, max_nn):
    xyz, nrm, off = _ball()
    inside = np.asarray([len(FR.neighbours(xyz[:400], i, 0.32, 128)) for i in range(0, 400, 40)])
    assert 25 <= inside.mean() <= 60, inside
    _assert_bits(_run(gpu, xyz, nrm, off, 0.32, max_nn), FR.fpfh(xyz, nrm, off, 0.32, max_nn), max_nn)


def _lattice(nx, ny, nz):
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ties_case():
    """integer lattices (ties at every distance, rows at distance exactly the radius) and duplicated rows (d2 = 0), below
    and above the grid threshold"""
    rng = np.random.default_rng(6)
    cont = rng.uniform(-1, 1, (90, 3)).astype(np.float32)
    dup = np.concatenate([cont, cont[:40], cont[10:30]])
    cont2 = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    dup2 = np.concatenate([cont2, cont2[:200], cont2[100:250]])
    parts = [_lattice(7, 6, 5), dup, _lattice(9, 8, 8), dup2]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    return xyz, _rough_normals(xyz, 8), off


@pytest.mark.parametrize("max_nn", (8, 33, 128))
def test_integer_lattice_and_duplicated_rows(gpu, max_nn):
    xyz, nrm, off = _ties_case()
    assert off[3] - off[2] >= GRID_MIN and off[4] - off[3] >= GRID_MIN and off[1] < GRID_MIN
    # radius 2.0: the lattice rows at distance exactly 2 are outside (26 others inside for an inner row, ties at 1, 2, 3)
    centre = int(np.nonzero((xyz[off[2]:off[3]] == (4, 4, 4)).all(1))[0][0])
    assert len(FR.neighbours(xyz[off[2]:off[3]], centre, 2.0, 128)) == 26
    _assert_bits(_run(gpu, xyz, nrm, off, 2.0, max_nn), FR.fpfh(xyz, nrm, off, 2.0, max_nn), max_nn)


def test_nonfinite_rows_normals_and_far_coordinates(gpu):
    sph = _sphere(600)
    nan = sph.copy()
    nan[17, 1] = np.nan
    nan[40, 0] = np.inf
    nan[599, 2] = -np.inf
    far = sph + np.float32([70.0, -70.0, 0.0])                      # a coordinate of 70
    flat = (0.2 * sph).astype(np.float32)                           # one coordinate of 10^6: its cell index clamps
    flat[:, 0] = 1.0e6
    small = sph[:80].copy()
    small[5, 0] = np.nan
    small[9, 2] = np.inf
    parts = [nan, far, small]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    nrm = _rough_normals(np.nan_to_num(xyz, posinf=0.0, neginf=0.0), 9)
    nrm[100] = 0.0                                                  # a zero-length normal
    nrm[101] = (np.nan, 0.0, 1.0)                                   # NaN normals
    nrm[off[2] + 20] = np.nan
    got = _run(gpu, xyz, nrm, off, 0.15, 32)
    _assert_bits(got, FR.fpfh(xyz, nrm, off, 0.15, 32))
    for r in (17, 40, 599, off[2] + 5, off[2] + 9):
        assert (got[r] == 0).all(), r                               # a non-finite row has no neighbour
    assert np.isfinite(got).all()
    fn = _rough_normals(flat, 10)
    _assert_bits(_run(gpu, flat, fn, [0, 600], 0.02, 16), FR.fpfh(flat, fn, [0, 600], 0.02, 16))


def test_a_ball_larger_than_the_on_chip_list(gpu):
    from corsair_amd import backend as B

    rng = np.random.default_rng(11)
    parts = [rng.uniform(-0.5, 0.5, (450, 3)).astype(np.float32), rng.uniform(-0.5, 0.5, (800, 3)).astype(np.float32)]
    xyz = np.concatenate(parts)
    off = [0, 450, 1250]
    nrm = _rough_normals(xyz, 12)
    s64 = parts[1].astype(np.float64)
    mid = int(np.argmin(((s64 - s64.mean(0)) ** 2).sum(1)))
    assert len(FR.neighbours(parts[1], mid, 0.6, 128)) == 127
    assert (((s64 - s64[mid]) ** 2).sum(1) < 0.36).sum() > 2 * LIST_CAP         # more candidates than the list holds
    os.environ["CS_FPFH_STATS"] = "1"
    try:
        B.fpfh_stats(reset=True)
        got = _run(gpu, xyz, nrm, off, 0.6, 128)
        found, parted = B.fpfh_stats(reset=True)
    finally:
        del os.environ["CS_FPFH_STATS"]
    _assert_bits(got, FR.fpfh(xyz, nrm, off, 0.6, 128))
    assert parted > 100 and found > 127 * 600, (found, parted)
    _run(gpu, xyz, nrm, off, 0.6, 128)
    assert B.fpfh_stats() == (0, 0)                                              # counted only when asked


def test_permuting_a_tie_free_segment_permutes_the_descriptors(gpu):
    for n in (300, 700):
        sph = _sphere(n, 30 + n)
        d2 = ((sph[:, None, :].astype(np.float64) - sph[None, :, :]) ** 2).sum(-1)
        assert len(np.unique(d2[np.triu_indices(n, 1)])) == n * (n - 1) // 2          # no two distances tie
        nrm = _rough_normals(sph, 31)
        perm = np.random.default_rng(8).permutation(n)
        a = _run(gpu, sph, nrm, [0, n], 0.2, 48)
        b = _run(gpu, sph[perm], nrm[perm], [0, n], 0.2, 48)
        assert _bits_equal(b, a[perm]), n


def _run_switch_cases(dev):
    out = {}
    xyz, nrm, off, _ = _mixed()
    out["mixed"] = _run(dev, xyz, nrm, off, 0.15, 100)
    xyz, nrm, off = _ties_case()
    out["ties"] = _run(dev, xyz, nrm, off, 2.0, 33)
    return out


def test_switch_in_a_child_process(gpu, tmp_path):
    """CS_FPFH_GRID=0 in a process of its own: the exhaustive scan alone gives the bits of the restatement."""
    env = dict(os.environ)
    env["CS_FPFH_GRID"] = "0"
    path = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_fpfh", path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = dict(np.load(path))
    _assert_bits(res["mixed"], _mixed()[3])
    here = _run_switch_cases(gpu)
    for k in here:
        assert _bits_equal(res[k], here[k]), k


def test_refused_arguments_and_empty_calls(gpu):
    from corsair_amd import _lib, backend as B

    x = torch.zeros((10, 3), device=gpu)
    n = torch.zeros((10, 3), device=gpu)
    for k in (3, 129, 0, -1):
        with pytest.raises(_lib.CorsairHipError, match="max_nn outside"):
            B.fpfh(x, [0, 10], n, 0.1, k)
    for radius in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.CorsairHipError, match="radius must be positive and finite"):
            B.fpfh(x, [0, 10], n, radius, 8)
    with pytest.raises(ValueError):
        B.fpfh(x, [0, 11], n, 0.1, 8)
    with pytest.raises(ValueError):
        B.fpfh(x, [0, 10], n[:5], 0.1, 8)
    with pytest.raises(_lib.CorsairHipError, match="bad segment"):
        B.fpfh(x, [0, 7, 5], n, 0.1, 8)
    with pytest.raises(TypeError):
        B.fpfh(x.double(), [0, 10], n, 0.1, 8)
    lib = _lib.load()
    off = (ctypes.c_int64 * 2)(0, 10)
    out = torch.empty((10, 33), device=gpu)
    f = lib.cs_fpfh
    px, pn, po = _lib.ptr(x), _lib.ptr(n), _lib.ptr(out)
    assert f(px, pn, off, 1, 0.1, 8, po, None) == 0
    assert f(None, pn, off, 1, 0.1, 8, po, None) < 0
    assert f(px, None, off, 1, 0.1, 8, po, None) < 0
    assert f(px, pn, off, 1, 0.1, 8, None, None) < 0
    assert f(px, pn, None, 1, 0.1, 8, po, None) < 0
    assert f(px, pn, off, -1, 0.1, 8, po, None) < 0
    assert f(px, pn, off, 1, 0.0, 8, po, None) < 0
    assert f(px, pn, off, 1, float("inf"), 8, po, None) < 0
    assert f(px, pn, off, 1, 0.1, 129, po, None) < 0
    assert f(px, pn, (ctypes.c_int64 * 2)(0, 2 ** 31), 1, 0.1, 8, po, None) < 0
    assert B.fpfh(x[:0], [0], n[:0], 0.1, 8).shape == (0, 33)
    assert B.fpfh(x[:0], [0, 0, 0], n[:0], 0.1, 8).shape == (0, 33)
    torch.cuda.synchronize()


def test_profile_family_sees_one_scope_per_call(gpu):
    from corsair_amd import _lib

    xyz, nrm, off, _ = _mixed()                    # segments of both paths in one call
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        _run(gpu, xyz, nrm, off, 0.15, 100)
        torch.cuda.synchronize()
        ms, n, units = _lib.prof_get("fpfh")
    finally:
        _lib.prof_enable(False)
    assert n == 1 and ms > 0 and units > 0


# ---- cs_orient_normals ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _orient_case():
    rng = np.random.default_rng(40)
    sizes = [0, 1, 300, 700, 0]
    xyz = (rng.standard_normal((sum(sizes), 3)) * 2).astype(np.float32)
    nrm = rng.standard_normal(xyz.shape).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    xyz[5] = (np.nan, 0, 0)                          # left out of the centroid; its own s is NaN: kept
    xyz[6] = (1.0e6, 0, 0)                           # left out of the centroid (2^15 and above), oriented all the same
    nrm[7] = (np.nan, 1, 0)
    nrm[8] = 0.0                                     # s == 0: kept
    xyz[400] = (0.5, 0.25, -1.0)
    nrm[400] = (2.0, -4.0, 0.0)                      # with the view point (0.5, 0.25, 3): d = (0, 0, -4), s == 0 exactly
    return xyz, nrm, off


@pytest.mark.parametrize("away", (True, False))
@pytest.mark.parametrize("given", (False, True))
def test_orient_normals_matches_reference(gpu, away, given):
    from corsair_amd import backend as B

    xyz, nrm, off = _orient_case()
    view = np.asarray([[0, 0, 0], [1, 2, 3], [0.1, -0.2, 0.3], [0.5, 0.25, 3.0], [0, 0, 0]], np.float64) if given else None
    want = FR.orient_normals(xyz, off, nrm, view, away)
    got = B.orient_normals(_t(gpu, xyz), off, _t(gpu, nrm), view, away).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    flipped = (got.view(np.int32) != nrm.view(np.int32)).any(1)
    assert 100 < flipped.sum() < len(xyz) - 100
    for r in (5, 7, 8) + ((400,) if given else ()):
        assert not flipped[r], r
    if not given:
        # the other sense flips exactly the other rows (but those with s == 0 or NaN)
        other = FR.orient_normals(xyz, off, nrm, None, not away)
        assert not ((other.view(np.int32) != nrm.view(np.int32)).any(1) & flipped).any()


def test_orient_normals_permuted_segment_and_refusals(gpu):
    from corsair_amd import _lib, backend as B

    xyz, nrm, off = _orient_case()
    a, b = off[3], off[4]
    perm = np.random.default_rng(41).permutation(b - a)
    one = B.orient_normals(_t(gpu, xyz[a:b]), [0, b - a], _t(gpu, nrm[a:b])).cpu().numpy()
    two = B.orient_normals(_t(gpu, xyz[a:b][perm]), [0, b - a], _t(gpu, nrm[a:b][perm])).cpu().numpy()
    assert np.array_equal(two.view(np.int32), one[perm].view(np.int32))
    # a segment without a row that enters the centroid keeps its normals
    far = np.full((4, 3), 1.0e5, np.float32)
    keep = B.orient_normals(_t(gpu, far), [0, 4], _t(gpu, nrm[:4])).cpu().numpy()
    assert np.array_equal(keep.view(np.int32), nrm[:4].view(np.int32))
    x, n = torch.zeros((10, 3), device=gpu), torch.zeros((10, 3), device=gpu)
    with pytest.raises(ValueError):
        B.orient_normals(x, [0, 11], n)
    with pytest.raises(ValueError):
        B.orient_normals(x, [0, 10], n[:5])
    with pytest.raises(ValueError):
        B.orient_normals(x, [0, 10], n, view=np.zeros((2, 3)))
    with pytest.raises(_lib.CorsairHipError, match="bad segment"):
        B.orient_normals(x, [0, 7, 5], n)
    lib = _lib.load()
    off2 = (ctypes.c_int64 * 2)(0, 10)
    f = lib.cs_orient_normals
    px, pn = _lib.ptr(x), _lib.ptr(n)
    assert f(px, off2, 1, None, 1, pn, None) == 0
    assert f(None, off2, 1, None, 1, pn, None) < 0
    assert f(px, off2, 1, None, 1, None, None) < 0
    assert f(px, None, 1, None, 1, pn, None) < 0
    assert f(px, off2, -1, None, 1, pn, None) < 0
    assert f(px, off2, 1, None, 2, pn, None) < 0
    assert f(px, (ctypes.c_int64 * 2)(0, 2 ** 31), 1, None, 1, pn, None) < 0
    assert f(px, (ctypes.c_int64 * 1)(0), 0, None, 1, pn, None) == 0
    torch.cuda.synchronize()


# ---- cs_knn_feat at 33 columns -------------------------------------------------------------------------------------------
def _knn_replay(q, t, k):
    """indices and distances by the canonical chain d = fma(diff, diff, d) over the columns in ascending order"""
    from tests.fpfh_ref import exact_fma

    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    idx = np.full((len(q), k), -1, np.int32)
    dist = np.full((len(q), k), np.inf)
    with np.errstate(all="ignore"):
        approx = ((q64[:, None, :] - t64[None, :, :]) ** 2).sum(-1)
    for i in range(len(q)):
        a = np.where(np.isfinite(approx[i]), approx[i], np.inf)
        if not np.isfinite(a).any():
            continue
        lim = np.partition(a, min(k, len(a)) - 1)[min(k, len(a)) - 1]
        rows = []
        for j in np.nonzero(a <= lim * (1 + 1e-12))[0]:
            d = 0.0
            for c in range(q.shape[1]):
                diff = float(q64[i, c]) - float(t64[j, c])
                d = exact_fma(diff, diff, d)
            if np.isfinite(d):
                rows.append((d, int(j)))
        rows.sort()
        for s, (d, j) in enumerate(rows[:k]):
            idx[i, s], dist[i, s] = j, np.sqrt(d)
    return idx, dist


@functools.lru_cache(maxsize=None)
def _knn_case():
    rng = np.random.default_rng(50)
    q = rng.uniform(0, 100, (200, 33)).astype(np.float32)
    t = rng.uniform(0, 100, (300, 33)).astype(np.float32)
    t[150] = t[20]                                   # a duplicated target: a tie, the smaller row first
    q[3] = t[20]
    t[77, 5] = np.nan
    q[9, 0] = np.nan
    short = rng.uniform(0, 100, (4, 33)).astype(np.float32)     # a target segment shorter than k = 5 and 8
    return q, t, short


@pytest.mark.parametrize("k", (1, 5, 8))
def test_knn_feat_at_33_columns(gpu, k):
    from corsair_amd import backend as B

    q, t, short = _knn_case()
    qq = np.concatenate([q, q[:50]])
    tt = np.concatenate([t, short])
    idx, dist = B.knn_feat(_t(gpu, qq), [0, 200, 250], _t(gpu, tt), [0, 300, 304], k, return_distance=True)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    for (qa, qb), tseg in (((0, 200), t), ((200, 250), short)):
        wi, wd = _knn_replay(qq[qa:qb], tseg, k)
        assert np.array_equal(idx[qa:qb], wi)
        assert np.array_equal(dist[qa:qb].view(np.int64), wd.view(np.int64))
    assert (idx[9] == -1).all() and idx[3, 0] == 20 and (k == 1 or idx[3, 1] == 150)
    assert not (idx[:200] == 77).any()
    if k > 4:
        finite = np.arange(50) != 9                  # row 9 of the queries holds a NaN
        assert (idx[200:, 4:] == -1).all() and (idx[200:][finite, :4] >= 0).all()


def test_sym_pose_batch_refuses_the_part_cut_on_33_columns(gpu):
    from corsair_amd import _lib, registration as R

    F = torch.zeros((20, 33), device=gpu)
    x = torch.zeros((20, 3), device=gpu)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        with pytest.raises(ValueError, match="use_symmetry"):
            R.sym_pose_batch(F, x, [0, 20], F, x, [0, 20], [1], 5, 0.2, 0, None, 100, 1000, 0.999, True)
        assert _lib.prof_get("knn")[1] == 0          # before any launch
    finally:
        _lib.prof_enable(False)


# ---- end to end on real geometry -----------------------------------------------------------------------------------------
# RRE (degrees) and RTE of the CPU pipeline on clouds 0, 3 and 5 -- the float implementation of tests/test_fpfh_cpu.py
# (float normals over 16 neighbours, oriented away from the centroid; radius 5 voxels, max_nn 100), then the oracle's 5-NN
# and RANSAC at seed 0 -- measured once:
CPU_RRE_DEG = (6.06, 3.90, 4.89)
CPU_RTE = (0.0619, 0.0139, 0.0206)
RRE_BOUND_DEG = min(15.0, 2.0 * max(CPU_RRE_DEG))
RTE_BOUND = min(0.15, 2.0 * max(CPU_RTE))


@functools.lru_cache(maxsize=None)
def _real_pairs():
    from corsair_amd import backend as B, synth
    from tests.test_gpu_real_clouds import _real_clouds

    dev = torch.device("cuda:0")
    clouds = _real_clouds()
    voxel = 0.03
    cad_xyz, q_xyz, Ts = [], [], []
    for p, ci in enumerate([0, 3, 5]):
        full = clouds[ci]
        T = synth.random_pose(100 + p, max_trans=0.5)
        cad, q_cad_frame = full[:10000], full[5000:]
        c_keep, _, _ = B.voxelize(torch.from_numpy(cad).to(dev), [0, len(cad)], voxel)
        q_posed = synth.apply_pose(q_cad_frame, T)
        q_keep, _, _ = B.voxelize(torch.from_numpy(q_posed).to(dev), [0, len(q_posed)], voxel)
        cad_xyz.append(cad[c_keep.cpu().numpy()])
        q_xyz.append(q_posed[q_keep.cpu().numpy()])
        Ts.append(T)
    off0 = np.concatenate([[0], np.cumsum([len(x) for x in q_xyz])]).tolist()
    off1 = np.concatenate([[0], np.cumsum([len(x) for x in cad_xyz])]).tolist()
    return np.concatenate(q_xyz).astype(np.float32), off0, np.concatenate(cad_xyz).astype(np.float32), off1, Ts, voxel


def test_fpfh_registers_real_clouds_without_a_checkpoint(gpu):
    """Clouds 0, 3 and 5 of the real-cloud fixtures, split, posed and voxelised as test_pipeline_recovers_a_known_pose
    does; registration.fpfh_features at 5 voxels / 100, sym_pose_batch(use_symmetry=False) with the default RANSAC.  The
    bound on RRE / RTE is twice the largest value of the CPU pipeline on the same inputs (CPU_RRE_DEG, CPU_RTE above), never
    looser than 15 degrees / 0.15 (the middle row of shapenet_eval.threshold_table).  The pose-dependent sign rule of
    cs_estimate_normals lands at 84 degrees and more on such inputs: that is what the bound tells apart.  A point-to-plane
    refinement must not worsen the Chamfer distance."""
    from corsair_amd import registration as R
    from corsair_amd.utils.eval_pose import eval_pose

    qx, off0, cx, off1, Ts, voxel = _real_pairs()
    q, c = _t(gpu, qx), _t(gpu, cx)
    Fq, _ = R.fpfh_features(q, off0, 5 * voxel, 100)
    Fc, nc = R.fpfh_features(c, off1, 5 * voxel, 100)
    assert Fq.shape == (len(qx), 33) and bool(torch.isfinite(Fq).all()) and bool(torch.isfinite(Fc).all())
    res = R.sym_pose_batch(Fq, q, off0, Fc, c, off1, [1, 1, 1], 5, 0.2, 0, None, 100, 100000, 0.999, False)
    T_est = res.T_best.cpu().numpy()
    for p in range(3):
        rte, rre = eval_pose(T_est[p], Ts[p], np.eye(4), 1)
        print("pair %d: RRE %.2f deg, RTE %.4f, Chamfer %.4f" % (p, np.rad2deg(rre), rte, float(res.cd_best[p])))
    for p in range(3):
        rte, rre = eval_pose(T_est[p], Ts[p], np.eye(4), 1)
        assert np.rad2deg(rre) <= RRE_BOUND_DEG and rte <= RTE_BOUND, (p, np.rad2deg(rre), rte)
    icp = R.sym_pose_batch(Fq, q, off0, Fc, c, off1, [1, 1, 1], 5, 0.2, 0, None, 100, 100000, 0.999, False,
                           icp_max_iter=30, icp_max_dist=2 * voxel, icp_estimation="plane")
    cd0, cd1 = icp.cd_best.cpu().numpy(), icp.cd_icp.cpu().numpy()
    print("Chamfer before / after the plane refinement:", cd0, cd1)
    assert (cd1 <= cd0).all()


def test_shapenet_eval_runs_on_fpfh_without_a_checkpoint(gpu):
    from corsair_amd import shapenet_eval as SE
    from tests.test_gpu_real_clouds import _real_clouds

    clouds = [c[:4000] for c in _real_clouds()[:2]]
    cfg = SE.Config(features="fpfh", n_poses_per_model=2, ransac_max_iter=20000)
    res = SE.evaluate(None, clouds, cfg)
    assert len(res) == 4
    keys = {"model", "pose_idx", "symmetry_label", "sym_success", "T_est_sym", "chamfer_dist_sym", "T_est_ransac",
            "chamfer_dist_ransac", "rte_sym", "rre_sym", "rte_ransac", "rre_ransac", "pose_gt"}
    for r in res:
        assert set(r) == keys and np.isfinite(r["rre_ransac"]) and r["T_est_sym"].shape == (4, 4)
    with pytest.raises(ValueError, match="features"):
        SE.evaluate(None, clouds, SE.Config(features="sift"))
    a = SE.build_parser().parse_args(["--data-dir", "x", "--features", "fpfh", "--fpfh-radius", "4", "--fpfh-max-nn", "64"])
    assert a.ckpt is None and a.features == "fpfh" and a.fpfh_radius == 4.0 and a.fpfh_max_nn == 64


if __name__ == "__main__":
    np.savez(sys.argv[1], **_run_switch_cases(torch.device("cuda:0")))
