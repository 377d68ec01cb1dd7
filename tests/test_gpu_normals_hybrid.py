"""cs_estimate_normals_hybrid on the GPU: every normal is BIT-EQUAL to tests/normals_hybrid_ref.py, on the cell-grid path
(segments of more than 512 rows) and on the exhaustive path (smaller segments, and everything under CS_NORMALS_GRID=0)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import normals_hybrid_ref as href
from tests import test_gpu_icp as pt
from tests import test_gpu_normals as knn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_MIN = 513     # the smallest segment that takes the grid path (NRM_GRID_MIN, normals.hip)
MAX_NNS = (3, 8, 16, 17, 32)
# on the mixed segments: per max_nn, a radius at which some rows of the grid-path segments find fewer than three rows, some
# between 3 and max_nn, some more than max_nn (test_mixed_segments_match_reference checks the three counts)
RADII = {3: 0.10, 8: 0.12, 16: 0.14, 17: 0.14, 32: 0.12}
RADIUS = RADII[16]
_bits_equal = knn._bits_equal


def _run(dev, xyz, off, max_nn, radius):
    from corsair_amd import backend as B

    x = torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)).to(dev)
    return B.estimate_normals(x, off, max_nn, radius=radius).cpu().numpy()


def _assert_bits(got, want, what=""):
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(1))[0]
    assert not len(bad), (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def _count_inside(seg, radius):
    """Rows inside the radius of every row (the row itself included), by the plain f64 distance."""
    s = seg.astype(np.float64)
    d2 = ((s[:, None, :] - s[None, :, :]) ** 2).sum(-1)
    return (d2 < radius * radius).sum(1)


@functools.lru_cache(maxsize=None)
def _mixed(max_nn):
    """0, 1, 2, 3, max_nn - 1, max_nn, max_nn + 1, 300 (exhaustive path), 513 (grid path) rows of one cloud in one call;
    empty segments in the middle and at the end.  max_nn = 32 adds a 1200-row segment: no radius leaves rows with fewer
    than three and rows with more than 32 neighbours in the same 513 rows."""
    from corsair_amd import synth

    rng = np.random.default_rng(200 + max_nn)
    cloud = synth.make_cloud(9, 4000)
    sizes = [0, 1, 2, 3, max_nn - 1, 0, max_nn, max_nn + 1, 300, GRID_MIN] + ([1200] if max_nn == 32 else []) + [0]
    xyz = np.concatenate([cloud[rng.choice(len(cloud), n, replace=False)] for n in sizes]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return xyz, off, href.estimate_normals(xyz, off, RADII[max_nn], max_nn)


@pytest.mark.parametrize("max_nn", MAX_NNS)
def test_mixed_segments_match_reference(gpu, max_nn):
    xyz, off, want = _mixed(max_nn)
    # the radius leaves all three kinds of row on the grid path
    radius = RADII[max_nn]
    inside = np.concatenate([_count_inside(xyz[off[s]:off[s + 1]], radius) for s in range(9, len(off) - 2)])
    few, mid, many = (inside < 3).sum(), ((inside >= 3) & (inside <= max_nn)).sum(), (inside > max_nn).sum()
    print("max_nn %d: rows with < 3 / 3..max_nn / > max_nn inside the radius: %d / %d / %d" % (max_nn, few, mid, many))
    assert few > 0 and mid > 0 and many > 0
    got = _run(gpu, xyz, off, max_nn, radius)
    _assert_bits(got, want, max_nn)
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-6
    assert _bits_equal(_run(gpu, xyz, off, max_nn, radius), got)          # two runs: identical bits


def test_batch_neighbours_and_segment_order_do_not_matter(gpu):
    xyz, off, want = _mixed(16)
    for s in (4, 8, 9):                       # max_nn - 1 rows, 300 rows, 513 rows
        seg = xyz[off[s]:off[s + 1]]
        assert _bits_equal(_run(gpu, seg, [0, len(seg)], 16, RADIUS), want[off[s]:off[s + 1]]), s
    order = [9, 1, 8, 4, 9, 3]
    sh = np.concatenate([xyz[off[s]:off[s + 1]] for s in order])
    soff = np.concatenate([[0], np.cumsum([off[s + 1] - off[s] for s in order])]).tolist()
    got = _run(gpu, sh, soff, 16, RADIUS)
    for i, s in enumerate(order):
        assert _bits_equal(got[soff[i]:soff[i + 1]], want[off[s]:off[s + 1]]), s


def _sphere(n, seed=3):
    rng = np.random.default_rng(seed)
    sph = rng.standard_normal((n, 3))
    return (0.5 * sph / np.linalg.norm(sph, axis=1, keepdims=True)).astype(np.float32)


def test_permuting_a_tie_free_segment_permutes_the_normals(gpu):
    sph = _sphere(700)
    d2 = ((sph[:, None, :].astype(np.float64) - sph[None, :, :]) ** 2).sum(-1)
    assert len(np.unique(d2[np.triu_indices(700, 1)])) == 700 * 699 // 2          # no two distances tie
    perm = np.random.default_rng(8).permutation(700)
    a = _run(gpu, sph, [0, 700], 16, 0.15)
    b = _run(gpu, sph[perm], [0, 700], 16, 0.15)
    assert _bits_equal(b, a[perm])
    _assert_bits(a, href.estimate_normals(sph, [0, 700], 0.15, 16))


def _lattice(nx, ny, nz):
    return np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ties_case():
    """The integer grid of tests/test_gpu_normals.py (210 rows, exhaustive path) and a 9 x 8 x 8 one (576 rows, grid path);
    duplicated rows (zero distances that tie) below and above the grid threshold."""
    rng = np.random.default_rng(6)
    cont = rng.uniform(-1, 1, (90, 3)).astype(np.float32)
    dup = np.concatenate([cont, cont[:40], cont[10:30]])
    cont2 = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    dup2 = np.concatenate([cont2, cont2[:200], cont2[100:250]])
    parts = [_lattice(7, 6, 5), dup, _lattice(9, 8, 8), dup2]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    return np.concatenate(parts), off


@pytest.mark.parametrize("max_nn", (8, 17, 32))
def test_integer_grid_and_duplicated_rows(gpu, max_nn):
    xyz, off = _ties_case()
    assert off[3] - off[2] >= GRID_MIN and off[4] - off[3] >= GRID_MIN and off[1] < GRID_MIN
    # radius 2.0: the lattice rows at distance exactly 2 are outside (27 rows inside for an inner row, ties at 1, 2, 3)
    _assert_bits(_run(gpu, xyz, off, max_nn, 2.0), href.estimate_normals(xyz, off, 2.0, max_nn), max_nn)
    centre = int(np.nonzero((xyz[off[2]:off[3]] == (4, 4, 4)).all(1))[0][0])
    assert len(href.neighbours(xyz[off[2]:off[3]], centre, 2.0, 32)) == 27


def test_nan_inf_far_and_clamped_rows(gpu):
    sph = _sphere(600)
    nan = sph.copy()
    nan[17, 1] = np.nan
    nan[40, 0] = np.inf
    nan[599, 2] = -np.inf
    far = sph + np.float32([70.0, -70.0, 0.0])                      # a coordinate of 70
    # one coordinate of 10^6 at radius 0.01: every cell index of that axis clamps to 32767
    flat = (0.2 * sph).astype(np.float32)
    flat[:, 0] = 1.0e6
    small = sph[:80].copy()
    small[5, 0] = np.nan
    small[9, 2] = np.inf
    parts = [nan, far, small]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    got = _run(gpu, xyz, off, 8, 0.15)
    _assert_bits(got, href.estimate_normals(xyz, off, 0.15, 8))
    for r in (17, 40, 599, off[2] + 5, off[2] + 9):
        assert np.array_equal(got[r], np.float32([0, 0, 1])), r
    radial = sph / np.linalg.norm(sph, axis=1, keepdims=True)
    assert np.abs(np.abs((got[off[1]:off[2]] * radial).sum(1)) - 1).max() < 0.05
    got = _run(gpu, flat, [0, 600], 16, 0.01)
    want = href.estimate_normals(flat, [0, 600], 0.01, 16)
    _assert_bits(got, want)
    inside = _count_inside(flat, 0.01)
    assert (inside >= 3).sum() > 100 and (inside < 3).sum() > 0
    assert np.array_equal(got[inside >= 3], np.tile(np.float32([1, 0, 0]), (int((inside >= 3).sum()), 1)))


@pytest.mark.parametrize("big", (False, True))
def test_exact_plane_line_and_point(gpu, big):
    nx, ny, nl, npt = (30, 20, 600, 520) if big else (6, 5, 9, 6)
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    plane = np.concatenate([g, np.full((len(g), 1), 0.75, np.float32)], 1)
    line = np.zeros((nl, 3), np.float32)
    line[:, 0] = np.arange(nl) * 0.5
    point = np.tile(np.float32([[0.3, -0.2, 0.9]]), (npt, 1))
    parts = [plane, line, point]
    assert all((len(p) >= GRID_MIN) == big for p in parts)
    xyz = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    got = _run(gpu, xyz, off, 8, 1.5)
    _assert_bits(got, href.estimate_normals(xyz, off, 1.5, 8))
    # the defined answers of cs_estimate_normals' header comment
    assert np.array_equal(got[off[0]:off[1]], np.tile(np.float32([0, 0, 1]), (len(plane), 1)))
    assert np.array_equal(got[off[1]:off[2]], np.tile(np.float32([0, 1, 0]), (len(line), 1)))
    assert np.array_equal(got[off[2]:off[3]], np.tile(np.float32([1, 0, 0]), (len(point), 1)))


@pytest.mark.parametrize("max_nn", (3, 16, 32))
def test_huge_radius_is_knn(gpu, max_nn):
    xyz, off, _ = _mixed(max_nn)
    want = knn._run(gpu, xyz, off, max_nn)
    assert _bits_equal(_run(gpu, xyz, off, max_nn, 1e150), want)       # r^2 = 1e300: the grid path, every row in two cells
    assert _bits_equal(_run(gpu, xyz, off, max_nn, 1e300), want)       # r^2 = +inf: the exhaustive path


def _run_switch_cases(dev):
    out = {}
    for max_nn in (8, 32):
        xyz, off, _ = _mixed(max_nn)
        out["mixed%d" % max_nn] = _run(dev, xyz, off, max_nn, RADII[max_nn])
    xyz, off = _ties_case()
    out["ties"] = _run(dev, xyz, off, 17, 2.0)
    return out


def test_switch_in_child_processes(gpu, tmp_path):
    """CS_NORMALS_GRID=0 and the default, each in a process of its own: identical bits, equal to this process's."""
    res = {}
    for setting in ("default", "0"):
        env = dict(os.environ)
        env.pop("CS_NORMALS_GRID", None)
        env["CS_NORMALS_STATS"] = "1"
        if setting == "0":
            env["CS_NORMALS_GRID"] = "0"
        path = str(tmp_path / ("out_%s.npz" % setting))
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_normals_hybrid", path], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[setting] = dict(np.load(path))
    a, b, here = res["default"], res["0"], _run_switch_cases(gpu)
    assert a.keys() == b.keys()
    for k in here:
        assert _bits_equal(a[k], b[k]) and _bits_equal(a[k], here[k]), k
    # the switch did select another path: 513 rows per mixed call (and the 1200 of max_nn = 32), two segments of the ties case
    xyz, off = _ties_case()
    assert a["stats"].tolist() == [2 * GRID_MIN + 1200 + (off[3] - off[2]) + (off[4] - off[3]), 0]
    assert b["stats"].tolist() == [0, 0]


def test_stats_count_only_when_asked(gpu, monkeypatch):
    from corsair_amd import backend as B

    xyz, off, _ = _mixed(8)
    B.normals_stats(reset=True)
    _run(gpu, xyz, off, 8, RADII[8])
    assert B.normals_stats() == (0, 0)
    monkeypatch.setenv("CS_NORMALS_STATS", "1")
    _run(gpu, xyz, off, 8, RADII[8])
    assert B.normals_stats(reset=True) == (GRID_MIN, 0) and B.normals_stats() == (0, 0)
    monkeypatch.setenv("CS_NORMALS_GRID", "0")                      # read per call
    _run(gpu, xyz, off, 8, RADII[8])
    assert B.normals_stats() == (0, 0)


def test_refused_arguments_and_empty_calls(gpu):
    from corsair_amd import _lib, backend as B

    x = torch.zeros((10, 3), device=gpu)
    for k in (2, 33, 0, -1):
        with pytest.raises(_lib.CorsairHipError, match="max_nn outside"):
            B.estimate_normals(x, [0, 10], k, radius=0.1)
    for radius in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.CorsairHipError, match="radius must be positive and finite"):
            B.estimate_normals(x, [0, 10], 8, radius=radius)
    with pytest.raises(ValueError):
        B.estimate_normals(x, [0, 11], 8, radius=0.1)
    with pytest.raises(ValueError):
        B.estimate_normals(x.reshape(-1), [0, 10], 8, radius=0.1)
    with pytest.raises(_lib.CorsairHipError, match="bad segment"):
        B.estimate_normals(x, [0, 7, 5], 8, radius=0.1)
    with pytest.raises(TypeError):
        B.estimate_normals(x.double(), [0, 10], 8, radius=0.1)
    lib = _lib.load()
    off = (ctypes.c_int64 * 2)(0, 10)
    out = torch.empty_like(x)
    f = lib.cs_estimate_normals_hybrid
    assert f(_lib.ptr(x), off, 1, 0.1, 8, _lib.ptr(out), None) == 0
    assert f(None, off, 1, 0.1, 8, _lib.ptr(out), None) < 0
    assert f(_lib.ptr(x), off, 1, 0.1, 8, None, None) < 0
    assert f(_lib.ptr(x), None, 1, 0.1, 8, _lib.ptr(out), None) < 0
    assert f(_lib.ptr(x), off, -1, 0.1, 8, _lib.ptr(out), None) < 0
    assert f(_lib.ptr(x), off, 1, 0.0, 8, _lib.ptr(out), None) < 0
    assert f(_lib.ptr(x), off, 1, float("inf"), 8, _lib.ptr(out), None) < 0
    assert f(_lib.ptr(x), off, 1, 0.1, 33, _lib.ptr(out), None) < 0
    assert f(_lib.ptr(x), (ctypes.c_int64 * 2)(0, 2 ** 31), 1, 0.1, 8, _lib.ptr(out), None) < 0
    # n_seg = 0 and empty segments are legal
    assert B.estimate_normals(x[:0], [0], 8, radius=0.1).shape == (0, 3)
    assert B.estimate_normals(x[:0], [0, 0, 0], 8, radius=0.1).shape == (0, 3)
    torch.cuda.synchronize()


def test_profile_family_sees_one_scope_per_call(gpu):
    from corsair_amd import _lib

    xyz, off, _ = _mixed(8)                    # segments of both paths in one call
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        _run(gpu, xyz, off, 8, RADII[8])
        torch.cuda.synchronize()
        ms, n, flop = _lib.prof_get("normals")
    finally:
        _lib.prof_enable(False)
    assert n == 1 and ms > 0 and flop > 0


def test_sym_pose_batch_and_harness_with_a_normal_radius(gpu):
    from corsair_amd import backend as B, harness as H, registration as R

    F0, x0, off0, F1, x1, off1, Ts = pt._pair_batch(gpu)
    kw = dict(k_nn=5, max_corr=0.2, seed=0, max_iter=2000, force_gate=True, icp_max_iter=5, icp_max_dist=0.06,
              icp_estimation="plane", icp_normal_k=8)
    nrm = B.estimate_normals(x1, off1, 8, radius=0.15)
    assert _bits_equal(nrm.cpu().numpy(), href.estimate_normals(x1.cpu().numpy(), off1, 0.15, 8))
    knn_nrm = B.estimate_normals(x1, off1, 8)
    assert not _bits_equal(nrm.cpu().numpy(), knn_nrm.cpu().numpy())
    with_r = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_normal_radius=0.15, **kw)
    given = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], normals1=nrm, **kw)
    plain = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], **kw)
    for name in ("T_icp", "cd_icp", "icp_fitness", "icp_rmse", "icp_iters"):
        a = getattr(with_r, name).cpu().numpy()
        assert a is not None and pt._same(a, getattr(given, name).cpu().numpy()), name
    assert not pt._same(with_r.T_icp.cpu().numpy(), plain.T_icp.cpu().numpy())
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="icp_normal_radius"):
            R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_normal_radius=bad, **kw)
    # the harness: a run with the radius set = one whose catalog was given those normals
    desc = torch.zeros((2, 0), dtype=torch.float32, device=gpu)
    qs, cat = H.EmbeddedSet(F0, x0, off0, desc), H.EmbeddedSet(F1, x1, off1, desc)
    args = (np.arange(2), np.arange(2), np.asarray([1, 2]), np.stack(Ts), np.stack([np.eye(4)] * 2))
    base = dict(ransac_max_iter=2000, icp_max_iter=5, icp_estimation="plane", icp_normal_k=8)
    cfg = H.Config(icp_normal_radius=0.15, **base)
    pipe = pt._Pipe(gpu, cfg)
    pipe.with_normals = lambda s: H.Pipeline.with_normals(pipe, s)
    carried = pipe.with_normals(cat)
    assert _bits_equal(carried.normal.cpu().numpy(), nrm.cpu().numpy())
    got = H.register_queries(pipe, qs, args[0], cat, *args[1:])
    want = H.register_queries(pt._Pipe(gpu, H.Config(**base)), qs, args[0],
                              H.EmbeddedSet(F1, x1, off1, desc, nrm), *args[1:])
    assert set(got) == set(want)
    for k in got:
        assert pt._same(got[k], want[k]), k
    with pytest.raises(ValueError, match="icp_normal_radius"):
        H.Config(icp_normal_radius=-1.0).check_icp()


if __name__ == "__main__":
    from corsair_amd import backend as _B

    _B.normals_stats(reset=True)
    _out = _run_switch_cases(torch.device("cuda:0"))
    _out["stats"] = np.array(_B.normals_stats(), np.int64)
    np.savez(sys.argv[1], **_out)
