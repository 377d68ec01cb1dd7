"""cs_dbscan and cs_cluster_largest on the GPU: labels, counts, mask and statistic EQUAL tests/dbscan_ref.py on
both paths (the exhaustive scan and the cell grid), the lock-free union-find gives the components whatever the order of the
rows, the result is free of the launch shape, and the harness keeps the largest cluster only when it is configured to."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dbscan_cases as DC
from tests import dbscan_ref as ref
from tests.test_dbscan_cpu import tie_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = DC.VOXEL
SIZES = (0, 1, 2, 3, 300, 513, 700, 1500)      # 513: the smallest segment on the grid; 300 / 513 / 700: two and three workgroups
PARAMS = ((2.5, 5), (2.5, 10), (1.2, 3))       # (eps in voxels, min_points)
GRID_ROWS = 513 + 700 + 1500
_cache = {}


def _surface(n, seed):
    """n rows of a box surface at one row per voxel: the box is sized for about 1.3 n voxels, n of them are kept"""
    if n == 0:
        return np.zeros((0, 3), np.float32)
    rng = np.random.default_rng(seed)
    side = max(np.sqrt(1.3 * n * V * V / 6.0), 2 * V)
    p = rng.uniform(-0.5, 0.5, (40 * n + 200, 3))
    face = rng.integers(0, 6, len(p))
    p[np.arange(len(p)), face % 3] = np.where(face < 3, -0.5, 0.5)
    p = (p * side).astype(np.float32)
    _, idx = np.unique(np.floor(p.astype(np.float64) / V).astype(np.int64), axis=0, return_index=True)
    p = p[np.sort(idx)]
    assert len(p) >= n
    return np.ascontiguousarray(p[:n])


def _mixed():
    """(xyz, offsets): surfaces of SIZES rows; the two largest carry five isolated rows, many voxels from the surface and
    from one another, and one detached patch of 40 rows at one row per voxel, all spread among the other rows."""
    if "mixed" in _cache:
        return _cache["mixed"]
    lone = np.float64([[8, 0, 0], [0, 9, 0], [0, 0, -10], [-8, -9, 0], [9, 0, 10]])
    gy, gz = np.meshgrid(np.arange(8), np.arange(5), indexing="ij")
    parts = []
    for s, n in enumerate(SIZES):
        p = _surface(n, 100 + s)
        if n >= 700:
            rng = np.random.default_rng(s)
            far = rng.uniform(-0.2, 0.2, (5, 3)) + lone
            patch = np.stack([np.full(40, 0.0), gy.ravel() * V, gz.ravel() * V], -1) + rng.uniform(0, 0.3 * V, (40, 3))
            patch += [p[:, 0].max() + 10 * V, 0.0, 0.0]
            at = rng.permutation(n)[:45]
            p[at[:5]] = far.astype(np.float32)
            p[at[5:]] = patch.astype(np.float32)
        parts.append(p)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    _cache["mixed"] = (np.concatenate(parts), off)
    return _cache["mixed"]


def _reference():
    """the restatement of the mixed call, computed once"""
    if "want" not in _cache:
        xyz, off = _mixed()
        want = {}
        for e, mp in PARAMS:
            label, count, core = ref.dbscan(xyz, off, e * V, mp)
            keep, stat = ref.cluster_largest(label, off)
            want[(e, mp)] = dict(label=label, count=count, core=core, keep=keep, stat=stat)
        _cache["want"] = want
    return _cache["want"]


def _dbscan(dev, xyz, off, eps, mp):
    from corsair_amd import backend as B

    label, count = B.dbscan(torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(dev), off, eps, mp)
    keep, stat = B.cluster_largest(label, off)
    return label.cpu().numpy(), count.cpu().numpy(), keep.cpu().numpy(), stat.cpu().numpy()


def _assert_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    assert not len(bad), (what, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])


def _check(dev, xyz, off, eps, mp, what=""):
    """one call against the restatement; returns (label, count, core of the restatement)"""
    label, count, keep, stat = _dbscan(dev, xyz, off, eps, mp)
    wlabel, wcount, wcore = ref.dbscan(xyz, off, eps, mp)
    wkeep, wstat = ref.cluster_largest(wlabel, off)
    _assert_equal(count, wcount, what + " count")
    _assert_equal(label, wlabel, what + " label")
    _assert_equal(stat, wstat, what + " stat")
    _assert_equal(keep, wkeep, what + " keep")
    assert label.dtype == np.int32 and count.dtype == np.int32 and stat.dtype == np.int32
    return label, count, wcore


def _run_mixed(dev):
    from corsair_amd import backend as B

    xyz, off = _mixed()
    out = {}
    for e, mp in PARAMS:
        name = "%g_%d" % (e, mp)
        B.dbscan_stats(reset=True)
        label, count, keep, stat = _dbscan(dev, xyz, off, e * V, mp)
        out["stats_" + name] = np.array(B.dbscan_stats(reset=True), np.int64)
        out["label_" + name], out["count_" + name], out["keep_" + name], out["stat_" + name] = label, count, keep, stat
    return out


@pytest.fixture(scope="module")
def mixed_run(gpu):
    old = os.environ.get("CS_DBSCAN_STATS")
    os.environ["CS_DBSCAN_STATS"] = "1"
    os.environ.pop("CS_DBSCAN_GRID", None)
    try:
        return _run_mixed(gpu)
    finally:
        if old is None:
            os.environ.pop("CS_DBSCAN_STATS", None)
        else:
            os.environ["CS_DBSCAN_STATS"] = old


@pytest.mark.parametrize("e,mp", PARAMS)
def test_mixed_segments_match_the_restatement(mixed_run, e, mp):
    xyz, off = _mixed()
    want = _reference()[(e, mp)]
    name = "%g_%d" % (e, mp)
    _assert_equal(mixed_run["count_" + name], want["count"], "count")
    _assert_equal(mixed_run["label_" + name], want["label"], "label")
    _assert_equal(mixed_run["stat_" + name], want["stat"], "stat")
    _assert_equal(mixed_run["keep_" + name], want["keep"], "keep")
    border = int(((want["label"] >= 0) & ~want["core"]).sum())
    print("eps %g voxels, %d points: clusters per segment %s, border rows %d"
          % (e, mp, want["stat"][:, 0].tolist(), border))
    assert mixed_run["stats_" + name].tolist() == [GRID_ROWS, border]        # fails if no grid ran
    # the inputs are what they are meant to be: the lone rows are noise, the surface and the patch are clusters
    label, stat = want["label"], want["stat"]
    assert stat[0].tolist() == [0, -1, 0] and stat[1].tolist() == [0, -1, 0]
    far = np.nonzero(np.abs(xyz).max(1) > 5)[0]
    assert len(far) == 10 and (label[far] == -1).all()
    if (e, mp) == (2.5, 5):
        assert stat[-1, 0] == 2 and stat[-2, 0] == 2 and sorted(np.bincount(label[off[-2]:][label[off[-2]:] >= 0])) == [40, 1455]
    if (e, mp) == (2.5, 10):
        assert border > 0


def test_switch_in_a_child_process(mixed_run, tmp_path):
    """CS_DBSCAN_GRID=0 in a process of its own: the exhaustive scan alone gives the values of the default paths."""
    env = dict(os.environ)
    env["CS_DBSCAN_STATS"] = "1"
    env["CS_DBSCAN_GRID"] = "0"
    path = str(tmp_path / "scan.npz")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_dbscan", path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    scan = dict(np.load(path))
    assert scan.keys() == mixed_run.keys()
    for name, v in scan.items():
        if name.startswith("stats_"):
            assert v.tolist() == [0, mixed_run[name][1]], name           # no row on the grid, the same border rows
        else:
            _assert_equal(v, mixed_run[name], name)


def _chain(n, step):
    return np.stack([np.arange(n) * step, np.zeros(n), np.zeros(n)], -1)


UF_N = 1500
UF_EPS = 0.1


def _uf_shapes():
    """name -> (f64 [1500,3], eps, min_points, expected labels or None): one segment each, on the grid path"""
    n, eps = UF_N, UF_EPS
    rng = np.random.default_rng(11)
    chain = _chain(n, 0.9 * eps)
    two = np.zeros((n, 3))
    two[0::2] = _chain(n // 2, 0.9 * eps)
    two[1::2] = _chain(n // 2, 0.9 * eps) + [0, 3 * eps, 0]
    ang = 2 * np.pi * np.arange(n) / n
    radius = 0.9 * eps / (2 * np.sin(np.pi / n))                  # chord between consecutive rows = 0.9 eps
    ring = np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(n)], -1)
    lat = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(15), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return {
        "ascending": (chain, eps, 2, np.zeros(n, np.int32)),
        "descending": (chain[::-1], eps, 2, np.zeros(n, np.int32)),
        "random": (chain[rng.permutation(n)], eps, 2, np.zeros(n, np.int32)),
        "interleaved": (two, eps, 2, (np.arange(n) % 2).astype(np.int32)),
        "ring": (ring[rng.permutation(n)], eps, 2, np.zeros(n, np.int32)),
        # every d2 of the integer lattice ties with many; eps just above sqrt(3): the 27 rows of a 3 x 3 x 3 block
        "lattice": (lat[rng.permutation(n)], 1.7320509, 27, None),
    }


@pytest.mark.parametrize("name", ["ascending", "descending", "random", "interleaved", "ring", "lattice"])
def test_union_find_shapes(gpu, name):
    xyz, eps, mp, expect = _uf_shapes()[name]
    xyz = np.ascontiguousarray(xyz, np.float32)
    assert len(xyz) == UF_N > 512
    label, count, core = _check(gpu, xyz, [0, UF_N], eps, mp, name)
    if expect is not None:
        _assert_equal(label, expect, name)
        assert core.all()
    else:
        assert core.sum() == 8 * 8 * 13 and count.max() == 27 and (label == 0).all()     # the inner rows; the rest are border
    again = _dbscan(gpu, xyz, [0, UF_N], eps, mp)[0]
    _assert_equal(again, label, name + ", second run")


def test_permutation_and_launch_shape(gpu):
    xyz, kind = DC.patch_cloud(5)
    n = len(xyz)
    eps, mp = 2.5 * V, 10
    label, count, keep, stat = _dbscan(gpu, xyz, [0, n], eps, mp)
    wlabel, wcount, wcore = ref.dbscan(xyz, [0, n], eps, mp)
    _assert_equal(label, wlabel)
    perm = np.random.default_rng(8).permutation(n)
    plabel, pcount, pkeep, pstat = _dbscan(gpu, xyz[perm], [0, n], eps, mp)
    _assert_equal(pcount, count[perm])                            # the same core set
    assert ref.same_partition(plabel, label[perm])                # (no border row of this fixture sits at an exact tie)
    assert sorted(np.bincount(plabel[plabel >= 0]).tolist()) == [5, 184, 1530] and pstat[0, 2] == stat[0, 2] == 1530
    assert np.array_equal(pkeep, keep[perm])
    # the same segment embedded among others, on another stream: other launch sizes, other workgroups, the same labels
    other, _ = _mixed()
    both = np.concatenate([other[:1400], xyz[perm], other[1400:3000], xyz])
    off = [0, 1400, 1400 + n, 3000 + n, 3000 + 2 * n]
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        blabel, bcount, bkeep, bstat = _dbscan(gpu, both, off, eps, mp)
        st.synchronize()
    _assert_equal(blabel[off[3]:], label)
    _assert_equal(blabel[off[1]:off[2]], plabel)
    _assert_equal(bcount[off[3]:], count)
    _assert_equal(bstat[3:4], stat)
    _assert_equal(bstat[1:2], pstat)
    assert np.array_equal(bkeep[off[3]:], keep) and np.array_equal(bkeep[off[1]:off[2]], pkeep)


def test_edge_cases(gpu):
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(8), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    L = 0.03125                                                   # the lattice's spacing, a power of two: every d2 is exact
    dup = np.concatenate([_surface(500, 1), _surface(500, 1)[:250], np.tile(np.float32([[0.1, 0.2, 0.5]]), (25, 1))])
    bad = _surface(700, 2)
    bad[5] = [np.nan, 0, 0]
    bad[300] = [0, np.inf, 0]
    bad[600] = [0, 0, -np.inf]
    small_bad = np.float32([[0, 0, 0], [np.nan, 1, 1], [V, 0, 0], [np.inf, 0, 0], [0, V, 0]])
    ties = [tie_case(False)[0], tie_case(True)[0]]
    parts = [g * np.float32(L), dup, bad, small_bad, g[:200] * np.float32(L)] + [t * np.float32(V) for t in ties]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    label, count, core = _check(gpu, xyz, off, L, 1, "a lattice at eps")      # the threshold is strict: nothing links
    assert count[:off[1]].tolist() == [1] * 648 and label[:off[1]].tolist() == list(range(648))
    label, count, core = _check(gpu, xyz, off, L * (1 + 2.0 ** -20), 7, "a lattice just inside eps")
    assert count[:off[1]].max() == 7 and core[:off[1]].sum() == 7 * 7 * 6 and (label[:off[1]][core[:off[1]]] == 0).all()
    assert label[0] == -1 and label[1] == -1 and label[9 * 8 + 8 + 1] == 0      # a corner, an edge row; a face row is a border row
    _check(gpu, xyz, off, 2.5 * V, 26, "many ties")
    label, count, core = _check(gpu, xyz, off, 1.1 * V, 4, "ties")
    assert label[off[5]:off[6]].tolist() == tie_case(False)[1] and label[off[6]:].tolist() == tie_case(True)[1]
    assert count[off[2] + 5] == 0 and label[off[2] + 5] == -1 and count[off[3] + 3] == 0
    label, count, core = _check(gpu, xyz, off, 1e-4 * V, 25, "copies")
    assert (label[off[2] - 25:off[2]] == 0).all() and (label[off[1]:off[2] - 25] == -1).all()      # 25 copies of one point
    label, count, core = _check(gpu, xyz, off, 1e-4 * V, 2, "pairs")
    assert label[off[1]:off[1] + 250].tolist() == list(range(250))            # each row and its copy: 250 clusters by row
    # far coordinates: a cell index at the clamp is still exact; a segment of one point on the grid
    a = _surface(700, 3) + np.float32([70.0, -70.0, 0.0])
    b = _surface(700, 4) + np.float32([1.0e6, 0.0, 0.0])
    c = _surface(40, 5) * np.float32(1.0e6)
    one = np.tile(np.float32([[0.3, -0.2, 0.9]]), (600, 1))
    one[7] = [np.nan, 0, 0]
    parts = [a, b, c, one]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    _check(gpu, xyz, off, 2.5 * V, 5, "far")
    _check(gpu, xyz, off, 0.3, 5, "far, wide")
    want = [0] * 1440 + [0] * 7 + [-1] + [0] * 592
    for eps in (1e150, 1e160):                                   # the scan; the square overflows: every finite row is linked
        label, count, keep, stat = _dbscan(gpu, xyz, off, eps, 5)
        assert label.tolist() == want and count.tolist() == [700] * 1400 + [40] * 40 + [599] * 7 + [0] + [599] * 592
        assert stat.tolist() == [[1, 0, 700], [1, 0, 700], [1, 0, 40], [1, 0, 599]] and keep.sum() == 2039 and not keep[1447]
    label, count, keep, stat = _dbscan(gpu, xyz, off, 1e-170, 1)        # the square underflows: not even the row itself
    assert (label == -1).all() and not count.any() and not keep.any() and stat.tolist() == [[0, -1, 0]] * 4
    # labels that are not cs_dbscan's: out of range counts as -1
    from corsair_amd import backend as B

    lab = np.int32([1, 1, 0, 0, -1, 2, 8, -5] + [-1, -1] + [3, 3, 3, 0])
    keep, stat = B.cluster_largest(torch.from_numpy(lab).to(gpu), [0, 8, 10, 10, 14])
    wkeep, wstat = ref.cluster_largest(lab, [0, 8, 10, 10, 14])
    assert stat.cpu().numpy().tolist() == wstat.tolist() == [[3, 0, 2], [0, -1, 0], [0, -1, 0], [2, 3, 3]]
    assert np.array_equal(keep.cpu().numpy(), wkeep)


def test_refusals(gpu):
    from corsair_amd import _lib, backend as B
    from corsair_amd._lib import CorsairHipError, i64_array, ptr, stream_ptr

    x = torch.zeros((8, 3), device=gpu)
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CorsairHipError, match="eps"):
            B.dbscan(x, [0, 8], eps, 5)
    for mp in (0, -3):
        with pytest.raises(CorsairHipError, match="min_points"):
            B.dbscan(x, [0, 8], 0.1, mp)
    with pytest.raises(CorsairHipError, match="bad segment"):
        B.dbscan(x, [0, 5, 3, 8], 0.1, 5)
    with pytest.raises(ValueError, match="offset table"):
        B.dbscan(x, [0, 9], 0.1, 5)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        B.dbscan(torch.zeros((8, 2), device=gpu), [0, 8], 0.1, 5)
    lib = _lib.load()
    lab = torch.zeros(8, dtype=torch.int32, device=gpu)
    keep = torch.zeros(8, dtype=torch.uint8, device=gpu)
    stat = torch.zeros((1, 3), dtype=torch.int32, device=gpu)
    assert lib.cs_dbscan(ptr(x), None, 1, 0.1, 5, ptr(lab), None, stream_ptr()) < 0                  # no offset table
    assert b"NULL offset table" in lib.cs_last_error()
    assert lib.cs_dbscan(ptr(x), i64_array([0, 8]), -1, 0.1, 5, ptr(lab), None, stream_ptr()) < 0    # a negative count
    assert lib.cs_dbscan(None, i64_array([0, 8]), 1, 0.1, 5, ptr(lab), None, stream_ptr()) < 0       # a null array with rows
    assert b"NULL" in lib.cs_last_error()
    assert lib.cs_dbscan(ptr(x), i64_array([0, 8]), 1, 0.1, 5, None, None, stream_ptr()) < 0
    assert lib.cs_dbscan(ptr(x), i64_array([0, 1 << 31]), 1, 0.1, 5, ptr(lab), None, stream_ptr()) < 0
    assert b"2^31" in lib.cs_last_error()
    assert lib.cs_dbscan(ptr(x), i64_array([0, 8]), 1, 0.1, 5, ptr(lab), None, stream_ptr()) == 0    # d_count may be NULL
    assert lib.cs_dbscan(None, i64_array([0, 0, 0]), 2, 0.1, 5, None, None, stream_ptr()) == 0       # empty segments
    assert lib.cs_dbscan(None, i64_array([0]), 0, 0.1, 5, None, None, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert lab.tolist() == [0] * 8                                            # eight copies of the origin
    assert lib.cs_cluster_largest(ptr(lab), None, 1, ptr(keep), ptr(stat), stream_ptr()) < 0
    assert lib.cs_cluster_largest(ptr(lab), i64_array([0, 8]), 1, ptr(keep), None, stream_ptr()) < 0
    assert lib.cs_cluster_largest(None, i64_array([0, 8]), 1, ptr(keep), ptr(stat), stream_ptr()) < 0
    assert lib.cs_cluster_largest(ptr(lab), i64_array([0, 8]), 1, None, ptr(stat), stream_ptr()) < 0
    assert lib.cs_cluster_largest(ptr(lab), i64_array([0, 8]), -1, ptr(keep), ptr(stat), stream_ptr()) < 0
    assert lib.cs_cluster_largest(None, i64_array([0]), 0, None, None, stream_ptr()) == 0
    with pytest.raises(ValueError, match="cover the offset table"):
        B.cluster_largest(lab, [0, 9])
    with pytest.raises(TypeError):
        B.cluster_largest(lab.to(torch.int64), [0, 8])


def test_patch_fixture_through_backend(gpu):
    """The three patch clouds in one call: the numbers of tests/test_dbscan_cpu.py, and one profile scope per call."""
    from corsair_amd import _lib, backend as B

    xyz, off, kind = DC.packed()
    x = torch.from_numpy(xyz).to(gpu)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        label, count = B.dbscan(x, off, 2.5 * V, 5)
        torch.cuda.synchronize()
        assert _lib.prof_get("cluster")[1] == 1
        keep, stat = B.cluster_largest(label, off)
        torch.cuda.synchronize()
        ms, n, units = _lib.prof_get("cluster")
        assert _lib.prof_get("outlier")[1] == 0 and _lib.prof_get("normals")[1] == 0
    finally:
        _lib.prof_enable(False)
    assert n == 2 and ms > 0 and units > 0
    label, keep, stat = label.cpu().numpy(), keep.cpu().numpy(), stat.cpu().numpy()
    wlabel, wcount, wcore = ref.dbscan(xyz, off, 2.5 * V, 5)
    _assert_equal(label, wlabel)
    _assert_equal(count.cpu().numpy(), wcount)
    for p, i in enumerate(DC.CLOUDS):
        sizes, noise, border, border10 = DC.TABLE[i]
        seg = slice(off[p], off[p + 1])
        assert stat[p, 0] == 2 and stat[p, 2] == sizes[0] and (label[seg] < 0).sum() == noise
        assert sorted(np.bincount(label[seg][label[seg] >= 0]).tolist()) == sorted(sizes)
        assert ((label[seg] >= 0) & ~wcore[seg]).sum() == border
    assert keep[kind == DC.REAL].all() and not keep[kind != DC.REAL].any()
    rkeep, _ = B.outlier_radius(x, off, 2.5 * V, 4)
    assert rkeep.cpu().numpy()[kind == DC.PATCH].all()                        # what the radius filter cannot do
    label10 = B.dbscan(x, off, 2.5 * V, 10)[0].cpu().numpy()
    wlabel10, _, wcore10 = ref.dbscan(xyz, off, 2.5 * V, 10)
    _assert_equal(label10, wlabel10)
    assert [int(((wlabel10[off[p]:off[p + 1]] >= 0) & ~wcore10[off[p]:off[p + 1]]).sum()) for p in range(3)] == \
        [DC.TABLE[i][3] for i in DC.CLOUDS]


def _rows(a):
    return {r.tobytes() for r in np.ascontiguousarray(a, np.float32)}


def test_harness_keeps_the_largest_cluster_only_when_configured(gpu):
    from corsair_amd import _lib, harness, synth
    from tests import outlier_ref as oref

    sd, emb = synth.make_state_dicts(31)
    clouds = [DC.patch_cloud(i)[0].astype(np.float64) for i in DC.CLOUDS]      # f64, as posed queries arrive
    kinds = [DC.patch_cloud(i)[1] for i in DC.CLOUDS]
    vox = harness.Config().voxel_size
    assert vox == V
    plain = harness.Pipeline(sd, emb, device=gpu)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        base = plain.embed_clouds(clouds)
        same = plain.embed_clouds(clouds, scan_filter=True)          # the default Config names no filter
        torch.cuda.synchronize()
        assert _lib.prof_get("cluster")[1] == 0 and _lib.prof_get("outlier")[1] == 0      # nothing new was launched
    finally:
        _lib.prof_enable(False)
    # (two rows of a shifted patch can share a voxel: the network, and the filter, see the first row of every voxel)
    voxels = [len(np.unique(np.floor(c / vox).astype(np.int64), axis=0)) for c in clouds]
    assert base.offsets == [0] + np.cumsum(voxels).tolist() and base.offsets[-1] < sum(len(c) for c in clouds)
    assert same.offsets == base.offsets and torch.equal(same.F, base.F) and torch.equal(same.desc, base.desc)
    pipe = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(scan_filter="cluster"))
    unfiltered = pipe.embed_clouds(clouds)                            # the catalog's call: scan_filter stays False
    assert unfiltered.offsets == base.offsets and torch.equal(unfiltered.F, base.F)
    got = pipe.embed_clouds(clouds, scan_filter=True)
    origin = got.origin.cpu().numpy()
    kept = 0
    dropped = 0
    for p, (c, k) in enumerate(zip(clouds, kinds)):
        seg = origin[got.offsets[p]:got.offsets[p + 1]]
        seen = base.origin[base.offsets[p]:base.offsets[p + 1]].cpu().numpy()       # the voxelised scan the filter saw
        label, _, _ = ref.dbscan(seen, [0, len(seen)], 2.5 * vox, 5)
        want, stat = ref.cluster_largest(label, [0, len(seen)])
        assert np.array_equal(seg, seen[want]), "the rows the restatement keeps, in their order"
        assert not (_rows(seg) & _rows(c[k != DC.REAL])), "a clutter or patch row reached the network"
        assert _rows(seg) == _rows(c[k == DC.REAL]) and len(seg) == stat[0, 2] == int((k == DC.REAL).sum())
        kept += len(seg)
        dropped += len(seen) - len(seg)
    assert dropped > 300
    assert got.offsets[-1] == kept == got.F.shape[0] == origin.shape[0] and got.desc.shape[0] == 3
    assert pipe.scan_filter_stat == {"rows_in": base.offsets[-1], "rows_kept": kept, "clouds_skipped": 0}
    # a cloud of 8 rows whose largest cluster has 5: it keeps all of its rows
    grid5 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1]], np.float64)
    lone = np.array([[40, 0, 0], [0, 40, 0], [0, 0, 40]], np.float64)
    tiny = ((np.concatenate([grid5, lone]) + 0.5) * vox).astype(np.float32).astype(np.float64)
    label, _, _ = ref.dbscan(tiny, [0, 8], 2.5 * vox, 5)
    assert label.tolist() == [0] * 5 + [-1] * 3
    pipe.scan_filter_stat = {"rows_in": 0, "rows_kept": 0, "clouds_skipped": 0}
    got = pipe.embed_clouds([clouds[1], tiny], scan_filter=True)
    assert got.offsets[2] - got.offsets[1] == 8
    assert _rows(got.origin[got.offsets[1]:got.offsets[2]].cpu().numpy()) == _rows(tiny)
    assert got.offsets[1] == DC.OC.ROWS[3][0]
    assert pipe.scan_filter_stat == {"rows_in": voxels[1] + 8, "rows_kept": DC.OC.ROWS[3][0] + 8, "clouds_skipped": 1}
    # the radius filter returns what it returned before
    rpipe = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(scan_filter="radius"))
    got = rpipe.embed_clouds([clouds[1]], scan_filter=True)
    seen = base.origin[base.offsets[1]:base.offsets[2]].cpu().numpy()
    rk, _ = oref.outlier_radius(seen, [0, len(seen)], 2.5 * vox, 4)
    assert got.offsets == [0, int(rk.sum())] and np.array_equal(got.origin.cpu().numpy(), seen[rk])
    assert int(rk.sum()) > DC.OC.ROWS[3][0] + 40                     # the radius filter keeps most of the patch


if __name__ == "__main__":
    np.savez(sys.argv[1], **_run_mixed(torch.device("cuda:0")))
