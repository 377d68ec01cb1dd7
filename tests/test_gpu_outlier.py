"""cs_knn_mean_dist, cs_outlier_statistical and cs_outlier_radius on the GPU: every output is BIT-EQUAL to
tests/outlier_ref.py on both paths (the exhaustive scan and the cell grid with its redo list), the statistic is free of the
rows' order and of the launch shape, and the harness cleans raw query scans only when it is configured to."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import outlier_cases as OC
from tests import outlier_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 2, 3, 300, 513, 700, 1025, 1500)      # 513 / 1025: the smallest segments of the radius / mean-distance grids
KS = (2, 8, 16, 20, 32)
RADIUS = 0.11
_want = {}


def _box(n, seed):
    """n surface samples of the unit box"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, (n, 3))
    face = rng.integers(0, 6, n)
    p[np.arange(n), face % 3] = np.where(face < 3, -0.5, 0.5)
    return p.astype(np.float32)


def _mixed():
    """(xyz, offsets): box surfaces of SIZES rows; the two largest carry five isolated rows each, many box sizes away from
    the box and from one another and spread among the other rows: not even at k = 2 does one of them find its k-th
    neighbour inside the distance its 27 cells cover, so the redo list is not empty."""
    lone = np.float64([[8, 0, 0], [0, 9, 0], [0, 0, -10], [-8, -9, 0], [9, 0, 10]])
    parts = []
    for s, n in enumerate(SIZES):
        p = _box(n, 100 + s)
        if n >= 1025:
            far = np.random.default_rng(s).uniform(-0.2, 0.2, (5, 3)) + lone
            p[np.arange(5) * (n // 5) + 7] = far.astype(np.float32)
        parts.append(p)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    return np.concatenate(parts), off


def _reference():
    """the restatement of the mixed call, computed once: means per k, counts"""
    if not _want:
        xyz, off = _mixed()
        for k in KS:
            _want["mean%d" % k] = ref.knn_mean_dist(xyz, off, k)
        _want["count"] = ref.radius_count(xyz, off, RADIUS)
    return _want


def _mean(dev, xyz, off, k):
    from corsair_amd import backend as B

    return B.knn_mean_dist(torch.from_numpy(np.ascontiguousarray(xyz)).to(dev), off, k).cpu().numpy()


def _stat(dev, xyz, off, k, std):
    from corsair_amd import backend as B

    keep, stat = B.outlier_statistical(torch.from_numpy(np.ascontiguousarray(xyz)).to(dev), off, k, std)
    return keep.cpu().numpy(), stat.cpu().numpy()


def _radius(dev, xyz, off, radius, nb):
    from corsair_amd import backend as B

    keep, count = B.outlier_radius(torch.from_numpy(np.ascontiguousarray(xyz)).to(dev), off, radius, nb)
    return keep.cpu().numpy(), count.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_bits(got, want, what=""):
    bad = np.nonzero(_bits(got).reshape(len(got), -1) != _bits(want).reshape(len(want), -1))[0]
    assert not len(bad), (what, len(bad), bad[:5], np.asarray(got)[bad[:5]], np.asarray(want)[bad[:5]])


def _run_mixed(dev):
    from corsair_amd import backend as B

    xyz, off = _mixed()
    out = {}
    for k in KS:
        B.outlier_stats(reset=True)
        out["mean%d" % k] = _mean(dev, xyz, off, k)
        out["stats%d" % k] = np.array(B.outlier_stats(reset=True), np.int64)
        keep, stat = _stat(dev, xyz, off, k, 2.0)
        out["keep%d" % k], out["stat%d" % k] = keep, stat
    B.outlier_stats(reset=True)
    out["rkeep"], out["count"] = _radius(dev, xyz, off, RADIUS, 4)
    out["rstats"] = np.array(B.outlier_stats(reset=True), np.int64)
    return out


@pytest.fixture(scope="module")
def mixed_run(gpu):
    old = os.environ.get("CS_OUTLIER_STATS")
    os.environ["CS_OUTLIER_STATS"] = "1"
    os.environ.pop("CS_OUTLIER_GRID", None)
    try:
        return _run_mixed(gpu)
    finally:
        if old is None:
            os.environ.pop("CS_OUTLIER_STATS", None)
        else:
            os.environ["CS_OUTLIER_STATS"] = old


@pytest.mark.parametrize("k", KS)
def test_mixed_segments_match_the_restatement(mixed_run, k):
    xyz, off = _mixed()
    want = _reference()
    _assert_bits(mixed_run["mean%d" % k], want["mean%d" % k], "mean")
    keep, stat = ref.outlier_statistical(want["mean%d" % k], off, 2.0)
    _assert_bits(mixed_run["stat%d" % k], stat, "stat")
    assert np.array_equal(mixed_run["keep%d" % k], keep)
    answered, redone = mixed_run["stats%d" % k].tolist()
    print("k = %d: grid rows %d, recomputed %d" % (k, answered, redone))
    assert answered == 1025 + 1500 and 10 <= redone < answered // 2      # the isolated rows at least; fails if no grid ran
    assert stat[0].tolist() == [0.0, 0.0, 0.0, 0.0] and stat[1].tolist() == [1.0, 0.0, 0.0, 0.0]     # 0 rows; 1 row: M = 0
    assert stat[2, 0] == 2.0 and stat[2, 2] == 0.0 and not keep[off[2]:off[3]].any()      # 2 rows: equal means, tau = mu
    far = np.nonzero(np.abs(xyz).max(1) > 5)[0]
    assert len(far) == 10 and not keep[far].any() and keep[off[-2]:].mean() > 0.9


def test_mixed_segments_radius_count(mixed_run):
    xyz, off = _mixed()
    want = _reference()["count"]
    assert np.array_equal(mixed_run["count"], want) and mixed_run["count"].dtype == np.int32
    assert np.array_equal(mixed_run["rkeep"], want > 4)
    assert mixed_run["rstats"].tolist() == [513 + 700 + 1025 + 1500, 0]
    assert want[off[1]] == 1 and want.max() > 8
    _, count = _radius(torch.device("cuda:0"), xyz, off, RADIUS, 0)        # keep may be NULL in the ABI; nb_points = 0
    assert np.array_equal(count, want)


def test_switch_in_a_child_process(mixed_run, tmp_path):
    """CS_OUTLIER_GRID=0 in a process of its own: the exhaustive scan alone gives the bits of the default paths."""
    env = dict(os.environ)
    env["CS_OUTLIER_STATS"] = "1"
    env["CS_OUTLIER_GRID"] = "0"
    path = str(tmp_path / "scan.npz")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_outlier", path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    scan = dict(np.load(path))
    assert scan.keys() == mixed_run.keys()
    for name, v in scan.items():
        if "stats" in name:
            assert v.tolist() == [0, 0], name
        elif v.dtype == np.float64:
            _assert_bits(v, mixed_run[name], name)
        else:
            assert np.array_equal(v, mixed_run[name]), name


def test_lattice_ties_duplicates_and_non_finite_rows(gpu):
    g = np.stack(np.meshgrid(np.arange(11), np.arange(11), np.arange(10), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    assert len(g) == 1210                                       # on the mean-distance grid: every d2 ties with many
    dup = np.concatenate([_box(800, 1), _box(800, 1)[:400], np.tile(np.float32([[0.1, 0.2, 0.5]]), (25, 1))])     # on the grid too
    bad = _box(1100, 2)
    bad[5] = [np.nan, 0, 0]
    bad[600] = [0, np.inf, 0]
    bad[900] = [0, 0, -np.inf]
    small_bad = np.float32([[0, 0, 0], [np.nan, 1, 1], [1, 0, 0], [np.inf, 0, 0], [0, 1, 0]])
    parts = [g, dup, bad, small_bad, g[:200]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    for k in (8, 20):
        got = _mean(gpu, xyz, off, k)
        want = ref.knn_mean_dist(xyz, off, k)
        _assert_bits(got, want, "k = %d" % k)
        keep, stat = _stat(gpu, xyz, off, k, 1.0)
        wkeep, wstat = ref.outlier_statistical(want, off, 1.0)
        _assert_bits(stat, wstat)
        assert np.array_equal(keep, wkeep)
    assert np.isnan(got[off[2] + 5]) and np.isnan(got[off[3] + 1]) and got[off[2] + 6] > 0
    assert (got[off[1] + 1200:off[2]] == 0).all() and not keep[off[1] + 1200:off[2]].any()      # 25 copies, k = 20: mean 0
    assert stat[2, 0] == 1097 and stat[3, 0] == 3
    for radius in (2.0, float(np.nextafter(2.0, 3.0)), 0.2):
        keep, count = _radius(gpu, xyz, off, radius, 6)
        wkeep, wcount = ref.outlier_radius(xyz, off, radius, 6)
        assert np.array_equal(count, wcount) and np.array_equal(keep, wkeep), radius
    assert count[off[2] + 5] == 0 and count[off[3] + 3] == 0


def test_far_coordinates_and_extreme_radii(gpu):
    a = _box(1100, 3) + np.float32([70.0, -70.0, 0.0])
    b = _box(1100, 4) + np.float32([1.0e6, 0.0, 0.0])           # a cell index would reach the clamp: the gated scan answers
    c = _box(40, 5) * np.float32(1.0e6)
    one = np.tile(np.float32([[0.3, -0.2, 0.9]]), (1100, 1))     # a box of size zero: off the grid on the device
    one[7] = [np.nan, 0, 0]
    parts = [a, b, c, one]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    got = _mean(gpu, xyz, off, 16)
    _assert_bits(got, ref.knn_mean_dist(xyz, off, 16))
    keep, count = _radius(gpu, xyz, off, 0.15, 4)
    assert np.array_equal(count, ref.radius_count(xyz, off, 0.15))
    _, count = _radius(gpu, xyz, off, 1e150, 4)                  # the grid with a cell of 1e150: every finite row
    assert count.tolist() == [1100] * 2200 + [40] * 40 + [1099] * 7 + [0] + [1099] * 1092
    _, big = _radius(gpu, xyz, off, 1e160, 4)                    # the square overflows
    assert np.array_equal(big, count)
    keep, none = _radius(gpu, xyz, off, 1e-170, 0)               # the square underflows: not even the row itself
    assert not none.any() and not keep.any()


def test_permutation_and_launch_shape_leave_the_statistic_alone(gpu):
    xyz, flag = OC.clutter_cloud(3)
    n = len(xyz)
    perm = np.random.default_rng(8).permutation(n)
    keep, stat = _stat(gpu, xyz, [0, n], 20, 2.0)
    mean = _mean(gpu, xyz, [0, n], 20)
    pkeep, pstat = _stat(gpu, xyz[perm], [0, n], 20, 2.0)
    _assert_bits(pstat, stat)
    assert np.array_equal(pkeep, keep[perm])
    _assert_bits(_mean(gpu, xyz[perm], [0, n], 20), mean[perm])
    rk, rc = _radius(gpu, xyz, [0, n], 2.5 * OC.VOXEL, 4)
    prk, prc = _radius(gpu, xyz[perm], [0, n], 2.5 * OC.VOXEL, 4)
    assert np.array_equal(prc, rc[perm]) and np.array_equal(prk, rk[perm])
    # the same segment embedded among others, on another stream: other launch sizes, other workgroups, the same bits
    other, _ = _mixed()
    both = np.concatenate([other[:1400], xyz[perm], other[1400:3000], xyz])
    off = [0, 1400, 1400 + n, 3000 + n, 3000 + 2 * n]
    st = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(st):
        bkeep, bstat = _stat(gpu, both, off, 20, 2.0)
        st.synchronize()
    _assert_bits(bstat[1:2], stat)
    _assert_bits(bstat[3:4], stat)
    assert np.array_equal(bkeep[off[3]:], keep) and np.array_equal(bkeep[off[1]:off[2]], keep[perm])


def test_refusals(gpu):
    from corsair_amd import _lib, backend as B
    from corsair_amd._lib import CorsairHipError, i64_array, ptr, stream_ptr

    x = torch.zeros((8, 3), device=gpu)
    for k in (1, 33):
        with pytest.raises(CorsairHipError, match="k outside"):
            B.knn_mean_dist(x, [0, 8], k)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CorsairHipError, match="radius"):
            B.outlier_radius(x, [0, 8], r, 4)
    with pytest.raises(CorsairHipError, match="nb_points"):
        B.outlier_radius(x, [0, 8], 0.1, -1)
    for r in (-0.5, float("nan"), float("inf")):
        with pytest.raises(CorsairHipError, match="std_ratio"):
            B.outlier_statistical(x, [0, 8], 20, r)
    with pytest.raises(ValueError, match="offset table"):
        B.knn_mean_dist(x, [0, 9], 20)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        B.outlier_radius(torch.zeros((8, 2), device=gpu), [0, 8], 0.1, 4)
    lib = _lib.load()
    m = torch.zeros(8, dtype=torch.float64, device=gpu)
    assert lib.cs_knn_mean_dist(None, i64_array([0, 8]), 1, 20, ptr(m), stream_ptr()) < 0          # a null pointer with rows
    assert b"NULL" in lib.cs_last_error()
    assert lib.cs_outlier_radius(ptr(x), i64_array([0, 8]), 1, 0.1, 4, None, None, stream_ptr()) < 0
    assert lib.cs_outlier_statistical(ptr(m), i64_array([0, 8]), 1, 2.0, None, ptr(m), stream_ptr()) < 0
    assert lib.cs_outlier_statistical(None, i64_array([0, 8]), 1, 2.0, ptr(m), ptr(m), stream_ptr()) < 0
    idx, off = B.select_rows(torch.tensor([1, 0, 1, 1, 0, 0, 1, 0], dtype=torch.bool, device=gpu), [0, 3, 3, 8])
    assert idx.tolist() == [0, 2, 3, 6] and off == [0, 2, 2, 4] and idx.dtype == torch.int64


def test_profile_scope(gpu):
    from corsair_amd import _lib

    xyz, off = _mixed()
    x = torch.from_numpy(xyz).to(gpu)
    from corsair_amd import backend as B

    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        B.knn_mean_dist(x, off, 20)
        torch.cuda.synchronize()
        assert _lib.prof_get("outlier")[1] == 1
        B.outlier_statistical(x, off, 20, 2.0)
        B.outlier_radius(x, off, RADIUS, 4)
        torch.cuda.synchronize()
        ms, n, units = _lib.prof_get("outlier")
        assert _lib.prof_get("normals")[1] == 0
    finally:
        _lib.prof_enable(False)
    assert n == 4 and ms > 0 and units > 0                 # one scope per call


def test_clutter_fixture_masks(gpu):
    """The three real clouds with clutter in one call: the masks of the restatement, which tests/test_outlier_cpu.py shows
    to drop every clutter row."""
    xyz, off, flag = OC.packed()
    want_mean = ref.knn_mean_dist(xyz, off, 20)
    _assert_bits(_mean(gpu, xyz, off, 20), want_mean)
    keep, stat = _stat(gpu, xyz, off, 20, 2.0)
    wkeep, wstat = ref.outlier_statistical(want_mean, off, 2.0)
    _assert_bits(stat, wstat)
    assert np.array_equal(keep, wkeep) and not keep[flag].any() and (~keep[~flag]).sum() == 2
    rkeep, count = _radius(gpu, xyz, off, 2.5 * OC.VOXEL, 4)
    wrkeep, wcount = ref.outlier_radius(xyz, off, 2.5 * OC.VOXEL, 4)
    assert np.array_equal(count, wcount) and np.array_equal(rkeep, wrkeep)
    assert not rkeep[flag].any() and rkeep[~flag].all()


def _rows(a):
    return {r.tobytes() for r in np.ascontiguousarray(a, np.float32)}


def test_harness_cleans_raw_scans_only_when_configured(gpu):
    from corsair_amd import _lib, harness, synth

    sd, emb = synth.make_state_dicts(31)
    clouds = [OC.clutter_cloud(i)[0].astype(np.float64) for i in OC.CLOUDS]      # f64, as posed queries arrive
    flags = [OC.clutter_cloud(i)[1] for i in OC.CLOUDS]
    plain = harness.Pipeline(sd, emb, device=gpu)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        base = plain.embed_clouds(clouds)
        same = plain.embed_clouds(clouds, scan_filter=True)          # the default Config names no filter
        torch.cuda.synchronize()
        assert _lib.prof_get("outlier")[1] == 0                       # nothing new was launched
    finally:
        _lib.prof_enable(False)
    assert base.offsets == [0] + np.cumsum([len(c) for c in clouds]).tolist()      # every row is a voxel of its own
    assert same.offsets == base.offsets
    for a, b in ((base.F, same.F), (base.origin, same.origin), (base.desc, same.desc)):
        assert torch.equal(a, b)
    assert plain.scan_filter_stat == {"rows_in": 0, "rows_kept": 0, "clouds_skipped": 0}
    pipe = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(scan_filter="statistical"))
    unfiltered = pipe.embed_clouds(clouds)                            # the catalog's call: scan_filter stays False
    assert unfiltered.offsets == base.offsets and torch.equal(unfiltered.F, base.F)
    got = pipe.embed_clouds(clouds, scan_filter=True)
    origin = got.origin.cpu().numpy()
    kept = 0
    for p, (c, f) in enumerate(zip(clouds, flags)):
        seg = origin[got.offsets[p]:got.offsets[p + 1]]
        want, _ = ref.outlier_statistical(ref.knn_mean_dist(c, [0, len(c)], 20), [0, len(c)], 2.0)
        assert not (_rows(seg) & _rows(c[f])), "a clutter row reached the network"
        assert _rows(seg) == _rows(c[want]) and len(seg) == int(want.sum())
        kept += len(seg)
    assert got.offsets[-1] == kept == got.F.shape[0] == origin.shape[0] and got.desc.shape[0] == 3
    assert pipe.scan_filter_stat == {"rows_in": base.offsets[-1], "rows_kept": kept, "clouds_skipped": 0}
    # a 12-row cloud that the filter would reduce to 9 keeps all 12
    vox = harness.Config().voxel_size
    grid9 = np.array([[i, j, 0] for i in range(3) for j in range(3)], np.float64)
    lone = np.array([[40, 0, 0], [0, 40, 0], [0, 0, 40]], np.float64)
    tiny = ((np.concatenate([grid9, lone]) + 0.5) * vox).astype(np.float32).astype(np.float64)
    rpipe = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(scan_filter="radius"))
    keep, _ = ref.outlier_radius(tiny, [0, 12], 2.5 * vox, 4)
    assert keep.tolist() == [True] * 9 + [False] * 3
    got = rpipe.embed_clouds([clouds[1], tiny], scan_filter=True)
    assert got.offsets[2] - got.offsets[1] == 12
    assert _rows(got.origin[got.offsets[1]:].cpu().numpy()) == _rows(tiny)
    rk, _ = ref.outlier_radius(clouds[1], [0, len(clouds[1])], 2.5 * vox, 4)
    assert got.offsets[1] == int(rk.sum()) == OC.ROWS[3][0]
    assert rpipe.scan_filter_stat == {"rows_in": len(clouds[1]) + 12, "rows_kept": int(rk.sum()) + 12, "clouds_skipped": 1}


if __name__ == "__main__":
    np.savez(sys.argv[1], **_run_mixed(torch.device("cuda:0")))
