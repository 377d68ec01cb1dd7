"""The support-plane step without a GPU: tests/plane_ref.py (the bit-exact restatement of cs_segment_plane that the GPU tests
compare with) against an independent float implementation on three real clouds standing on a floor, the fixture's table, why
the step exists (DBSCAN alone keeps floor and patch), the limit without an up direction, the defined cases of the header,
harness.is_support_plane, Config.check_scan_plane, the parser, the sources and the ABI's refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import dbscan_ref
from tests import outlier_cases as OC
from tests import plane_cases as PC
from tests import plane_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST, ITERS = 1.0 * PC.VOXEL, 1024
# the restatement at seed 0, 1 voxel, 1 024 hypotheses: stat, real rows lost, clutter rows lost
TABLE = {0: ([1, 429, 1135, 1, 1116, 2370, 7, 3493], 24, 7),
         3: ([1, 648, 623, 1, 606, 1069, 3, 1678], 30, 1),
         5: ([1, 473, 1579, 1, 1546, 1308, 1, 2855], 251, 5)}
MAX_REAL_LOSS = {0: 0.05, 3: 0.05, 5: 0.20}     # the chairs; the table, whose base slab lies in the floor's band
_runs = {}


def _counts(maker, i, seed):
    key = (maker.__name__, i, seed)
    if key not in _runs:
        _runs[key] = ref.counts(maker(i)[0], DIST, ITERS, seed)
    return _runs[key]


def _run(maker, i, seed=0, iters=ITERS):
    return ref.segment_plane_one(maker(i)[0], DIST, iters, seed, count=_counts(maker, i, seed))


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.degrees(math.acos(min(1.0, abs(float(a @ b)) / float(np.linalg.norm(a) * np.linalg.norm(b)))))


def _cfg(**kw):
    from corsair_amd import harness as H

    return H, H.Config(**kw)


@pytest.mark.parametrize("i", PC.CLOUDS)
def test_restatement_against_float_implementation(i):
    xyz, _ = PC.floor_cloud(i)
    plane, stat, inl = _run(PC.floor_cloud, i)
    triples = [ref.triple(0, t, len(xyz)) for t in range(ITERS)]
    t, mask, normal, centroid, gap = PC.float_plane(xyz, DIST, ITERS, 0, triples)
    assert gap > 1e-9                                   # no row's s^2 within a relative 1e-9 of a bound: roundings decide nothing
    assert stat[1] == t and np.array_equal(mask, inl)
    assert _angle(normal, plane[:3]) < 1e-3             # measured 5e-5 .. 1.8e-4 degrees
    assert abs(float(np.dot(plane[:3], centroid)) + plane[3]) < 1e-6
    assert abs(math.sqrt(sum(v * v for v in plane[:3])) - 1.0) < 1e-15


@pytest.mark.parametrize("i", PC.CLOUDS)
def test_fixture_table(i):
    H, cfg = _cfg()
    xyz, kind = PC.floor_cloud(i)
    assert (len(xyz), int((kind == PC.FLOOR).sum())) == PC.ROWS[i]
    plane, stat, inl = _run(PC.floor_cloud, i)
    assert stat == TABLE[i][0]
    assert (int(((kind == PC.REAL) & inl).sum()), int(((kind == PC.CLUTTER) & inl).sum())) == TABLE[i][1:]
    fl = xyz[kind == PC.FLOOR].astype(np.float64)
    floor_normal = np.linalg.eigh(np.cov((fl - fl.mean(0)).T))[1][:, 0]
    real = int((kind == PC.REAL).sum())
    for seed in range(4):                               # the conditions hold for every seed and both budgets
        for iters in (256, ITERS):
            plane, stat, inl = _run(PC.floor_cloud, i, seed, iters)
            found, _, _, _, final, n_pos, n_neg, finite = stat
            assert found and finite == len(xyz)
            assert not ((kind == PC.FLOOR) & ~inl).any()                                  # no floor row survives
            assert int(((kind == PC.REAL) & inl).sum()) <= MAX_REAL_LOSS[i] * real
            assert n_neg / (n_pos + n_neg) < 0.01 and final / finite >= 0.3
            assert _angle(floor_normal, plane[:3]) < 1.0
            assert plane[2] > 0.99                                                        # towards the object
            assert H.is_support_plane(stat, plane, cfg)


@pytest.mark.parametrize("i", PC.CLOUDS)
def test_why_the_step_exists(i):
    """DBSCAN alone keeps every floor and patch row; after the plane step it keeps neither, nor clutter."""
    xyz, kind = PC.floor_patch_cloud(i)
    eps = 2.5 * PC.VOXEL
    label, _, _ = dbscan_ref.dbscan(xyz, [0, len(xyz)], eps, 5)
    keep, _ = dbscan_ref.cluster_largest(label, [0, len(xyz)])
    assert keep[kind == PC.FLOOR].all() and keep[kind == PC.PATCH].all()
    H, cfg = _cfg()
    plane, stat, inl = _run(PC.floor_patch_cloud, i)
    assert H.is_support_plane(stat, plane, cfg)
    rest = np.nonzero(~inl)[0]
    label, _, _ = dbscan_ref.dbscan(xyz[rest], [0, len(rest)], eps, 5)
    keep, _ = dbscan_ref.cluster_largest(label, [0, len(rest)])
    left = kind[rest[keep]]
    assert not (left == PC.FLOOR).any() and not (left == PC.PATCH).any() and not (left == PC.CLUTTER).any()
    assert (left == PC.REAL).sum() >= 0.85 * (kind == PC.REAL).sum()            # measured 99.6 %, 100 %, 87.5 %


def _bare(i):
    return OC.clutter_cloud(i)[0], None


def test_without_a_floor_and_the_limit_of_the_rule():
    H, cfg = _cfg()
    for i in (0, 3):                                    # the chairs: rows on both sides of every plane, rule (b) fails
        plane, stat, _ = _run(_bare, i)
        assert stat[0] == 1 and stat[6] / (stat[5] + stat[6]) > 0.05
        assert not H.is_support_plane(stat, plane, cfg)
    # THE LIMIT: a bare table seen from above is one-sided like a floor and loses its top without a hint of what is up
    plane, stat, _ = _run(_bare, 5)
    assert stat[6] <= 2 and stat[5] > 1000 and plane[2] < -0.99
    assert H.is_support_plane(stat, plane, cfg)
    assert not H.is_support_plane(stat, plane, H.Config(scan_plane_up=(0.0, 0.0, 1.0)))
    # the floor under the same table passes with the hint
    plane, stat, _ = _run(PC.floor_cloud, 5)
    assert H.is_support_plane(stat, plane, H.Config(scan_plane_up=(0.0, 0.0, 2.0)))
    assert not H.is_support_plane(stat, plane, H.Config(scan_plane_up=(1.0, 0.0, 0.0)))


def test_is_support_plane_rules():
    H, cfg = _cfg()
    up = (0.0, 0.0, 1.0)
    assert not H.is_support_plane([0, -1, 0, 0, 0, 0, 0, 50], [0.0] * 4, cfg)
    assert H.is_support_plane([1, 0, 20, 1, 20, 80, 0, 100], [0, 0, 1, 0], cfg)
    assert not H.is_support_plane([1, 0, 20, 1, 19, 81, 0, 100], [0, 0, 1, 0], cfg)       # (a) 19 < 0.2 * 100
    assert H.is_support_plane([1, 0, 20, 1, 50, 49, 1, 100], [0, 0, 1, 0], cfg)           # (b) 1 <= 0.02 * 50
    assert not H.is_support_plane([1, 0, 20, 1, 50, 48, 2, 100], [0, 0, 1, 0], cfg)
    tilt = lambda deg: [math.sin(math.radians(deg)), 0.0, math.cos(math.radians(deg)), 0.0]
    c = H.Config(scan_plane_up=up)
    assert H.is_support_plane([1, 0, 20, 1, 50, 50, 0, 100], tilt(29.9), c)
    assert not H.is_support_plane([1, 0, 20, 1, 50, 50, 0, 100], tilt(30.1), c)
    assert H.is_support_plane([1, 0, 20, 1, 50, 50, 0, 100], tilt(30.1), H.Config(scan_plane_up=up, scan_plane_max_tilt=31.0))


def lattice_case():
    """A 9 x 9 lattice in z = 0 (spacing 0.25) and five rows well off it."""
    g = np.arange(9) * 0.25
    lat = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3)
    off = [[0.5, 0.5, 1.0], [1.0, 0.25, 2.0], [0.25, 1.5, 0.75], [1.5, 1.5, 1.25], [0.75, 1.0, 3.0]]
    return np.float32(np.concatenate([lat, off]))


def tie_case():
    """Eight rows of the plane z = 0 and eight of the plane x = 5, three or more units above the first: a hypothesis inside
    one plane counts 8, and a mixed one at most a line of each."""
    g = np.float32([[0, 0], [1, 0], [0, 1], [1, 1], [2, 0], [0, 2], [2, 1], [1, 2]])
    a = np.concatenate([g, np.zeros((8, 1), np.float32)], 1)
    b = np.concatenate([np.full((8, 1), 5, np.float32), g[:, :1], g[:, 1:] + 3], 1)
    return np.concatenate([a, b])


def defined_cases():
    """name -> (rows f32 [m,3], dist, iters, seed); shared with tests/test_gpu_plane.py."""
    rng = np.random.default_rng(7)
    lat = lattice_case()
    bad = np.concatenate([lat, np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, -np.inf], [np.nan] * 3])])
    line = np.float32([[t, 2 * t, -t] for t in range(12)])
    cases = {
        "lattice": (lat, 0.1, 64, 0),
        "copies": (np.tile(np.float32([[0.25, -1.0, 3.0]]), (9, 1)), 0.1, 32, 0),
        "collinear": (line, 0.1, 32, 0),
        "rows0": (np.zeros((0, 3), np.float32), 0.1, 8, 0),
        "rows1": (lat[:1], 0.1, 8, 0),
        "rows2": (lat[:2], 0.1, 8, 0),
        "tie": (tie_case(), 0.05, 64, 3),
        "nonfinite": (bad[rng.permutation(len(bad))], 0.1, 64, 1),
        "dist_overflow": (lat, 1e160, 16, 0),
        "dist_underflow": (lat, 1e-170, 16, 0),
        "offset70": ((lat.astype(np.float64) + 70.0).astype(np.float32), 0.1, 64, 0),
        "offset1e6": ((lat.astype(np.float64) * 64 + 1e6).astype(np.float32), 4.0, 64, 0),
        "iters1": (PC.floor_cloud(3)[0], DIST, 1, 5),
    }
    return cases


def test_defined_cases():
    cases = defined_cases()
    out = {k: ref.segment_plane_one(*v) for k, v in cases.items()}
    plane, stat, inl = out["lattice"]
    assert [abs(v) for v in plane] == [0.0, 0.0, 1.0, 0.0] and plane[2] == 1.0           # exactly, oriented to the rows off it
    assert stat[0] == 1 and stat[2:] == [81, 1, 81, 5, 0, 86] and inl.tolist() == [True] * 81 + [False] * 5
    for name in ("copies", "collinear", "rows0", "rows1", "rows2", "dist_overflow", "dist_underflow"):
        plane, stat, inl = out[name]
        m = len(cases[name][0])
        assert plane == [0.0] * 4 and stat == [0, -1, 0, 0, 0, 0, 0, m] and not inl.any(), name
    # two planes of eight rows: the first hypothesis that counts 8 wins, not a later one
    rows, dist, iters, seed = cases["tie"]
    count = ref.counts(rows, dist, iters, seed)
    assert count.max() == 8 and (count == 8).sum() >= 2
    plane, stat, inl = out["tie"]
    first = int(np.nonzero(count == 8)[0][0])
    assert stat[1] == first and stat[2] == 8 and (count[:first] < 8).all()
    s64 = rows.astype(np.float64)
    sides = set()
    for t in np.nonzero(count == 8)[0]:
        o, n, _, bound = ref.hypothesis(s64, ref.triple(seed, int(t), len(rows)), dist * dist)
        sides.add(bool(ref.classify(s64, o, n, bound)[0][:8].all()))
    assert sides == {True, False}                        # both planes occur among the tied hypotheses
    # non-finite rows: never inliers, counted out of rows_finite, the plane is the lattice's
    rows = cases["nonfinite"][0]
    plane, stat, inl = out["nonfinite"]
    fin = np.isfinite(rows).all(1)
    assert stat[0] == 1 and stat[7] == 86 and stat[4] == 81 and not inl[~fin].any() and abs(plane[2]) == 1.0
    for name, z in (("offset70", 70.0), ("offset1e6", 1e6)):
        plane, stat, inl = out[name]
        assert stat[0] == 1 and stat[3] == 1 and stat[4] == 81 and plane[:3] == [0.0, 0.0, 1.0] and plane[3] == -z, name
    plane, stat, inl = out["iters1"]
    assert stat[1] in (0, -1) and (stat[0] == 0 or stat[2] >= 3)


def test_refit_is_free_of_the_order():
    xyz, _ = PC.floor_cloud(3)
    s64 = xyz.astype(np.float64)
    count = _counts(PC.floor_cloud, 3, 0)
    t = int(np.argmax(count))
    o, n_s, nn, bound = ref.hypothesis(s64, ref.triple(0, t, len(xyz)), DIST * DIST)
    inl = ref.classify(s64, o, n_s, bound)[0]
    want = ref.refit(s64, inl, o, n_s, nn)
    perm = np.random.default_rng(1).permutation(len(xyz))
    got = ref.refit(s64[perm], inl[perm], o, n_s, nn)
    assert want[2] == 1 and got == want                  # floats compared by value: the same bits (no NaN, no zero)
    # the generator is common.h's: the first draws of seed 0 on 1 000 rows, and every draw is in range
    assert all(0 <= v < 7 for t in range(200) for v in ref.triple(11, t, 7))
    assert ref.rng_u64(0, 0, 0) == 0xE220A8397B1DCDAF    # splitmix64's first output for seed 0


def test_config_parser_and_readme():
    H, c = _cfg()
    assert H.SCAN_FILTERS == ("none", "statistical", "radius", "cluster") and H.SCAN_PLANES == ("none", "remove")
    assert (c.scan_plane, c.scan_plane_dist, c.scan_plane_iters, c.scan_plane_min_share, c.scan_plane_max_below,
            c.scan_plane_up, c.scan_plane_max_tilt) == ("none", 1.0, 1024, 0.2, 0.02, None, 30.0)
    c.check_scan_plane()
    H.Config(scan_plane="remove", scan_plane_up=[0, 0, 1], scan_plane_max_tilt=90.0, scan_plane_iters=65536).check_scan_plane()
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(scan_plane="floor"), "scan_plane"), (dict(scan_plane_dist=0.0), "scan_plane_dist"),
                     (dict(scan_plane_dist=-1.0), "scan_plane_dist"), (dict(scan_plane_dist=nan), "scan_plane_dist"),
                     (dict(scan_plane_dist=inf), "scan_plane_dist"), (dict(scan_plane_iters=0), "scan_plane_iters"),
                     (dict(scan_plane_iters=65537), "scan_plane_iters"), (dict(scan_plane_iters=2.5), "scan_plane_iters"),
                     (dict(scan_plane_iters=True), "scan_plane_iters"), (dict(scan_plane_min_share=-0.1), "scan_plane_min_share"),
                     (dict(scan_plane_min_share=1.5), "scan_plane_min_share"), (dict(scan_plane_min_share=nan), "scan_plane_min_share"),
                     (dict(scan_plane_max_below=-0.1), "scan_plane_max_below"), (dict(scan_plane_max_below=nan), "scan_plane_max_below"),
                     (dict(scan_plane_up=(0, 0)), "scan_plane_up"), (dict(scan_plane_up=(0, 0, 0)), "scan_plane_up"),
                     (dict(scan_plane_up=(0, nan, 1)), "scan_plane_up"), (dict(scan_plane_up=(0, inf, 1)), "scan_plane_up"),
                     (dict(scan_plane_up="up"), "scan_plane_up"), (dict(scan_plane_up=1.0), "scan_plane_up"),
                     (dict(scan_plane_max_tilt=0.0), "scan_plane_max_tilt"), (dict(scan_plane_max_tilt=90.5), "scan_plane_max_tilt"),
                     (dict(scan_plane_max_tilt=nan), "scan_plane_max_tilt")):
        with pytest.raises(ValueError, match=word):
            H.Config(**kw).check_scan_plane()
    base = ["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"]
    a = H.build_parser().parse_args(base)
    assert (a.scan_plane, a.scan_plane_dist, a.scan_plane_iters, a.scan_plane_min_share, a.scan_plane_max_below,
            a.scan_plane_up, a.scan_plane_max_tilt) == ("none", 1.0, 1024, 0.2, 0.02, None, 30.0)
    a = H.build_parser().parse_args(base + ["--scan-plane", "remove", "--scan-plane-dist", "1.5", "--scan-plane-iters", "256",
                                            "--scan-plane-min-share", "0.3", "--scan-plane-max-below", "0.01",
                                            "--scan-plane-up", "0", "0", "1", "--scan-plane-max-tilt", "20",
                                            "--scan-filter", "cluster"])
    assert (a.scan_plane, a.scan_plane_dist, a.scan_plane_iters, a.scan_plane_min_share, a.scan_plane_max_below,
            a.scan_plane_up, a.scan_plane_max_tilt, a.scan_filter) == ("remove", 1.5, 256, 0.3, 0.01, [0.0, 0.0, 1.0], 20.0,
                                                                        "cluster")
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(base + ["--scan-plane-up", "0", "1"])
    help_text = " ".join(H.build_parser().format_help().split())
    assert help_text.count("untuned, no real scan measured") >= 2 + 7            # the cluster filter's two, and every flag here
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    at = readme.index("--scan-plane remove")
    para = readme[at:at + 3000]
    assert "untuned, no real scan measured" in para and "table top" in para and "--scan-plane-up" in para
    assert readme.index("--scan-filter cluster") < at


def test_source_layout():
    header = open(os.path.join(ROOT, "include", "corsair_hip.h")).read()
    assert "int cs_segment_plane(" in header and '"plane"' in header
    at = header.index("cs_segment_plane:")
    block = " ".join(header[at:header.index("int cs_segment_plane(")].split())
    for words in ("Differences from [O3D-knowledge] Open3D", "no probabilistic early exit", "strict", "fixed-point covariance",
                  "REFITTED", "ransac_n is 3", "ties to the SMALLEST t"):
        assert words in block, words
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    text = open(os.path.join(csrc, "plane.hip")).read()
    assert '#include "horn.h"' in text and "jacobi3(" in text and "rng_index(" in text
    assert not re.search(r"void jacobi\w*\(", text) and "sweep" not in text        # no Jacobi of its own
    for word in ("hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync"):
        assert word not in text, word
    assert "atomicAdd(" in text and "atomicMax(" in text and "atomicCAS" not in text and "hipStreamSynchronize" not in text
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "plane.hip" in make and "plane.o: horn.h" in make
    runtime = open(os.path.join(csrc, "runtime.hip")).read()
    assert '"plane"' in runtime


def test_library_exports_and_refusals_without_a_device():
    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    sigs = _lib._declare(lib)
    assert "cs_segment_plane" in sigs
    f = lib.cs_segment_plane
    off0 = (ctypes.c_int64 * 2)(0, 0)
    one = (ctypes.c_int64 * 2)(0, 4)
    bad = (ctypes.c_int64 * 2)(5, 2)
    neg = (ctypes.c_int64 * 2)(-1, 2)
    huge = (ctypes.c_int64 * 2)(0, 1 << 31)
    nan, inf = float("nan"), float("inf")
    INVALID, UNSUPPORTED = -1, -5
    # argument checks come before any device work: a call without segments needs no GPU
    assert f(None, off0, 0, 0.1, 1024, 0, None, None, None, None) == 0
    for d in (0.0, -1.0, nan, inf, -inf):
        assert f(None, off0, 0, d, 1024, 0, None, None, None, None) == INVALID
        assert b"dist" in lib.cs_last_error()
    for it in (0, -1, 65537):
        assert f(None, off0, 0, 0.1, it, 0, None, None, None, None) == INVALID
        assert b"iters" in lib.cs_last_error()
    assert f(None, off0, 0, 0.1, 65536, 2 ** 64 - 1, None, None, None, None) == 0
    assert f(None, None, 1, 0.1, 8, 0, None, None, None, None) == INVALID
    assert f(None, off0, -1, 0.1, 8, 0, None, None, None, None) == INVALID
    assert f(None, bad, 1, 0.1, 8, 0, None, None, None, None) == INVALID
    assert f(None, neg, 1, 0.1, 8, 0, None, None, None, None) == INVALID
    assert f(None, huge, 1, 0.1, 8, 0, None, None, None, None) == UNSUPPORTED
    assert f(None, off0, 1, 0.1, 8, 0, None, None, None, None) == INVALID          # NULL d_plane / d_stat with a segment
    buf = (ctypes.c_double * 8)()
    assert f(None, one, 1, 0.1, 8, 0, buf, buf, None, None) == INVALID              # NULL d_xyz / d_inlier while a row exists
    assert b"NULL" in lib.cs_last_error()
