"""The outlier filters without a GPU: tests/outlier_ref.py (the bit-exact restatement of cs_knn_mean_dist,
cs_outlier_statistical and cs_outlier_radius that the GPU tests compare with) against a float implementation (cKDTree,
mean, std(ddof=1), query_ball_point) on three bundled real clouds with clutter, the integer statistic against exact
rational arithmetic, the defined cases of the header, the ABI's refusals and Config.check_scan_filter."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import outlier_cases as OC
from tests import outlier_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, STD, RADIUS, MIN_NB = 20, 2.0, 2.5 * OC.VOXEL, 4
_means = {}


def _mean(i):
    if i not in _means:
        xyz, _ = OC.clutter_cloud(i)
        _means[i] = ref.knn_mean_dist(xyz, [0, len(xyz)], K)
    return _means[i]


@pytest.mark.parametrize("i", OC.CLOUDS)
def test_fixture_is_the_stated_one(i):
    xyz, flag = OC.clutter_cloud(i)
    assert (int((~flag).sum()), int(flag.sum())) == OC.ROWS[i]
    assert xyz.dtype == np.float32 and np.isfinite(xyz).all()


@pytest.mark.parametrize("i", OC.CLOUDS)
def test_statistical_against_the_float_implementation(i):
    """Means to 1e-12, mu and sigma to 1e-8 relative (the 31-bit quantisation costs about 1e-10: measured 1.5e-10 at most
    on these clouds), identical masks; no mean lies within 1.5 % of tau, so rounding cannot flip a row.  Statistical 20 / 2.0
    drops every clutter row and at most 1 % of the real rows (0, 2 and 0 here)."""
    xyz, flag = OC.clutter_cloud(i)
    off = [0, len(xyz)]
    want_keep, want_mean, mu, sigma, tau = OC.float_statistical(xyz, K, STD)
    mean = _mean(i)
    assert np.max(np.abs(mean - want_mean) / want_mean) < 1e-12
    keep, stat = ref.outlier_statistical(mean, off, STD)
    print("cloud %d: mu %.3g (rel %.2g) sigma %.3g (rel %.2g)" % (i, stat[0, 1], abs(stat[0, 1] - mu) / mu, stat[0, 2],
                                                                   abs(stat[0, 2] - sigma) / sigma))
    assert stat[0, 0] == len(xyz)
    assert abs(stat[0, 1] - mu) <= 1e-8 * mu and abs(stat[0, 2] - sigma) <= 1e-8 * sigma
    assert abs(stat[0, 3] - tau) <= 1e-8 * tau
    assert np.min(np.abs(want_mean - tau)) > 0.015 * tau, "fixture changed: a mean lies within 1.5 % of tau"
    assert np.array_equal(keep, want_keep)
    assert not keep[flag].any(), "a clutter row survived"
    dropped_real = int((~keep[~flag]).sum())
    assert dropped_real <= 0.01 * (~flag).sum()
    assert dropped_real == {0: 0, 3: 2, 5: 0}[i]


@pytest.mark.parametrize("i", OC.CLOUDS)
def test_radius_against_the_float_implementation(i):
    """Identical counts and masks; no pair lies within 3e-6 relative of the radius.  Radius 2.5 voxels / 4 drops every
    clutter row and no real row."""
    xyz, flag = OC.clutter_cloud(i)
    want_count, dist = OC.float_radius(xyz, RADIUS)
    assert np.min(np.abs(dist - RADIUS)) > 3e-6 * RADIUS, "fixture changed: a pair lies within 3e-6 of the radius"
    keep, count = ref.outlier_radius(xyz, [0, len(xyz)], RADIUS, MIN_NB)
    assert np.array_equal(count, want_count)
    assert np.array_equal(keep, want_count > MIN_NB)
    assert not keep[flag].any() and keep[~flag].all()


@pytest.mark.parametrize("i", OC.CLOUDS)
def test_sigma_from_the_integer_sums_is_exact_to_1e15(i):
    """sigma of the header's sequence against fractions.Fraction arithmetic on the same q_i."""
    n, M, s, q = ref.quantise(_mean(i))
    _, mu, sigma, _ = ref.finish(n, M, s, q, STD)
    fq = [Fraction(v) for v in q]
    m = sum(fq) / n
    var = sum((v - m) ** 2 for v in fq) / (n - 1)
    scale = Fraction(2) ** -s
    # the square root of the exact rational, by an integer square root with 200 extra bits
    root = Fraction(math.isqrt((var.numerator << 400) // var.denominator), 1 << 200) * scale
    assert abs(Fraction(sigma) - root) <= Fraction(1, 10 ** 15) * root
    assert abs(Fraction(mu) - m * scale) <= Fraction(1, 10 ** 15) * m * scale
    assert max(q) <= 1 << 31 and max(q) > 1 << 30


def test_defined_cases_of_the_statistic():
    nan = float("nan")
    # M = 0: everything is 0 and nothing is kept
    keep, stat = ref.outlier_statistical(np.zeros(5), [0, 5], 2.0)
    assert stat.tolist() == [[5.0, 0.0, 0.0, 0.0]] and not keep.any()
    # n_valid = 0, 1, 2; an empty segment in between
    keep, stat = ref.outlier_statistical(np.array([nan, nan, 3.0, nan, 1.0, 2.0]), [0, 2, 2, 4, 6], 2.0)
    assert stat[0].tolist() == [0.0, 0.0, 0.0, 0.0] and stat[1].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert stat[2].tolist() == [1.0, 3.0, 0.0, 3.0]                        # sigma = 0: tau = mu, the strict test drops the row
    assert stat[3, 0] == 2.0 and stat[3, 1] == 1.5 and abs(stat[3, 2] - math.sqrt(0.5)) < 1e-9
    assert keep.tolist() == [False, False, False, False, True, True]
    # inf and negative means are not valid; std_ratio = 0 keeps the rows strictly below the mean
    keep, stat = ref.outlier_statistical(np.array([1.0, 2.0, 4.0, float("inf"), -1.0]), [0, 5], 0.0)
    assert stat[0, 0] == 3.0 and keep.tolist() == [True, True, False, False, False]
    # the shift where 2^s would leave the f64 range
    assert ref.shift_of(2.0 ** -1000) == 1023 and ref.shift_of(1.0) == 30 and ref.shift_of(0.0) == 31
    assert ref.shift_of(0.75) == 31 and ref.shift_of(3.0e38) == 31 - 128


def test_defined_cases_of_the_mean_distance():
    seg = np.float32([[0, 0, 0], [1, 0, 0], [3, 0, 0]])
    m = ref.knn_mean_dist(seg, [0, 3], 8)                                   # k above the segment's rows: c = 3
    assert m.tolist() == [(0.0 + 1.0 + 3.0) / 3.0, (0.0 + 1.0 + 2.0) / 3.0, (0.0 + 2.0 + 3.0) / 3.0]
    assert ref.knn_mean_dist(seg, [0, 3], 2).tolist() == [0.5, 0.5, 1.0]
    # k or more copies of one point get mean 0 and are dropped ([O3D-knowledge])
    dup = np.float32([[1, 2, 3]] * 4 + [[5, 5, 5], [5, 5, 6], [5, 6, 5], [6, 5, 5]])
    m = ref.knn_mean_dist(dup, [0, 8], 4)
    assert m[:4].tolist() == [0.0] * 4 and (m[4:] > 0).all()
    keep, _ = ref.outlier_statistical(m, [0, 8], 10.0)
    assert keep.tolist() == [False] * 4 + [True] * 4
    # a row with a non-finite coordinate finds nothing and is found by nobody
    bad = np.float32([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [np.inf, 0, 0]])
    m = ref.knn_mean_dist(bad, [0, 4], 3)
    assert m[0] == 0.5 and m[2] == 0.5 and np.isnan(m[1]) and np.isnan(m[3])
    assert m[1:2].view(np.uint64)[0] == 0x7FF8000000000000
    assert ref.knn_mean_dist(np.zeros((0, 3), np.float32), [0, 0, 0], 2).shape == (0,)


def test_strict_radius_on_the_integer_lattice():
    g = np.stack(np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    centre = int(np.nonzero((g == (3, 3, 2)).all(1))[0][0])
    _, count = ref.outlier_radius(g, [0, len(g)], 2.0, 4)
    assert count[centre] == 27                              # d2 in {0, 1, 2, 3}; the six rows at distance exactly 2 are outside
    assert ref.radius_count(g, [0, len(g)], np.nextafter(2.0, 3.0))[centre] == 33
    assert ref.radius_count(g, [0, len(g)], 1e-200).tolist() == [0] * len(g)       # the square underflows: nothing
    few = np.float32([[0, 0, 0], [1e6, 70, 0], [np.nan, 0, 0], [3e38, 0, 0]])
    assert ref.radius_count(few, [0, 4], 1e160).tolist() == [3, 3, 0, 3]         # the square overflows: the finite rows
    keep, _ = ref.outlier_radius(g[:3], [0, 3], 1.5, 2)
    assert keep.tolist() == [False, True, False]           # counts 2, 3, 2: kept with MORE than nb_points


def test_surface_is_declared():
    from corsair_amd import _lib, backend as B

    names = {"cs_knn_mean_dist", "cs_outlier_statistical", "cs_outlier_radius", "cs_outlier_stats"}
    assert names <= set(_lib.header_symbols())
    header = open(os.path.join(ROOT, "include", "corsair_hip.h")).read()
    for word in ("remove_statistical_outlier", "remove_radius_outlier", "CS_OUTLIER_GRID", "CS_OUTLIER_STATS", '"outlier"',
                 "S2lo", "tau = fma(std_ratio, sigma, mu)"):
        assert word in header, word
    for f in ("knn_mean_dist", "outlier_statistical", "outlier_radius", "outlier_stats", "select_rows"):
        assert callable(getattr(B, f)), f
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    text = open(os.path.join(csrc, "outlier.hip")).read()
    assert '#include "normals_grid.h"' in text and "cg_probe<" in text and "nrm_grid_build(" in text
    assert "q = floor(" not in text                          # the cell function lives in the shared header alone
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "outlier.hip" in make and "outlier.o: nn_common.h cellgrid.h normals_grid.h" in make


def test_library_exports_and_refusals_without_a_device():
    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    sigs = _lib._declare(lib)
    assert {"cs_knn_mean_dist", "cs_outlier_statistical", "cs_outlier_radius", "cs_outlier_stats"} <= set(sigs)
    off0 = (ctypes.c_int64 * 2)(0, 0)
    one = (ctypes.c_int64 * 2)(0, 4)
    bad = (ctypes.c_int64 * 2)(5, 2)
    nan, inf = float("nan"), float("inf")
    # argument checks come before any device work: an empty call needs no GPU
    mean = lib.cs_knn_mean_dist
    assert mean(None, off0, 0, 20, None, None) == 0 and mean(None, off0, 1, 20, None, None) == 0
    for k in (1, 33, 0, -1):
        assert mean(None, off0, 1, k, None, None) < 0
        assert b"k outside [2, 32]" in lib.cs_last_error()
    assert mean(None, None, 1, 20, None, None) < 0 and mean(None, off0, -1, 20, None, None) < 0
    assert mean(None, bad, 1, 20, None, None) < 0 and mean(None, one, 1, 20, None, None) < 0
    stat = lib.cs_outlier_statistical
    assert stat(None, off0, 0, 2.0, None, None, None) == 0
    for r in (-1.0, -1e-300, nan, inf):
        assert stat(None, off0, 0, r, None, None, None) < 0
        assert b"std_ratio" in lib.cs_last_error()
    assert stat(None, None, 1, 2.0, None, None, None) < 0 and stat(None, bad, 1, 2.0, None, None, None) < 0
    assert stat(None, one, 1, 2.0, None, None, None) < 0 and stat(None, off0, 1, 2.0, None, None, None) < 0    # NULL d_stat
    rad = lib.cs_outlier_radius
    assert rad(None, off0, 0, 0.1, 4, None, None, None) == 0 and rad(None, off0, 1, 0.1, 0, None, None, None) == 0
    for r in (0.0, -1.0, nan, inf, -inf):
        assert rad(None, off0, 1, r, 4, None, None, None) < 0
        assert b"radius" in lib.cs_last_error()
    assert rad(None, off0, 1, 0.1, -1, None, None, None) < 0
    assert rad(None, None, 1, 0.1, 4, None, None, None) < 0 and rad(None, one, 1, 0.1, 4, None, None, None) < 0
    out = (ctypes.c_uint64 * 2)(7, 7)
    lib.cs_outlier_stats(out, 1)
    assert (out[0], out[1]) == (0, 0)


def test_config_scan_filter_defaults_and_refusals():
    from corsair_amd import harness as H

    c = H.Config()
    assert (c.scan_filter, c.scan_filter_k, c.scan_filter_std, c.scan_filter_radius, c.scan_filter_min_nb) == \
        ("none", 20, 2.0, 2.5, 4)
    c.check_scan_filter()
    H.Config(scan_filter="statistical", scan_filter_k=2, scan_filter_std=0.0).check_scan_filter()
    H.Config(scan_filter="radius", scan_filter_min_nb=0).check_scan_filter()
    for kw, word in ((dict(scan_filter="median"), "scan_filter"), (dict(scan_filter_k=1), "scan_filter_k"),
                     (dict(scan_filter_k=33), "scan_filter_k"), (dict(scan_filter_k=2.5), "scan_filter_k"),
                     (dict(scan_filter_k=True), "scan_filter_k"), (dict(scan_filter_std=-0.1), "scan_filter_std"),
                     (dict(scan_filter_std=float("nan")), "scan_filter_std"),
                     (dict(scan_filter_std=float("inf")), "scan_filter_std"),
                     (dict(scan_filter_radius=0.0), "scan_filter_radius"),
                     (dict(scan_filter_radius=float("nan")), "scan_filter_radius"),
                     (dict(scan_filter_radius=float("inf")), "scan_filter_radius"),
                     (dict(scan_filter_min_nb=-1), "scan_filter_min_nb"), (dict(scan_filter_min_nb=1.5), "scan_filter_min_nb")):
        with pytest.raises(ValueError, match=word):
            H.Config(**kw).check_scan_filter()
    base = ["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"]
    a = H.build_parser().parse_args(base)
    assert (a.scan_filter, a.scan_filter_k, a.scan_filter_std, a.scan_filter_radius, a.scan_filter_min_nb) == \
        ("none", 20, 2.0, 2.5, 4)
    a = H.build_parser().parse_args(base + ["--scan-filter", "radius", "--scan-filter-k", "16", "--scan-filter-std", "1.5",
                                            "--scan-filter-radius", "3", "--scan-filter-min-nb", "6"])
    assert (a.scan_filter, a.scan_filter_k, a.scan_filter_std, a.scan_filter_radius, a.scan_filter_min_nb) == \
        ("radius", 16, 1.5, 3.0, 6)
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "--scan-filter" in readme and "**untuned, no real scan measured**" in readme
