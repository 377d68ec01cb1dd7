"""The hybrid (radius, max_nn) normals without a GPU: tests/normals_hybrid_ref.py (the bit-exact restatement of
cs_estimate_normals_hybrid the GPU tests compare with) against cKDTree.query_ball_point + sort + truncation +
numpy.linalg.eigh, the huge-radius and strict-threshold rules, and the ABI's refusals."""
import ctypes
import os

import numpy as np
import pytest

from tests import normals_hybrid_ref as href
from tests import normals_ref as ref
from tests.test_normals_cpu import _clouds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |sin| of the angle between the restated normal (f32) and eigh's eigenvector (f64) of the same neighbourhood: the largest
# value measured on the cases below is 4.2e-8 (the f32 cast, 2^-24 = 6e-8 per component, dominates); x10.
SIN_TOL = 4.2e-7
# (radius, max_nn) per surface: the smallest radius of a 0.01 raster at which every one of the 400 rows finds three
# neighbours and a well-conditioned neighbourhood (9 to 12 neighbours on average -- at the radius of 8 on average up to
# 2 % of the rows find fewer than three), and the radius of 16 to 17 on average, where max_nn = 16 truncates most rows.
CASES = {"box": ((0.22, 32), (0.25, 16)), "sphere": ((0.14, 32), (0.20, 16)), "cylinder": ((0.13, 32), (0.16, 16))}


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("shape", ("box", "sphere", "cylinder"))
def test_restatement_against_ball_query_and_eigh(shape, which):
    """Measured maximum of |sin| over the six cases: 4.2e-8 (cylinder, r = 0.16); asserted below SIN_TOL = 4.2e-7.  No row
    is skipped: every row's (l1 - l0) / l2 is asserted to lie above the 1e-3 at which a row could be left out."""
    from scipy.spatial import cKDTree

    radius, max_nn = CASES[shape][which]
    c = _clouds()[shape]
    got = href.estimate_normals(c, [0, len(c)], radius, max_nn).astype(np.float64)
    c64 = c.astype(np.float64)
    ball = cKDTree(c64).query_ball_point(c64, radius)
    worst, counts = 0.0, []
    for i in range(len(c)):
        d = np.linalg.norm(c64[ball[i]] - c64[i], axis=1)
        want = [j for _, j in sorted(zip(d.tolist(), ball[i]))][:max_nn]
        assert [j for _, j in href.neighbours(c, i, radius, max_nn)] == want          # the same neighbours, the same order
        assert len(want) >= 3
        counts.append(len(ball[i]))
        w, v = np.linalg.eigh(np.cov(c64[want].T, bias=True))
        assert (w[1] - w[0]) / w[2] >= 1e-3, "input chosen so that no row is skipped"
        worst = max(worst, float(np.linalg.norm(np.cross(got[i], v[:, 0]))))
        assert abs(np.linalg.norm(got[i]) - 1.0) < 1e-6
    print("max |sin| %s r=%.2f max_nn=%d: %.3g, neighbours inside the radius %.1f on average, %d at most"
          % (shape, radius, max_nn, worst, np.mean(counts), max(counts)))
    assert (max(counts) > max_nn) == (which == 1)
    assert worst < SIN_TOL


def _mixed(k):
    from tests.test_gpu_normals import _mixed as mixed

    return mixed(k)


@pytest.mark.parametrize("max_nn", (3, 16))
def test_huge_radius_is_knn(max_nn):
    xyz, off, want = _mixed(max_nn)
    got = href.estimate_normals(xyz, off, 1e150, max_nn)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    seg = xyz[off[-3]:off[-2]]                     # the 513-row segment: the lists themselves, distances included
    assert href.neighbours(seg, len(seg) - 5, 1e150, max_nn) == ref.neighbours(seg, len(seg) - 5, max_nn)


def test_strict_threshold_on_the_integer_grid():
    g = np.stack(np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    centre = int(np.nonzero((g == (3, 3, 2)).all(1))[0][0])
    nb = href.neighbours(g, centre, 2.0, 32)
    # d2 in {0, 1, 2, 3}: 1 + 6 + 12 + 8 rows; the six lattice rows at distance exactly 2 (d2 = 4) are outside
    assert len(nb) == 27 and max(d for d, _ in nb) == 3.0
    assert sorted(d for d, _ in href.neighbours(g, centre, np.nextafter(2.0, 3.0), 32))[-1] == 4.0
    # a radius whose square underflows finds nothing, not even the row itself
    assert href.neighbours(g, centre, 1e-200, 8) == []
    assert np.array_equal(href.estimate_normals(g[:9], [0, 9], 1e-200, 8), np.tile(np.float32([0, 0, 1]), (9, 1)))


def test_surface_is_declared():
    from corsair_amd import _lib, backend as B

    header = open(os.path.join(ROOT, "include", "corsair_hip.h")).read()
    assert {"cs_estimate_normals_hybrid", "cs_normals_stats"} <= set(_lib.header_symbols())
    for word in ("KDTreeSearchParamHybrid", "CS_NORMALS_GRID", "CS_NORMALS_STATS", "d2 < radius * radius"):
        assert word in header, word
    assert callable(B.normals_stats)
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    for unit in ("pairs.hip", "normals.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "cellgrid.h"' in text and "cg_probe<" in text, unit
        assert "q = floor(" not in text, unit           # the cell function lives in the shared header alone
    assert "q = floor(x / cell)" in open(os.path.join(csrc, "cellgrid.h")).read()
    assert "cellgrid.h" in open(os.path.join(csrc, "Makefile")).read()


def test_python_surfaces_keep_their_defaults():
    import inspect

    from corsair_amd import backend as B, harness as H, registration as R, shapenet_eval as S

    assert inspect.signature(B.estimate_normals).parameters["radius"].default is None
    assert inspect.signature(B.estimate_normals).parameters["k"].default == 16
    assert inspect.signature(R.sym_pose_batch).parameters["icp_normal_radius"].default is None
    for cfg in (H.Config(), S.Config()):
        assert cfg.icp_normal_radius == 0.0 and cfg.normal_radius() is None          # 0.0 = k-NN
    assert H.Config(icp_normal_radius=0.075).normal_radius() == 0.075
    assert S.Config(icp_normal_radius=0.075).normal_radius() == 0.075
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="icp_normal_radius"):
            H.Config(icp_normal_radius=bad).check_icp()
        with pytest.raises(ValueError, match="icp_normal_radius"):
            S.Config(icp_normal_radius=bad).normal_radius()
    base = ["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"]
    assert H.build_parser().parse_args(base).icp_normal_radius == 0.0
    assert H.build_parser().parse_args(base + ["--icp-normal-radius", "0.075"]).icp_normal_radius == 0.075
    sbase = ["--model-ckpt", "c", "--data-dir", "d"]
    assert S.build_parser().parse_args(sbase).icp_normal_radius == 0.0
    assert S.build_parser().parse_args(sbase + ["--icp-normal-radius", "0.075"]).icp_normal_radius == 0.075
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--icp-normal-radius" in readme and "**no radius has been tuned**" in " ".join(readme.split())
    assert "--normal-radius" in open(os.path.join(ROOT, "tools", "icp_bench.py")).read()


def test_library_exports_and_refusals_without_a_device():
    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.cs_estimate_normals_hybrid
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_double, ctypes.c_int,
                  ctypes.c_void_p, ctypes.c_void_p]
    off = (ctypes.c_int64 * 2)(0, 0)
    # argument checks come before any device work: an empty call needs no GPU
    assert f(None, off, 0, 0.1, 16, None, None) == 0
    assert f(None, off, 1, 0.1, 16, None, None) == 0          # one empty segment
    for max_nn in (2, 33, 0, -1):
        assert f(None, off, 1, 0.1, max_nn, None, None) < 0
    for radius in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert f(None, off, 1, radius, 16, None, None) < 0
    assert f(None, None, 1, 0.1, 16, None, None) < 0
    assert f(None, off, -1, 0.1, 16, None, None) < 0
    bad = (ctypes.c_int64 * 2)(5, 2)
    assert f(None, bad, 1, 0.1, 16, None, None) < 0
    one = (ctypes.c_int64 * 2)(0, 4)
    assert f(None, one, 1, 0.1, 16, None, None) < 0            # rows, but NULL arrays
    lib.cs_normals_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    lib.cs_normals_stats.restype = None
    out = (ctypes.c_uint64 * 2)(7, 7)
    lib.cs_normals_stats(out, 1)
    assert (out[0], out[1]) == (0, 0)
