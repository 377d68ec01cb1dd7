"""The normals without a GPU: tests/normals_ref.py (the bit-exact restatement of cs_estimate_normals the GPU tests compare
with) against cKDTree.query(k) + numpy.linalg.eigh, the sweep count of jacobi3, and the defined answers of the degenerate
inputs."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import normals_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |sin| of the angle between the restated normal (f32) and eigh's eigenvector (f64) of the same neighbourhood: the
# largest value measured on the clouds below is 4.2e-8 (the f32 cast, 2^-24 = 6e-8 per component, dominates); x10.
SIN_TOL = 4.2e-7


@functools.lru_cache(maxsize=None)
def _clouds(n=400):
    """Random continuous samples of a box surface, a sphere and a cylinder: no two distances tie."""
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.5, 0.5, (n, 3))
    p[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-0.5, 0.5], n)
    q = rng.standard_normal((n, 3))
    q = 0.5 * q / np.linalg.norm(q, axis=1, keepdims=True)
    a = rng.uniform(0, 2 * np.pi, n)
    c = np.stack([0.3 * np.cos(a), 0.3 * np.sin(a), rng.uniform(-0.5, 0.5, n)], 1)
    return {"box": p.astype(np.float32), "sphere": q.astype(np.float32), "cylinder": c.astype(np.float32)}


@pytest.mark.parametrize("k", (8, 16))
@pytest.mark.parametrize("shape", ("box", "sphere", "cylinder"))
def test_restatement_against_kdtree_and_eigh(shape, k):
    """Measured maximum of |sin| over the three clouds and both k: 4.2e-8; asserted below SIN_TOL = 4.2e-7.  No row is
    skipped: the smallest (l1 - l0) / l2 over all rows is 2.7e-2, far above the 1e-3 at which a row could be left out."""
    from scipy.spatial import cKDTree

    c = _clouds()[shape]
    got = ref.estimate_normals(c, [0, len(c)], k).astype(np.float64)
    c64 = c.astype(np.float64)
    _, idx = cKDTree(c64).query(c64, k)
    worst = 0.0
    for i in range(len(c)):
        assert sorted(j for _, j in ref.neighbours(c, i, k)) == sorted(idx[i].tolist())     # the same neighbour set
        w, v = np.linalg.eigh(np.cov(c64[idx[i]].T, bias=True))
        assert (w[1] - w[0]) / w[2] >= 1e-3, "input chosen so that no row is skipped"
        worst = max(worst, float(np.linalg.norm(np.cross(got[i], v[:, 0]))))
        assert abs(np.linalg.norm(got[i]) - 1.0) < 1e-6
    print("max |sin| %s k=%d: %.3g" % (shape, k, worst))
    assert worst < SIN_TOL


def _offdiag(a):
    off = math.sqrt(2 * (a[0][1] ** 2 + a[0][2] ** 2 + a[1][2] ** 2))
    dg = math.sqrt(a[0][0] ** 2 + a[1][1] ** 2 + a[2][2] ** 2)
    return off / dg if dg > 0 else 0.0


def test_sweep_count():
    """The justification of jacobi3's five sweeps (corsair_amd/csrc/horn.h): the relative off-diagonal norm is at most
    2.4e-7 after 3 sweeps and 1.4e-28 after 4 on scatter matrices of 3, 8, 16 and 32 neighbours; sweeps 6 to 8 change no bit
    of a normal."""
    rng = np.random.default_rng(1)
    after = {3: 0.0, 4: 0.0, 5: 0.0}
    for c in _clouds().values():
        for k in (3, 8, 16, 32):
            for i in rng.choice(len(c), 40, replace=False):
                S = ref.scatter(c, int(i), [j for _, j in ref.neighbours(c, int(i), k)])
                for sw in after:
                    a = [r[:] for r in S]
                    ref.jacobi3(a, sw)
                    after[sw] = max(after[sw], _offdiag(a))
                assert ref.normal_of(S, 5) == ref.normal_of(S, 8)
    print("relative off-diagonal after 3 / 4 / 5 sweeps:", after)
    assert after[3] < 1e-5 and after[4] < 1e-20 and after[5] < 1e-40
    assert ref.SWEEPS == 5
    text = open(os.path.join(ROOT, "corsair_amd", "csrc", "horn.h")).read()
    assert "jacobi3" in text and "sweep < 5" in text.split("void jacobi3(")[1]


def test_sign_rule():
    # the component of largest magnitude is positive; the first such component on ties
    for S, want in (([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 0.0]], [0, 0, 1.0]),
                    ([[2.0, 0, 0], [0, 0.0, 0], [0, 0, 3.0]], [0, 1.0, 0])):
        assert ref.normal_of(S) == want
    # the (1, -1, 0) / sqrt 2 direction: |n_x| = |n_y|, x is the first and becomes positive
    n = ref.normal_of([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 5.0]])
    assert n[0] > 0 and n[1] < 0 and abs(n[0]) == abs(n[1]) and n[2] == 0.0
    c = _clouds()["sphere"]
    got = ref.estimate_normals(c[:120], [0, 120], 8)
    lead = np.abs(got).argmax(axis=1)
    assert (got[np.arange(len(got)), lead] > 0).all()
    # mirrored cloud: the direction mirrors, the sign rule is applied again
    neg = ref.estimate_normals(-c[:120], [0, 120], 8)
    assert np.array_equal(neg, got)


def test_fewer_than_three_rows_and_k_larger_than_the_segment():
    c = _clouds()["box"]
    for n in (1, 2):
        assert np.array_equal(ref.estimate_normals(c[:n], [0, n], 8), np.tile(np.float32([0, 0, 1]), (n, 1)))
    # empty segments and mixed sizes: a row's normal depends on its segment alone
    off = [0, 0, 2, 2, 7, 40]
    got = ref.estimate_normals(c[:40], off, 16)
    assert np.array_equal(got[:2], np.tile(np.float32([0, 0, 1]), (2, 1)))
    assert np.array_equal(got[2:7], ref.estimate_normals(c[2:7], [0, 5], 16))
    assert np.array_equal(got[7:], ref.estimate_normals(c[7:40], [0, 33], 16))
    assert np.array_equal(ref.estimate_normals(c[2:7], [0, 5], 16), ref.estimate_normals(c[2:7], [0, 5], 5))


def test_exact_plane_line_point_and_nan():
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    plane = np.concatenate([g, np.full((len(g), 1), 0.75, np.float32)], 1)
    assert np.array_equal(ref.estimate_normals(plane, [0, len(plane)], 8), np.tile(np.float32([0, 0, 1]), (len(plane), 1)))
    # the same plane as x = const: the zero eigenvalue sits in column 0
    assert np.array_equal(ref.estimate_normals(plane[:, [2, 0, 1]], [0, len(plane)], 8),
                          np.tile(np.float32([1, 0, 0]), (len(plane), 1)))
    line = np.zeros((9, 3), np.float32)
    line[:, 0] = np.arange(9) * 0.5
    # two zero eigenvalues (columns 1 and 2): the smaller column, (0, 1, 0)
    assert np.array_equal(ref.estimate_normals(line, [0, 9], 5), np.tile(np.float32([0, 1, 0]), (9, 1)))
    same = np.tile(np.float32([[0.3, -0.2, 0.9]]), (6, 1))
    assert np.array_equal(ref.estimate_normals(same, [0, 6], 4), np.tile(np.float32([1, 0, 0]), (6, 1)))
    # a NaN row: its own normal is (0, 0, 1) and it is nobody's neighbour
    c = _clouds()["box"][:60].copy()
    clean = ref.estimate_normals(np.delete(c, 17, axis=0), [0, 59], 8)
    c[17, 1] = np.nan
    got = ref.estimate_normals(c, [0, 60], 8)
    assert np.array_equal(got[17], np.float32([0, 0, 1]))
    assert np.array_equal(np.delete(got, 17, axis=0), clean)
    # an inf row likewise; with only two finite rows left every normal is (0, 0, 1)
    c3 = _clouds()["box"][:3].copy()
    c3[0, 0] = np.inf
    assert np.array_equal(ref.estimate_normals(c3, [0, 3], 3), np.tile(np.float32([0, 0, 1]), (3, 1)))


def test_ties_go_to_the_smaller_row():
    # integer grid: row 0 has three neighbours at distance 1 and k = 3 keeps itself and the two smaller rows
    g = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    nb = ref.neighbours(g, 0, 3)
    assert [j for _, j in nb] == [0, 1, 3] and [d for d, _ in nb] == [0.0, 1.0, 1.0]
    dup = np.concatenate([g[:5], g[:5]])
    assert [j for _, j in ref.neighbours(dup, 7, 3)] == [2, 7, 1]        # rows 2 and 7 are the same point


def test_surface_is_declared():
    from corsair_amd import _lib, backend as B, harness as H

    header = open(os.path.join(ROOT, "include", "corsair_hip.h")).read()
    assert {"cs_estimate_normals", "cs_icp_plane_batch"} <= set(_lib.header_symbols())
    for word in ('"normals"', "[O3D-knowledge]", "jacobi3", "k in [3, 32]"):
        assert word in header, word
    assert callable(B.estimate_normals)
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    assert "normals.hip" in open(os.path.join(csrc, "Makefile")).read()
    assert '"normals"' in open(os.path.join(csrc, "runtime.hip")).read()
    unit = open(os.path.join(csrc, "normals.hip")).read()
    assert '#include "horn.h"' in unit and "jacobi3(" in unit and "void jacobi3" not in unit
    cfg = H.Config()
    assert cfg.icp_estimation == "point" and cfg.icp_normal_k == 16
    a = H.build_parser().parse_args(["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"])
    assert a.icp_estimation == "point" and a.icp_normal_k == 16
    a = H.build_parser().parse_args(["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b", "--icp-estimation",
                                     "plane", "--icp-normal-k", "8"])
    assert a.icp_estimation == "plane" and a.icp_normal_k == 8
    with pytest.raises(ValueError, match="icp_estimation"):
        H.Config(icp_estimation="spline").check_icp()


def test_library_exports_and_refusals_without_a_device():
    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.cs_estimate_normals.restype = ctypes.c_int
    lib.cs_estimate_normals.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p]
    off = (ctypes.c_int64 * 2)(0, 0)
    # argument checks come before any device work: an empty call needs no GPU
    assert lib.cs_estimate_normals(None, off, 0, 16, None, None) == 0
    assert lib.cs_estimate_normals(None, off, 1, 16, None, None) == 0          # one empty segment
    assert lib.cs_estimate_normals(None, off, 1, 2, None, None) < 0
    assert lib.cs_estimate_normals(None, off, 1, 33, None, None) < 0
    assert lib.cs_estimate_normals(None, None, 1, 16, None, None) < 0
    assert lib.cs_estimate_normals(None, off, -1, 16, None, None) < 0
    bad = (ctypes.c_int64 * 2)(5, 2)
    assert lib.cs_estimate_normals(None, bad, 1, 16, None, None) < 0
    one = (ctypes.c_int64 * 2)(0, 4)
    assert lib.cs_estimate_normals(None, one, 1, 16, None, None) < 0            # rows, but NULL arrays
    assert hasattr(lib, "cs_icp_plane_batch")
