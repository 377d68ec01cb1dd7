"""The point-to-plane ICP without a GPU: tests/icp_plane_ref.py (the bit-exact restatement of cs_icp_plane_batch the GPU
tests compare with) against an independent loop -- SciPy's KD-tree, numpy.linalg.solve, plain f64 --, against Open3D's
Rz Ry Rx form of the update, its fixed-point bounds, the clamp, and the stop rules."""
import functools
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import icp_plane_ref as ref
from tests import icp_ref
from tests import normals_ref
from tests.test_icp_cpu import _fixture

FIXTURES = ((1, 300, 1400), (2, 257, 513), (3, 120, 1200))


@functools.lru_cache(maxsize=None)
def _fix(seed, ns, nt):
    src, tgt, T0, Tgt = _fixture(seed, ns, nt)
    return src, tgt, normals_ref.estimate_normals(tgt, [0, len(tgt)], 16), T0, Tgt


def _cayley(a):
    q = np.array([1.0, a[0] / 2, a[1] / 2, a[2] / 2])
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _euler(a):
    cx, sx, cy, sy, cz, sz = math.cos(a[0]), math.sin(a[0]), math.cos(a[1]), math.sin(a[1]), math.cos(a[2]), math.sin(a[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _solve_icp(src, tgt, nrm, T0, max_dist, max_iter, rotation=_cayley, rf=1e-6, rr=1e-6):
    """Open3D's loop with SciPy's KD-tree and numpy.linalg.solve on the 6x6 normal equations, everything in plain f64.
    The update is the specification's: linearised about the midpoint o of the target's bounding box, p <- R (p - o) + t' + o
    (about another origin the linear solution is the same and the rotation applied to it differs at second order)."""
    src, tgt, nrm = src.astype(np.float64), tgt.astype(np.float64), nrm.astype(np.float64)
    o = 0.5 * (tgt.min(0) + tgt.max(0))
    tree = cKDTree(tgt)
    T = np.asarray(T0, np.float32).astype(np.float64).reshape(4, 4).copy()

    def evaluate(T):
        p = src @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(p)
        keep = d * d < max_dist * max_dist
        n = int(keep.sum())
        return p, j, keep, n / len(src), (math.sqrt(float((d[keep] ** 2).sum()) / n) if n else 0.0), n

    p, j, keep, fit, rm, n = evaluate(T)
    it = 0
    for _ in range(max_iter):
        if n < 6:
            break
        P, Q, N = p[keep], tgt[j[keep]], nrm[j[keep]]
        r = ((P - Q) * N).sum(1)
        J = np.concatenate([np.cross(P - o, N), N], 1)
        x = np.linalg.solve(J.T @ J, -(J.T @ r))
        U = np.eye(4)
        U[:3, :3] = rotation(x[:3])
        U[:3, 3] = x[3:] + o - U[:3, :3] @ o
        T = U @ T
        it += 1
        pf, pr = fit, rm
        p, j, keep, fit, rm, n = evaluate(T)
        if abs(fit - pf) < rf and abs(rm - pr) < rr:
            break
    return T, it, np.where(keep, j, -1), fit, rm


@pytest.mark.parametrize("seed,ns,nt", FIXTURES)
def test_restatement_against_kdtree_and_solve(seed, ns, nt):
    """Correspondences identical (no ties in these clouds), the same number of updates, the final transform within 2.4e-14
    (max abs over the 16 entries) of the independent loop's.  Measured on the three fixtures: 6.4e-16, 2.4e-15, 4.4e-16
    after 5, 7 and 4 updates; the bound is the largest with a margin of 10.  What separates the two: the truncation of the
    fixed-point sums, the unpivoted Cholesky against LAPACK's LU, and the order of the f64 sums."""
    src, tgt, nrm, T0, _ = _fix(seed, ns, nt)
    got = ref.icp(src, tgt, nrm, T0, 0.1, 30)
    Tk, itk, corr_k, fit_k, rm_k = _solve_icp(src, tgt, nrm, T0, 0.1, 30)
    diff = float(np.abs(got["T"].reshape(4, 4) - Tk).max())
    print("seed %d: updates %d / %d, max |T - T_solve| = %.3g" % (seed, got["iters"], itk, diff))
    assert got["iters"] == itk and 1 < itk < 30
    assert np.array_equal(got["corr"], corr_k)
    quantum = 2.0 ** -icp_ref.frame(tgt, ns, 0.1)["s2"]
    assert got["fitness"] == fit_k and abs(got["rmse"] ** 2 - rm_k ** 2) <= quantum + 1e-12 * rm_k ** 2
    assert diff <= 2.4e-14
    first = ref.icp(src, tgt, nrm, T0, 0.1, 0)
    assert first["iters"] == 0 and np.array_equal(first["T32"], T0.reshape(16))
    assert np.array_equal(first["corr"], corr_k if itk == 0 else _solve_icp(src, tgt, nrm, T0, 0.1, 0)[2])


@pytest.mark.parametrize("seed,ns,nt", FIXTURES)
def test_cayley_against_open3d_euler_update(seed, ns, nt):
    """The Cayley rotation of the solved vector against Open3D's Rz Ry Rx of the same three numbers: both loops stop by the
    same criteria (|d fitness| < 1e-6 and |d rmse| < 1e-6) and their final evaluations agree within those criteria.
    Measured on the three fixtures (sources that are subsamples of their targets, so both loops converge fast): update
    counts equal (5, 7, 4), fitness equal, |rmse difference| at most 5.3e-11, max |T - T_euler| 6.7e-16, 7.8e-9 and
    5.0e-16; asserted: fitness and rmse differences below the criteria (1e-6 each), the transforms within 1e-6.  (Where
    the loops converge slowly -- a source outside its target -- they may stop one update apart, each within its own
    criterion of the common fixed point.)"""
    src, tgt, nrm, T0, _ = _fix(seed, ns, nt)
    Tc, itc, _, fit_c, rm_c = _solve_icp(src, tgt, nrm, T0, 0.1, 30)
    Te, ite, _, fit_e, rm_e = _solve_icp(src, tgt, nrm, T0, 0.1, 30, rotation=_euler)
    got = ref.icp(src, tgt, nrm, T0, 0.1, 30)
    dT = float(np.abs(got["T"].reshape(4, 4) - Te).max())
    print("seed %d: updates %d / %d, |d fitness| %.3g, |d rmse| %.3g, max |T - T_euler| %.3g"
          % (seed, itc, ite, abs(fit_c - fit_e), abs(rm_c - rm_e), dT))
    assert abs(got["fitness"] - fit_e) < 1e-6 and abs(got["rmse"] - rm_e) < 1e-6
    assert itc == ite and dT < 1e-6


def test_plane_needs_fewer_updates_than_point_and_reaches_the_pose():
    """Measured on fixture 1 (300 sources, a subsample of the 1 400 targets, 3 degrees / 1 cm off): plane 5 updates, point
    9; max |T - T_true| goes from 4.5e-2 to 1.7e-8 (a factor of 3.7e-7), asserted below 1e-6 of the initial value."""
    src, tgt, nrm, T0, Tgt = _fix(*FIXTURES[0])
    plane = ref.icp(src, tgt, nrm, T0, 0.1, 30)
    point = icp_ref.icp(src, tgt, T0, 0.1, 30)
    e0 = float(np.abs(T0.astype(np.float64) - Tgt).max())
    e1 = float(np.abs(plane["T"].reshape(4, 4) - Tgt).max())
    print("updates plane %d point %d; max |T - T_true| %.3g -> %.3g" % (plane["iters"], point["iters"], e0, e1))
    assert plane["iters"] < point["iters"]
    assert e0 > 0.01 and e1 <= 1e-6 * e0 and plane["fitness"] == 1.0


@pytest.mark.parametrize("scale,max_dist", ((1.0, 0.1), (50.0, 3.0)))
def test_no_term_reaches_its_clamp(scale, max_dist):
    """Unit-sized and 50-unit clouds: the largest scaled term stays below its clamp 2^(61 - eN) and every sum below 2^61."""
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[1])
    S = np.diag([scale, scale, scale, 1.0])
    T0s = (S @ T0.astype(np.float64) @ np.linalg.inv(S)).astype(np.float32)
    watch = {}
    got = ref.icp((src * scale).astype(np.float32), (tgt * scale).astype(np.float32), nrm, T0s, max_dist, 3, watch=watch)
    print("scale %g: largest |term| / clamp = %.3g, largest |sum| = 2^%.1f" % (scale, watch["term"], math.log2(watch["sum"])))
    assert got["ncorr"] > 128 and got["iters"] >= 2
    assert watch["term"] < 1.0 and watch["sum"] < 2 ** 61


def test_scales_and_their_bounds():
    rng = np.random.default_rng(0)
    for n_src, scale, max_dist in ((1, 1.0, 0.1), (5000, 1.0, 0.06), (2 ** 31 - 1, 50.0, 3.0), (257, 1e-3, 1e-4),
                                   (1000, 3e38, 1.0)):
        tgt = (rng.uniform(-1, 1, (64, 3)) * scale).astype(np.float32)
        fr = ref.plane_frame(icp_ref.frame(tgt, n_src, max_dist))
        lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
        M = float(np.max(0.5 * (hi - lo))) + max_dist
        c = fr["clamp"]
        # the bounds of the header comment, each with its extra bit: |a| <= 2 M, |n| <= 1, |r| < max_dist
        assert 2 * (4 * M * M) * fr["sc_rr"] <= c and 2 * (2 * M) * fr["sc_rt"] <= c and 2 * 1.0 * fr["sc_tt"] <= c
        assert 2 * (2 * M * max_dist) * fr["sc_rd"] <= c and 2 * max_dist * fr["sc_td"] <= c
        for k in ("rr", "rt", "tt", "rd", "td"):
            assert fr["sc_" + k] * fr["inv_" + k] == 1.0 and -1022 < fr["s_" + k] < 1023


def test_long_normals_are_clamped():
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[1])
    watch = {}
    got = ref.icp(src, tgt, nrm * np.float32(1e3), T0, 0.1, 30, watch=watch)
    assert watch["term"] >= 1.0                                 # terms did reach the clamp ...
    assert all(abs(v) < 2 ** 61 for v in got["sums"])           # ... and the sums stayed inside the bound
    assert np.all(np.isfinite(got["T"]))
    bad = nrm.copy()
    bad[::7] = np.nan
    got = ref.icp(src, tgt, bad, T0, 0.1, 30)
    assert all(abs(v) < 2 ** 61 for v in got["sums"]) and np.all(np.isfinite(got["T"]))
    # normals scaled by a power of two that stays inside the bounds: the same solution up to rounding (A and b scale)
    twice = ref.icp(src, tgt, nrm * np.float32(0.5), T0, 0.1, 1)
    once = ref.icp(src, tgt, nrm, T0, 0.1, 1)
    assert np.abs(twice["T"] - once["T"]).max() < 1e-9


def test_exact_plane_stops_with_the_initial_transform():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) * 0.05
    tgt = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(tgt), 1))
    src = (tgt[10:100] + np.float32([0.004, -0.003, 0.01])).astype(np.float32)
    T0 = np.eye(4, dtype=np.float32)
    fr = ref.plane_frame(icp_ref.frame(tgt, len(src), 0.1))
    corr, P, D = icp_ref.associate([float(v) for v in T0.reshape(16)], src, tgt, 0.01)
    A, _ = ref.normal_equations(ref.sums_of(corr, P, D, tgt, nrm, fr), fr)
    # J = (p'_y, -p'_x, 0, 0, 0, 1): rows and columns 2, 3 and 4 are exactly zero -- the pivot of column 2 is an exact 0
    assert all(A[i][j] == 0.0 for i in (2, 3, 4) for j in range(6)) and A[0][0] > 0 and A[1][1] > 0 and A[5][5] == len(src)
    got = ref.icp(src, tgt, nrm, T0, 0.1, 30)
    assert got["iters"] == 0 and got["ncorr"] == len(src) and got["fitness"] == 1.0 and got["rmse"] > 0.01
    assert np.array_equal(got["T"], T0.reshape(16).astype(np.float64)) and np.array_equal(got["T32"], T0.reshape(16))


def test_five_pairs_stop_six_go_on():
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[0])
    five = ref.icp(src[:5], tgt, nrm, T0, 0.1, 30)
    assert five["ncorr"] == 5 and five["iters"] == 0 and np.array_equal(five["T32"], T0.reshape(16))
    # six pairs pass the count rule: the update is attempted (and applied when the six rows constrain the pose)
    six = ref.icp(src[:6], tgt, nrm, T0, 0.1, 0)
    fr = ref.plane_frame(icp_ref.frame(tgt, 6, 0.1))
    solved = ref.cholesky_solve(*ref.normal_equations(six["sums"], fr)) is not None
    assert six["ncorr"] == 6 and ref.icp(src[:6], tgt, nrm, T0, 0.1, 30)["iters"] >= (1 if solved else 0)
    assert ref.icp(src[:40], tgt, nrm, T0, 0.1, 30)["iters"] >= 1
    for s, t, n in ((src[:0], tgt, nrm), (src, tgt[:0], nrm[:0])):
        r = ref.icp(s, t, n, T0, 0.1, 30)
        assert (r["fitness"], r["rmse"], r["iters"], r["ncorr"]) == (0.0, 0.0, 0, 0)


def test_cholesky_against_numpy():
    rng = np.random.default_rng(4)
    J = rng.standard_normal((40, 6))
    A, b = J.T @ J, rng.standard_normal(6)
    x = ref.cholesky_solve(A.tolist(), b.tolist())
    assert np.abs(np.asarray(x) - np.linalg.solve(A, -b)).max() < 1e-12
    A[:, 3] = A[:, 0]
    A[3, :] = A[0, :]                                           # column 3 = column 0: its pivot is a rounding residue
    assert ref.cholesky_solve(A.tolist(), b.tolist()) is None
    A = (J.T @ J)
    A[2, 2] = math.nan
    assert ref.cholesky_solve(A.tolist(), b.tolist()) is None
    # the Cayley rotation is a rotation, and the identity for x = 0
    R = np.asarray(ref.cayley(0.3, -0.2, 0.1))
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
    assert ref.cayley(0.0, 0.0, 0.0) == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def test_surface_is_declared():
    import inspect
    import os

    from corsair_amd import _lib, backend as B, registration as R

    header = open(_lib.HEADER_PATH).read()
    assert "cs_icp_plane_batch" in _lib.header_symbols()
    for word in ("d_tgt_normal", "Cholesky", "2^-30", "[O3D-knowledge]"):
        assert word in header, word
    assert "tgt_normals" in inspect.signature(B.icp_batch).parameters
    sig = inspect.signature(R.sym_pose_batch).parameters
    assert sig["icp_estimation"].default == "point" and sig["icp_normal_k"].default == 16 and sig["normals1"].default is None
    from tests.helpers import assert_five_icp_kernels

    assert_five_icp_kernels()          # frame, exact, f16, step, init: the plane path adds no kernel of its own
