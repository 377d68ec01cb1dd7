"""Generalized ICP without a GPU: tests/gicp_ref.py (the bit-exact restatement of cs_icp_gicp_batch the GPU tests compare
with) against an independent loop -- SciPy's KD-tree, numpy.linalg.inv / solve, plain f64 --, on the lattice fixture of
DESIGN 19 against the point and the plane restatements, at epsilon = 1, on bad normals, on its fixed-point bounds and on its
stop rules; and the Python surfaces that need no device."""
import functools
import inspect
import math
import random

import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import gicp_ref as ref
from tests import icp_plane_ref
from tests import icp_ref
from tests import normals_ref
from tests.test_icp_cpu import _fixture
from tests.test_icp_plane_cpu import _cayley

FIXTURES = ((1, 300, 1400), (2, 257, 513))


@functools.lru_cache(maxsize=None)
def _fix(seed, ns, nt):
    src, tgt, T0, Tgt = _fixture(seed, ns, nt)
    return (src, normals_ref.estimate_normals(src, [0, len(src)], 16), tgt, normals_ref.estimate_normals(tgt, [0, len(tgt)], 16),
            T0, Tgt)


def test_fast_fma_is_the_exact_fma():
    r = random.Random(1)
    for i in range(20000):
        a = r.uniform(-1, 1) * 2.0 ** r.randint(-300, 300)
        b = r.uniform(-1, 1) * 2.0 ** r.randint(-300, 300)
        c = -a * b * (1 + r.uniform(-1e-15, 1e-15)) if i % 2 else r.uniform(-1, 1) * 2.0 ** r.randint(-600, 600)
        x, y = icp_ref.fma(a, b, c), ref.fma(a, b, c)
        assert x == y and math.copysign(1, x) == math.copysign(1, y), (a, b, c)
    for args in ((0.0, 5.0, -0.0), (1e-320, 1e-5, 0.0), (math.inf, 1.0, 1.0), (math.nan, 1.0, 1.0), (3.0, -2.0, 6.0)):
        x, y = icp_ref.fma(*args), ref.fma(*args)
        assert (x != x and y != y) or (x == y and math.copysign(1, x) == math.copysign(1, y)), args


def _solve_gicp(src, snrm, tgt, tnrm, T0, max_dist, max_iter, eps, rf=1e-6, rr=1e-6):
    """Open3D's loop with SciPy's KD-tree, numpy.linalg.inv for every pair's weight and numpy.linalg.solve on the 6 x 6
    normal equations, everything in plain f64; linearised about the midpoint o of the target's bounding box as the
    specification is."""
    src, snrm, tgt, tnrm = (np.asarray(a, np.float32).astype(np.float64) for a in (src, snrm, tgt, tnrm))
    o = 0.5 * (tgt.min(0) + tgt.max(0))
    tree = cKDTree(tgt)
    T = np.asarray(T0, np.float32).astype(np.float64).reshape(4, 4).copy()
    I3 = np.eye(3)

    def evaluate(T):
        p = src @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(p)
        keep = d * d < max_dist * max_dist
        n = int(keep.sum())
        return p, j, keep, n / len(src), (math.sqrt(float((d[keep] ** 2).sum()) / n) if n else 0.0), n

    def cov(n):
        return I3 - (1 - eps) * np.outer(n, n) / (n @ n)

    p, j, keep, fit, rm, n = evaluate(T)
    it = 0
    for _ in range(max_iter):
        if n < 6:
            break
        A, b = np.zeros((6, 6)), np.zeros(6)
        for i in np.nonzero(keep)[0]:
            W = np.linalg.inv(cov(tnrm[j[i]]) + cov(T[:3, :3] @ snrm[i]))
            q = p[i] - o
            G = np.array([[0, q[2], -q[1]], [-q[2], 0, q[0]], [q[1], -q[0], 0]])      # d(omega x p') / d omega = -[p']x
            J = np.concatenate([G, I3], 1)
            A += J.T @ W @ J
            b += J.T @ W @ (p[i] - tgt[j[i]])
        x = np.linalg.solve(A, -b)
        U = np.eye(4)
        U[:3, :3] = _cayley(x[:3])
        U[:3, 3] = x[3:] + o - U[:3, :3] @ o
        T = U @ T
        it += 1
        pf, pr = fit, rm
        p, j, keep, fit, rm, n = evaluate(T)
        if abs(fit - pf) < rf and abs(rm - pr) < rr:
            break
    return T, it, np.where(keep, j, -1), fit, rm


@pytest.mark.parametrize("seed,ns,nt", FIXTURES)
def test_restatement_against_kdtree_inv_and_solve(seed, ns, nt):
    """Same updates, same correspondences, T within 1e-6 (the tolerance tests/test_icp_plane_cpu.py uses when it compares
    two loops) of the independent loop; the figure is printed."""
    src, snrm, tgt, tnrm, T0, _ = _fix(seed, ns, nt)
    got = ref.icp(src, snrm, tgt, tnrm, T0, 0.1, 30, epsilon=1e-3)
    Tk, itk, corr_k, fit_k, rm_k = _solve_gicp(src, snrm, tgt, tnrm, T0, 0.1, 30, 1e-3)
    diff = float(np.abs(got["T"].reshape(4, 4) - Tk).max())
    print("seed %d: updates %d / %d, max |T - T_solve| = %.3g, mrmse %.4g" % (seed, got["iters"], itk, diff, got["mrmse"]))
    assert got["iters"] == itk and 1 < itk < 30
    assert np.array_equal(got["corr"], corr_k)
    assert got["fitness"] == fit_k and abs(got["rmse"] - rm_k) < 1e-6       # (both are rounding residue: the source lies ON the target)
    assert diff < 1e-6
    first = ref.icp(src, snrm, tgt, tnrm, T0, 0.1, 0, epsilon=1e-3)
    assert first["iters"] == 0 and np.array_equal(first["T32"], T0.reshape(16))


def test_lattice_fixture_gicp_beats_point_and_plane():
    """DESIGN 19's fixture.  Measured (updates, RRE in degrees, RTE): point (10, 1.851, 9.89e-3 -- the half-voxel lock),
    plane (8, 0.262, 1.12e-4), GICP at epsilon = 1e-3 (4, 0.0114, 8.39e-5).  Asserted: GICP's RRE and RTE are each strictly
    smaller than those of the point and of the plane restatement, and GICP stops by its criteria within 30 updates."""
    f = ref.lattice_fixture()
    assert len(f["tgt"]) == 1625 and len(f["src"]) == 1265
    runs = ref.lattice_runs()
    err = {k: ref.pose_errors(v["T"], f["G"]) for k, v in runs.items()}
    for k in ("point", "plane", "gicp"):
        print("%-5s updates %2d  RRE %.4g deg  RTE %.4g  fitness %.3f rmse %.5f" %
              (k, runs[k]["iters"], err[k][0], err[k][1], runs[k]["fitness"], runs[k]["rmse"]))
    for other in ("point", "plane"):
        assert err["gicp"][0] < err[other][0] and err["gicp"][1] < err[other][1], (other, err)
    assert 0 < runs["gicp"]["iters"] < 30
    assert runs["gicp"]["mrmse"] > 0 and math.isfinite(runs["gicp"]["mrmse"])


def test_epsilon_one_weights_every_pair_by_half_the_identity():
    src, snrm, tgt, tnrm, T0, _ = _fix(*FIXTURES[1])
    watch = {}
    got = ref.icp(src, snrm, tgt, tnrm, T0, 0.1, 2, epsilon=1.0, watch=watch)
    half = [[0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.5]]
    assert len(watch["W"]) > 2 * 128 and all(W == half for W in watch["W"])
    # the sums are those of an isotropic weighting: normals do not matter, and the Mahalanobis cost is half the squared
    # distance (both scales are powers of two; only the truncation of each term differs)
    other = ref.icp(src, snrm[::-1], tgt, np.roll(tnrm, 5, 0), T0, 0.1, 2, epsilon=1.0)
    assert np.array_equal(got["T"], other["T"]) and got["sums"] == other["sums"]
    assert abs(got["mrmse"] ** 2 - 0.5 * got["rmse"] ** 2) < 1e-12
    assert ref.weight_exponent(1.0) == -1 and ref.weight_exponent(0.5) == 0 and ref.weight_exponent(1e-3) == 9
    assert ref.weight_exponent(2.0 ** -10) == 9 and ref.weight_exponent(0.51) == 0 and ref.weight_exponent(0.49) == 1


def test_bad_normals_give_the_documented_covariance():
    eps = 1e-3
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for n in ([0.0, 0.0, 0.0], [math.nan, 0.0, 1.0], [0.0, math.inf, 0.0], [1e-30 * 1e-300, 0.0, 0.0]):
        assert ref.covariance(n, eps) == eye, n
    # a non-unit normal of either sign: the covariance of its direction
    unit = np.array([2.0, -1.0, 2.0]) / 3.0
    want = np.eye(3) - (1 - eps) * np.outer(unit, unit)
    for s in (1.0, -1.0, 1e3, -1e-3, 1e30):
        assert np.abs(np.asarray(ref.covariance(list(unit * s), eps)) - want).max() < 1e-15, s
    # a pair with one bad normal: the inverse of I + C(n); with both bad: I / 2
    W = np.asarray(ref.weight_of([0.0, 0.0, 0.0], list(unit * 7), 1 - eps))
    assert np.abs(W - np.linalg.inv(np.eye(3) + want)).max() < 1e-13
    assert ref.weight_of([math.nan, 1.0, 0.0], [0.0, 0.0, 0.0], 1 - eps) == [[0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.5]]
    # the whole loop with such rows in both arrays stays finite and inside the bound
    src, snrm, tgt, tnrm, T0, _ = _fix(*FIXTURES[1])
    bs, bt = snrm.copy(), tnrm.copy()
    bs[::5], bs[1::5], bs[2::5] = 0.0, np.nan, bs[2::5] * np.float32(-40.0)
    bt[::7], bt[1::7], bt[2::7] = np.nan, 0.0, bt[2::7] * np.float32(1e3)
    got = ref.icp(src, bs, tgt, bt, T0, 0.1, 30, epsilon=1e-3)
    assert np.all(np.isfinite(got["T"])) and got["iters"] > 1 and all(abs(v) < 2 ** 61 for v in got["sums"])


def test_fixed_point_bound_on_the_adversarial_input():
    """Every pair at a distance just under max_dist, both normals along the residual (n_t = m, the weight 1 / (2 epsilon) on
    e), epsilon = 2^-10, the sources in the corners of the target's box: the largest scaled term stays below the clamp and
    every sum below 2^61."""
    eps, md = 2.0 ** -10, 0.25
    g = np.stack(np.meshgrid(*[np.array([-1.0, 1.0])] * 3, indexing="ij"), -1).reshape(-1, 3)
    tgt = np.repeat(g, 32, 0).astype(np.float32)                         # 256 targets in the 8 corners
    d = g / np.linalg.norm(g, axis=1, keepdims=True)
    src = (np.repeat(g, 32, 0) - np.repeat(d, 32, 0) * (md * (1 - 1e-6))).astype(np.float32)
    nrm = np.repeat(d, 32, 0).astype(np.float32)
    watch = {}
    got = ref.icp(src, nrm, tgt, nrm, np.eye(4, dtype=np.float32), md, 0, epsilon=eps, watch=watch)
    fr = ref.gicp_frame(icp_ref.frame(tgt, len(src), md), eps)
    print("largest |term| / clamp = %.3g, largest |sum| = 2^%.1f, eW = %d" % (watch["term"], math.log2(watch["sum"]), fr["eW"]))
    assert got["ncorr"] == 256 and got["rmse"] > 0.999 * md * (1 - 1e-6)
    assert max(abs(W[i][j]) for W in watch["W"] for i in range(3) for j in range(3)) > 0.3 / (2 * eps)
    assert watch["term"] < 1.0 and watch["sum"] < 2 ** 61
    # the Mahalanobis cost of such a pair is |e|^2 / (2 epsilon)
    assert abs(got["mrmse"] ** 2 - got["rmse"] ** 2 / (2 * eps)) < 1e-6 * got["mrmse"] ** 2
    # the bounds of the header comment with their extra bit, for several frames
    rng = np.random.default_rng(0)
    for n_src, scale, max_dist, e in ((1, 1.0, 0.1, 1.0), (5000, 1.0, 0.06, 1e-3), (2 ** 31 - 1, 50.0, 3.0, eps),
                                      (257, 1e-3, 1e-4, 0.3), (1000, 3e38, 1.0, eps)):
        t = (rng.uniform(-1, 1, (64, 3)) * scale).astype(np.float32)
        fr = ref.gicp_frame(icp_ref.frame(t, n_src, max_dist), e)
        M = float(np.max(0.5 * (t.max(0).astype(np.float64) - t.min(0).astype(np.float64)))) + max_dist
        w, c = 1.0 / (2.0 * e), fr["clamp"]
        assert w <= 2.0 ** fr["eW"] < 2 * w or fr["eW"] == -1
        assert 2 * (3 * M * M * w) * fr["sc_rr"] <= c and 2 * (math.sqrt(3) * M * w) * fr["sc_rt"] <= c
        assert 2 * w * fr["sc_tt"] <= c and 2 * (math.sqrt(3) * M * w * max_dist) * fr["sc_rd"] <= c
        assert 2 * (w * max_dist) * fr["sc_td"] <= c and 2 * (max_dist * max_dist * w) * fr["sc_rd"] <= c
        for k in ("rr", "rt", "tt", "rd", "td"):
            assert fr["sc_" + k] * fr["inv_" + k] == 1.0 and -1022 < fr["s_" + k] < 1023


def test_stop_rules():
    src, snrm, tgt, tnrm, T0, _ = _fix(*FIXTURES[0])
    five = ref.icp(src[:5], snrm[:5], tgt, tnrm, T0, 0.1, 30)
    assert five["ncorr"] == 5 and five["iters"] == 0 and np.array_equal(five["T32"], T0.reshape(16))
    assert ref.icp(src[:40], snrm[:40], tgt, tnrm, T0, 0.1, 30)["iters"] >= 1
    for s, sn, t, tn in ((src[:0], snrm[:0], tgt, tnrm), (src, snrm, tgt[:0], tnrm[:0])):
        r = ref.icp(s, sn, t, tn, T0, 0.1, 30)
        assert (r["fitness"], r["rmse"], r["mrmse"], r["iters"], r["ncorr"]) == (0.0, 0.0, 0.0, 0, 0)
    # a degenerate A: six sources on one point constrain no rotation about it -- a rotational pivot is an exact zero or a
    # rounding residue, the problem stops with T0
    one = np.tile(src[:1], (6, 1))
    r = ref.icp(one, np.tile(snrm[:1], (6, 1)), tgt, tnrm, T0, 0.1, 30)
    assert r["ncorr"] == 6 and r["iters"] == 0 and np.array_equal(r["T32"], T0.reshape(16))
    # a single plane.  Point-to-plane is singular there (tests/test_icp_plane_cpu.py: 0 updates, T = T0).  GICP is NOT: in
    # the plane's directions the pairs pull with the weight 1 / 2, like a point-to-point estimation, so no pivot fails, the
    # problem runs to its criteria, closes the offset along the normal and locks onto the lattice in the plane
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) * 0.05
    ptgt = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
    pn = np.tile(np.float32([0, 0, 1]), (len(ptgt), 1))
    psrc = (ptgt[10:100] + np.float32([0.004, -0.003, 0.01])).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)
    plane = icp_plane_ref.icp(psrc, ptgt, pn, eye, 0.1, 30)
    got = ref.icp(psrc, pn[:len(psrc)], ptgt, pn, eye, 0.1, 30)
    assert plane["iters"] == 0 and 0 < got["iters"] < 30 and got["ncorr"] == len(psrc)
    t = got["T"].reshape(4, 4)[:3, 3]
    print("single plane: %d updates, t = %s, rmse %.3g" % (got["iters"], t, got["rmse"]))
    assert np.abs(t - np.array([-0.004, 0.003, -0.01])).max() < 1e-6 and got["rmse"] < 1e-6
    A, _ = icp_plane_ref.normal_equations(ref.icp(psrc, pn[:len(psrc)], ptgt, pn, eye, 0.1, 0)["sums"],
                                          ref.gicp_frame(icp_ref.frame(ptgt, len(psrc), 0.1), 1e-3))
    assert A[3][3] == 0.5 * len(psrc) and A[4][4] == 0.5 * len(psrc) and abs(A[5][5] - len(psrc) / 2e-3) < 1e-6


def test_surfaces_are_declared():
    from corsair_amd import _lib, backend as B, harness, registration as R, shapenet_eval

    assert "cs_icp_gicp_batch" in _lib.header_symbols()
    header = open(_lib.HEADER_PATH).read()
    for word in ("d_src_normal", "adjugate", "[2^-10, 1]", "T C_s T^T", "W^(1/2)", "d_mrmse"):
        assert word in header, word
    sig = inspect.signature(B.icp_batch).parameters
    for name, default in (("estimation", None), ("src_normals", None), ("gicp_epsilon", 1e-3)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default
    assert list(sig)[:17] == ["src", "soff", "tgt", "toff", "src_seg", "tgt_seg", "T0", "max_dist", "max_iter",
                              "relative_fitness", "relative_rmse", "return_corr", "tgt_normals", "kernel", "kernel_scale",
                              "with_scaling", "scale_bounds"]
    # mrmse is an attribute of the result, None unless GICP ran; the tuple keeps its ten fields (tests/test_icp_scale_cpu.py
    # pins "scale" as the last of them)
    plain = B.IcpResult(*range(8))
    assert plain.mrmse is None and "mrmse" not in B.IcpResult._fields and len(B.IcpResult._fields) == 10
    full = B.GicpResult(*range(10), mrmse=7)
    assert isinstance(full, B.IcpResult) and full.mrmse == 7 and tuple(full) == tuple(range(10)) and full.scale == 9
    # the positional signature of sym_pose_batch is what it was: the new options are keyword-only behind it
    names = list(inspect.signature(R.sym_pose_batch).parameters)
    assert names[0] == "baseF" and names[-2:] == ["icp_kernel", "icp_kernel_scale"]
    assert "normals0" not in names and "gicp_epsilon" not in names and "icp_mrmse" in R.SymPoseResult.__dataclass_fields__
    harness.Config(icp_estimation="gicp").check_icp()
    harness.Config(icp_estimation="gicp", icp_max_iter=5, gicp_epsilon=2.0 ** -10).check_icp()
    assert harness.Config(icp_estimation="gicp", icp_max_iter=5).icp_plane() and not harness.Config(icp_estimation="gicp").icp_plane()
    for bad in (dict(icp_kernel="huber"), dict(icp_with_scaling=True, icp_max_iter=3), dict(gicp_epsilon=0.0),
                dict(gicp_epsilon=1.5), dict(gicp_epsilon=math.nan)):
        with pytest.raises(ValueError):
            harness.Config(icp_estimation="gicp", **bad).check_icp()
    x = np.zeros((4, 3), np.float32)
    for kw in (dict(kernel="huber", kernel_scale=0.1), dict(with_scaling=True)):
        with pytest.raises(ValueError, match="out of scope"):
            B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], np.eye(4, dtype=np.float32)[None], 0.1, 1, tgt_normals=x,
                        estimation="gicp", src_normals=x, **kw)
    for kw in (dict(icp_kernel="tukey", icp_kernel_scale=0.1), dict(icp_with_scaling=True)):
        with pytest.raises(ValueError, match="out of scope"):
            R.sym_pose_batch(None, None, [0], None, None, [0], [], icp_max_iter=3, icp_max_dist=0.1, icp_estimation="gicp", **kw)
    for mod in (harness, shapenet_eval):
        req = ["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"] if mod is harness else ["--ckpt", "c"]
        a = mod.build_parser().parse_args(req + ["--icp-estimation", "gicp", "--gicp-epsilon", "0.01"])
        assert a.icp_estimation == "gicp" and a.gicp_epsilon == 0.01
        assert mod.build_parser().parse_args(req).gicp_epsilon == 1e-3
    assert shapenet_eval.Config().gicp_epsilon == 1e-3
