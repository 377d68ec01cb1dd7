"""The robust point-to-plane ICP without a GPU: tests/icp_robust_ref.py (the bit-exact restatement of
cs_icp_plane_robust_batch the GPU tests compare with) against tests/icp_plane_ref.py for kernel = L2, against an independent
weighted loop -- SciPy's KD-tree, NumPy weights, numpy.linalg.solve --, its fixed-point bounds, the edges of the weights and
the clutter fixture that motivates the kernels."""
import functools
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import icp_plane_ref as plane_ref
from tests import icp_ref
from tests import icp_robust_ref as ref
from tests.test_icp_plane_cpu import FIXTURES, _cayley, _fix

KERNELS = (("huber", 0.01), ("cauchy", 0.01), ("tukey", 0.02))
FIELDS = ("T", "T32", "fitness", "rmse", "iters", "ncorr", "corr", "sums")


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the clutter fixture ---------------------------------------------------------------------------------------------
BOX = np.array([0.5, 0.3, 0.4])
CLUTTER_MAX_DIST = 0.06


def _box_surface(rng, n):
    """n uniform samples of the surface of the box [-BOX, BOX] with the faces' outward normals."""
    area = np.array([BOX[1] * BOX[2], BOX[0] * BOX[2], BOX[0] * BOX[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    sign = rng.choice([-1.0, 1.0], n)
    pts = rng.uniform(-1, 1, (n, 3)) * BOX
    nrm = np.zeros((n, 3))
    pts[np.arange(n), axis] = sign * BOX[axis]
    nrm[np.arange(n), axis] = sign
    return pts, nrm


def _rotation(axis, deg):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def pose_errors(T, Tgt):
    """(RRE in degrees, RTE) of the 4x4 T against the true pose."""
    T, Tgt = np.asarray(T, np.float64).reshape(4, 4), np.asarray(Tgt, np.float64).reshape(4, 4)
    c = (np.trace(T[:3, :3] @ Tgt[:3, :3].T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, c))))), float(np.linalg.norm(T[:3, 3] - Tgt[:3, 3]))


@functools.lru_cache(maxsize=None)
def clutter_fixture():
    """Target: 900 samples of a box surface with its analytic normals.  Source: 360 further samples of it and 140 rows of
    clutter (28 %) on two slabs 0.035 outside the +x and the +y face, each within 0.05 of a target row and so inside
    max_dist = 0.06, moved by the inverse of a 25 degree pose.  Start: the true pose perturbed by 2 degrees and 0.012.
    Returns (src, tgt, nrm, T0, Tgt)."""
    rng = np.random.default_rng(1)
    tgt, nrm = _box_surface(rng, 900)
    good, _ = _box_surface(rng, 360)
    tree = cKDTree(tgt)
    slab = []
    for axis in (0, 1):
        rows = 0
        while rows < 70:
            c = rng.uniform(-1, 1, 3) * BOX
            c[axis] = BOX[axis] + 0.035
            if tree.query(c)[0] < 0.05:
                slab.append(c)
                rows += 1
    slab = np.array(slab)
    Tgt = np.eye(4)
    Tgt[:3, :3] = _rotation([0.3, -0.5, 0.8], 25.0)
    Tgt[:3, 3] = [0.2, -0.1, 0.15]
    Tinv = np.linalg.inv(Tgt)
    src = np.concatenate([good, slab]) @ Tinv[:3, :3].T + Tinv[:3, 3]
    D = np.eye(4)
    D[:3, :3] = _rotation([0.6, 0.7, -0.4], 2.0)
    T0 = D @ Tgt
    d = np.array([0.5, -0.6, 0.62])
    T0[:3, 3] = Tgt[:3, 3] + 0.012 * d / np.linalg.norm(d)
    return src.astype(np.float32), tgt.astype(np.float32), nrm.astype(np.float32), T0.astype(np.float32), Tgt


@functools.lru_cache(maxsize=None)
def clutter_ref(kernel, scale):
    src, tgt, nrm, T0, _ = clutter_fixture()
    return ref.icp(src, tgt, nrm, T0, CLUTTER_MAX_DIST, 30, kernel=kernel, kernel_scale=scale)


def test_clutter_fixture_shows_the_bias_and_tukey_removes_it():
    """Measured on the restatement (RRE degrees / RTE / updates): start 2.000 / 0.01200; L2 0.232 / 0.01980 / 5; Huber(0.01)
    0.252 / 0.00938 / 6; Cauchy(0.01) 0.096 / 0.00279 / 6; Tukey(0.02) 0.025 / 0.000091 / 4 -- RTE(L2) / RTE(Tukey) = 217.
    Asserted: the L2 refinement leaves the translation WORSE than the start (the fixture shows the bias), Tukey's RTE is
    below a tenth of L2's, and the fixture's ratio stays above 50."""
    src, tgt, nrm, T0, Tgt = clutter_fixture()
    assert len(src) == 500 and len(tgt) == 900
    start = pose_errors(T0, Tgt)
    print("start: RRE %.3f RTE %.5f" % start)
    err = {}
    for name, k in (("l2", 1.0),) + KERNELS:
        r = clutter_ref(name, k)
        err[name] = pose_errors(r["T"], Tgt)
        print("%s(%g): updates %d RRE %.4f RTE %.6f fitness %.3f wfitness %.3f"
              % (name, k, r["iters"], err[name][0], err[name][1], r["fitness"], r["wfitness"]))
    assert abs(start[0] - 2.0) < 1e-3 and abs(start[1] - 0.012) < 1e-6
    assert err["l2"][1] > start[1]
    assert err["tukey"][1] < err["l2"][1] / 10
    assert err["l2"][1] / err["tukey"][1] > 50
    # the gate keeps the clutter (L2's fitness counts it); Tukey's weighted share stays below the 72 % that are surface
    assert clutter_ref("l2", 1.0)["fitness"] > 0.9 and 0.5 < clutter_ref("tukey", 0.02)["wfitness"] < 0.72


# ---- L2 identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,ns,nt", FIXTURES[1:])
def test_l2_is_the_plane_restatement(seed, ns, nt):
    src, tgt, nrm, T0, _ = _fix(seed, ns, nt)
    for max_iter in (0, 30):
        want = plane_ref.icp(src, tgt, nrm, T0, 0.1, max_iter)
        got = ref.icp(src, tgt, nrm, T0, 0.1, max_iter, kernel="l2", kernel_scale=math.nan)     # the scale is ignored
        for k in FIELDS[:-1]:
            assert _bits_equal(got[k], want[k]), k
        assert got["sums"][:29] == want["sums"]
        assert got["wfitness"] == got["fitness"]                  # every weight is 1
        assert got["sums"][29] == want["sums"][0] * 2 ** (61 - icp_ref.frame(tgt, ns, 0.1)["eN"])


# ---- independent loop ------------------------------------------------------------------------------------------------
def _np_weight(kernel, r, k):
    a = np.abs(r)
    if kernel == "huber":
        return np.where(a <= k, 1.0, k / np.maximum(a, 1e-300))
    if kernel == "cauchy":
        return 1.0 / (1.0 + (r / k) ** 2)
    if kernel == "tukey":
        return np.where(a < k, (1.0 - (r / k) ** 2) ** 2, 0.0)
    return np.ones_like(r)


def _solve_icp(src, tgt, nrm, T0, max_dist, max_iter, kernel, k, rf=1e-6, rr=1e-6):
    """Open3D's loop with SciPy's KD-tree, NumPy weights and numpy.linalg.solve on the weighted 6x6 normal equations, in
    plain f64; the update is the specification's Cayley rotation about the midpoint o of the target's bounding box."""
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
    it, wfit = 0, 0.0
    for _ in range(max_iter + 1):
        P, Q, N = p[keep], tgt[j[keep]], nrm[j[keep]]
        r = ((P - Q) * N).sum(1)
        w = _np_weight(kernel, r, k)
        wfit = float(w.sum()) / len(src)
        if n < 6 or it == max_iter:
            break
        J = np.concatenate([np.cross(P - o, N), N], 1)
        x = np.linalg.solve((J * w[:, None]).T @ J, -((J * w[:, None]).T @ r))
        U = np.eye(4)
        U[:3, :3] = _cayley(x[:3])
        U[:3, 3] = x[3:] + o - U[:3, :3] @ o
        T = U @ T
        it += 1
        pf, pr = fit, rm
        p, j, keep, fit, rm, n = evaluate(T)
        if abs(fit - pf) < rf and abs(rm - pr) < rr:
            P, Q, N = p[keep], tgt[j[keep]], nrm[j[keep]]
            wfit = float(_np_weight(kernel, ((P - Q) * N).sum(1), k).sum()) / len(src)
            break
    return T, it, np.where(keep, j, -1), fit, rm, wfit


# largest max |T - T_solve| measured over the cases below: 5.4e-15 (clutter fixture, Tukey); asserted with a margin of 10
INDEPENDENT_BOUND = 5.4e-14


@pytest.mark.parametrize("kernel,k", KERNELS)
def test_restatement_against_kdtree_weights_and_solve(kernel, k):
    """Correspondences and update counts identical, wfitness within 1e-12, the final transform within INDEPENDENT_BOUND (max
    abs over the 16 entries) of the independent loop's, on the clutter fixture (scales of KERNELS) and on fixture 2 of the
    plane tests (257 x 513, scale 3 k).  Measured max |T - T_solve|, clutter / fixture 2: Huber 3.3e-15 / 6.0e-16, Cauchy
    3.2e-15 / 1.5e-15, Tukey 5.4e-15 / 2.1e-15 (6, 6, 4 and 9, 9, 9 updates).  What separates the two: the truncation of the fixed-point sums, the
    unpivoted Cholesky against LAPACK's LU and the order of the f64 sums."""
    src, tgt, nrm, T0, _ = clutter_fixture()
    cases = [("clutter", src, tgt, nrm, T0, CLUTTER_MAX_DIST, k, clutter_ref(kernel, k))]
    s2, t2, n2, T2, _ = _fix(*FIXTURES[1])
    cases.append(("fixture 2", s2, t2, n2, T2, 0.1, 3 * k, ref.icp(s2, t2, n2, T2, 0.1, 30, kernel=kernel, kernel_scale=3 * k)))
    for name, s, t, n, T, md, kk, got in cases:
        Tk, itk, corr_k, fit_k, rm_k, wfit_k = _solve_icp(s, t, n, T, md, 30, kernel, kk)
        diff = float(np.abs(got["T"].reshape(4, 4) - Tk).max())
        print("%s %s(%g): updates %d / %d, max |T - T_solve| = %.3g, wfitness %.6f / %.6f"
              % (name, kernel, kk, got["iters"], itk, diff, got["wfitness"], wfit_k))
        assert got["iters"] == itk and 1 < itk < 30
        assert np.array_equal(got["corr"], corr_k)
        assert got["fitness"] == fit_k and abs(got["wfitness"] - wfit_k) < 1e-12
        assert diff <= INDEPENDENT_BOUND


# ---- bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,max_dist", ((1.0, 0.1), (50.0, 3.0)))
def test_no_weighted_term_reaches_its_clamp(scale, max_dist):
    """Unit-sized and 50-unit clouds, every kernel: the weights lie in [0, 1], the largest scaled weighted term stays below
    its clamp 2^(61 - eN), every sum (the 30th included) within 2^61, and no weighted term exceeds the unweighted one."""
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[1])
    S = np.diag([scale, scale, scale, 1.0])
    T0s = (S @ T0.astype(np.float64) @ np.linalg.inv(S)).astype(np.float32)
    srcs, tgts = (src * scale).astype(np.float32), (tgt * scale).astype(np.float32)
    plain = {}
    plane_ref.icp(srcs, tgts, nrm, T0s, max_dist, 0, watch=plain)
    for kernel, k in KERNELS:
        watch = {}
        got = ref.icp(srcs, tgts, nrm, T0s, max_dist, 3, kernel=kernel, kernel_scale=k * scale, watch=watch)
        print("scale %g %s: largest |term| / clamp = %.3g, largest |sum| = 2^%.1f, w in [%.3g, %.3g]"
              % (scale, kernel, watch["term"], math.log2(watch["sum"]), watch["wmin"], watch["wmax"]))
        assert got["ncorr"] > 128 and got["iters"] >= 2
        assert 0.0 <= watch["wmin"] <= watch["wmax"] <= 1.0
        assert watch["term"] < 1.0 and watch["sum"] <= 2 ** 61
        assert 0.0 <= got["wfitness"] <= got["fitness"]
        first = {}
        ref.icp(srcs, tgts, nrm, T0s, max_dist, 0, kernel=kernel, kernel_scale=k * scale, watch=first)
        assert first["term"] <= plain["term"]


def test_long_and_nan_normals_give_defined_sums():
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[1])
    bad = nrm.copy()
    bad[::7] = np.nan
    for kernel, k in KERNELS:
        watch = {}
        got = ref.icp(src, tgt, nrm * np.float32(1e3), T0, 0.1, 30, kernel=kernel, kernel_scale=k, watch=watch)
        assert all(abs(v) <= 2 ** 61 for v in got["sums"]) and np.all(np.isfinite(got["T"]))
        assert 0.0 <= watch["wmin"] <= watch["wmax"] <= 1.0
        got = ref.icp(src, tgt, bad, T0, 0.1, 30, kernel=kernel, kernel_scale=k)
        assert all(abs(v) <= 2 ** 61 for v in got["sums"]) and np.all(np.isfinite(got["T"]))
        assert math.isfinite(got["wfitness"]) and 0.0 <= got["wfitness"] <= got["fitness"]


# ---- weight edges ----------------------------------------------------------------------------------------------------
def test_weight_edges():
    for kernel in (ref.L2, ref.HUBER, ref.CAUCHY, ref.TUKEY):
        assert ref.weight(kernel, 0.0, 0.25) == 1.0 and ref.weight(kernel, -0.0, 1e-300) == 1.0
        assert ref.weight(kernel, math.nan, 0.25) in (0.0, 1.0) and ref.weight(kernel, math.nan, 0.25) == (kernel == ref.L2)
        for r in (1e-9, -0.1, 0.24999, 0.25, -0.25, 0.26, 7.0, 1e200, -math.inf):
            assert 0.0 <= ref.weight(kernel, r, 0.25) <= 1.0
    assert ref.weight(ref.HUBER, 0.25, 0.25) == 1.0 and ref.weight(ref.HUBER, -0.5, 0.25) == 0.5
    assert ref.weight(ref.TUKEY, 0.25, 0.25) == 0.0 and ref.weight(ref.TUKEY, -0.25, 0.25) == 0.0
    assert ref.weight(ref.TUKEY, 0.125, 0.25) == 0.5625 and ref.weight(ref.CAUCHY, 0.25, 0.25) == 0.5
    assert ref.weight(ref.CAUCHY, 1e200, 0.25) == 0.0 and ref.weight(ref.HUBER, math.inf, 0.25) == 0.0


def edge_case():
    """A source exactly k = 0.25 above a z = 0 grid with normals (0, 0, 1): r = 0.25 for every pair, exact in f32."""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2) * 0.0625
    tgt = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(tgt), 1))
    src = (tgt[8:48] + np.float32([0.0, 0.0, 0.25])).astype(np.float32)
    return src, tgt, nrm, np.eye(4, dtype=np.float32)


def test_residual_equal_to_the_scale_and_all_zero_weights():
    src, tgt, nrm, eye = edge_case()
    huber = ref.icp(src, tgt, nrm, eye, 0.3, 0, kernel="huber", kernel_scale=0.25)
    assert huber["ncorr"] == len(src) and huber["wfitness"] == 1.0            # |r| = k exactly: Huber's weight is 1
    assert huber["sums"][:29] == plane_ref.icp(src, tgt, nrm, eye, 0.3, 0)["sums"]
    tukey = ref.icp(src, tgt, nrm, eye, 0.3, 30, kernel="tukey", kernel_scale=0.25)
    assert tukey["ncorr"] == len(src) and tukey["fitness"] == 1.0 and tukey["rmse"] == 0.25
    assert all(v == 0 for v in tukey["sums"][1:28]) and tukey["sums"][29] == 0  # ... and Tukey's is 0: A = 0 exactly
    assert tukey["iters"] == 0 and tukey["wfitness"] == 0.0                   # the pivot rule stops it with T = T0
    assert np.array_equal(tukey["T"], eye.reshape(16).astype(np.float64)) and np.array_equal(tukey["T32"], eye.reshape(16))
    below = ref.icp(src, tgt, nrm, eye, 0.3, 0, kernel="tukey", kernel_scale=0.5)
    assert below["wfitness"] == 0.5625                                        # (1 - 0.25)^2 for every pair


def test_surface_is_declared():
    import inspect
    import os

    from corsair_amd import _lib, backend as B, harness, registration as R, shapenet_eval as S

    header = open(_lib.HEADER_PATH).read()
    assert "cs_icp_plane_robust_batch" in _lib.header_symbols()
    for word in ("CS_ICP_KERNEL_L2 0", "CS_ICP_KERNEL_HUBER 1", "CS_ICP_KERNEL_CAUCHY 2", "CS_ICP_KERNEL_TUKEY 3",
                 "d_wfitness", "[O3D-knowledge]", "kernel_scale"):
        assert word in header, word
    assert B.ICP_KERNELS == ref.KERNELS
    sig = inspect.signature(B.icp_batch).parameters
    assert sig["kernel"].default == "l2" and sig["kernel_scale"].default is None
    assert "wfitness" in B.IcpResult._fields
    sig = inspect.signature(R.sym_pose_batch).parameters
    assert list(sig)[-2:] == ["icp_kernel", "icp_kernel_scale"] and sig["icp_kernel"].default == "l2"
    assert R.SymPoseResult.__dataclass_fields__["icp_wfitness"].default is None
    for Config in (harness.Config, S.Config):
        c = Config()
        assert c.icp_kernel == "l2" and c.icp_kernel_scale == 0.0 and c.icp_scale() == c.voxel_size
        assert Config(icp_kernel_scale=0.5).icp_scale() == 0.5
    from tests.helpers import assert_five_icp_kernels

    assert_five_icp_kernels()          # the robust path adds no kernel of its own


def test_config_and_command_lines():
    from corsair_amd import harness, shapenet_eval as S

    harness.Config(icp_estimation="plane", icp_kernel="tukey").check_icp()
    harness.Config().check_icp()
    with pytest.raises(ValueError, match="icp_kernel"):
        harness.Config(icp_estimation="plane", icp_kernel="gm").check_icp()
    with pytest.raises(ValueError, match="plane"):
        harness.Config(icp_estimation="point", icp_kernel="huber").check_icp()
    base = ["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"]
    a = harness.build_parser().parse_args(base + ["--icp-kernel", "cauchy", "--icp-kernel-scale", "0.02"])
    assert a.icp_kernel == "cauchy" and a.icp_kernel_scale == 0.02
    a = harness.build_parser().parse_args(base)
    assert a.icp_kernel == "l2" and a.icp_kernel_scale == 0.0
    a = S.build_parser().parse_args(["--ckpt", "c", "--icp-kernel", "tukey", "--icp-kernel-scale", "0.5"])
    assert a.icp_kernel == "tukey" and a.icp_kernel_scale == 0.5
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(["--ckpt", "c", "--icp-kernel", "gm"])
