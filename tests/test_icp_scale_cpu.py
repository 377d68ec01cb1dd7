"""The ICP with an isotropic scale without a GPU: tests/icp_scale_ref.py (the bit-exact restatement of cs_icp_scale_batch the
GPU tests compare with) against the rigid restatements it shares its code with, against an independent loop -- SciPy's
KD-tree, an SVD Umeyama fit, numpy.linalg.solve on the 7x7 system, plain f64 --, on a recovery fixture with a known size
mismatch, its fixed-point bounds, its stop rules, and the cache's separate scale name."""
import functools
import math
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import icp_plane_ref, icp_ref
from tests import icp_scale_ref as ref
from tests import normals_ref
from tests.test_icp_cpu import _fixture, _perturbed

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_scale_boxes.npz")
FIXTURES = ((1, 300, 1400), (2, 257, 513))


@functools.lru_cache(maxsize=None)
def _fix(seed, ns, nt, scale=1.0):
    """tests/test_icp_cpu.py's fixture with the source shrunk by `scale` about the origin of its own frame."""
    src, tgt, T0, Tgt = _fixture(seed, ns, nt)
    src = (src.astype(np.float64) / scale).astype(np.float32)
    return src, tgt, normals_ref.estimate_normals(tgt, [0, len(tgt)], 16), T0, Tgt


def _cayley(a):
    q = np.array([1.0, a[0] / 2, a[1] / 2, a[2] / 2])
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _umeyama(P, Q):
    """U = [s R | t] minimising sum |s R p + t - q|^2 (Umeyama 1991), by NumPy's SVD."""
    mp, mq = P.mean(0), Q.mean(0)
    Pc, Qc = P - mp, Q - mq
    Uu, D, Vt = np.linalg.svd(Qc.T @ Pc / len(P))
    E = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Uu) * np.linalg.det(Vt) > 0 else -1.0])
    R = Uu @ E @ Vt
    var = (Pc * Pc).sum() / len(P)
    s = float((D * np.diag(E)).sum() / var) if var > 0 else math.nan
    return s, R, mq - s * (R @ mp)


def _indep_icp(src, tgt, nrm, T0, max_dist, max_iter, bounds=(0.5, 2.0), scaling=True, rf=1e-6, rr=1e-6):
    """Open3D's loop with SciPy's KD-tree, everything in plain f64: Umeyama by SVD (nrm None) or numpy.linalg.solve on the
    7x7 normal equations with the specification's update about the midpoint o of the target's bounding box.  Returns
    (T, scale, updates, correspondences, fitness, rmse)."""
    src, tgt = src.astype(np.float64), tgt.astype(np.float64)
    plane = nrm is not None
    if plane:
        nrm = nrm.astype(np.float64)
    o = 0.5 * (tgt.min(0) + tgt.max(0))
    tree = cKDTree(tgt)
    T = np.asarray(T0, np.float32).astype(np.float64).reshape(4, 4).copy()
    nmin = (7 if scaling else 6) if plane else 3

    def evaluate(T):
        p = src @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(p)
        keep = d * d < max_dist * max_dist
        n = int(keep.sum())
        return p, j, keep, n / len(src), (math.sqrt(float((d[keep] ** 2).sum()) / n) if n else 0.0), n

    p, j, keep, fit, rm, n = evaluate(T)
    it, scale = 0, 1.0
    for _ in range(max_iter):
        if n < nmin:
            break
        P, Q = p[keep], tgt[j[keep]]
        U = np.eye(4)
        if plane:
            N = nrm[j[keep]]
            r = ((P - Q) * N).sum(1)
            cols = [np.cross(P - o, N), N] + ([((P - o) * N).sum(1)[:, None]] if scaling else [])
            J = np.concatenate(cols, 1)
            try:
                x = np.linalg.solve(J.T @ J, -(J.T @ r))
            except np.linalg.LinAlgError:
                break
            su = 1.0 + x[6] if scaling else 1.0
            U[:3, :3] = su * _cayley(x[:3])
            U[:3, 3] = x[3:6] + o - U[:3, :3] @ o
        else:
            su, R, t = _umeyama(P, Q)
            if not scaling:
                su, t = 1.0, Q.mean(0) - R @ P.mean(0)
            U[:3, :3], U[:3, 3] = su * R, t
        if not (math.isfinite(su) and su > 0 and bounds[0] <= su * scale <= bounds[1]):
            break
        T, scale = U @ T, su * scale
        it += 1
        pf, pr = fit, rm
        p, j, keep, fit, rm, n = evaluate(T)
        if abs(fit - pf) < rf and abs(rm - pr) < rr:
            break
    return T, scale, it, np.where(keep, j, -1), fit, rm


# ---- (a) what the scaled restatement shares with the rigid ones ----------------------------------------------------------
@pytest.mark.parametrize("seed,ns,nt", FIXTURES)
def test_scaling_off_is_the_rigid_restatement(seed, ns, nt):
    """with_scaling = False runs this file's loop, sums and solvers with six columns / 17 sums: T, T32, fitness, rmse,
    correspondences, counts AND the sums are the bits of icp_ref.icp and icp_plane_ref.icp."""
    src, tgt, nrm, T0, _ = _fix(seed, ns, nt)
    for normals, want in ((None, icp_ref.icp(src, tgt, T0, 0.1, 30)), (nrm, icp_plane_ref.icp(src, tgt, nrm, T0, 0.1, 30))):
        got = ref.icp(src, tgt, normals, T0, 0.1, 30, with_scaling=False)
        assert got["iters"] == want["iters"] > 1 and got["ncorr"] == want["ncorr"] and got["sums"] == want["sums"]
        assert np.array_equal(got["corr"], want["corr"]) and got["scale"] == 1.0
        assert got["T"].tobytes() == want["T"].tobytes() and got["T32"].tobytes() == want["T32"].tobytes()
        assert (got["fitness"], got["rmse"]) == (want["fitness"], want["rmse"])


@pytest.mark.parametrize("seed,ns,nt", FIXTURES)
def test_bounds_one_one_keep_the_start(seed, ns, nt):
    """The interval (1, 1) admits only s_u = 1 exactly, so the first update is refused by the interval rule (its s_u is
    printed) and the answer is the rigid entry's for max_iter = 0, bit for bit: T = T0, the correspondences, counts, fitness
    and rmse of the first evaluation, 0 updates.  That is the case in which the specification makes T equal to a rigid
    result; with a wider interval the first update already differs by its scale.  The first 17 sums of the point layout
    and the count / d2 sums of the plane layout are the rigid ones for the same association."""
    src, tgt, nrm, T0, _ = _fix(seed, ns, nt)
    for normals, want in ((None, icp_ref.icp(src, tgt, T0, 0.1, 0)), (nrm, icp_plane_ref.icp(src, tgt, nrm, T0, 0.1, 0))):
        got = ref.icp(src, tgt, normals, T0, 0.1, 30, scale_bounds=(1.0, 1.0))
        free = ref.icp(src, tgt, normals, T0, 0.1, 1)
        print("first s_u = %.17g" % free["scale"])
        assert free["iters"] == 1 and free["scale"] != 1.0
        assert got["iters"] == 0 and got["scale"] == 1.0 and got["T"].tobytes() == want["T"].tobytes()
        assert np.array_equal(got["corr"], want["corr"]) and got["ncorr"] == want["ncorr"]
        assert (got["fitness"], got["rmse"]) == (want["fitness"], want["rmse"])
        if normals is None:
            assert got["sums"][:17] == want["sums"]
        else:
            assert (got["sums"][0], got["sums"][36]) == (want["sums"][0], want["sums"][28])


# ---- (b) the independent loop ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", (False, True))
@pytest.mark.parametrize("seed,ns,nt,scale", ((1, 300, 1400, 1.05), (2, 257, 513, 0.95)))
def test_restatement_against_kdtree_svd_and_solve(seed, ns, nt, scale, plane):
    """Correspondences identical (no ties in these clouds), the same number of updates; transform and scale within the
    measured largest difference x 10.  Measured over the four cases, max |T - T_indep| and |scale - scale_indep|:
    point 1.0e-15 / 8.9e-16 (7 and 12 updates), plane 1.09e-14 / 3.2e-15 (5 and 8 updates) -> asserted 1.0e-14 and 1.1e-13
    on T, 8.9e-15 and 3.2e-14 on the scale.  What separates the two: the truncation of the fixed-point sums, Horn's
    quaternion against the SVD, the unpivoted Cholesky against LAPACK's LU, and the order of the f64 sums."""
    src, tgt, nrm, T0, _ = _fix(seed, ns, nt, scale)
    normals = nrm if plane else None
    got = ref.icp(src, tgt, normals, T0, 0.1, 40)
    Tk, sk, itk, corr_k, fit_k, rm_k = _indep_icp(src, tgt, normals, T0, 0.1, 40)
    dT = float(np.abs(got["T"].reshape(4, 4) - Tk).max())
    ds = abs(got["scale"] - sk)
    print("seed %d %s: updates %d / %d, scale %.6f, max |T - T_indep| = %.3g, |scale - scale_indep| = %.3g"
          % (seed, "plane" if plane else "point", got["iters"], itk, got["scale"], dT, ds))
    assert got["iters"] == itk and 1 < itk < 40
    assert np.array_equal(got["corr"], corr_k)
    assert got["fitness"] == fit_k
    assert dT <= (1.1e-13 if plane else 1.0e-14) and ds <= (3.2e-14 if plane else 8.9e-15)
    # the scale is the factor the call added: the cube root of the determinant of T's upper block (T0 is rigid)
    det = float(np.linalg.det(got["T"].reshape(4, 4)[:3, :3])) / float(np.linalg.det(T0.astype(np.float64)[:3, :3]))
    assert abs(det ** (1.0 / 3.0) - got["scale"]) < 1e-12


# ---- (c) recovery -------------------------------------------------------------------------------------------------------------
def _errors(T, scale_est, Tgt, s_true):
    """(RRE degrees, RTE, scale error) of a similarity T against s_true * R_gt, t_gt."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    R = T[:3, :3] / scale_est
    c = (np.trace(R @ Tgt[:3, :3].T) - 1.0) / 2.0
    return (math.degrees(math.acos(min(1.0, max(-1.0, c)))), float(np.linalg.norm(T[:3, 3] - Tgt[:3, 3])),
            abs(scale_est / s_true - 1.0))


@functools.lru_cache(maxsize=None)
def _boxes():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _recovery_case(view, s_true):
    """The fixture's source of that view, shrunk by s_true and moved by a pose; the start is the true ROTATION and
    translation perturbed by 5 degrees / 0.02 with scale 1."""
    from corsair_amd import synth

    z = _boxes()
    seed = 11 + (0 if view == "full" else 1)
    Tgt = synth.random_pose(seed, max_trans=0.3)
    src_t = z["src_" + view].astype(np.float64)               # in the target's frame, true size
    # tgt = s R x + t  <=>  x = R^T (tgt - t) / s
    src = ((src_t - Tgt[:3, 3]) @ Tgt[:3, :3]) / s_true
    return src.astype(np.float32), z["tgt"], z["nrm"], _perturbed(Tgt, 5.0, 0.02, seed), Tgt, float(z["voxel"])


@functools.lru_cache(maxsize=None)
def _recovery_run(view, s_true, plane, scaling, restated):
    src, tgt, nrm, T0, Tgt, voxel = _recovery_case(view, s_true)
    normals = nrm if plane else None
    if restated:
        r = ref.icp(src, tgt, normals, T0, 2 * voxel, 60, with_scaling=scaling)
        T, sc, it = r["T"], r["scale"], r["iters"]
    else:
        T, sc, it = _indep_icp(src, tgt, normals, T0, 2 * voxel, 60, scaling=scaling)[:3]
    return _errors(T, sc, Tgt, s_true) + (it,)


@pytest.mark.parametrize("view", ("full", "half"))
@pytest.mark.parametrize("s_true", (1.05, 0.9))
def test_recovery_of_a_size_mismatch(view, s_true):
    """tests/golden/icp_scale_boxes.npz (a box-set chair, one sample per 0.04 voxel; a full view and a half-space view),
    true scale 1.05 and 0.9, start 5 degrees / 0.02 off with scale 1, max_dist = 2 voxels, max_iter 60.  The rigid
    estimations end with scale error = the mismatch |1 / s - 1| by construction.  Required of the restatement AND of the
    independent loop: plane + scale ends at most 0.25 of the mismatch off, point + scale at most 0.5, both with a smaller RRE
    and RTE than their rigid siblings.  The measured figures are printed and recorded in DESIGN 16."""
    mismatch = abs(1.0 / s_true - 1.0)
    for restated in (False, True):
        for plane, bar in ((True, 0.25), (False, 0.5)):
            rigid = _recovery_run(view, s_true, plane, False, restated)
            scaled = _recovery_run(view, s_true, plane, True, restated)
            print("%s s=%.2f %s %s: rigid RRE %.3f RTE %.4f (%d updates) | scaled RRE %.3f RTE %.4f scale error %.5f = %.3f of "
                  "the mismatch (%d updates)" % (view, s_true, "restated" if restated else "independent",
                                                 "plane" if plane else "point", rigid[0], rigid[1], rigid[3], scaled[0],
                                                 scaled[1], scaled[2], scaled[2] / mismatch, scaled[3]))
            assert abs(rigid[2] - mismatch) < 1e-12
            assert scaled[2] <= bar * mismatch
            assert scaled[0] < rigid[0] and scaled[1] < rigid[1]


@pytest.mark.parametrize("view", ("full", "half"))
def test_scaling_costs_nothing_when_the_sizes_agree(view):
    """True scale 1.0: scaling on leaves RRE and RTE within a factor of 2 of scaling off (both estimations, restated)."""
    for plane in (True, False):
        rigid = _recovery_run(view, 1.0, plane, False, True)
        scaled = _recovery_run(view, 1.0, plane, True, True)
        print("%s %s: rigid RRE %.4f RTE %.5f | scaled RRE %.4f RTE %.5f scale error %.5f"
              % (view, "plane" if plane else "point", rigid[0], rigid[1], scaled[0], scaled[1], scaled[2]))
        assert scaled[0] <= 2.0 * rigid[0] and scaled[1] <= 2.0 * rigid[1]


# ---- (d) bounds of the sums ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", (False, True))
@pytest.mark.parametrize("size,max_dist", ((1.0, 0.1), (50.0, 3.0)))
def test_no_term_reaches_its_clamp(size, max_dist, plane):
    """Unit-sized and 50-unit clouds: the largest scaled term stays below its clamp 2^(61 - eN) and every sum below 2^61."""
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[1], 1.05)
    S = np.diag([size, size, size, 1.0])
    T0s = (S @ T0.astype(np.float64) @ np.linalg.inv(S)).astype(np.float32)
    watch = {}
    got = ref.icp((src * size).astype(np.float32), (tgt * size).astype(np.float32), nrm if plane else None, T0s, max_dist, 3,
                  watch=watch)
    print("size %g: largest |term| / clamp = %.3g, largest |sum| = 2^%.1f" % (size, watch["term"], math.log2(watch["sum"])))
    assert got["ncorr"] > 128 and got["iters"] >= 2
    assert watch["term"] < 1.0 and watch["sum"] < 2 ** 61


def test_scales_and_their_bounds():
    rng = np.random.default_rng(0)
    for n_src, size, max_dist in ((1, 1.0, 0.1), (5000, 1.0, 0.06), (2 ** 31 - 1, 50.0, 3.0), (257, 1e-3, 1e-4),
                                  (1000, 3e38, 1.0)):
        tgt = (rng.uniform(-1, 1, (64, 3)) * size).astype(np.float32)
        fr = ref.scale_frame(icp_ref.frame(tgt, n_src, max_dist))
        lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
        M = float(np.max(0.5 * (hi - lo))) + max_dist
        c = fr["clamp"]
        # p'.p' <= 3 M^2 < 4 M^2 <= 2^(2 eM + 2); J_6 = p'.n with |J_6| <= sqrt(3) M < 2 M joins the rotational classes
        assert 3 * M * M * fr["sc_pp"] < c and fr["sc_pp"] * fr["inv_pp"] == 1.0 and -1022 < fr["s_pp"] < 1023
        assert fr["sc_pp"] * 4 == fr["sc2"]
        j6 = math.sqrt(3.0) * M
        assert 2 * (j6 * j6) * fr["sc_rr"] <= c and 2 * (j6 * 2 * M) * fr["sc_rr"] <= c and 2 * j6 * fr["sc_rt"] <= c
        assert 2 * (j6 * max_dist) * fr["sc_rd"] <= c
    assert [ref.cls(i, 6) for i in range(7)] == ["rr", "rr", "rr", "rt", "rt", "rt", "rr"]
    assert [ref.cls(i, j) for i in range(6) for j in range(i, 6)] == \
        [icp_plane_ref._cls(i, j) for i in range(6) for j in range(i, 6)]


def test_long_normals_and_nan_rows_give_defined_answers():
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[1], 1.05)
    watch = {}
    got = ref.icp(src, tgt, nrm * np.float32(1e3), T0, 0.1, 30, watch=watch)
    assert watch["term"] >= 1.0                                 # terms did reach the clamp ...
    assert all(abs(v) < 2 ** 61 for v in got["sums"])           # ... and the sums stayed inside the bound
    assert np.all(np.isfinite(got["T"])) and math.isfinite(got["scale"]) and 0.5 <= got["scale"] <= 2.0
    bad = nrm.copy()
    bad[::7] = np.nan
    got = ref.icp(src, tgt, bad, T0, 0.1, 30)
    assert all(abs(v) < 2 ** 61 for v in got["sums"]) and np.all(np.isfinite(got["T"])) and math.isfinite(got["scale"])
    for normals in (None, nrm):
        s2, t2 = src.copy(), tgt.copy()
        s2[::5] = np.nan
        t2[::9] = np.nan
        got = ref.icp(s2, t2, normals, T0, 0.1, 30)
        assert all(abs(v) < 2 ** 61 for v in got["sums"]) and np.all(np.isfinite(got["T"])) and got["iters"] >= 1
        assert np.all(got["corr"][::5] == -1) and 0.5 <= got["scale"] <= 2.0


# ---- (e) stop rules -----------------------------------------------------------------------------------------------------------
def test_identical_posed_sources_stop_on_the_denominator():
    """Every source row the same dyadic point: the 18th sum equals sum_a sp_a mp_a exactly, the denominator is an exact 0
    and the point estimation stops with T = T0, scale 1, 0 updates."""
    tgt = (np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
           * 0.25).astype(np.float32)
    src = np.tile(np.float32([0.375, 0.5, 0.125]), (8, 1))
    T0 = np.eye(4, dtype=np.float32)
    got = ref.icp(src, tgt, None, T0, 0.5, 30)
    S, fr = got["sums"], ref.scale_frame(icp_ref.frame(tgt, 8, 0.5))
    den = float(S[17]) * fr["inv_pp"] - sum((float(S[1 + c]) * fr["inv1"]) ** 2 / 8.0 for c in range(3))
    assert den == 0.0 and got["ncorr"] == 8 and got["iters"] == 0 and got["scale"] == 1.0
    assert np.array_equal(got["T"], T0.reshape(16).astype(np.float64))


def test_pair_minimum():
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[0], 1.05)
    two = ref.icp(src[:2], tgt, None, T0, 0.1, 30)
    assert two["ncorr"] == 2 and two["iters"] == 0 and two["scale"] == 1.0 and np.array_equal(two["T32"], T0.reshape(16))
    assert ref.icp(src[:3], tgt, None, T0, 0.1, 30)["iters"] >= 1
    six = ref.icp(src[:6], tgt, nrm, T0, 0.1, 30)
    assert six["ncorr"] == 6 and six["iters"] == 0 and six["scale"] == 1.0 and np.array_equal(six["T32"], T0.reshape(16))
    # the rigid plane estimation goes on with six pairs where the scaled one needs seven
    assert icp_plane_ref.icp(src[:6], tgt, nrm, T0, 0.1, 0)["ncorr"] == 6
    assert ref.icp(src[:40], tgt, nrm, T0, 0.1, 30)["iters"] >= 1
    for normals in (None, nrm):
        for s, t, n in ((src[:0], tgt, normals), (src, tgt[:0], None if normals is None else normals[:0])):
            r = ref.icp(s, t, n, T0, 0.1, 30)
            assert (r["fitness"], r["rmse"], r["iters"], r["ncorr"], r["scale"]) == (0.0, 0.0, 0, 0, 1.0)


def test_exact_plane_stops_with_the_initial_transform():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) * 0.05
    tgt = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(tgt), 1))
    src = (tgt[10:100] + np.float32([0.004, -0.003, 0.01])).astype(np.float32)
    T0 = np.eye(4, dtype=np.float32)
    got = ref.icp(src, tgt, nrm, T0, 0.1, 30)
    A, _ = ref.normal_equations(got["sums"], ref.scale_frame(icp_ref.frame(tgt, len(src), 0.1)), 7)
    # J = (p'_y, -p'_x, 0, 0, 0, 1, p'_z): rows and columns 2, 3 and 4 are exactly zero -- the pivot of column 2 is an exact 0
    assert all(A[i][j] == 0.0 for i in (2, 3, 4) for j in range(7)) and A[0][0] > 0 and A[5][5] == len(src) and A[6][6] > 0
    assert got["iters"] == 0 and got["ncorr"] == len(src) and got["scale"] == 1.0
    assert np.array_equal(got["T"], T0.reshape(16).astype(np.float64))
    # the point estimation has no such rule: on the same planar target it goes on
    assert ref.icp(src, tgt, None, T0, 0.1, 30)["iters"] >= 1


@pytest.mark.parametrize("plane,bounds,applied", ((False, (0.95, 1.05), 1), (True, (0.95, 1.05), 0), (True, (0.9, 1.1), 1)))
def test_an_update_that_leaves_the_interval_is_not_applied(plane, bounds, applied):
    """A source 15 % too small inside a narrow interval: the update whose accumulated scale would pass the upper bound is
    refused, T and scale are those of before it and iters counts the applied updates only -- the state of a run that was
    given exactly that many updates.  With [0.95, 1.05] the plane fit's FIRST update (1.071) is refused, the point fit's
    second (1.043, then 1.086); with [0.9, 1.1] the plane fit applies one update (1.071) and is refused the second (1.120)."""
    src, tgt, nrm, T0, _ = _fix(*FIXTURES[0], 1.15)
    normals = nrm if plane else None
    free = ref.icp(src, tgt, normals, T0, 0.1, 30)
    got = ref.icp(src, tgt, normals, T0, 0.1, 30, scale_bounds=bounds)
    assert free["scale"] > 1.1 and free["iters"] > got["iters"] == applied
    assert bounds[0] <= got["scale"] <= bounds[1] and (got["scale"] != 1.0) == (applied > 0)
    upto = ref.icp(src, tgt, normals, T0, 0.1, got["iters"])
    one_more = ref.icp(src, tgt, normals, T0, 0.1, got["iters"] + 1)
    print("%s: stopped after %d applied updates at scale %.5f; the refused update would have given %.5f"
          % ("plane" if plane else "point", got["iters"], got["scale"], one_more["scale"]))
    assert one_more["scale"] > bounds[1] and one_more["iters"] == got["iters"] + 1
    assert got["T"].tobytes() == upto["T"].tobytes() and got["scale"] == upto["scale"]
    assert np.array_equal(got["corr"], upto["corr"]) and (got["fitness"], got["rmse"]) == (upto["fitness"], upto["rmse"])


def test_scale_step_rules():
    assert ref.scale_ok(1.0, 1.0, (1.0, 1.0)) == (True, 1.0)
    for su in (0.0, -1.0, math.nan, math.inf):
        assert not ref.scale_ok(su, 1.0, (0.5, 2.0))[0]
    assert not ref.scale_ok(1.1, 1.9, (0.5, 2.0))[0] and ref.scale_ok(1.05, 1.9, (0.5, 2.0))[0]
    assert not ref.scale_ok(0.9, 0.55, (0.5, 2.0))[0]


def test_cholesky_seven_against_numpy():
    rng = np.random.default_rng(4)
    J = rng.standard_normal((40, 7))
    A, b = J.T @ J, rng.standard_normal(7)
    x = ref.cholesky_solve(A.tolist(), b.tolist())
    assert np.abs(np.asarray(x) - np.linalg.solve(A, -b)).max() < 1e-12
    assert ref.cholesky_solve(A[:6, :6].tolist(), b[:6].tolist()) == icp_plane_ref.cholesky_solve(A[:6, :6].tolist(),
                                                                                                    b[:6].tolist())
    A[:, 6] = A[:, 0]
    A[6, :] = A[0, :]                                           # column 6 = column 0: the seventh pivot is a rounding residue
    assert ref.cholesky_solve(A.tolist(), b.tolist()) is None


def test_refused_bounds_and_surface():
    import inspect

    from corsair_amd import _lib, backend as B

    header = open(_lib.HEADER_PATH).read()
    assert "cs_icp_scale_batch" in _lib.header_symbols()
    for word in ("scale_min", "scale_max", "d_scale", "scale_min <= 0", "scale_min > 1", "scale_max < 1", "POSED"):
        assert word in header, word
    sig = inspect.signature(B.icp_batch).parameters
    assert sig["with_scaling"].default is False and sig["scale_bounds"].default == (0.5, 2.0)
    assert B.IcpResult._fields[-1] == "scale" and B.IcpResult._field_defaults["scale"] is None
    # the Python layer refuses before the library is reached (no GPU here): robust kernels with a scale, bad intervals
    z = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="robust"):
        B.icp_batch(z, [0, 4], z, [0, 4], [0], [0], np.eye(4, dtype=np.float32)[None], 0.1, tgt_normals=z, kernel="huber",
                    kernel_scale=0.1, with_scaling=True)
    for bad in ((0.0, 2.0), (-1.0, 2.0), (1.1, 2.0), (0.5, 0.9), (0.5, math.inf), (math.nan, 2.0)):
        with pytest.raises(ValueError, match="scale_bounds"):
            B.icp_batch(z, [0, 4], z, [0, 4], [0], [0], np.eye(4, dtype=np.float32)[None], 0.1, with_scaling=True,
                        scale_bounds=bad)
    from tests.helpers import assert_five_icp_kernels

    assert_five_icp_kernels()   # no kernel was added


# ---- (f) the cache ------------------------------------------------------------------------------------------------------------
def test_cache_scale_name_round_trip(tmp_path):
    from corsair_amd import cache as C

    assert C.NAMES == ("Ts_est_ransac", "Ts_est_best", "t_losses_ransac", "t_losses_sym", "r_losses_ransac",
                       "r_losses_sym", "sym_ransac_success", "chamfer_dist_ransac", "chamfer_dist_sym")
    assert C.ICP_NAMES == ("Ts_est_icp", "t_losses_icp", "r_losses_icp", "chamfer_dist_icp", "icp_iters")
    assert set(C.ICP_DTYPES) == set(C.ICP_NAMES) and C.ICP_SCALE_NAMES == ("icp_scale",)
    assert not set(C.ICP_SCALE_NAMES) & (set(C.NAMES) | set(C.ICP_NAMES))
    rng = np.random.default_rng(0)
    res = {k: (rng.standard_normal((3, 4, 4)) if k.startswith("Ts_est") else rng.standard_normal(3)).astype(
        dict(C.DTYPES, **C.ICP_DTYPES)[k]) for k in C.NAMES + C.ICP_NAMES}
    d = str(tmp_path / "plain")
    C.save_results(d, "chair", True, res)
    # a cache of an unscaled ICP run: a hit for plain and ICP runs with their old key sets, a miss only when a scale is asked
    assert set(C.load_results(d, "chair", True)) == set(C.NAMES)
    assert set(C.load_results(d, "chair", True, icp=True)) == set(C.NAMES) | set(C.ICP_NAMES)
    assert C.load_results(d, "chair", True, icp=True, icp_scale=True) is None
    assert not any("icp_scale" in f for f in os.listdir(d))
    d2 = str(tmp_path / "scaled")
    res["icp_scale"] = np.float64([1.05, 0.9, 1.0])
    C.save_results(d2, "chair", True, res)
    got = C.load_results(d2, "chair", True, icp=True, icp_scale=True)
    assert set(got) == set(C.NAMES) | set(C.ICP_NAMES) | set(C.ICP_SCALE_NAMES)
    assert got["icp_scale"].dtype == C.ICP_SCALE_DTYPES["icp_scale"] and np.array_equal(got["icp_scale"], res["icp_scale"])
    # ... and the scale is returned only when asked for
    assert set(C.load_results(d2, "chair", True, icp=True)) == set(C.NAMES) | set(C.ICP_NAMES)
    assert set(C.load_results(d2, "chair", True)) == set(C.NAMES)


def test_config_refusals_and_flags():
    import inspect

    from corsair_amd import harness as H, registration as R, shapenet_eval as S

    H.Config().check_icp()
    H.Config(icp_max_iter=5, icp_with_scaling=True).check_icp()
    H.Config(icp_max_iter=5, icp_estimation="plane", icp_with_scaling=True, icp_scale_bounds=(0.9, 1.1)).check_icp()
    assert H.Config().icp_with_scaling is False and tuple(H.Config().icp_scale_bounds) == (0.5, 2.0)
    with pytest.raises(ValueError, match="robust"):
        H.Config(icp_max_iter=5, icp_estimation="plane", icp_kernel="huber", icp_with_scaling=True).check_icp()
    with pytest.raises(ValueError, match="icp_max_iter"):
        H.Config(icp_with_scaling=True).check_icp()
    for bad in ((0.0, 2.0), (1.1, 2.0), (0.5, 0.9), (0.5, math.inf)):
        with pytest.raises(ValueError, match="icp_scale_bounds"):
            H.Config(icp_max_iter=5, icp_with_scaling=True, icp_scale_bounds=bad).check_icp()
    need = ["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"]
    a = H.build_parser().parse_args(need)
    assert (a.icp_with_scaling, a.icp_scale_min, a.icp_scale_max) == (False, 0.5, 2.0)
    a = H.build_parser().parse_args(need + ["--icp-with-scaling", "--icp-scale-min", "0.8", "--icp-scale-max", "1.25"])
    assert (a.icp_with_scaling, a.icp_scale_min, a.icp_scale_max) == (True, 0.8, 1.25)
    a = S.build_parser().parse_args(["--ckpt", "c", "--max-log-scale", "0.1", "--icp-with-scaling", "--icp-scale-max", "1.5"])
    assert (a.max_log_scale, a.icp_with_scaling, a.icp_scale_min, a.icp_scale_max) == (0.1, True, 0.5, 1.5)
    assert S.build_parser().parse_args(["--ckpt", "c"]).max_log_scale == 0.0 and S.Config().max_log_scale == 0.0
    # after every parameter that callers pass positionally; icp_kernel / icp_kernel_scale stay the last two, which
    # tests/test_icp_robust_cpu.py pins, and the library's own callers pass the tail by keyword
    names = list(inspect.signature(R.sym_pose_batch).parameters)
    assert names[-5:] == ["icp_normal_radius", "icp_with_scaling", "icp_scale_bounds", "icp_kernel", "icp_kernel_scale"]
    sig = inspect.signature(R.sym_pose_batch).parameters
    assert sig["icp_with_scaling"].default is False and sig["icp_scale_bounds"].default is None
    z = np.zeros((0, 16), np.float32)
    with pytest.raises(ValueError, match="out of scope"):
        R.sym_pose_batch(z, z, [0], z, z, [0], [], icp_max_iter=3, icp_max_dist=0.1, icp_estimation="plane",
                         icp_kernel="huber", icp_kernel_scale=0.1, icp_with_scaling=True)
    # the sharded evaluation keeps refusing ICP, with or without a scale, before it touches a rank or a cloud
    from corsair_amd import sharding

    class _Pipe:
        device = "cpu"

    for cfg in (H.Config(icp_max_iter=5), H.Config(icp_max_iter=5, icp_with_scaling=True)):
        pipe = _Pipe()
        pipe.cfg = cfg
        with pytest.raises(ValueError, match="ICP refinement"):
            sharding.run_eval_sharded(pipe, object(), 0, 2, [], [], [], None, None, None, [])
