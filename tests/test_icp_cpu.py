"""The ICP without a GPU: tests/icp_ref.py (the bit-exact restatement of cs_icp_batch the GPU tests compare with) against
an independent implementation -- SciPy's KD-tree and an SVD Kabsch loop --, its fixed-point bounds and edge rules, the
library's exports, and the Python surface around the call."""
import ctypes
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import icp_ref as ref


def _perturbed(T, deg, trans, seed):
    rng = np.random.default_rng(seed)
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    D[:3, 3] = rng.uniform(-trans, trans, 3)
    return (D @ T).astype(np.float32)


def _fixture(seed, ns, nt):
    """Target = the first nt points of a synthetic cloud; source = ns other rows of the same cloud in another pose (a
    subsample of the target when the rows lie inside it); start = the true pose perturbed by 3 degrees / 1 cm."""
    from corsair_amd import synth

    cloud = synth.make_cloud(seed, 4000)
    Tgt = synth.random_pose(seed, max_trans=0.3)
    src = synth.apply_pose(cloud[1000:1000 + ns], np.linalg.inv(Tgt))
    return src, cloud[:nt], _perturbed(Tgt, 3.0, 0.01, seed), Tgt


FIXTURES = ((1, 300, 900), (2, 257, 513), (3, 120, 2000))


def _kabsch_icp(src, tgt, T0, max_dist, max_iter, rf=1e-6, rr=1e-6):
    """Open3D's loop with SciPy's KD-tree and NumPy's SVD, everything in plain f64."""
    src, tgt = src.astype(np.float64), tgt.astype(np.float64)
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
        if n < 3:
            break
        P, Q = p[keep], tgt[j[keep]]
        mp, mq = P.mean(0), Q.mean(0)
        U, _, Vt = np.linalg.svd((P - mp).T @ (Q - mq))
        R = Vt.T @ np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
        Up = np.eye(4)
        Up[:3, :3], Up[:3, 3] = R, mq - R @ mp
        T = Up @ T
        it += 1
        pf, pr = fit, rm
        p, j, keep, fit, rm, n = evaluate(T)
        if abs(fit - pf) < rf and abs(rm - pr) < rr:
            break
    return T, it, np.where(keep, j, -1), fit, rm


def _rre_rte(T, Tgt):
    R = T[:3, :3] @ Tgt[:3, :3].T
    return math.acos(min(1.0, max(-1.0, (np.trace(R) - 1) / 2))), float(np.linalg.norm(T[:3, 3] - Tgt[:3, 3]))


@pytest.mark.parametrize("seed,ns,nt", FIXTURES)
def test_restatement_against_kdtree_and_svd(seed, ns, nt):
    """Correspondences identical (the clouds have no ties), the same number of updates, and the final transform within
    3e-14 (max abs over the 16 entries) of the SVD loop's.  Measured on these three fixtures: 7.6e-15, 1.4e-15, 4.4e-16
    after 11, 11 and 4 updates; the bound is the largest of them with a margin of 4.  What separates the two: the
    truncation of the fixed-point sums (a mean carries up to 2^(eM + eN - 61) <= 4.4e-16 here: eM = 1, eN <= 9), Horn's
    quaternion from a characteristic polynomial against LAPACK's SVD, and the order of the f64 sums -- a few ulp per
    update, carried through the product of the updates."""
    src, tgt, T0, _ = _fixture(seed, ns, nt)
    got = ref.icp(src, tgt, T0, 0.1, 30)
    Tk, itk, corr_k, fit_k, rm_k = _kabsch_icp(src, tgt, T0, 0.1, 30)
    diff = float(np.abs(got["T"].reshape(4, 4) - Tk).max())
    print("seed %d: updates %d / %d, max |T - T_svd| = %.3g" % (seed, got["iters"], itk, diff))
    assert got["iters"] == itk and 1 < itk < 30
    assert np.array_equal(got["corr"], corr_k)
    # every d^2 is truncated to a multiple of 2^-s2 before it is summed, so the mean square sits at most one quantum low
    quantum = 2.0 ** -ref.frame(tgt, ns, 0.1)["s2"]
    assert got["fitness"] == fit_k and abs(got["rmse"] ** 2 - rm_k ** 2) <= quantum + 1e-12 * rm_k ** 2
    assert diff <= 3e-14
    # the first association (T0 only) as well, and max_iter = 0 changes nothing
    first = ref.icp(src, tgt, T0, 0.1, 0)
    assert first["iters"] == 0 and np.array_equal(first["T32"], T0.reshape(16))
    assert np.array_equal(first["corr"], _kabsch_icp(src, tgt, T0, 0.1, 0)[2])


def test_refinement_improves_a_perturbed_pose():
    """A posed subsample of the target cloud, started 3 degrees / ~1 cm off: the restatement converges onto the true
    pose.  Measured on this fixture: RRE 5.24e-2 rad -> 0 (below the acos resolution), RTE 1.11e-2 -> 3.3e-9, i.e.
    factors of 0 and 3.0e-7; asserted: both below 1e-6 of the initial error."""
    src, tgt, T0, Tgt = _fixture(3, 120, 2000)
    got = ref.icp(src, tgt, T0, 0.1, 30)
    r0, t0 = _rre_rte(T0.astype(np.float64), Tgt)
    r1, t1 = _rre_rte(got["T"].reshape(4, 4), Tgt)
    print("RRE %.3g -> %.3g rad, RTE %.3g -> %.3g" % (r0, r1, t0, t1))
    assert r0 > 0.05 and t0 > 0.01
    assert r1 <= 1e-6 * r0 and t1 <= 1e-6 * t0           # measured factors: 0 and 3.0e-7
    assert got["fitness"] == 1.0 and got["rmse"] < 1e-7 and got["iters"] < 30


def test_fixed_point_bounds():
    rng = np.random.default_rng(0)
    # the derivation of icp.hip: every scaled term stays below 2^(61 - eN), every sum below 2^61
    for n_src, scale, max_dist in ((1, 1.0, 0.1), (5000, 1.0, 0.06), (2 ** 31 - 1, 50.0, 3.0), (257, 1e-3, 1e-4),
                                   (1000, 3e38, 1.0)):
        tgt = (rng.uniform(-1, 1, (64, 3)) * scale).astype(np.float32)
        fr = ref.frame(tgt, n_src, max_dist)
        lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
        M = float(np.max(0.5 * (hi - lo))) + max_dist
        assert M < 2.0 ** fr["eM"] and n_src <= 2 ** fr["eN"]
        assert M * fr["sc1"] < fr["clamp"] and M * M * fr["sc2"] < fr["clamp"]
        assert fr["clamp"] * 2 ** fr["eN"] == 2.0 ** 61
        assert fr["sc1"] * fr["inv1"] == 1.0 and fr["sc2"] * fr["inv2"] == 1.0
    # the clamp in front of the conversion: any value, NaN included, becomes an integer inside the bound
    fr = ref.frame(np.zeros((1, 3), np.float32), 4, 0.1)
    for v in (1e300, -1e300, math.inf, -math.inf, math.nan):
        assert abs(ref.fix(v, fr["sc1"], fr["clamp"])) == 2 ** 59
    assert ref.fix(0.75 * 2.0 ** -fr["s1"], fr["sc1"], fr["clamp"]) == 0 == ref.fix(-0.75 * 2.0 ** -fr["s1"], fr["sc1"], fr["clamp"])
    # an empty or non-finite target segment: origin 0
    assert ref.frame(np.zeros((0, 3), np.float32), 10, 0.1)["o"] == [0.0, 0.0, 0.0]
    assert ref.frame(np.float32([[np.inf, 0, 0], [0, 0, 0]]), 10, 0.1)["o"] == [0.0, 0.0, 0.0]


def test_edge_rules():
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-0.5, 0.5, (100, 3)).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)
    # ties go to the smaller row; the threshold is strict
    tgt[60] = tgt[20]
    r = ref.icp(tgt[20:21], tgt, eye, 0.1, 0)
    assert r["corr"].tolist() == [20] and r["rmse"] == 0.0 and r["fitness"] == 1.0
    src = np.float32([[2.0, 0.0, 0.0]])
    one = np.float32([[2.25, 0.0, 0.0]])
    assert ref.icp(src, one, eye, 0.25, 0)["ncorr"] == 0 and ref.icp(src, one, eye, 0.2500001, 0)["ncorr"] == 1
    # fewer than three pairs: no update; empty segments are answered
    r = ref.icp(tgt[:2], tgt, eye, 0.1, 30)
    assert r["ncorr"] == 2 and r["iters"] == 0 and np.array_equal(r["T"], eye.reshape(16).astype(np.float64))
    for s, t in ((tgt[:0], tgt), (tgt, tgt[:0])):
        r = ref.icp(s, t, eye, 0.1, 30)
        assert (r["fitness"], r["rmse"], r["iters"], r["ncorr"]) == (0.0, 0.0, 0, 0)
    # a source that is already on the target: one update (the identity to rounding), then the stop rule
    r = ref.icp(tgt[:50], tgt, eye, 0.1, 30)
    assert r["iters"] == 1 and r["fitness"] == 1.0 and np.abs(r["T"] - eye.reshape(16)).max() < 1e-15


def test_both_solvers_give_the_rotation():
    rng = np.random.default_rng(8)
    from corsair_amd import synth

    R = synth.random_pose(11)[:3, :3]
    P = rng.standard_normal((40, 3))
    Q = P @ R.T
    S = [[float(np.sum((P[:, a] - P[:, a].mean()) * (Q[:, b] - Q[:, b].mean()))) for b in range(3)] for a in range(3)]
    for force in (False, True):
        assert np.abs(np.asarray(ref.rotation_of(S, force_jacobi=force)) - R).max() < 1e-12
    assert ref.horn_qcp(S, ref.horn_matrix(S)) is not None
    # a degenerate covariance (all points on a line): the polynomial solver declines, Jacobi answers
    L = np.outer(np.arange(5.0), [1.0, 0.0, 0.0])
    S = [[float(np.sum(L[:, a] * L[:, b])) for b in range(3)] for a in range(3)]
    assert ref.horn_qcp(S, ref.horn_matrix(S)) is None
    assert np.all(np.isfinite(ref.rotation_of(S)))


def test_library_exports_header_and_shared_solver():
    import os

    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cs_icp_batch", "cs_icp_stats"):
        assert hasattr(lib, name) and name in _lib.header_symbols()
    lib.cs_icp_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    lib.cs_icp_stats.restype = None
    out = (ctypes.c_uint64 * 2)(7, 7)
    lib.cs_icp_stats(out, 1)
    assert list(out) == [0, 0]
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for word in ("CS_ICP_F16", "CS_ICP_STATS", '"icp"', "[O3D-knowledge]"):
        assert word in text
    # one definition of the eigen-solvers, included by both users: the hypothesis unit of the RANSAC and the step unit of the ICP
    from tests.helpers import ICP_UNITS, assert_five_icp_kernels, icp_unit_texts

    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH))
    ransac_units = ("ransac.hip", "ransac_hyp.hip", "ransac_prefilter.hip", "ransac_count.hip", "ransac.h")
    units = {n: open(os.path.join(csrc, n)).read() for n in ("horn.h",) + ransac_units}
    units.update(icp_unit_texts())
    for fn in ("bool horn_qcp(", "void jacobi4("):
        assert fn in units["horn.h"]
        for n in ICP_UNITS + ransac_units:
            assert fn not in units[n], n
    assert '#include "horn.h"' in units["ransac_hyp.hip"] and '#include "horn.h"' in units["icp_step.hip"]
    for n in ICP_UNITS:
        assert n == "icp_step.hip" or '#include "horn.h"' not in units[n], n
    assert_five_icp_kernels()


def test_python_surface(tmp_path):
    from corsair_amd import backend as B, cache as C, harness as H, registration as R, sharding

    assert callable(B.icp_batch) and callable(B.icp_stats)
    cfg = H.Config()
    assert cfg.icp_max_iter == 0 and cfg.icp_max_dist == 0.0 and cfg.icp_distance() == 2 * cfg.voxel_size
    assert H.Config(icp_max_dist=0.1).icp_distance() == 0.1
    a = H.build_parser().parse_args(["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"])
    assert a.icp_iters == 0 and a.icp_max_dist == 0.0
    a = H.build_parser().parse_args(["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b", "--icp-iters", "30",
                                     "--icp-max-dist", "0.05"])
    assert a.icp_iters == 30 and a.icp_max_dist == 0.05
    res = R.SymPoseResult(None, None, None, None, None, None, 0)
    assert res.T_icp is None and res.cd_icp is None and res.icp_fitness is None and res.icp_rmse is None \
        and res.icp_iters is None
    # the nine names are what they were; the extra files sit beside them
    assert len(C.NAMES) == 9 and not set(C.NAMES) & set(C.ICP_NAMES) and set(C.ICP_DTYPES) == set(C.ICP_NAMES)
    q = 3
    nine = {k: np.zeros((q, 4, 4) if k.startswith("Ts_est") else q, C.DTYPES[k]) for k in C.NAMES}
    extra = {k: np.ones((q, 4, 4) if k.startswith("Ts_est") else q, C.ICP_DTYPES[k]) for k in C.ICP_NAMES}
    C.save_results(str(tmp_path / "a"), "chair", True, nine)
    assert C.load_results(str(tmp_path / "a"), "chair", True) is not None
    assert C.load_results(str(tmp_path / "a"), "chair", True, icp=True) is None        # a miss when ICP is asked for
    C.save_results(str(tmp_path / "b"), "chair", True, dict(nine, **extra))
    back = C.load_results(str(tmp_path / "b"), "chair", True, icp=True)
    assert set(back) == set(C.NAMES) | set(C.ICP_NAMES) and back["Ts_est_icp"].shape == (q, 4, 4)
    assert all(back[k].dtype == C.ICP_DTYPES[k] for k in C.ICP_NAMES)
    assert set(C.load_results(str(tmp_path / "b"), "chair", True)) == set(C.NAMES)

    class Pipe:
        cfg = H.Config(icp_max_iter=5)
        device = "cpu"

    with pytest.raises(ValueError, match="ICP"):
        sharding.run_eval_sharded(Pipe(), object(), 0, 2, [], [], [], None, [], [], [])
