"""Feature-matching RANSAC without a GPU: tests/featmatch_ref.py (the bit-exact restatement of cs_corr_mutual and
cs_ransac_fm_batch that the GPU tests compare with) against an independent float implementation, why the estimator exists
(a planted problem the 10-pair recipe cannot solve), the three real CAD / partial-view pairs, the defined cases of the header,
the mutual filter, the options of sym_pose_batch and shapenet_eval, the sources and the ABI's refusals."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import featmatch_cases as FC
from tests import featmatch_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
M, SHARE, ITERS = 400, 0.15, 4096
# The float implementation and the restatement disagree by at most 6.1e-12 of max_corr on any distance of any valid
# hypothesis of the four planted problems below (measured); the margin is ten times that, rounded up.
MARGIN = 1e-10
_tables = {}


def _planted(seed):
    if seed not in _tables:
        s, q, R, t, keep = FC.planted(M, SHARE, seed)
        _tables[seed] = (s, q, R, t, keep, ref.Table(s, q, FC.MAX_CORR, 3, 0.9, True, ITERS, seed))
    return _tables[seed]


@pytest.mark.parametrize("seed", range(4))
def test_restatement_against_float_implementation(seed):
    s, q, _, _, _, tab = _planted(seed)
    T, stat, rmse, inl = tab.result()
    draws = [ref.draws(seed, t, 3, M) for t in range(ITERS)]
    t_best, count, f_inl, valid, gap, poses = FC.float_ransac_fm(s, q, draws, FC.MAX_CORR)
    print("seed %d: smallest relative distance of a comparison from its threshold %.3g" % (seed, gap))
    assert gap > MARGIN                                  # no checker or inlier comparison is decided by a rounding
    assert stat[1] == t_best and stat[2] == count and np.array_equal(inl, f_inl) and tab.valid() == valid
    dev = 0.0
    s64 = s.astype(np.float64)
    for t in valid:
        Rf, tf = poses[t]
        Rr = np.asarray(tab.R[t]).reshape(3, 4)
        df = np.linalg.norm(s64 @ Rf.T + tf - q, axis=1)
        dr = np.linalg.norm(s64 @ Rr[:, :3].T + Rr[:, 3] - q, axis=1)
        dev = max(dev, float(np.abs(df - dr).max() / FC.MAX_CORR))
    print("seed %d: largest deviation of a distance between the two implementations %.3g of max_corr" % (seed, dev))
    assert 10.0 * dev <= MARGIN


@pytest.mark.parametrize("seed", range(4))
def test_why_the_estimator_exists(seed, oracle_native):
    """400 pairs, 60 of them exact inliers of one pose: 4 096 three-pair hypotheses with the checkers recover it; the
    oracle's RANSAC at ransac_n = 10 (a clean sample once in 10^8) with as many hypotheses finds 2 - 3 pairs."""
    s, q, R, t, keep, tab = _planted(seed)
    T, stat, rmse, inl = tab.result()
    T = np.asarray(T).reshape(4, 4)
    assert stat[0] == 1 and stat[2] == int(keep.sum()) == 60 and inl[keep].all() and not inl[~keep].any()
    assert np.abs(T[:3, :3] - R).max() < 1e-6 and np.abs(T[:3, 3] - t).max() < 1e-6       # measured 5.5e-8 / 1.7e-8 at most
    assert rmse < 1e-6                                                                    # the f32 rounding of the targets
    assert 3 <= stat[3] <= 40                                                             # measured 5, 9, 8, 18 valid of 4 096
    _, o_inl, _, _ = oracle_native.ransac(s, q, FC.MAX_CORR, 10, ITERS, 0.999, seed)
    print("seed %d: ransac_fm %d inliers, %d valid hypotheses; 10-pair recipe %d inliers" % (seed, stat[2], stat[3], o_inl))
    assert o_inl <= 5                                                                     # measured 2, 2, 3, 3


# ---- the three real CAD / partial-view pairs of README section FPFH ---------------------------------------------------------
# tests/fpfh_ref.py descriptors (float normals over 16 neighbours, oriented away from the centroid; radius 5 voxels, max_nn
# 100) of clouds 0, 3 and 5, split, posed and voxelised as tests/test_gpu_fpfh.py does.  Measured here at seed 0:
#   ransac_fm, 4 096 hypotheses, mutual filter (1 199 / 727 / 939 matches):  RRE 2.42 / 1.26 / 2.18 deg, RTE 0.0383 / 0.0209 / 0.0239
#   5-NN lists, ransac_n = 10 (the oracle), 4 096 hypotheses:                RRE 5.69 / 4.11 / 7.54 deg, RTE 0.1085 / 0.0514 / 0.0419
#   the same at 100 000 (tests/test_gpu_fpfh.py's CPU_RRE_DEG / CPU_RTE):    RRE 6.06 / 3.90 / 4.89 deg, RTE 0.0619 / 0.0139 / 0.0206
# Seeds move the new recipe (seeds 1 and 2: 7.24 / 1.95 / 5.47 and 5.87 / 0.98 / 4.08 deg); only three pairs exist.
FM_RRE_DEG = (2.42, 1.26, 2.18)
FM_RTE = (0.0383, 0.0209, 0.0239)


@pytest.mark.parametrize("p", range(3))
def test_real_pairs_against_the_ten_pair_recipe(p, oracle_native):
    from scipy.spatial import cKDTree

    from corsair_amd import synth
    from corsair_amd.utils.eval_pose import eval_pose
    from tests import fpfh_ref as FR
    from tests.test_fpfh_cpu import _pca_normals, _voxelize
    from tests.test_gpu_real_clouds import _real_clouds

    voxel = 0.03
    full = _real_clouds()[[0, 3, 5][p]]
    T_gt = synth.random_pose(100 + p, max_trans=0.5)
    cad = _voxelize(full[:10000], voxel)
    q = _voxelize(synth.apply_pose(full[5000:], T_gt), voxel)
    Fc = FR.fpfh(cad, _pca_normals(cad, 16), [0, len(cad)], 5 * voxel, 100)
    Fq = FR.fpfh(q, _pca_normals(q, 16), [0, len(q)], 5 * voxel, 100)
    tree = cKDTree(Fc)
    fwd = tree.query(Fq, 1)[1].astype(np.int32)
    bwd = cKDTree(Fq).query(Fc, 1)[1].astype(np.int32)
    src, tgt, m, stat = ref.mutual(fwd, bwd, q, [0, len(q)], cad, [0, len(cad)], 3, True)
    T, st, rmse = ref.ransac_fm_batch(src, tgt, [0, len(q)], 0.2, m=m, iterations=ITERS, seed=0)
    rte, rre = eval_pose(T[0].astype(np.float32), T_gt, np.eye(4), 1)
    nn5 = tree.query(Fq, 5)[1]
    To, o_inl, _, _ = oracle_native.ransac(np.repeat(q, 5, 0), cad[nn5.reshape(-1)], 0.2, 10, ITERS, 0.999, 0)
    o_rte, o_rre = eval_pose(To, T_gt, np.eye(4), 1)
    print("pair %d: %d mutual matches of %d rows; ransac_fm RRE %.2f deg RTE %.4f (%d inliers, %d valid of %d); "
          "5-NN / ransac_n 10 RRE %.2f deg RTE %.4f (%d inliers of %d)"
          % (p, stat[0, 0], len(q), np.rad2deg(rre), rte, st[0, 2], st[0, 3], ITERS, np.rad2deg(o_rre), o_rte, o_inl, 5 * len(q)))
    assert st[0, 0] == 1 and stat[0, 1] == 0
    assert np.rad2deg(rre) <= 2.0 * FM_RRE_DEG[p] and rte <= 2.0 * FM_RTE[p]


def _run(case):
    s, q, kw = case
    return ref.ransac_fm_one(s, q, **kw)


def test_defined_cases():
    cases = FC.defined_cases()
    out = {k: _run(v) for k, v in cases.items()}
    identity = list(ref.IDENTITY)
    for name in ("m0", "m1", "m2", "m3_n4"):                      # fewer pairs than a sample: found by nothing
        T, stat, rmse, inl = out[name]
        assert T == identity and stat == [0, -1, 0, 0] and rmse == 0.0 and not inl.any(), name
    for name in ("m3", "m4"):                                     # every draw is with replacement: some hypotheses repeat a pair
        T, stat, rmse, inl = out[name]
        s, q, kw = cases[name]
        repeats = sum(len(set(ref.draws(0, t, 3, len(s)))) < 3 for t in range(kw["iterations"]))
        assert repeats > 0 and stat[3] <= kw["iterations"] - repeats, name     # a repeated pair never gives a valid fit here
        assert stat[0] == 1 and stat[2] >= 3, name
    for name in ("copies", "collinear", "rejected", "corr_underflow", "corr_underflow_no_check"):
        T, stat, rmse, inl = out[name]
        assert T == identity and stat[:3] == [0, -1, 0] and rmse == 0.0 and not inl.any(), name
    assert out["copies"][1][3] == 0 and out["collinear"][1][3] == 0                        # coincident and collinear samples
    assert out["rejected"][1][3] == 0                                                      # the target scaled by 2: n_valid = 0
    assert out["corr_underflow"][1][3] == 0 and out["corr_underflow_no_check"][1][3] > 0   # valid, but nothing is counted
    # two exact pose clusters of 12 pairs: the smaller t wins, and both clusters occur among the tied hypotheses
    for name in ("clusters", "edge1"):
        s, q, kw = cases[name]
        tab = ref.Table(s, q, **kw)
        T, stat, rmse, inl = tab.result()
        tied = [t for t in tab.valid() if tab.count[t] == 12]
        g, gq, in_a, in_b = FC.two_clusters()
        sides = {bool(tab.masks[t][in_a].all()) for t in tied}
        assert stat[0] == 1 and stat[2] == 12 and stat[1] == min(tied) and sides == {True, False}, name
        assert rmse < 1e-9 and ((inl == in_a).all() or (inl == in_b).all())
        assert all(abs(float(v) - round(float(v))) < 1e-12 for v in T)                    # a quarter turn and an integer shift
    # non-finite rows are never inliers and never part of a valid sample
    for name in ("nonfinite", "nonfinite_no_edge"):
        T, stat, rmse, inl = out[name]
        assert stat[0] == 1 and not inl[[3, 7, 11, 20]].any() and all(math.isfinite(v) for v in T) and math.isfinite(rmse)
    T, stat, rmse, inl = out["corr_overflow"]                      # thr2 = +inf: every finite pair counts
    assert stat[0] == 1 and stat[2] == 40 and math.isfinite(rmse)
    assert out["edge0"][1][3] > out["n4"][1][3]                    # the edge checker rejects before the fit
    assert out["edge0"][1][0] == 1 and out["n4"][1][0] == 1 and out["no_distance_check"][1][3] >= out["n4"][1][3]
    T, stat, rmse, inl = out["iters1"]
    assert stat[1] in (0, -1) and stat[3] in (0, 1)
    # a prefix of the hypotheses: the result of fewer iterations comes from the same table
    s, q, kw = cases["n4"]
    assert ref.Table(s, q, **kw).result(100)[:3] == ref.ransac_fm_one(s, q, **dict(kw, iterations=100))[:3]
    assert ref.draws(0, 0, 3, 7) == [ref.rng_index(0, 0, j, 7) for j in range(3)]


def test_mutual_filter():
    d = FC.mutual_lists(3)
    src, tgt, m, stat = ref.mutual(d["fwd"], d["bwd"], d["x0"], FC.M_OFF0, d["x1"], FC.M_OFF1, 3, True)
    valid = [int(((d["fwd"][a:b] >= 0)).sum()) for a, b in zip(FC.M_OFF0[:-1], FC.M_OFF0[1:])]
    assert stat[:, 0].tolist() == FC.M_MUTUAL
    assert stat[:, 1].tolist() == [0, 1, 1, 1, 0, 0]               # 8 = 3 * 3 - 1 falls back, 9 does not; empty pairs fall back to nothing
    assert m.tolist() == [120, 0, 0, valid[3], 9, 150] and valid[3] > 8
    # the order is that of the query rows, and the slots past the count are zero
    for p in (0, 3, 4, 5):
        a0, b0 = FC.M_OFF0[p], FC.M_OFF1[p]
        rows = [i for i in range(FC.M_OFF0[p + 1] - a0) if d["fwd"][a0 + i] >= 0 and
                (stat[p, 1] == 1 or d["bwd"][b0 + d["fwd"][a0 + i]] == i)]
        assert len(rows) == m[p] and rows == sorted(rows)
        assert np.array_equal(src[a0:a0 + m[p]], d["x0"][a0 + np.asarray(rows)])
        assert np.array_equal(tgt[a0:a0 + m[p]], d["x1"][b0 + d["fwd"][a0 + np.asarray(rows)]])
        assert not src[a0 + m[p]:FC.M_OFF0[p + 1]].any() and not tgt[a0 + m[p]:FC.M_OFF0[p + 1]].any()
    # ransac_n = 4 moves the threshold to 12: the pair with 9 falls back too
    _, _, m4, stat4 = ref.mutual(d["fwd"], d["bwd"], d["x0"], FC.M_OFF0, d["x1"], FC.M_OFF1, 4, True)
    assert stat4[:, 1].tolist() == [0, 1, 1, 1, 1, 0] and m4[4] == valid[4]
    # mutual = 0 only assembles the valid 1-NN pairs and reads no backward list
    _, _, m0, stat0 = ref.mutual(d["fwd"], None, d["x0"], FC.M_OFF0, d["x1"], FC.M_OFF1, 3, False)
    assert m0.tolist() == valid and stat0[:, 0].tolist() == valid and not stat0[:, 1].any()
    # an entry past the CAD's rows is no match either
    fwd = d["fwd"].copy()
    fwd[0] = 280
    assert ref.mutual(fwd, None, d["x0"], FC.M_OFF0, d["x1"], FC.M_OFF1, 3, False)[2][0] == valid[0] - (d["fwd"][0] >= 0)


def test_options_config_and_parser():
    from corsair_amd import featmatch, harness as H, registration as R, shapenet_eval as SE

    assert list(inspect.signature(featmatch.ransac_fm_batch).parameters) == [
        "src", "tgt", "offsets", "max_corr", "m", "ransac_n", "edge_similarity", "check_distance", "iterations", "seed"]
    assert list(inspect.signature(featmatch.mutual_correspondences).parameters) == [
        "nn_fwd", "nn_bwd", "xyz0", "off0", "xyz1", "off1", "ransac_n", "mutual"]
    d = {k: v.default for k, v in inspect.signature(featmatch.ransac_fm_batch).parameters.items()}
    assert (d["m"], d["ransac_n"], d["edge_similarity"], d["check_distance"], d["iterations"], d["seed"]) == \
        (None, 3, 0.9, True, 100000, 0)
    assert featmatch.FmResult._fields == ("T", "inliers", "rmse", "found", "t_best", "n_valid")
    assert featmatch.torch is __import__("torch") and not hasattr(__import__("corsair_amd.backend").backend, "ransac_fm_batch")
    assert R.check_fm_options(3, 0.9, True, 100000) == (3, 0.9, True, 100000)
    nan = float("nan")
    for args, word in (((2, 0.9, True, 10), "fm_ransac_n"), ((5, 0.9, True, 10), "fm_ransac_n"), ((True, 0.9, True, 10), "fm_ransac_n"),
                       ((3, -0.1, True, 10), "fm_edge_similarity"), ((3, 1.5, True, 10), "fm_edge_similarity"),
                       ((3, nan, True, 10), "fm_edge_similarity"), ((3, "a", True, 10), "fm_edge_similarity"),
                       ((3, 0.9, 1, 10), "fm_mutual"), ((3, 0.9, True, 0), "fm_iterations"),
                       ((3, 0.9, True, 2 ** 31), "fm_iterations"), ((3, 0.9, True, 2.5), "fm_iterations")):
        with pytest.raises(ValueError, match=word):
            R.check_fm_options(*args)
    z = np.zeros((0, 33), np.float32)
    with pytest.raises(ValueError, match="registration"):
        R.sym_pose_batch(z, z, [0], z, z, [0], [], registration="fm")
    with pytest.raises(ValueError, match="fm_ransac_n"):
        R.sym_pose_batch(z, z, [0], z, z, [0], [], registration="ransac_fm", use_symmetry=False, fm_ransac_n=10)
    c = SE.Config()
    assert (c.registration, c.fm_ransac_n, c.fm_edge_similarity, c.fm_mutual, c.fm_iterations) == ("ransac", 3, 0.9, True, 100000)
    c.check_registration()
    SE.Config(registration="ransac_fm", fm_ransac_n=4, fm_edge_similarity=0.0, fm_mutual=False, fm_iterations=1).check_registration()
    for kw, word in ((dict(registration="icp"), "registration"), (dict(fm_ransac_n=10), "fm_ransac_n"),
                     (dict(fm_edge_similarity=2.0), "fm_edge_similarity"), (dict(fm_mutual="yes"), "fm_mutual"),
                     (dict(fm_iterations=0), "fm_iterations")):
        with pytest.raises(ValueError, match=word):
            SE.Config(**kw).check_registration()
    a = SE.build_parser().parse_args([])
    assert (a.registration, a.fm_ransac_n, a.fm_edge_similarity, a.fm_no_mutual, a.fm_iterations) == ("ransac", 3, 0.9, False, 100000)
    a = SE.build_parser().parse_args(["--registration", "ransac_fm", "--fm-ransac-n", "4", "--fm-edge-similarity", "0.8",
                                      "--fm-no-mutual", "--fm-iterations", "500"])
    assert (a.registration, a.fm_ransac_n, a.fm_edge_similarity, a.fm_no_mutual, a.fm_iterations) == ("ransac_fm", 4, 0.8, True, 500)
    with pytest.raises(SystemExit):
        SE.build_parser().parse_args(["--fm-ransac-n", "10"])
    help_text = " ".join(SE.build_parser().format_help().split())
    assert help_text.count("untuned, no real scan measured") >= 4
    # out of scope there: the harness refuses the value by name
    with pytest.raises(ValueError, match="ransac_fm"):
        H.Config(registration="ransac_fm").check_icp()
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b", "--registration", "ransac_fm"])


def test_source_layout_and_documents():
    header = open(os.path.join(ROOT, "include", "corsair_hip.h")).read()
    assert "int cs_corr_mutual(" in header and "int cs_ransac_fm_batch(" in header and '"featmatch"' in header
    at = header.index("cs_ransac_fm_batch:")
    block = " ".join(header[at:header.index("int cs_corr_mutual(")].split())
    for words in ("Differences from [O3D-knowledge] Open3D", "no confidence-based early exit", "SMALLEST t", "strict",
                  "counter-based generator", "NO final refit", "fixed-point sum", "rng_index(seed, t, j, m)", "horn_qcp"):
        assert words in block, words
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    text = open(os.path.join(csrc, "featmatch.hip")).read()
    assert '#include "horn.h"' in text and "horn_qcp(" in text and "rng_index(" in text and "ransac.h\"" not in text
    assert not re.search(r"bool horn_qcp\(", text) and "jacobi" not in text.replace("Jacobi", "")
    for word in ("hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "hipStreamSynchronize", "hipDeviceSynchronize",
                 "atomicCAS", "hipMalloc("):
        assert word not in text, word
    assert "atomicAdd(" in text and "atomicMax(" in text and "PoolBuf<" in text and 'ProfScope prof("featmatch"' in text
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "featmatch.hip" in make and "featmatch.o: horn.h" in make
    assert '"featmatch"' in open(os.path.join(csrc, "runtime.hip")).read()
    backend = open(os.path.join(ROOT, "corsair_amd", "backend.py")).read()
    assert "ransac_fm" not in backend and "corr_mutual" not in backend
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for words in ("cs_corr_mutual", "cs_ransac_fm_batch", "--registration ransac_fm", "untuned, no real scan measured"):
        assert words in readme, words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 25." in design and "cs_ransac_fm_batch" in design and "not measured" in design.lower()
    for name, word in (("INTEGRATION.md", "CS_FM_SLICE"), ("tools/README.md", "featmatch_bench.py"),
                       ("profiles/README.md", "featmatch_bench.json")):
        assert word in open(os.path.join(ROOT, name)).read(), name


def test_library_exports_and_refusals_without_a_device():
    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    sigs = _lib._declare(lib)
    assert "cs_corr_mutual" in sigs and "cs_ransac_fm_batch" in sigs
    assert {"cs_corr_mutual", "cs_ransac_fm_batch"} <= set(_lib.header_symbols())
    INVALID, UNSUPPORTED = -1, -5
    off0 = (ctypes.c_int64 * 2)(0, 0)
    one = (ctypes.c_int64 * 2)(0, 4)
    bad = (ctypes.c_int64 * 2)(5, 2)
    neg = (ctypes.c_int64 * 2)(-1, 2)
    huge = (ctypes.c_int64 * 2)(0, 1 << 31)
    nan, inf = float("nan"), float("inf")
    f = lib.cs_ransac_fm_batch
    # argument checks come before any device work: a call without problems needs no GPU
    ok = lambda **kw: f(None, None, kw.get("off", off0), None, kw.get("n", 0), kw.get("corr", 0.1), kw.get("rn", 3),
                        kw.get("es", 0.9), 1, kw.get("it", 100), 0, None, None, None, None)
    assert ok() == 0 and ok(rn=4) == 0 and ok(es=0.0) == 0 and ok(es=1.0) == 0 and ok(it=2 ** 31 - 1) == 0
    for c in (0.0, -1.0, nan, inf, -inf):
        assert ok(corr=c) == INVALID and b"max_corr" in lib.cs_last_error()
    for e in (-0.1, 1.1, nan, inf):
        assert ok(es=e) == INVALID and b"edge_similarity" in lib.cs_last_error()
    for it in (0, -1):
        assert ok(it=it) == INVALID and b"iterations" in lib.cs_last_error()
    assert ok(it=2 ** 31) == UNSUPPORTED and b"iterations" in lib.cs_last_error()
    for rn in (0, 2, 5, 10):
        assert ok(rn=rn) == UNSUPPORTED and b"ransac_n" in lib.cs_last_error()
    assert f(None, None, None, None, 1, 0.1, 3, 0.9, 1, 100, 0, None, None, None, None) == INVALID
    assert ok(n=-1) == INVALID and ok(off=bad, n=1) == INVALID and ok(off=neg, n=1) == INVALID
    assert ok(off=huge, n=1) == UNSUPPORTED
    assert ok(n=1) == INVALID and b"NULL" in lib.cs_last_error()                  # NULL outputs with a problem
    buf = (ctypes.c_double * 16)()
    assert f(None, None, one, None, 1, 0.1, 3, 0.9, 1, 100, 0, buf, buf, buf, None) == INVALID      # NULL pairs while a slot exists
    g = lib.cs_corr_mutual
    mk = lambda **kw: g(None, None, None, kw.get("o0", off0), None, kw.get("o1", off0), kw.get("n", 0), kw.get("rn", 3),
                        kw.get("mu", 1), None, None, None, None, None)
    assert mk() == 0 and mk(mu=0) == 0 and mk(rn=1) == 0
    assert mk(rn=0) == INVALID and b"ransac_n" in lib.cs_last_error()
    assert mk(mu=2) == INVALID and b"mutual" in lib.cs_last_error()
    assert g(None, None, None, None, None, off0, 0, 3, 1, None, None, None, None, None) == INVALID
    assert mk(n=-1) == INVALID and mk(o0=bad, n=1) == INVALID and mk(o1=neg, n=1) == INVALID
    assert mk(o0=huge, n=1) == UNSUPPORTED and mk(o1=huge, n=1) == UNSUPPORTED
    assert mk(n=1) == INVALID and b"NULL" in lib.cs_last_error()
