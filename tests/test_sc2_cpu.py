"""The compatibility-graph estimator without a GPU: tests/sc2_ref.py (the bit-exact restatement of cs_sc2_batch
that the GPU tests compare with) against an independent float implementation, why the estimator exists (planted problems at
inlier shares of 4 % and 1 % that the feature-matching RANSAC cannot solve), the defined cases of the header, the symmetry
of the matrix, the options of sym_pose_batch and shapenet_eval, the ABI's refusals and the sources."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

from tests import featmatch_cases as FC
from tests import featmatch_ref as fm_ref
from tests import sc2_cases as CS
from tests import sc2_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (pairs, planted share, noise, tau): the four rows of the issue's table; seeds 0, 1, 2 each
PLANTED = ((400, 0.15, 0.0, 0.005), (1000, 0.04, 0.002, 0.01), (2000, 0.02, 0.002, 0.01), (2000, 0.01, 0.002, 0.01))
SEEDS = 256        # the float comparison tries the 256 rows of the largest degree (the winners have ranks 0, 1 and 4)
# Measured on the twelve problems: the distances of the two implementations differ by at most 4.44e-13 of max_corr
# on any pair under the poses of the first 64 valid seeds (row 1, seed 0), and their length differences | |e| - |f| | by a few
# 2^-52 of lengths below 2, under 1e-13 of tau; the margin is ten times the larger, rounded up.  The smallest relative distance
# of any comparison from its threshold was 2.1e-6 (row 3, seed 1), 6.6e-4 on the exact row.
MARGIN = 1e-11
_graphs = {}


def _planted(row, seed):
    if (row, seed) not in _graphs:
        m, share, noise, tau = PLANTED[row]
        s, q, R, t, keep = FC.planted(m, share, seed, noise=noise)
        _graphs[(row, seed)] = (s, q, R, t, keep, ref.Graph(s, q, tau, CS.MAX_CORR))
    return _graphs[(row, seed)]


def _angle(Ra, Rb):
    return math.acos(min(1.0, max(-1.0, (np.trace(Ra.T @ Rb) - 1.0) / 2.0)))


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("row", range(len(PLANTED)))
def test_restatement_against_float_implementation(row, seed):
    s, q, _, _, _, g = _planted(row, seed)
    tau = PLANTED[row][3]
    T, stat, rmse, inl = g.result(SEEDS, 20)
    f = CS.float_sc2(s, q, CS.MAX_CORR, tau, SEEDS, 20)
    print("row %d seed %d: smallest relative distance of a comparison from its threshold %.3g; %d pairs of rows took the "
          "exact chain" % (row, seed, f["gap"], g.n_exact))
    assert f["gap"] > MARGIN                             # no compatibility, acceptance or inlier comparison is a rounding
    assert np.array_equal(g.C, f["C"])                   # every compatibility bit
    assert g.order[:SEEDS].tolist() == f["seeds"]        # the seed list
    valid = []
    for r in range(len(f["seeds"])):
        A, R, _, _ = g.hypothesis(r, 20)
        assert A == f["sets"][r], r                      # every consensus set
        if R is not None:
            valid.append(r)
    assert valid == f["valid"] and stat[3] == len(valid)
    assert (stat[4], stat[1], stat[2]) == (f["rank"], f["row"], f["count"]) and np.array_equal(inl, f["mask"])
    dev = 0.0
    s64 = s.astype(np.float64)
    for r in valid[:64]:
        Rr = np.asarray(g.hypothesis(r, 20)[1]).reshape(3, 4)
        A = g.hypothesis(r, 20)[0]
        P, Q = s64[A], q.astype(np.float64)[A]
        U, sv, Vt = np.linalg.svd((P - P.mean(0)).T @ (Q - Q.mean(0)))
        Rf = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
        tf = Q.mean(0) - Rf @ P.mean(0)
        df = np.linalg.norm(s64 @ Rf.T + tf - q, axis=1)
        dr = np.linalg.norm(s64 @ Rr[:, :3].T + Rr[:, 3] - q, axis=1)
        dev = max(dev, float(np.abs(df - dr).max() / CS.MAX_CORR))
    print("row %d seed %d: largest deviation of a distance between the two implementations %.3g of max_corr" % (row, seed, dev))
    assert 10.0 * dev <= MARGIN


# the largest rotation error the restatement measures on the problems below (radians), per share; the prototype of the issue
# measured 1.9e-3 and 2.1e-2 (as a matrix norm)
ROT_ERR = {0.04: 2.09e-3, 0.01: 2.37e-2}      # per seed: 1.59e-3, 1.29e-3, 2.09e-3 and 8.34e-3, 1.38e-2, 2.37e-2


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("m,share", [(1000, 0.04), (2000, 0.01)])
def test_why_the_estimator_exists(m, share, seed):
    """Inlier shares of 4 % and 1 %: the graph search finds every planted pair from the defaults (1 024 seeds, K = 20); 4 096
    three-pair hypotheses of the feature-matching RANSAC (a clean sample once in 1.6e4 and once in 1e6) find fewer than half."""
    s, q, R, t, keep = FC.planted(m, share, seed, noise=0.002)
    T, stat, rmse, inl = ref.sc2_one(s, q, CS.MAX_CORR, CS.TAU)
    T = np.asarray(T).reshape(4, 4)
    err = _angle(T[:3, :3], R)
    _, f_stat, _ = fm_ref.ransac_fm_batch(s, q, [0, m], CS.MAX_CORR, iterations=4096, seed=seed)
    print("%d pairs, %d planted, seed %d: sc2 %d inliers (%d planted), rotation error %.3g rad, seed rank %d, degree %d; "
          "ransac_fm at 4 096: %d inliers" % (m, keep.sum(), seed, stat[2], (inl & keep).sum(), err, stat[4], stat[5], f_stat[0, 2]))
    assert stat[0] == 1 and inl[keep].all()              # every planted pair is an inlier of the result
    assert err < 2.0 * ROT_ERR[share]
    assert 2 * int(f_stat[0, 2]) < int(keep.sum())


def test_defined_cases_of_the_header():
    cases = CS.defined_cases()
    out = {name: ref.sc2_one(s, q, **kw) for name, (s, q, kw) in cases.items()}
    for m in (0, 1, 2):
        assert out["m%d" % m][1] == [0, -1, 0, 0, -1, 0] and out["m%d" % m][0] == ref.IDENTITY and out["m%d" % m][2] == 0.0
    for m in (3, 4):                                     # exact planted pairs: every row is a valid seed, the first one wins
        T, stat, rmse, inl = out["m%d" % m]
        assert stat == [1, 0, m, m, 0, m - 1] and inl.all()
    assert out["copies"][1] == [0, -1, 0, 0, -1, 0]      # zero lengths: nothing is compatible
    T, stat, rmse, inl = out["collinear"]                # compatible everywhere, and no rotation about the line is fixed
    assert stat[0] == 0 and stat[3] == 0
    assert out["invalid"][1][0] == 0 and out["invalid"][1][3] == 0
    g, gq, first, second = FC.two_clusters()
    T, stat, rmse, inl = out["clusters"]                 # two exact clusters of 12: the seed of the smallest rank wins the tie
    assert stat[0] == 1 and stat[2] == 12 and stat[5] >= 11
    assert np.array_equal(inl, first if first[stat[1]] else second)
    G = ref.Graph(g, gq, 1e-3, 0.5)
    counts = [G.hypothesis(r, 20)[2] for r in range(30)]
    print("clusters: counts by rank", counts, "degrees by rank", G.deg[G.order].tolist())
    assert max(counts) == 12 and counts.index(12) == stat[4] and counts.count(12) >= 2
    assert G.order[stat[4]] == stat[1] and all(G.deg[G.order[r]] >= G.deg[G.order[r + 1]] for r in range(29))
    # k-NN duplicates: the three matches of one source point are compatible with no one of themselves
    s, q, kw = cases["knn_duplicates"]
    G = ref.Graph(s, q, kw["compat_dist"], kw["max_corr"])
    assert not G.C[:3, :3].any() and out["knn_duplicates"][1][0] == 1 and out["knn_duplicates"][3][[1, 2]].sum() == 0
    T, stat, rmse, inl = out["nonfinite"]
    s, q, kw = cases["nonfinite"]
    G = ref.Graph(s, q, kw["compat_dist"], kw["max_corr"])
    assert stat[0] == 1 and not inl[[3, 7, 11, 20]].any() and all(math.isfinite(v) for v in T) and math.isfinite(rmse)
    assert not G.C[[3, 7, 11, 20]].any() and not G.C[:, [3, 7, 11, 20]].any()
    T, stat, rmse, inl = out["tau_overflow"]             # tau2 = +inf: every two distinct finite rows are compatible
    assert stat[5] == 39 and stat[3] == 40
    # tau2 = 0: a * a < 4 (ls2 * lt2) is left to its rounding, which only lengths that agree to the last bits can pass -- here
    # some of the 24 exact planted pairs (the first rows) among themselves, and no other row
    s, q, kw = cases["tau_underflow"]
    G = ref.Graph(s, q, kw["compat_dist"], kw["max_corr"])
    assert G.tau2 == 0.0 and not G.C[24:].any() and not G.C[:, 24:].any() and G.C.sum() < 24 * 23
    T, stat, rmse, inl = out["corr_overflow"]            # thr2 = +inf: every finite pair counts
    assert stat[0] == 1 and stat[2] == 40 and math.isfinite(rmse)
    assert out["corr_underflow"][1][0] == 0 and out["corr_underflow"][1][3] > 0
    assert out["k_above_every_degree"][1][0] == 1 and out["k2"][1][0] == 1
    full = ref.sc2_one(*cases["seeds_m"][:2], **cases["seeds_m"][2])
    assert out["seeds_m"][:3] == full[:3] == out["seeds_m_plus_5"][:3]
    s, q, kw = cases["seeds_m"]
    assert ref.sc2_one(s, q, **dict(kw, n_seeds=0))[:3] == full[:3]
    assert out["seeds1"][1][3] <= 1 and out["seeds1"][1][4] in (0, -1)
    T, stat, rmse, inl = out["all_compatible"]           # the identity on a grid: every row has degree m - 1
    assert stat == [1, 0, 16, 16, 0, 15] and inl.all() and rmse == 0.0
    assert np.array_equal(np.asarray(T).reshape(4, 4), np.eye(4))
    # a prefix of the seeds: fewer seeds come from the same graph
    s, q, kw = cases["k2"]
    G = ref.Graph(s, q, kw["compat_dist"], kw["max_corr"])
    assert G.result(5, 20)[:3] == ref.sc2_one(s, q, **dict(kw, n_seeds=5, k_consensus=20))[:3]


def test_the_matrix_is_symmetric_to_the_bit():
    rng = np.random.default_rng(0)
    n = 317                                              # 317^2 > 10^5 ordered pairs of rows
    s = (rng.uniform(-1e6, 1e6, (n, 3))).astype(np.float32)
    R, t = FC.pose(rng)
    q = (s.astype(np.float64) @ R.T + t + rng.normal(0, 0.3, (n, 3))).astype(np.float32)
    s64, q64 = s.astype(np.float64), q.astype(np.float64)
    for tau in (0.5, 1.0, 1e3):
        C, n_exact = ref.compat_matrix(s64, q64, tau * tau)
        assert np.array_equal(C, C.T) and not C.diagonal().any()
        if tau == 0.5:
            assert 0 < C.sum() < n * (n - 1)             # both answers occur
    # the exact chain itself, both orders, on the pairs of rows nearest to the threshold
    ls = np.linalg.norm(s64[:, None] - s64[None], axis=2)
    lt = np.linalg.norm(q64[:, None] - q64[None], axis=2)
    near = np.argsort(np.abs(np.abs(ls - lt) - 1.0), axis=None)[:2000]
    rows = lambda a, i: [float(v) for v in a[i]]
    C, _ = ref.compat_matrix(s64, q64, 1.0)
    for i, j in zip(*np.unravel_index(near, ls.shape)):
        a = ref.compat_exact(rows(s64, i), rows(q64, i), rows(s64, j), rows(q64, j), 1.0)
        b = ref.compat_exact(rows(s64, j), rows(q64, j), rows(s64, i), rows(q64, i), 1.0)
        assert a == b == bool(C[i, j])


def test_the_fit_is_the_feature_matching_fit():
    """sc2_ref.fit is featmatch_ref.fit with tests/gicp_ref.py's faster exact fma in the solver: the same bits."""
    s, q, _, _, keep = FC.planted(64, 0.5, 9, noise=0.002)
    rows = lambda a, idx: [[float(v) for v in a[i]] for i in idx]
    for n in (3, 4, 21, 64):
        idx = list(range(n))
        assert ref.fit(rows(s, idx), rows(q, idx)) == fm_ref.fit(rows(s, idx), rows(q, idx))
    line = [[float(t), 2.0 * t, -float(t)] for t in range(5)]
    assert ref.fit(line, line) is None and fm_ref.fit(line, line) is None


def test_options_config_and_parser():
    from corsair_amd import harness as H, registration as R, sc2, shapenet_eval as SE

    assert list(inspect.signature(sc2.sc2_batch).parameters) == [
        "src", "tgt", "offsets", "max_corr", "compat_dist", "m", "n_seeds", "k_consensus", "return_inliers"]
    d = {k: v.default for k, v in inspect.signature(sc2.sc2_batch).parameters.items()}
    assert (d["m"], d["n_seeds"], d["k_consensus"], d["return_inliers"]) == (None, 1024, 20, False)
    assert sc2.Sc2Result._fields == ("T", "inliers", "rmse", "found", "seed_row", "n_valid", "seed_rank", "seed_degree", "mask")
    assert sc2.torch is __import__("torch") and sc2.FAMILY == "sc2"
    assert not hasattr(__import__("corsair_amd.backend").backend, "sc2_batch")
    assert R.check_sc2_options(0.05, 1024, 20, 0.2) == (0.05, 1024, 20)
    assert R.check_sc2_options(None, 0, 2, 0.2) == (0.1, 0, 2)
    nan = float("nan")
    for args, word in (((0.0, 8, 20), "sc2_compat_dist"), ((-1.0, 8, 20), "sc2_compat_dist"), ((nan, 8, 20), "sc2_compat_dist"),
                       ((float("inf"), 8, 20), "sc2_compat_dist"), (("a", 8, 20), "sc2_compat_dist"),
                       ((True, 8, 20), "sc2_compat_dist"), ((0.1, -1, 20), "sc2_seeds"), ((0.1, 2.5, 20), "sc2_seeds"),
                       ((0.1, 2 ** 31, 20), "sc2_seeds"), ((0.1, 8, 1), "sc2_k"), ((0.1, 8, 65), "sc2_k"), ((0.1, 8, 2.0), "sc2_k")):
        with pytest.raises(ValueError, match=word):
            R.check_sc2_options(*args, 0.2)
    z = np.zeros((0, 33), np.float32)
    with pytest.raises(ValueError, match="'sc2'"):
        R.sym_pose_batch(z, z, [0], z, z, [0], [], registration="sc")
    with pytest.raises(ValueError, match="sc2_k"):
        R.sym_pose_batch(z, z, [0], z, z, [0], [], registration="sc2", use_symmetry=False, sc2_k=100)
    c = SE.Config()
    assert (c.registration, c.sc2_compat_dist, c.sc2_seeds, c.sc2_k) == ("ransac", 1.0, 1024, 20)
    c.check_registration()
    SE.Config(registration="sc2", sc2_compat_dist=0.5, sc2_seeds=0, sc2_k=64).check_registration()
    for kw, word in ((dict(sc2_compat_dist=0.0), "sc2_compat_dist"), (dict(sc2_compat_dist="x"), "sc2_compat_dist"),
                     (dict(sc2_seeds=-1), "sc2_seeds"), (dict(sc2_k=1), "sc2_k"), (dict(sc2_k=65), "sc2_k")):
        with pytest.raises(ValueError, match=word):
            SE.Config(**kw).check_registration()
    a = SE.build_parser().parse_args([])
    assert (a.registration, a.sc2_compat_dist, a.sc2_seeds, a.sc2_k) == ("ransac", 1.0, 1024, 20)
    a = SE.build_parser().parse_args(["--registration", "sc2", "--sc2-compat-dist", "0.5", "--sc2-seeds", "0", "--sc2-k", "32"])
    assert (a.registration, a.sc2_compat_dist, a.sc2_seeds, a.sc2_k) == ("sc2", 0.5, 0, 32)
    help_text = " ".join(SE.build_parser().format_help().split())
    assert help_text.count("untuned, no real scan measured") >= 7
    # out of scope there: the harness refuses the value by name, with the words it uses for ransac_fm
    with pytest.raises(ValueError, match="'sc2' .* is not wired into the harness, the sharded evaluation or the cache format"):
        H.Config(registration="sc2").check_icp()
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b", "--registration", "sc2"])


def test_library_exports_and_refusals_without_a_device():
    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    sigs = _lib._declare(lib)
    assert "cs_sc2_batch" in sigs and "cs_sc2_batch" in set(_lib.header_symbols())
    INVALID, UNSUPPORTED = -1, -5
    off0 = (ctypes.c_int64 * 2)(0, 0)
    one = (ctypes.c_int64 * 2)(0, 4)
    bad = (ctypes.c_int64 * 2)(5, 2)
    neg = (ctypes.c_int64 * 2)(-1, 2)
    most = (ctypes.c_int64 * 2)(0, 32768)
    huge = (ctypes.c_int64 * 2)(0, 32769)
    nan, inf = float("nan"), float("inf")
    f = lib.cs_sc2_batch
    # argument checks come before any device work: a call without problems needs no GPU
    ok = lambda **kw: f(None, None, kw.get("off", off0), None, kw.get("n", 0), kw.get("tau", 0.01), kw.get("corr", 0.1),
                        kw.get("seeds", 8), kw.get("k", 20), None, None, None, None, None)
    assert ok() == 0 and ok(seeds=0) == 0 and ok(k=2) == 0 and ok(k=64) == 0 and ok(seeds=2 ** 31 - 1) == 0
    for c in (0.0, -1.0, nan, inf, -inf):
        assert ok(corr=c) == INVALID and b"max_corr" in lib.cs_last_error()
        assert ok(tau=c) == INVALID and b"compat_dist" in lib.cs_last_error()
    assert ok(seeds=-1) == INVALID and b"n_seeds" in lib.cs_last_error()
    for k in (-1, 0, 1, 65, 1000):
        assert ok(k=k) == UNSUPPORTED and b"k_consensus" in lib.cs_last_error()
    assert f(None, None, None, None, 1, 0.01, 0.1, 8, 20, None, None, None, None, None) == INVALID
    assert ok(n=-1) == INVALID and ok(off=bad, n=1) == INVALID and ok(off=neg, n=1) == INVALID
    assert ok(off=huge, n=1) == UNSUPPORTED and b"smaller k_nn" in lib.cs_last_error()
    assert ok(off=most, n=1) == INVALID and b"NULL" in lib.cs_last_error()        # 32 768 slots pass; NULL outputs do not
    assert ok(n=1) == INVALID and b"NULL" in lib.cs_last_error()
    buf = (ctypes.c_double * 16)()
    assert f(None, None, one, None, 1, 0.01, 0.1, 8, 20, buf, buf, buf, None, None) == INVALID      # NULL pairs while a slot exists


def test_source_layout_and_documents():
    header = open(os.path.join(ROOT, "include", "corsair_hip.h")).read()
    assert "int cs_sc2_batch(" in header and '"sc2"' in header
    at = header.index("cs_sc2_batch:")
    block = " ".join(header[at:header.index("int cs_sc2_batch(")].split())
    for words in ("Differences from SC2-PCR and spectral matching", "NO eigenvector", "no non-maximum suppression",
                  "ONE consensus stage", "UNWEIGHTED fit", "HARD compatibility", "ranked by its inlier count", "NO final refit",
                  "ASCENDING ROW INDEX", "SMALLEST rank", "horn_qcp ALONE", "A permutation of the pairs", "CS_SC2_CHUNK_BYTES",
                  "CS_SC2_SLICE", "CS_SC2_SPAN", "a smaller k_nn", "a * a < 4.0 * (ls2 * lt2)"):
        assert words in block, words
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    text = open(os.path.join(csrc, "sc2.hip")).read()
    assert '#include "horn.h"' in text and "horn_qcp(" in text and '#include "sc2_plan.h"' in text and "ransac.h\"" not in text
    assert "jacobi" not in text.replace("Jacobi", "")
    for word in ("hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "hipStreamSynchronize", "hipDeviceSynchronize",
                 "atomicCAS", "hipMalloc("):
        assert word not in text, word
    for word in ("atomicAdd(", "atomicMax(", "PoolBuf<", 'ProfScope prof("sc2"', "__popcll(", "sc2_check_args(", "sc2_plan("):
        assert word in text, word
    plan = open(os.path.join(csrc, "sc2_plan.h")).read()
    assert "hip" not in plan.replace("HIP header", "").replace("sc2.hip", "").replace("corsair_hip.h", "")      # plain C++
    assert "int main(" in open(os.path.join(ROOT, "tools", "sc2_plan_check.cpp")).read()
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "sc2.hip" in make and "sc2.o: horn.h nn_common.h sc2_plan.h" in make
    assert '"sc2"' in open(os.path.join(csrc, "runtime.hip")).read()
    assert "sc2" not in open(os.path.join(ROOT, "corsair_amd", "backend.py")).read()
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    for words in ("cs_sc2_batch", "--registration sc2", "untuned, no real scan measured"):
        assert words in readme, words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 27." in design and "cs_sc2_batch" in design
    tail = design[design.index("## 27."):]
    for words in ("not measured", "real scans", "hardware counters", "22 k-pair"):
        assert words in tail.lower() or words in tail, words
    for name, word in (("INTEGRATION.md", "CS_SC2_CHUNK_BYTES"), ("tools/README.md", "sc2_bench.py")):
        assert word in open(os.path.join(ROOT, name)).read(), name
