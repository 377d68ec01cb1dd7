"""Candidate verification without a GPU: the restatement of cs_chamfer_2dir against SciPy's KD-tree, the ordering
rule, the refusals of Config / run_eval / the command line, the result cache with the verification arrays, and the statistics
of the re-ranked list."""
import os
import types

import numpy as np
import pytest

from tests import verify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = q
    T[:3, 3] = rng.normal(scale=0.2, size=3)
    return T


@pytest.mark.parametrize("ns,nt", [(1, 1), (1, 300), (257, 64), (400, 513)])
def test_restatement_matches_scipy_kdtree_in_both_directions(ns, nt):
    from scipy.spatial import cKDTree

    rng = np.random.default_rng(1000 * ns + nt)
    src = rng.normal(size=(ns, 3)).astype(np.float32)
    tgt = rng.normal(size=(nt, 3)).astype(np.float32)
    tgt[nt // 2] = tgt[0]                                       # a duplicate target
    T = _rigid(rng)
    posed = (T.astype(np.float64)[:3, :3] @ src.astype(np.float64).T).T + T.astype(np.float64)[:3, 3]
    fwd, bwd = ref.chamfer_2dir(src, tgt, T)
    assert fwd == pytest.approx(float(np.mean(cKDTree(tgt.astype(np.float64)).query(posed)[0])), rel=1e-12, abs=0)
    assert bwd == pytest.approx(float(np.mean(cKDTree(posed).query(tgt.astype(np.float64))[0])), rel=1e-12, abs=0)
    batch = ref.chamfer_2dir_batch(np.concatenate([src, src]), [0, ns, 2 * ns], tgt, [0, nt], [1, 0], [0, 0], np.stack([T, T]))
    assert np.array_equal(batch, np.asarray([[fwd, bwd], [fwd, bwd]]))


def test_restatement_special_values():
    inf, nan = float("inf"), float("nan")
    rng = np.random.default_rng(5)
    a = rng.normal(size=(9, 3)).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)
    empty = np.zeros((0, 3), np.float32)
    assert ref.chamfer_2dir(a, a, eye) == (0.0, 0.0)
    f, b = ref.chamfer_2dir(empty, a, eye)
    assert np.isnan(f) and b == inf
    f, b = ref.chamfer_2dir(a, empty, eye)
    assert f == inf and np.isnan(b)
    f, b = ref.chamfer_2dir(empty, empty, eye)
    assert np.isnan(f) and np.isnan(b)
    # a far outlier of the target moves the backward value alone: the directions are not interchangeable
    far = np.concatenate([a, [[100.0, 0.0, 0.0]]]).astype(np.float32)
    f, b = ref.chamfer_2dir(a, far, eye)
    assert f == 0.0 and b == pytest.approx(np.min(np.linalg.norm(far[-1].astype(np.float64) - a, axis=1)) / 10, rel=1e-12)
    # a NaN target row is nobody's nearest and has no partner itself; a NaN source row likewise
    bad = a.copy()
    bad[3, 1] = nan
    assert ref.chamfer_2dir(a, bad, eye)[1] == inf and np.isfinite(ref.chamfer_2dir(a, bad, eye)[0])
    assert ref.chamfer_2dir(bad, a, eye)[0] == inf and np.isfinite(ref.chamfer_2dir(bad, a, eye)[1])
    bad[3, 1] = inf
    assert ref.chamfer_2dir(a, bad, eye)[1] == inf and ref.chamfer_2dir(bad, a, eye)[0] == inf
    Tn = eye.copy()
    Tn[1, 3] = nan
    assert ref.chamfer_2dir(a, a, Tn) == (inf, inf)


# ---- the ordering rule -------------------------------------------------------------------------------------------------
def test_order_ties_nan_inf_and_rows_without_a_finite_score():
    from corsair_amd import harness as H

    inf, nan = float("inf"), float("nan")
    cases = {
        "sorted": ([0.1, 0.2, 0.3], [0, 1, 2]),
        "reversed": ([0.3, 0.2, 0.1], [2, 1, 0]),
        "ties keep the retrieval order": ([0.5, 0.1, 0.5, 0.1], [1, 3, 0, 2]),
        "signed zeros tie": ([0.0, -0.0, 0.0], [0, 1, 2]),
        "nan last": ([nan, 0.4, 0.2], [2, 1, 0]),
        "inf last": ([inf, 0.4, 0.2], [2, 1, 0]),
        "nan and inf after the finite ones, in retrieval order": ([inf, 3.0, nan, 1.0, inf], [3, 1, 0, 2, 4]),
        "-inf is not finite": ([-inf, 1.0], [1, 0]),
        "nothing finite: nothing moves": ([nan, inf, nan], [0, 1, 2]),
        "all inf": ([inf, inf], [0, 1]),
        "one candidate": ([nan], [0]),
    }
    for name, (scores, want) in cases.items():
        got = H.verify_order(scores)
        assert got.dtype == np.int32 and got.tolist() == want, name
        assert ref.order(scores).tolist() == want, name
    table = np.asarray([c[0] for c in cases.values() if len(c[0]) == 3], np.float64)
    assert np.array_equal(H.verify_order(table), np.stack([ref.order(r) for r in table]))
    rng = np.random.default_rng(3)
    rnd = rng.integers(0, 4, size=(200, 7)).astype(np.float64)
    rnd[rng.random(rnd.shape) < 0.2] = nan
    rnd[rng.random(rnd.shape) < 0.1] = inf
    assert np.array_equal(H.verify_order(rnd), np.stack([ref.order(r) for r in rnd]))


def test_scores_symmetric_and_forward():
    from corsair_amd import harness as H

    fb = np.asarray([[[0.25, 0.5], [1.0, float("inf")]], [[float("nan"), 1.0], [0.125, 0.0]]])
    sym = H.verify_scores(fb, "symmetric")
    assert sym.dtype == np.float64 and sym[0, 0] == 0.75 and sym[0, 1] == float("inf") and np.isnan(sym[1, 0]) and sym[1, 1] == 0.125
    assert np.array_equal(H.verify_scores(fb, "forward"), fb[..., 0], equal_nan=True)
    with pytest.raises(ValueError, match="score"):
        H.verify_scores(fb, "trimmed")


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_config_defaults_and_refusals():
    from corsair_amd import harness as H

    c = H.Config()
    assert (c.verify_top_k, c.verify_score) == (0, "symmetric") and c.verify_k() == 0
    assert H.Config(verify_top_k=1).verify_k() == 0 and H.Config(verify_top_k=2).verify_k() == 2
    assert H.Config(verify_top_k=32, verify_score="forward").verify_k() == 32
    for bad in (-1, 33, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="verify_top_k"):
            H.Config(verify_top_k=bad).check_verify()
    for bad in ("chamfer", "", None, "Symmetric"):
        with pytest.raises(ValueError, match="verify_score"):
            H.Config(verify_score=bad).check_verify()


def test_run_eval_refuses_before_it_touches_the_device():
    from corsair_amd import harness as H, sharding

    clouds = [np.zeros((4, 3), np.float32)] * 3
    args = (clouds, clouds, [0, 1, 2], np.zeros((3, 3)), None, None, [1, 1, 1])
    pipe = types.SimpleNamespace(cfg=H.Config(verify_top_k=2))
    with pytest.raises(ValueError, match="register_top1"):
        H.run_eval(pipe, *args, register_top1=False)
    pipe = types.SimpleNamespace(cfg=H.Config(verify_top_k=4))
    with pytest.raises(ValueError, match="exceeds the catalog"):
        H.run_eval(pipe, *args)
    pipe = types.SimpleNamespace(cfg=H.Config(verify_top_k=40))
    with pytest.raises(ValueError, match="verify_top_k"):
        H.run_eval(pipe, *args)
    pipe = types.SimpleNamespace(cfg=H.Config(verify_top_k=2, verify_score="both"))
    with pytest.raises(ValueError, match="verify_score"):
        H.run_eval(pipe, *args)
    pipe = types.SimpleNamespace(cfg=H.Config(verify_top_k=2), device="cpu")
    with pytest.raises(NotImplementedError, match="verify_top_k"):
        sharding.run_eval_sharded(pipe, object(), 0, 2, *args)


def test_command_line_options_and_the_register_gt_refusal():
    from corsair_amd import harness as H

    base = ["--checkpoint", "none.pth", "--catalog-dir", "none", "--query-dir", "none"]
    a = H.build_parser().parse_args(base)
    assert (a.verify_top_k, a.verify_score) == (0, "symmetric")
    a = H.build_parser().parse_args(base + ["--verify-top-k", "5", "--verify-score", "forward"])
    assert (a.verify_top_k, a.verify_score) == (5, "forward")
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(base + ["--verify-score", "both"])
    with pytest.raises(ValueError, match="--register-gt"):
        H.main(base + ["--verify-top-k", "3", "--register-gt"])
    with pytest.raises(ValueError, match="verify_top_k"):
        H.main(base + ["--verify-top-k", "33"])


# ---- the result cache --------------------------------------------------------------------------------------------------
def _nine(q, fill=0.0):
    from corsair_amd import cache as C

    return {k: np.full((q, 4, 4) if k.startswith("Ts_est") else q, fill, C.DTYPES[k]) for k in C.NAMES}


def _verified(q, k, seed, icp=False):
    """A self-consistent result of a run with verification: the winners' poses are the scored poses of the first-ranked
    candidates (Ts_est_icp when the refinement ran, else Ts_est_best)."""
    from corsair_amd import cache as C

    rng = np.random.default_rng(seed)
    res = _nine(q, float(seed + 1))
    res.update(verify_cand=rng.integers(0, 9, (q, k)).astype(np.int64), verify_score=rng.random((q, k)),
               verify_order=np.argsort(rng.random((q, k)), 1).astype(np.int32),
               verify_T=rng.random((q, k, 4, 4)).astype(np.float32))
    won = res["verify_T"][np.arange(q), res["verify_order"][:, 0]]
    if icp:
        res.update({n: np.full((q, 4, 4) if n.startswith("Ts_est") else q, seed + 2, C.ICP_DTYPES[n]) for n in C.ICP_NAMES})
        res["Ts_est_icp"] = won.copy()
    else:
        res["Ts_est_best"] = won.copy()
    return res


def test_cache_round_trip_and_misses(tmp_path):
    from corsair_amd import cache as C

    assert C.VERIFY_NAMES == ("verify_cand", "verify_score", "verify_order", "verify_T")
    assert set(C.VERIFY_DTYPES) == set(C.VERIFY_NAMES)
    assert not set(C.VERIFY_NAMES) & (set(C.NAMES) | set(C.ICP_NAMES) | set(C.ICP_SCALE_NAMES))
    q, k = 5, 3
    res = _verified(q, k, seed=0)
    res["verify_score"][1, 2] = np.nan
    d = str(tmp_path / "v")
    C.save_results(d, "chair", True, res)
    # a file set of its own: the reference's nine names are not touched by a run with verification
    assert sorted(os.listdir(d)) == sorted(f"{n}_chair_top1_verify.npy" for n in C.NAMES + C.VERIFY_NAMES)
    back = C.load_results(d, "chair", True, verify=k)
    assert set(back) == set(C.NAMES) | set(C.VERIFY_NAMES)
    for n in C.VERIFY_NAMES:
        assert back[n].dtype == C.VERIFY_DTYPES[n] and back[n].shape == res[n].shape, n
        assert np.array_equal(back[n], res[n], equal_nan=True), n
    for n in C.NAMES:
        assert np.array_equal(back[n], res[n]), n
    # another K is a miss; a run without verification never reads the winners' arrays
    assert C.load_results(d, "chair", True, verify=2) is None and C.load_results(d, "chair", True, verify=4) is None
    assert C.load_results(d, "chair", True) is None and C.load_results(d, "chair", True, verify=1) is None
    assert C.load_results(d, "chair", False, verify=k) is None and C.load_results(d, "chair", True, icp=True, verify=k) is None
    # winners that are not the first-ranked candidates' scored poses are a miss
    moved = dict(res, verify_order=np.roll(res["verify_order"], 1, axis=1))
    C.save_results(d, "chair", True, moved)
    assert C.load_results(d, "chair", True, verify=k) is None
    C.save_results(d, "chair", True, res)
    assert C.load_results(d, "chair", True, verify=k) is not None
    # a missing file is a miss
    os.remove(os.path.join(d, "verify_T_chair_top1_verify.npy"))
    assert C.load_results(d, "chair", True, verify=k) is None


def test_cache_verified_plain_verified_in_one_directory(tmp_path):
    """The A/B sequence K -> 0 -> K (and with / without the refinement) in one cache directory: no run ever reads arrays that
    another kind of run wrote, and each kind keeps hitting its own set."""
    from corsair_amd import cache as C

    d, q, k = str(tmp_path), 6, 3
    ver = _verified(q, k, seed=1)
    plain = _nine(q, 7.0)
    C.save_results(d, "chair", True, ver)                                   # K = 3
    assert C.load_results(d, "chair", True) is None                         # K = 0: a miss, recomputed and saved
    C.save_results(d, "chair", True, plain)
    for _ in range(2):                                                      # ... and plain runs hit from then on
        back = C.load_results(d, "chair", True)
        assert set(back) == set(C.NAMES) and all(np.array_equal(back[n], plain[n]) for n in C.NAMES)
    back = C.load_results(d, "chair", True, verify=k)                       # K = 3 again: its own winners, not the top-1 arrays
    assert all(np.array_equal(back[n], ver[n]) for n in C.NAMES + C.VERIFY_NAMES)
    assert not np.array_equal(back["Ts_est_best"], plain["Ts_est_best"])
    # with the refinement the winners are ranked by the refined pose: another result, which replaces the set as a whole
    ver_icp = _verified(q, k, seed=2, icp=True)
    assert C.load_results(d, "chair", True, icp=True, verify=k) is None
    C.save_results(d, "chair", True, ver_icp)
    back = C.load_results(d, "chair", True, icp=True, verify=k)
    assert all(np.array_equal(back[n], ver_icp[n]) for n in C.NAMES + C.ICP_NAMES + C.VERIFY_NAMES)
    assert C.load_results(d, "chair", True, verify=k) is None               # read without the refinement: a miss
    C.save_results(d, "chair", True, ver)                                   # ... recomputed: the stale ICP files go
    assert not [f for f in os.listdir(d) if f.endswith("_verify.npy") and f.startswith(tuple(C.ICP_NAMES))]
    assert C.load_results(d, "chair", True, icp=True, verify=k) is None
    assert C.load_results(d, "chair", True, verify=k) is not None
    back = C.load_results(d, "chair", True)                                 # the plain set was never touched
    assert all(np.array_equal(back[n], plain[n]) for n in C.NAMES)
    assert sorted(os.listdir(d)) == sorted([f"{n}_chair_top1.npy" for n in C.NAMES] +
                                           [f"{n}_chair_top1_verify.npy" for n in C.NAMES + C.VERIFY_NAMES])


def test_cache_written_without_verification_loads_as_before(tmp_path):
    from corsair_amd import cache as C

    res = _nine(4, 2.0)
    d = str(tmp_path / "plain")
    C.save_results(d, "table", True, res)
    assert sorted(os.listdir(d)) == sorted(f"{n}_table_top1.npy" for n in C.NAMES)
    for args in ((), (False, False), (False, False, 0), (False, False, 1)):
        back = C.load_results(d, "table", True, *args)
        assert set(back) == set(C.NAMES) and all(np.array_equal(back[n], res[n]) for n in C.NAMES)
    assert C.load_results(d, "table", True, verify=3) is None          # verification asked for: a miss


# ---- the statistics of the re-ranked list ------------------------------------------------------------------------------
def test_verify_stat_on_a_hand_made_table_and_rank():
    from corsair_amd import harness as H
    from corsair_amd.utils import retrieval

    n = 20                                                   # pos_n = 2
    table = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.float64)      # neighbours of c: c, c-1, c+1, ...
    best = np.asarray([3, 7, 11, 15])
    rank = np.asarray([[5, 3, 4, 9],            # the true CAD second
                       [7, 8, 1, 2],            # already first
                       [0, 1, 11, 12],          # third
                       [14, 16, 2, 15]])        # outside the verified columns
    order = np.asarray([[1, 0, 2], [0, 1, 2], [2, 0, 1], [0, 1, 2]], np.int32)
    new = H.verify_rerank(rank, order)
    assert new.tolist() == [[3, 5, 4, 9], [7, 8, 1, 2], [11, 0, 1, 12], [14, 16, 2, 15]]
    v = H.verify_stat(rank, order, table, best, 2, "forward")
    want = retrieval.scan2cad_retrieval_eval_rank(new, table, best, 2)
    for key in ("precision", "top1_error", "top1_predict", "gt"):
        assert v[key] == want[key], key
    assert v["gt"] == best.tolist() and v["top1_predict"] == [3, 7, 11, 14]
    assert v["moved"] == 2 and v["top1_hit"] == 0.75 and v["top1_hit_before"] == 0.25
    assert v["top1_error"] == 0.25 and (v["k"], v["score"]) == (3, "forward")
    # precision: |{3,5} & {3,2}|, |{7,8} & {7,6}|, |{11,0} & {11,10}|, |{14,16} & {15,14}| of 2 each
    assert v["precision"] == 50.0
    before = retrieval.scan2cad_retrieval_eval_rank(rank, table, best, 2)
    assert before["top1_predict"] == [5, 7, 0, 14]
    # the identity order changes nothing
    same = H.verify_stat(rank, np.tile(np.arange(3, dtype=np.int32), (4, 1)), table, best, 2)
    assert same["moved"] == 0 and same["top1_hit"] == same["top1_hit_before"] == 0.25
    assert same["precision"] == before["precision"] and same["top1_error"] == before["top1_error"]


def test_report_block_only_when_verification_ran():
    from corsair_amd import harness as H

    pq = _nine(3, 0.5)
    stat = {"precision": 1.0, "top1_error": 0.0, "top1_predict": [0, 1, 2], "gt": [0, 1, 2]}
    plain = H.finish_eval(stat, pq, False)
    assert "candidate verification" not in plain.report
    v = dict(stat, moved=1, top1_hit=1.0, top1_hit_before=2 / 3, k=3, score="symmetric")
    res = H.finish_eval(dict(stat, verify=v), pq, False)
    assert res.report.startswith(plain.report) and "candidate verification (top-3" in res.report
    assert "queries whose top-1 changed: 1" in res.report


def test_declared_everywhere():
    import inspect

    from corsair_amd import _lib, backend

    assert "cs_chamfer_2dir" in _lib.header_symbols()
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    assert "cs_chamfer_2dir" in open(os.path.join(csrc, "chamfer.hip")).read()
    assert '"chamfer2"' in open(os.path.join(csrc, "runtime.hip")).read()
    head = open(_lib.HEADER_PATH).read()
    for word in ("cs_chamfer_2dir", '"chamfer2"', "backward", "Non-finite"):
        assert word in head, word
    assert list(inspect.signature(backend.chamfer_2dir).parameters) == ["src", "soff", "tgt", "toff", "src_seg", "tgt_seg", "T"]
    lib = _lib.load()
    assert hasattr(lib, "cs_chamfer_2dir")
