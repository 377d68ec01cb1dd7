"""cs_fgr_batch on the GPU: transforms (f32 and f64), inliers, rmse, updates and tuple counts are BIT-EQUAL to
tests/fgr_ref.py -- lane tails and wave / block boundaries of the working list, the < 10 rule, the floor of mu, the tuple
test with its cap reached in the first chunk of trials, in a later one and never, degenerate frames, independence of
neighbours, runs and (test off) pair order, and every refusal."""
import functools

import numpy as np
import pytest
import torch

from tests import fgr_ref as ref

pytestmark = pytest.mark.gpu

MAX_CORR = 0.05
RAGGED = (0, 3, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1000)
CHUNK_TRIALS = 2048          # trials per chunk of the kernel (4 per lane, 512 lanes)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _run(dev, src, tgt, offsets, max_corr=MAX_CORR, **kw):
    from corsair_amd import backend as B

    r = B.fgr_batch(torch.from_numpy(np.ascontiguousarray(src, np.float32).reshape(-1, 3)).to(dev),
                    torch.from_numpy(np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)).to(dev), offsets, max_corr, **kw)
    return {"T32": r.T.cpu().numpy().reshape(-1, 16), "T": r.T64.cpu().numpy().reshape(-1, 16),
            "inliers": r.inliers.cpu().numpy(), "rmse": r.rmse.cpu().numpy(), "iters": r.iters.cpu().numpy(),
            "n_tuple": r.n_tuple.cpu().numpy()}


def _check(got, want, what=""):
    for p, w in enumerate(want):
        tag = "%s problem %d" % (what, p)
        assert _same(got["T"][p], w["T"]), (tag, got["T"][p], w["T"])
        assert _same(got["T32"][p], w["T32"]), tag
        assert got["inliers"][p] == w["inliers"], (tag, got["inliers"][p], w["inliers"])
        assert _same(got["rmse"][p], np.float64(w["rmse"])), (tag, got["rmse"][p], w["rmse"])
        assert got["iters"][p] == w["iters"], (tag, got["iters"][p], w["iters"])
        assert got["n_tuple"][p] == w["n_tuple"], (tag, got["n_tuple"][p], w["n_tuple"])


def _is_identity(got, p):
    return np.array_equal(got["T"][p], np.asarray(ref.IDENTITY)) and got["iters"][p] == 0


@functools.lru_cache(maxsize=None)
def _ragged():
    """One problem per size of RAGGED: a fifth of the targets are outliers, every problem in its own pose."""
    parts = [ref.outlier_case(n, 0.2, 100 + n)[:2] for n in RAGGED]
    off = np.concatenate([[0], np.cumsum(RAGGED)]).tolist()
    src, tgt = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return src, tgt, off, ref.fgr_batch(src, tgt, off, MAX_CORR, iteration_number=8, tuple_test_on=False)


@functools.lru_cache(maxsize=None)
def _outliers300():
    src, tgt, R, t = ref.outlier_case(300, 0.8, 7)
    return src, tgt


@functools.lru_cache(maxsize=None)
def _outliers300_ref(max_tuple, seed=0):
    src, tgt = _outliers300()
    return ref.fgr(src, tgt, MAX_CORR, max_tuple=max_tuple, seed=seed)


def test_ragged_batch_without_tuple_test(gpu):
    src, tgt, off, want = _ragged()
    got = _run(gpu, src, tgt, off, iteration_number=8, tuple_test=False)
    _check(got, want, "ragged")
    for p, n in enumerate(RAGGED):
        assert want[p]["iters"] == (8 if n >= 10 else 0) and want[p]["n_tuple"] == -1
        if n < 10:
            assert _is_identity(got, p)
    assert got["inliers"][0] == 0 and got["rmse"][0] == 0.0          # the empty problem
    # the order of the pairs does not matter with the test off
    perm = np.random.default_rng(5).permutation(1000)
    a, b = off[-2], off[-1]
    shuffled = _run(gpu, src[a:b][perm], tgt[a:b][perm], [0, 1000], iteration_number=8, tuple_test=False)
    assert all(_same(shuffled[k][0], got[k][-1]) for k in got)


def test_default_iterations_reach_the_floor_of_mu(gpu):
    src, tgt, _, _ = ref.outlier_case(200, 0.1, 11)
    for tuple_test in (False, True):
        want = ref.fgr(src, tgt, MAX_CORR, tuple_test_on=tuple_test)
        assert want["iters"] == 64 and want["mu"] < 0.025
        _check(_run(gpu, src, tgt, [0, 200], tuple_test=tuple_test), [want], "defaults, tuple test %s" % tuple_test)


def test_tuple_cap_in_first_chunk(gpu):
    src, tgt, _, _ = ref.outlier_case(40, 0.0, 12)
    trials = []
    fr = ref.frame(src, tgt)
    ref.tuple_test((src.astype(np.float64) - fr[0]) / fr[2], (tgt.astype(np.float64) - fr[1]) / fr[2], 0, 0.95, 16,
                   trials=trials)
    assert len(trials) == 16 and trials[-1] < CHUNK_TRIALS
    want = ref.fgr(src, tgt, MAX_CORR, max_tuple=16)
    assert want["n_tuple"] == 16
    _check(_run(gpu, src, tgt, [0, 40], max_tuple=16), [want], "cap in the first chunk")


def test_tuple_cap_in_a_later_chunk(gpu):
    src, tgt = _outliers300()
    trials = []
    fr = ref.frame(src, tgt)
    ref.tuple_test((src.astype(np.float64) - fr[0]) / fr[2], (tgt.astype(np.float64) - fr[1]) / fr[2], 0, 0.95, 64,
                   trials=trials)
    assert len(trials) == 64 and trials[-1] >= CHUNK_TRIALS
    want = _outliers300_ref(64)
    assert want["n_tuple"] == 64
    _check(_run(gpu, src, tgt, [0, 300], max_tuple=64), [want], "cap in a later chunk")


def test_tuple_cap_never_reached(gpu):
    src, tgt = _outliers300()
    want = _outliers300_ref(1000)
    assert 10 < want["n_tuple"] < 1000                                 # all 30 000 trials ran
    got = _run(gpu, src, tgt, [0, 300])
    _check(got, [want], "cap never reached")
    # two runs with one seed agree; another seed draws other trials
    again = _run(gpu, src, tgt, [0, 300])
    assert all(_same(got[k], again[k]) for k in got)
    other = _run(gpu, src, tgt, [0, 300], seed=1)
    _check(other, [_outliers300_ref(1000, 1)], "seed 1")
    assert other["n_tuple"][0] != got["n_tuple"][0]


def test_zero_tuples(gpu):
    src, _, _, _ = ref.outlier_case(100, 0.0, 13)
    tgt = (3.0 * src).astype(np.float32)
    want = ref.fgr(src, tgt, MAX_CORR)
    assert want["n_tuple"] == 0
    got = _run(gpu, src, tgt, [0, 100])
    _check(got, [want], "zero tuples")
    assert _is_identity(got, 0) and got["n_tuple"][0] == 0


@pytest.mark.parametrize("tuple_test", [False, True])
def test_degenerate_inputs(gpu, tuple_test):
    src, tgt, _, _ = ref.outlier_case(50, 0.0, 14)
    one = np.tile(np.asarray([[0.25, -1.0, 3.0]], np.float32), (50, 1))
    nan_src = src.copy()
    nan_src[17, 1] = np.nan
    inf_tgt = tgt.copy()
    inf_tgt[3, 2] = np.inf
    S = np.concatenate([one, nan_src, src, src])
    Q = np.concatenate([one, tgt, inf_tgt, tgt])
    off = [0, 50, 100, 150, 200]
    want = ref.fgr_batch(S, Q, off, MAX_CORR, tuple_test_on=tuple_test)
    got = _run(gpu, S, Q, off, tuple_test=tuple_test)
    _check(got, want, "degenerate")
    assert all(_is_identity(got, p) for p in range(3)) and not _is_identity(got, 3)
    assert got["inliers"][0] == 50 and got["rmse"][0] == 0.0          # all pairs at one point: g = 0


def test_problem_alone_and_between_neighbours(gpu):
    src, tgt, off, want = _ragged()
    o_src, o_tgt = _outliers300()
    a, b = off[-2], off[-1]
    for kw, w in (({"iteration_number": 8, "tuple_test": False}, want[-1]), ({"max_tuple": 64}, None)):
        if w is None:
            ps, pt, w = o_src, o_tgt, _outliers300_ref(64)
        else:
            ps, pt = src[a:b], tgt[a:b]
        n = len(ps)
        alone = _run(gpu, ps, pt, [0, n], **kw)
        _check(alone, [w], "alone")
        S = np.concatenate([src[off[8]:off[9]], ps, o_src[:77]])
        Q = np.concatenate([tgt[off[8]:off[9]], pt, o_tgt[:77]])
        n0 = off[9] - off[8]
        mid = _run(gpu, S, Q, [0, n0, n0 + n, n0 + n + 77], **kw)
        assert all(_same(mid[k][1], alone[k][0]) for k in alone)


def _raw(dev, m=20, **over):
    """The C entry itself with one valid 20-pair problem; `over` replaces arguments."""
    from corsair_amd import _lib

    lib = _lib.load()
    src = torch.rand((m, 3), device=dev)
    tgt = torch.rand((m, 3), device=dev)
    out = {"T": torch.empty(16, device=dev), "T64": torch.empty(16, dtype=torch.float64, device=dev),
           "inl": torch.empty(1, dtype=torch.int32, device=dev), "rmse": torch.empty(1, dtype=torch.float64, device=dev),
           "it": torch.empty(1, dtype=torch.int32, device=dev), "nt": torch.empty(1, dtype=torch.int32, device=dev)}
    a = {"src": _lib.ptr(src), "tgt": _lib.ptr(tgt), "off": _lib.i64_array([0, m]), "n_prob": 1, "max_corr": 0.05,
         "mu_floor": 0.025, "division_factor": 1.4, "iteration_number": 4, "tuple_test": 1, "tuple_scale": 0.95,
         "max_tuple": 100, "seed": 0, "T": _lib.ptr(out["T"]), "T64": _lib.ptr(out["T64"]), "inl": _lib.ptr(out["inl"]),
         "rmse": _lib.ptr(out["rmse"]), "it": _lib.ptr(out["it"]), "nt": _lib.ptr(out["nt"])}
    a.update(over)
    rc = lib.cs_fgr_batch(a["src"], a["tgt"], a["off"], a["n_prob"], a["max_corr"], a["mu_floor"], a["division_factor"],
                          a["iteration_number"], a["tuple_test"], a["tuple_scale"], a["max_tuple"], a["seed"], a["T"],
                          a["T64"], a["inl"], a["rmse"], a["it"], a["nt"], _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


CS_ERR_INVALID, CS_ERR_UNSUPPORTED = -1, -5       # include/corsair_hip.h


def test_refusals(gpu):
    from corsair_amd import _lib

    assert _raw(gpu) == 0
    assert _raw(gpu, T64=None) == 0                                    # the f64 copy is optional
    nan, inf = float("nan"), float("inf")
    for over in ({"off": None}, {"T": None}, {"inl": None}, {"rmse": None}, {"it": None}, {"nt": None}, {"src": None},
                 {"tgt": None}, {"max_corr": 0.0}, {"max_corr": -1.0}, {"max_corr": nan}, {"max_corr": inf},
                 {"mu_floor": 0.0}, {"mu_floor": nan}, {"mu_floor": inf}, {"division_factor": 1.0},
                 {"division_factor": nan}, {"tuple_scale": 0.0}, {"tuple_scale": 1.0}, {"tuple_scale": nan},
                 {"max_tuple": 0}, {"off": _lib.i64_array([20, 0])}):
        assert _raw(gpu, **over) == CS_ERR_INVALID, over
    for over in ({"iteration_number": -1}, {"iteration_number": 1001}, {"max_tuple": ref.MAX_TUPLE_CAP + 1},
                 {"off": _lib.i64_array([0, 1 << 31])}):
        assert _raw(gpu, **over) == CS_ERR_UNSUPPORTED, over
    assert _raw(gpu, iteration_number=0) == 0 and _raw(gpu, iteration_number=1000, max_tuple=4) == 0


def test_no_problem_is_ok(gpu):
    assert _raw(gpu, n_prob=0) == 0
    assert _raw(gpu, n_prob=0, T=None, inl=None, rmse=None, it=None, nt=None, src=None, tgt=None) == 0
    from corsair_amd import backend as B

    r = B.fgr_batch(torch.zeros((0, 3), device=gpu), torch.zeros((0, 3), device=gpu), [0], MAX_CORR)
    assert r.T.shape == (0, 4, 4) and r.n_tuple.numel() == 0
    assert isinstance(r, B.FgrResult)
