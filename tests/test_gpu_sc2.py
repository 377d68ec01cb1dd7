"""cs_sc2_batch on the device against tests/sc2_ref.py, bit for bit; the same bits in every schedule and launch
shape; the stream contract and the stale-memory schedules through the helpers of tests/stream_cases.py and
tests/stale_cases.py with corsair_amd.sc2 in backend's place; sym_pose_batch with registration = "sc2" on the real CAD /
partial-view pairs; and that the defaults launch nothing of the family."""
import functools

import numpy as np
import pytest
import torch

from tests import sc2_cases as CS
from tests import sc2_ref as ref
from tests import stale_cases as ST
from tests import stream_cases as SC

pytestmark = pytest.mark.gpu

SEED = 1
# (n_seeds, K): every n_seeds of {1, 7, 256, 0} and every K of {2, 20, 64}
PARAMS = ((1, 20), (7, 2), (7, 64), (256, 2), (256, 20), (256, 64), (0, 20))
ONE_MATRIX = 8 * 4097 * 65      # the bytes of the largest problem's matrix
# every launch shape the unit reads from the environment
SHAPES = ({}, {"CS_SC2_CHUNK_BYTES": str(ONE_MATRIX)}, {"CS_SC2_CHUNK_BYTES": str(2 * ONE_MATRIX)}, {"CS_SC2_CHUNK_BYTES": "1"},
          {"CS_SC2_SLICE": "64"}, {"CS_SC2_SLICE": "300", "CS_SC2_SPAN": "1"}, {"CS_SC2_SPAN": "3"})
ALL_SHAPES = ((256, 20), (0, 20))   # the parameters that run under every shape; the others run under the default


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return (t.detach().contiguous().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).tobytes()


@functools.lru_cache(maxsize=None)
def _graphs():
    d = CS.batch(SEED)
    return d, [ref.Graph(*CS.problem(d, p), CS.TAU, CS.MAX_CORR) for p in range(len(CS.SIZES))]


@functools.lru_cache(maxsize=None)
def _want(n_seeds, K):
    _, graphs = _graphs()
    T, stat, rmse = [], [], []
    mask = np.zeros(CS.OFF[-1], np.uint8)
    for p, g in enumerate(graphs):
        Tp, sp, rp, inl = g.result(n_seeds, K)
        T.append(Tp)
        stat.append(sp)
        rmse.append(rp)
        mask[CS.OFF[p]:CS.OFF[p] + CS.SIZES[p]] = inl
    return (np.asarray(T, np.float64).reshape(-1, 4, 4), np.asarray(stat, np.int32), np.asarray(rmse, np.float64), mask)


def _same(r, want, what):
    T, stat, rmse, mask = want
    got_stat = torch.stack([r.found, r.seed_row, r.inliers, r.n_valid, r.seed_rank, r.seed_degree], 1)
    assert _bits(got_stat) == _bits(stat), (what, got_stat.cpu().numpy().tolist(), stat.tolist())
    assert _bits(r.T) == _bits(T), what
    assert _bits(r.rmse) == _bits(rmse), (what, r.rmse.cpu().numpy(), rmse)
    if mask is not None:
        assert _bits(r.mask) == _bits(mask), what


def test_bit_equality_with_the_restatement(gpu):
    from corsair_amd import sc2 as S2

    d, _ = _graphs()
    src, tgt, m = _t(gpu, d["src"]), _t(gpu, d["tgt"]), _t(gpu, d["m"])
    for n_seeds, K in PARAMS:
        want = _want(n_seeds, K)
        assert want[1][CS.INVALID].tolist() == [0, -1, 0, 0, -1, 0]            # every seed of that problem is invalid
        for env in (SHAPES if (n_seeds, K) in ALL_SHAPES else SHAPES[:1]):
            with SC.environment(env):
                r = S2.sc2_batch(src, tgt, CS.OFF, CS.MAX_CORR, CS.TAU, m=m, n_seeds=n_seeds, k_consensus=K,
                                 return_inliers=True)
            _same(r, want, (n_seeds, K, env))
    found = _want(0, 20)[1][:, 0].tolist()
    assert found[:3] == [0, 0, 0] and all(found[3:CS.INVALID])                  # m = 0, 1, 2 are found by nothing
    # d_m = NULL: every list is full, the capacities are the problems
    off = np.concatenate([[0], np.cumsum(CS.SIZES)]).tolist()
    rows = np.concatenate([np.arange(CS.OFF[p], CS.OFF[p] + CS.SIZES[p]) for p in range(len(CS.SIZES))])
    T, stat, rmse, mask = _want(256, 20)
    r = S2.sc2_batch(_t(gpu, d["src"][rows]), _t(gpu, d["tgt"][rows]), off, CS.MAX_CORR, CS.TAU, n_seeds=256, k_consensus=20,
                     return_inliers=True)
    _same(r, (T, stat, rmse, mask[rows]), "d_m = NULL")
    assert S2.sc2_batch(src, tgt, CS.OFF, CS.MAX_CORR, CS.TAU, m=m).mask is None


def test_defined_cases_on_the_device(gpu):
    from corsair_amd import sc2 as S2

    for name, (s, q, kw) in CS.defined_cases().items():
        T, stat, rmse, inl = ref.sc2_one(s, q, **kw)
        r = S2.sc2_batch(_t(gpu, np.asarray(s, np.float32).reshape(-1, 3)), _t(gpu, np.asarray(q, np.float32).reshape(-1, 3)),
                         [0, len(s)], kw["max_corr"], kw["compat_dist"], None, kw["n_seeds"], kw["k_consensus"], True)
        _same(r, (np.asarray(T).reshape(1, 4, 4), np.asarray([stat], np.int32), np.asarray([rmse]), inl.astype(np.uint8)), name)


def test_the_same_bits_in_every_schedule(gpu):
    from corsair_amd import sc2 as S2

    d, graphs = _graphs()
    p = CS.SIZES.index(257)
    s, q = (_t(gpu, x) for x in CS.problem(d, p))
    Tp, sp, rp, inl = graphs[p].result(256, 20)
    want = (np.asarray(Tp).reshape(1, 4, 4), np.asarray([sp], np.int32), np.asarray([rp]), inl.astype(np.uint8))
    kw = dict(n_seeds=256, k_consensus=20, return_inliers=True)
    alone = S2.sc2_batch(s, q, [0, 257], CS.MAX_CORR, CS.TAU, **kw)
    _same(alone, want, "alone")
    twice = S2.sc2_batch(torch.cat([s, s]), torch.cat([q, q]), [0, 257, 514], CS.MAX_CORR, CS.TAU, **kw)
    _same(twice, tuple(np.concatenate([w, w]) for w in want), "twice in one call")
    st = torch.cuda.Stream(device=gpu)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other = S2.sc2_batch(s, q, [0, 257], CS.MAX_CORR, CS.TAU, **kw)
    st.synchronize()
    _same(other, want, "another stream")
    for k in range(2):
        _same(S2.sc2_batch(s, q, [0, 257], CS.MAX_CORR, CS.TAU, **kw), want, "run %d in a row" % k)
    # the slots behind the pairs are not part of the problem: the same problem inside a larger capacity
    pad = torch.rand((70, 3), device=gpu)
    held = S2.sc2_batch(torch.cat([s, pad]), torch.cat([q, pad + 0.5]), [0, 327], CS.MAX_CORR, CS.TAU,
                        m=torch.tensor([257], dtype=torch.int32, device=gpu), **kw)
    _same(held, want[:3] + (np.concatenate([want[3], np.zeros(70, np.uint8)]),), "inside a larger capacity")


# ---- the stream contract and stale memory, with the module in backend's place ------------------------------------------------
def _op_sc2(B, d):
    return tuple(B.sc2_batch(d["src"], d["tgt"], CS.S_OFF, CS.MAX_CORR, CS.TAU, m=d["m"], n_seeds=256, k_consensus=20,
                             return_inliers=True))


CASES = [SC.Case("sc2_batch", CS.stream_batch, _op_sc2)]


@pytest.fixture(scope="module")
def plain(gpu):
    from corsair_amd import sc2 as S2

    snaps, times = {}, {}
    for case in CASES:
        first, _ = SC.run_plain(S2, case, gpu)
        snaps[case.name], times[case.name] = SC.run_plain(S2, case, gpu)
        assert SC.first_difference(first, snaps[case.name]) is None, case.name
    delay = SC.Delay(gpu)
    delay_ms = max(SC.MIN_DELAY_MS, 3.0 * max(times.values()))
    assert delay.measure(delay_ms) >= 0.8 * delay_ms, "the delay is shorter than asked for"
    return {"B": S2, "snaps": snaps, "delay": delay, "delay_ms": delay_ms}


@pytest.mark.parametrize("kind", ["side", "default"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_late_inputs_give_the_plain_bits(gpu, plain, case, kind):
    st = SC.fresh_streams(gpu, plain["delay"])[0] if kind == "side" else torch.cuda.default_stream(gpu)
    snap, saw, early = SC.run_late(plain["B"], case, gpu, st, plain["delay"], plain["delay_ms"])
    print("stream case %s st=%s: control saw the %s, host returned %s the inputs were ready"
          % (case.name, kind, saw, "BEFORE" if early else "after"))
    assert saw == "decoy", "the positive control saw the %s data: the delay was too short, the run proves nothing" % saw
    diff = SC.first_difference(snap, plain["snaps"][case.name])
    assert diff is None, "%s with the %s stream as caller differs from the plain schedule: %s" % (case.name, kind, diff)


@pytest.mark.parametrize("schedule", ST.SCHEDULES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_stale_memory_schedules(gpu, plain, case, schedule, monkeypatch):
    snap, info = ST.run_schedule(plain["B"], case, gpu, schedule, monkeypatch)
    diff = SC.first_difference(snap, plain["snaps"][case.name])
    assert diff is None, "%s under %s differs from the plain schedule: %s (%r)" % (case.name, schedule, diff, info)
    if schedule.startswith("scratch"):
        assert info["blocks"] > 0 and info["bytes"] > 0          # the unit's scratch comes from the pool
    if schedule.startswith("outputs"):
        assert info["allocations"] >= 4                          # every output is allocated uninitialised through the module's torch


# ---- sym_pose_batch(registration="sc2") on real geometry -------------------------------------------------------------------
QUERY_ROWS = 400      # query voxels kept per pair (every n-th row): 5-NN lists of about 2 000 pairs keep the restatement quick
SC2_SEEDS = 256


@functools.lru_cache(maxsize=None)
def _real():
    from corsair_amd import registration as R
    from tests.test_gpu_fpfh import _real_pairs

    dev = torch.device("cuda:0")
    qx, off0, cx, off1, Ts, voxel = _real_pairs()
    q, c = _t(dev, qx), _t(dev, cx)
    Fq, _ = R.fpfh_features(q, off0, 5 * voxel, 100)
    Fc, _ = R.fpfh_features(c, off1, 5 * voxel, 100)
    rows = np.concatenate([np.arange(off0[p], off0[p + 1], -(-(off0[p + 1] - off0[p]) // QUERY_ROWS)) for p in range(3)])
    offs = np.concatenate([[0], np.cumsum([((rows >= off0[p]) & (rows < off0[p + 1])).sum() for p in range(3)])]).tolist()
    rows = torch.from_numpy(rows).to(dev)
    return q[rows].contiguous(), offs, c, off1, Fq[rows].contiguous(), Fc, Ts, voxel


def test_sym_pose_batch_with_sc2_equals_the_restatement(gpu):
    from corsair_amd import _lib, backend as B, registration as R
    from corsair_amd.utils.eval_pose import eval_pose

    q, off0, c, off1, Fq, Fc, Ts, voxel = _real()
    args = (Fq, q, off0, Fc, c, off1, [1, 1, 1], 5, 0.2, 0, None, 100, 100000, 0.999)
    kw = dict(registration="sc2", sc2_compat_dist=0.1, sc2_seeds=SC2_SEEDS, sc2_k=20)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        res = R.sym_pose_batch(*args, False, **kw)
        torch.cuda.synchronize()
        launches = _lib.prof_get("sc2")[1]
    finally:
        _lib.prof_enable(False)
    assert launches == 1                                                   # one scope per call
    # the 5-NN lists, rebuilt: the pairs of query row i stand in the slots 5 i .. 5 i + 4 of its problem
    nn = B.knn_feat(Fq, off0, Fc, off1, 5).cpu().numpy()
    qn, cn = q.cpu().numpy(), c.cpu().numpy()
    src = np.repeat(qn, 5, axis=0)
    tgt = np.concatenate([cn[off1[p] + nn[off0[p]:off0[p + 1]].reshape(-1)] for p in range(3)])
    offs = [5 * v for v in off0]
    T, st, rmse, _ = ref.sc2_batch(src, tgt, offs, 0.2, 0.1, n_seeds=SC2_SEEDS, k_consensus=20)
    assert _bits(res.T_ransac) == _bits(T.astype(np.float32)) and _bits(res.T_best) == _bits(T.astype(np.float32))
    assert res.inliers.cpu().numpy().tolist() == st[:, 2].tolist() and res.iters.cpu().numpy().tolist() == st[:, 3].tolist()
    assert res.n_problems == 3 and not res.ok.any() and st[:, 0].all()
    for p in range(3):
        rte, rre = eval_pose(res.T_best[p].cpu().numpy(), Ts[p], np.eye(4), 1)
        print("pair %d: sc2 RRE %.2f deg, RTE %.4f, %d inliers of %d, %d valid seeds, winner of rank %d and degree %d"
              % (p, np.rad2deg(rre), rte, st[p, 2], offs[p + 1] - offs[p], st[p, 3], st[p, 4], st[p, 5]))
    # the ICP options compose: a point-to-plane refinement behind it must not worsen the Chamfer distance
    icp = R.sym_pose_batch(*args, False, icp_max_iter=30, icp_max_dist=2 * voxel, icp_estimation="plane", **kw)
    assert _bits(icp.T_best) == _bits(res.T_best)
    assert (icp.cd_icp.cpu().numpy() <= icp.cd_best.cpu().numpy()).all()
    # use_symmetry=True works (16-wide descriptors, as the part cut takes them): the part configurations ride in the same
    # call, and the vanilla problems do not feel them
    F16 = (Fq[:, :16].contiguous(), q, off0, Fc[:, :16].contiguous(), c, off1, [1, 2, 1]) + args[7:]
    plain = R.sym_pose_batch(*F16, False, **kw)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        sym = R.sym_pose_batch(*F16, True, True, **kw)                     # force_gate: every pair gets its configurations
        torch.cuda.synchronize()
        assert _lib.prof_get("sc2")[1] == 1
    finally:
        _lib.prof_enable(False)
    assert sym.n_problems >= 3 and _bits(sym.T_ransac) == _bits(plain.T_ransac)
    assert torch.isfinite(sym.T_all).all() and len(sym.prob_pair) == sym.n_problems
    print("use_symmetry=True: %d problems in the one call" % sym.n_problems)
    # descriptors that are not finite are refused as they are today, with the same words
    bad = Fq.clone()
    bad[off0[1] + 5, 7] = float("nan")
    with pytest.raises(ValueError, match="query descriptors of pair 1"):
        R.sym_pose_batch(bad, *args[1:], False, **kw)


def test_sc2_compat_dist_none_is_half_of_max_corr_by_position_keyword_and_default(gpu):
    """sc2_compat_dist = None means max_corr / 2 of THIS call's max_corr, whether that arrives by position, by keyword or not at
    all: each call equals sc2.sc2_batch at that compat_dist on the rebuilt 5-NN lists, bit for bit."""
    import inspect

    from corsair_amd import backend as B, registration as R, sc2 as S2

    q, off0, c, off1, Fq, Fc, _, _ = _real()
    # two pairs of about a hundred query voxels (every 4th row of the builder's), the CAD sides whole
    rows = [torch.arange(off0[p], off0[p + 1], 4, device=gpu) for p in range(2)]
    offq = [0, len(rows[0]), len(rows[0]) + len(rows[1])]
    rows = torch.cat(rows)
    q, Fq, c, Fc, off1 = q[rows].contiguous(), Fq[rows].contiguous(), c[:off1[2]], Fc[:off1[2]], off1[:3]
    assert off1[0] == 0 and Fq.shape[1] == 33 and all(90 <= offq[p + 1] - offq[p] <= 110 for p in range(2))
    nn = B.knn_feat(Fq, offq, Fc, off1, 5).long()
    src = q.repeat_interleave(5, 0)
    tgt = torch.cat([c[off1[p] + nn[offq[p]:offq[p + 1]].reshape(-1)] for p in range(2)])
    offs = [5 * v for v in offq]
    assert any((offs[p + 1] - offs[p]) % 64 for p in range(2))

    def direct(max_corr, compat_dist):
        r = S2.sc2_batch(src, tgt, offs, max_corr, compat_dist, n_seeds=SC2_SEEDS, k_consensus=20)
        return _bits(r.T.to(torch.float32)), _bits(r.inliers), _bits(r.n_valid)

    def got(res):
        assert res.n_problems == 2
        return _bits(res.T_all), _bits(res.inliers), _bits(res.iters)

    head = (Fq, q, offq, Fc, c, off1, [1, 1], 5)
    kw = dict(registration="sc2", sc2_compat_dist=None, sc2_seeds=SC2_SEEDS, sc2_k=20)
    default = inspect.signature(R.sym_pose_batch).parameters["max_corr"].default
    other = 0.3
    assert other != default
    by_position = got(R.sym_pose_batch(*head, other, 0, None, 100, 100000, 0.999, False, **kw))
    by_keyword = got(R.sym_pose_batch(*head, max_corr=other, use_symmetry=False, **kw))
    by_default = got(R.sym_pose_batch(*head, use_symmetry=False, **kw))
    assert by_position == by_keyword
    assert by_position == direct(other, other / 2) and by_keyword == direct(other, other / 2)
    assert by_default == direct(default, default / 2)
    # the control: on these lists the threshold is felt, so a call that took half of ANOTHER max_corr would have been seen
    assert direct(other, default / 2) != direct(other, other / 2)


def test_defaults_launch_nothing_of_the_family(gpu):
    from corsair_amd import _lib, registration as R, shapenet_eval as SE
    from tests.test_gpu_real_clouds import _real_clouds

    q, off0, c, off1, Fq, Fc, Ts, voxel = _real()
    args = (Fq, q, off0, Fc, c, off1, [1, 1, 1], 5, 0.2, 0, None, 100, 2000, 0.999, False)
    clouds = [x[:3000] for x in _real_clouds()[:1]]
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        R.sym_pose_batch(*args)
        R.sym_pose_batch(*args, registration="ransac")
        R.sym_pose_batch(*args, registration="fgr")
        R.sym_pose_batch(*args, registration="ransac_fm", fm_iterations=256)
        SE.evaluate(None, clouds, SE.Config(features="fpfh", n_poses_per_model=1, ransac_max_iter=2000))
        torch.cuda.synchronize()
        assert _lib.prof_get("sc2")[1] == 0
        out = SE.evaluate(None, clouds, SE.Config(features="fpfh", n_poses_per_model=1, registration="sc2", sc2_seeds=SC2_SEEDS))
        torch.cuda.synchronize()
        assert _lib.prof_get("sc2")[1] == 1 and len(out) == 1             # the control: the option does launch it
        assert np.isfinite(out[0]["T_est_ransac"]).all() and out[0]["sym_success"] is False
    finally:
        _lib.prof_enable(False)
