"""cs_corr_mutual and cs_ransac_fm_batch on the device against tests/featmatch_ref.py, bit for bit; the same bits
in every schedule; the stream contract and the stale-memory schedules of both entry points through the helpers of
tests/stream_cases.py and tests/stale_cases.py with corsair_amd.featmatch in backend's place; sym_pose_batch with
registration = "ransac_fm" on the real CAD / partial-view pairs; and that the defaults launch nothing of the family."""
import functools

import numpy as np
import pytest
import torch

from tests import featmatch_cases as FC
from tests import featmatch_ref as ref
from tests import stale_cases as ST
from tests import stream_cases as SC

pytestmark = pytest.mark.gpu

ITERATIONS = (1, 255, 256, 257, 1024)
# every launch shape the unit reads from the environment: the pairs per slice of the count kernel and the hypotheses per chunk
SHAPES = ({}, {"CS_FM_SLICE": "1"}, {"CS_FM_SLICE": "256"}, {"CS_FM_SLICE": "300"}, {"CS_FM_CHUNK": "256"},
          {"CS_FM_CHUNK": "512", "CS_FM_SLICE": "64"})


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return (t.detach().contiguous().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).tobytes()


@functools.lru_cache(maxsize=None)
def _tables(seed, n):
    d = FC.batch(seed)
    return d, [ref.Table(*FC.problem(d, p), FC.MAX_CORR, n, 0.9, True, max(ITERATIONS), seed) for p in range(len(FC.SIZES))]


def _want(tabs, iterations):
    T, stat, rmse = [], [], []
    for tab in tabs:
        Tp, sp, rp, _ = tab.result(iterations)
        T.append(Tp)
        stat.append(sp)
        rmse.append(rp)
    return (np.asarray(T, np.float64).reshape(-1, 4, 4), np.asarray(stat, np.int32), np.asarray(rmse, np.float64))


def _same(r, want, what):
    T, stat, rmse = want
    got_stat = torch.stack([r.found, r.t_best, r.inliers, r.n_valid], 1)
    assert _bits(got_stat) == _bits(stat), (what, got_stat.cpu().numpy().tolist(), stat.tolist())
    assert _bits(r.T) == _bits(T), what
    assert _bits(r.rmse) == _bits(rmse), (what, r.rmse.cpu().numpy(), rmse)


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("seed", [1, 2])
def test_bit_equality_with_the_restatement(gpu, seed, n):
    from corsair_amd import featmatch as FM

    d, tabs = _tables(seed, n)
    src, tgt, m = _t(gpu, d["src"]), _t(gpu, d["tgt"]), _t(gpu, d["m"])
    for iterations in ITERATIONS:
        want = _want(tabs, iterations)
        assert want[1][FC.REJECTED].tolist() == [0, -1, 0, 0]              # every hypothesis of that problem is rejected
        for env in SHAPES:
            with SC.environment(env):
                r = FM.ransac_fm_batch(src, tgt, FC.OFF, FC.MAX_CORR, m=m, ransac_n=n, iterations=iterations, seed=seed)
            _same(r, want, (seed, n, iterations, env))
    found = _want(tabs, max(ITERATIONS))[1][:, 0].tolist()
    assert found[:3] == [0, 0, 0] and all(found[4:FC.REJECTED])            # m = 0, 1, 2 are found by nothing


def test_defined_cases_on_the_device(gpu):
    from corsair_amd import featmatch as FM

    for name, (s, q, kw) in FC.defined_cases().items():
        T, stat, rmse, _ = ref.ransac_fm_one(s, q, **kw)
        r = FM.ransac_fm_batch(_t(gpu, np.asarray(s, np.float32).reshape(-1, 3)), _t(gpu, np.asarray(q, np.float32).reshape(-1, 3)),
                               [0, len(s)], kw["max_corr"], None, kw["ransac_n"], kw["edge_similarity"], kw["check_distance"],
                               kw["iterations"], kw["seed"])
        _same(r, (np.asarray(T).reshape(1, 4, 4), np.asarray([stat], np.int32), np.asarray([rmse])), name)


def test_the_same_bits_in_every_schedule(gpu):
    from corsair_amd import featmatch as FM

    d, tabs = _tables(1, 3)
    p = FC.SIZES.index(513)
    s, q = (_t(gpu, x) for x in FC.problem(d, p))
    want = _want([tabs[p]], 1024)
    kw = dict(iterations=1024, seed=1)
    alone = FM.ransac_fm_batch(s, q, [0, 513], FC.MAX_CORR, **kw)
    _same(alone, want, "alone")
    twice = FM.ransac_fm_batch(torch.cat([s, s]), torch.cat([q, q]), [0, 513, 1026], FC.MAX_CORR, **kw)
    _same(twice, tuple(np.concatenate([w, w]) for w in want), "twice in one call")
    st = torch.cuda.Stream(device=gpu)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other = FM.ransac_fm_batch(s, q, [0, 513], FC.MAX_CORR, **kw)
    st.synchronize()
    _same(other, want, "another stream")
    for k in range(2):
        _same(FM.ransac_fm_batch(s, q, [0, 513], FC.MAX_CORR, **kw), want, "run %d in a row" % k)
    # the slots behind the pairs are not part of the problem: the same problem inside a larger capacity
    pad = torch.full((40, 3), 9.0, device=gpu)
    held = FM.ransac_fm_batch(torch.cat([s, pad]), torch.cat([q, -pad]), [0, 553], FC.MAX_CORR,
                              m=torch.tensor([513], dtype=torch.int32, device=gpu), **kw)
    _same(held, want, "inside a larger capacity")


@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("n", [3, 4])
def test_mutual_filter(gpu, n, mutual):
    from corsair_amd import featmatch as FM

    d = FC.mutual_lists(3)
    want = ref.mutual(d["fwd"], d["bwd"] if mutual else None, d["x0"], FC.M_OFF0, d["x1"], FC.M_OFF1, n, mutual)
    got = FM.mutual_correspondences(_t(gpu, d["fwd"]), _t(gpu, d["bwd"]) if mutual else None, _t(gpu, d["x0"]), FC.M_OFF0,
                                    _t(gpu, d["x1"]), FC.M_OFF1, n, mutual)
    for g, w, what in zip(got, want, ("src", "tgt", "m", "stat")):
        assert _bits(g) == _bits(w), (what, n, mutual)
    if mutual:                                                             # both sides of the fallback threshold were met
        assert want[3][:, 1].tolist() == ([0, 1, 1, 1, 0, 0] if n == 3 else [0, 1, 1, 1, 1, 0])
    # the compacted lists go straight into the RANSAC: counts on the device, capacities on the host
    r = FM.ransac_fm_batch(got.src, got.tgt, FC.M_OFF0, 0.3, m=got.m, ransac_n=n, iterations=256, seed=4)
    _same(r, ref.ransac_fm_batch(want[0], want[1], FC.M_OFF0, 0.3, m=want[2], ransac_n=n, iterations=256, seed=4),
          ("from the filter", n, mutual))


# ---- the stream contract and stale memory, with the module in backend's place ------------------------------------------------
def _op_fm(B, d):
    return tuple(B.ransac_fm_batch(d["src"], d["tgt"], FC.OFF, FC.MAX_CORR, m=d["m"], iterations=1024, seed=7))


def _op_mutual(B, d):
    return tuple(B.mutual_correspondences(d["fwd"], d["bwd"], d["x0"], FC.M_OFF0, d["x1"], FC.M_OFF1, 3, True))


CASES = [SC.Case("ransac_fm_batch", FC.batch, _op_fm), SC.Case("mutual_correspondences", FC.mutual_lists, _op_mutual)]


@pytest.fixture(scope="module")
def plain(gpu):
    from corsair_amd import featmatch as FM

    snaps, times = {}, {}
    for case in CASES:
        first, _ = SC.run_plain(FM, case, gpu)
        snaps[case.name], times[case.name] = SC.run_plain(FM, case, gpu)
        assert SC.first_difference(first, snaps[case.name]) is None, case.name
    delay = SC.Delay(gpu)
    delay_ms = max(SC.MIN_DELAY_MS, 3.0 * max(times.values()))
    assert delay.measure(delay_ms) >= 0.8 * delay_ms, "the delay is shorter than asked for"
    return {"B": FM, "snaps": snaps, "delay": delay, "delay_ms": delay_ms}


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
        assert info["allocations"] >= 3                          # every output is allocated uninitialised through the module's torch


# ---- sym_pose_batch(registration="ransac_fm") on real geometry -----------------------------------------------------------
FM_ITERS = 2048


@functools.lru_cache(maxsize=None)
def _real():
    from corsair_amd import registration as R
    from tests.test_gpu_fpfh import _real_pairs

    dev = torch.device("cuda:0")
    qx, off0, cx, off1, Ts, voxel = _real_pairs()
    q, c = _t(dev, qx), _t(dev, cx)
    Fq, _ = R.fpfh_features(q, off0, 5 * voxel, 100)
    Fc, _ = R.fpfh_features(c, off1, 5 * voxel, 100)
    return q, off0, c, off1, Fq, Fc, Ts, voxel


def test_sym_pose_batch_with_ransac_fm_equals_the_restatement(gpu):
    from corsair_amd import _lib, backend as B, registration as R
    from corsair_amd.utils.eval_pose import eval_pose

    q, off0, c, off1, Fq, Fc, Ts, voxel = _real()
    args = (Fq, q, off0, Fc, c, off1, [1, 1, 1], 5, 0.2, 0, None, 100, 100000, 0.999)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        res = R.sym_pose_batch(*args, False, registration="ransac_fm", fm_iterations=FM_ITERS)
        torch.cuda.synchronize()
        launches = _lib.prof_get("featmatch")[1]
    finally:
        _lib.prof_enable(False)
    assert launches == 2                                                   # one scope per call: the filter and the RANSAC
    fwd, bwd = B.knn_feat(Fq, off0, Fc, off1, 1), B.knn_feat(Fc, off1, Fq, off0, 1)
    src, tgt, m, stat = ref.mutual(fwd.cpu().numpy(), bwd.cpu().numpy(), q.cpu().numpy(), off0, c.cpu().numpy(), off1, 3, True)
    print("mutual matches per pair:", stat[:, 0].tolist(), "of", np.diff(off0).tolist(), "query rows")
    T, st, rmse = ref.ransac_fm_batch(src, tgt, off0, 0.2, m=m, iterations=FM_ITERS, seed=0)
    assert _bits(res.T_ransac) == _bits(T.astype(np.float32)) and _bits(res.T_best) == _bits(T.astype(np.float32))
    assert res.inliers.cpu().numpy().tolist() == st[:, 2].tolist() and res.iters.cpu().numpy().tolist() == st[:, 3].tolist()
    assert res.n_problems == 3 and not res.ok.any() and st[:, 0].all()
    for p in range(3):
        rte, rre = eval_pose(res.T_best[p].cpu().numpy(), Ts[p], np.eye(4), 1)
        print("pair %d: ransac_fm RRE %.2f deg, RTE %.4f, %d inliers of %d, %d valid hypotheses of %d"
              % (p, np.rad2deg(rre), rte, st[p, 2], m[p], st[p, 3], FM_ITERS))
    # the ICP options compose: a point-to-plane refinement behind it must not worsen the Chamfer distance
    icp = R.sym_pose_batch(*args, False, registration="ransac_fm", fm_iterations=FM_ITERS, icp_max_iter=30,
                           icp_max_dist=2 * voxel, icp_estimation="plane")
    assert _bits(icp.T_best) == _bits(res.T_best)
    assert (icp.cd_icp.cpu().numpy() <= icp.cd_best.cpu().numpy()).all()
    with pytest.raises(ValueError, match="use_symmetry"):
        R.sym_pose_batch(*args, True, registration="ransac_fm")
    # descriptors that are not finite are refused as they are today, with the same words
    bad = Fq.clone()
    bad[off0[1] + 5, 7] = float("nan")
    with pytest.raises(ValueError, match="query descriptors of pair 1"):
        R.sym_pose_batch(bad, *args[1:], False, registration="ransac_fm", fm_iterations=256)


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
        SE.evaluate(None, clouds, SE.Config(features="fpfh", n_poses_per_model=1, ransac_max_iter=2000))
        torch.cuda.synchronize()
        assert _lib.prof_get("featmatch")[1] == 0
        out = SE.evaluate(None, clouds, SE.Config(features="fpfh", n_poses_per_model=1, registration="ransac_fm",
                                                  fm_iterations=FM_ITERS))
        torch.cuda.synchronize()
        assert _lib.prof_get("featmatch")[1] == 2 and len(out) == 1       # the control: the option does launch it
        assert np.isfinite(out[0]["T_est_ransac"]).all() and out[0]["sym_success"] is False
    finally:
        _lib.prof_enable(False)
