"""cs_ppf_batch on the device against tests/ppf_ref.py, bit for bit, every output and every candidate; the same
bits on both accumulator paths, in every chunking and in every schedule; the defined cases of the header; the stream
contract and the stale-memory schedules through the helpers of tests/stream_cases.py and tests/stale_cases.py with
corsair_amd.ppf in backend's place; sym_pose_batch with registration = "ppf" on the real CAD / scan pairs; and that the
defaults launch nothing of the family."""
import functools
import sys

import numpy as np
import pytest
import torch

from tests import ppf_cases as PC
from tests import ppf_ref as ref
from tests import stale_cases as ST
from tests import stream_cases as SC

pytestmark = pytest.mark.gpu

ONE_PROBLEM = 12 * 1500 * 1500 + 8 * 216001 + 256 * 120 * 1500      # the bytes of the largest problem (table and slabs)
# every launch shape the unit reads from the environment
SHAPES = ({}, {"CS_PPF_ACC": "global"}, {"CS_PPF_ACC": "lds"}, {"CS_PPF_CHUNK_BYTES": str(ONE_PROBLEM)},
          {"CS_PPF_CHUNK_BYTES": "1"})
# (ref_step, n_cand, problems, shapes): the whole batch at ref_step 7, the quick problems at 1, 2 and a step above every scene
CALLS = ((7, 7, None, SHAPES), (1, 64, PC.SMALL_PROBLEMS, SHAPES), (2, 1, PC.SMALL_PROBLEMS, SHAPES),
         (1000, 7, PC.SMALL_PROBLEMS, SHAPES))


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return (t.detach().contiguous().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).tobytes()


def _stat(r):
    return torch.stack([r.found, r.votes, r.scene_row, r.model_row, r.alpha_bin, r.count, r.rank, r.n_ref], 1)


def _same(r, want, what):
    T, Ti, stat, rmse, cT, cS = want
    assert _bits(_stat(r)) == _bits(stat), (what, _stat(r).cpu().numpy().tolist(), stat.tolist())
    assert _bits(r.cand_stat) == _bits(cS), (what, r.cand_stat.cpu().numpy().tolist(), cS.tolist())
    assert _bits(r.T) == _bits(T) and _bits(r.T_inv) == _bits(Ti), what
    assert _bits(r.cand_T) == _bits(cT), what
    assert _bits(r.rmse) == _bits(rmse), (what, r.rmse.cpu().numpy(), rmse)


@functools.lru_cache(maxsize=None)
def _batch():
    d, soff, moff, sseg, mseg, steps = PC.batch()
    probs = [ref.Problem(d["scene"][soff[s]:soff[s + 1]], d["scene_n"][soff[s]:soff[s + 1]], d["model"][moff[m]:moff[m + 1]],
                         d["model_n"][moff[m]:moff[m + 1]], steps[p]) for p, (s, m) in enumerate(zip(sseg, mseg))]
    return d, soff, moff, sseg, mseg, steps, probs


def test_bit_equality_with_the_restatement(gpu):
    from corsair_amd import ppf

    d, soff, moff, sseg, mseg, steps, probs = _batch()
    dev = {k: _t(gpu, v) for k, v in d.items()}
    for ref_step, n_cand, which, shapes in CALLS:
        which = list(range(len(sseg))) if which is None else list(which)
        want = ref.pack([probs[p].result(PC.MAX_DIST, ref_step, n_cand) for p in which], n_cand)
        for env in shapes:
            with SC.environment(env):
                r = ppf.ppf_batch(dev["scene"], dev["scene_n"], soff, dev["model"], dev["model_n"], moff, [sseg[p] for p in which],
                                  [mseg[p] for p in which], [steps[p] for p in which], PC.MAX_DIST, ref_step, n_cand)
            _same(r, want, (ref_step, n_cand, env))
    found = ref.pack([probs[p].result(PC.MAX_DIST, 7, 7) for p in range(len(sseg))], 7)[2][:, 0].tolist()
    print("found per problem:", found)
    assert found[:2] == [0, 0] and found[12:14] == [0, 0] and all(found[2:12]) and all(found[14:])    # empty and one-row
                                                                                                    # segments find nothing


def test_defined_cases_on_the_device(gpu):
    from corsair_amd import ppf

    for name, (s, sn, m, mn, kw) in PC.defined_cases().items():
        want = ref.pack([ref.ppf_one(s, sn, m, mn, **kw)], kw["n_cand"])
        for env in SHAPES[:2]:
            with SC.environment(env):
                r = ppf.ppf_batch(_t(gpu, s), _t(gpu, sn), [0, len(s)], _t(gpu, m), _t(gpu, mn), [0, len(m)], [0], [0],
                                  kw["dist_step"], kw["max_dist"], kw["ref_step"], kw["n_cand"])
            _same(r, want, (name, env))


def test_the_same_bits_in_every_schedule(gpu):
    from corsair_amd import ppf

    d, soff, moff, sseg, mseg, steps, probs = _batch()
    p = 8                                                # 65 scene rows against the 700-row model
    s, sn = (_t(gpu, d[k][soff[sseg[p]]:soff[sseg[p] + 1]]) for k in ("scene", "scene_n"))
    m, mn = (_t(gpu, d[k][moff[mseg[p]]:moff[mseg[p] + 1]]) for k in ("model", "model_n"))
    want = ref.pack([probs[p].result(PC.MAX_DIST, 7, 7)], 7)
    call = lambda: ppf.ppf_batch(s, sn, [0, len(s)], m, mn, [0, len(m)], [0], [0], steps[p], PC.MAX_DIST, 7, 7)
    _same(call(), want, "alone")
    twice = ppf.ppf_batch(torch.cat([s, s]), torch.cat([sn, sn]), [0, len(s), 2 * len(s)], m, mn, [0, len(m)], [0, 1], [0, 0],
                          steps[p], PC.MAX_DIST, 7, 7)
    _same(twice, tuple(np.concatenate([w, w]) for w in want), "twice in one call")
    st = torch.cuda.Stream(device=gpu)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other = call()
    st.synchronize()
    _same(other, want, "another stream")
    for k in range(2):
        _same(call(), want, "run %d in a row" % k)
    # rows outside the two segments are not part of the problem: the same problem inside larger arrays
    pad = torch.rand((70, 3), device=gpu)
    held = ppf.ppf_batch(torch.cat([pad, s, pad]), torch.cat([pad, sn, pad]), [0, 70, 70 + len(s), 140 + len(s)],
                         torch.cat([pad, m, pad]), torch.cat([pad, mn, pad]), [0, 70, 70 + len(m)], [1], [1], steps[p],
                         PC.MAX_DIST, 7, 7)
    _same(held, want, "inside larger arrays")


# ---- the stream contract and stale memory, with the module in backend's place ------------------------------------------------
def _op_ppf(B, d):
    return tuple(B.ppf_batch(d["scene"], d["scene_n"], PC.S_SOFF, d["model"], d["model_n"], PC.S_MOFF,
                             list(range(len(PC.S_SCENES))), [k for _, k in PC.S_SCENES], PC.S_STEP, PC.MAX_DIST, 3, 8))


CASES = [SC.Case("ppf_batch", PC.stream_batch, _op_ppf), SC.Case("ppf_batch_slabs", PC.stream_batch, _op_ppf, {"CS_PPF_ACC": "global"})]


@pytest.fixture(scope="module")
def plain(gpu):
    from corsair_amd import ppf

    snaps, times = {}, {}
    for case in CASES:
        first, _ = SC.run_plain(ppf, case, gpu)
        snaps[case.name], times[case.name] = SC.run_plain(ppf, case, gpu)
        assert SC.first_difference(first, snaps[case.name]) is None, case.name
    assert SC.first_difference(snaps["ppf_batch"], snaps["ppf_batch_slabs"]) is None
    delay = SC.Delay(gpu)
    delay_ms = max(SC.MIN_DELAY_MS, 3.0 * max(times.values()))
    assert delay.measure(delay_ms) >= 0.8 * delay_ms, "the delay is shorter than asked for"
    return {"B": ppf, "snaps": snaps, "delay": delay, "delay_ms": delay_ms}


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
        assert info["allocations"] >= 6                          # every output is allocated uninitialised through the module's torch


# ---- sym_pose_batch(registration="ppf") on real geometry -------------------------------------------------------------------
PAIR_ROWS = 450       # the bundled pairs (voxel 0.03) are voxelised once more, each at the first voxel of PAIR_VOXELS that leaves
PAIR_VOXELS = (0.07, 0.1, 0.14, 0.2, 0.3)      # both clouds at most PAIR_ROWS rows: the restatement's m^2 table stays quick
                                               # (the first pair is a volumetric cloud: 3 314 rows at 0.07)


@functools.lru_cache(maxsize=None)
def _real():
    from corsair_amd import backend as B
    from tests.test_gpu_fpfh import _real_pairs

    dev = torch.device("cuda:0")
    qx, off0, cx, off1, Ts, _ = _real_pairs()
    qs, cs = [], []
    for p in range(3):
        for voxel in PAIR_VOXELS:
            pair = []
            for x, off in ((qx, off0), (cx, off1)):
                seg = _t(dev, x[off[p]:off[p + 1]])
                keep, _, _ = B.voxelize(seg, [0, len(seg)], voxel)
                pair.append(seg[keep].contiguous())
            if max(len(pair[0]), len(pair[1])) <= PAIR_ROWS:
                break
        assert max(len(pair[0]), len(pair[1])) <= PAIR_ROWS, (p, len(pair[0]), len(pair[1]))
        qs.append(pair[0]), cs.append(pair[1])
    o0 = np.concatenate([[0], np.cumsum([len(x) for x in qs])]).tolist()
    o1 = np.concatenate([[0], np.cumsum([len(x) for x in cs])]).tolist()
    q, c = torch.cat(qs).contiguous(), torch.cat(cs).contiguous()
    nq = B.orient_normals(q, o0, B.estimate_normals(q, o0, 16))
    nc = B.orient_normals(c, o1, B.estimate_normals(c, o1, 16))
    return q, o0, nq, c, o1, nc, Ts, 0.1


def test_sym_pose_batch_with_ppf_equals_the_restatement(gpu):
    from corsair_amd import _lib, ppf, registration as R
    from corsair_amd.utils.eval_pose import eval_pose

    q, off0, nq, c, off1, nc, Ts, voxel = _real()
    max_corr = 2 * voxel
    args = (None, q, off0, None, c, off1, [1, 1, 1], 5, max_corr, 0, None, 100, 100000, 0.999)
    kw = dict(registration="ppf", ppf_ref_step=5, ppf_n_cand=8, normals0=nq, normals1=nc)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        res = R.sym_pose_batch(*args, False, **kw)
        torch.cuda.synchronize()
        launches = _lib.prof_get("ppf")[1]
    finally:
        _lib.prof_enable(False)
    assert launches == 1                                                   # one scope per call
    qn, cn, nqn, ncn = (t.cpu().numpy() for t in (q, c, nq, nc))
    steps = ppf.default_dist_step(c, off1)
    T, Ti, st, rmse, _, _ = ref.ppf_batch(qn, nqn, off0, cn, ncn, off1, [0, 1, 2], [0, 1, 2], steps, max_corr, 5, 8)
    assert _bits(res.T_ransac) == _bits(T.astype(np.float32)) and _bits(res.T_best) == _bits(T.astype(np.float32))
    assert res.inliers.cpu().numpy().tolist() == st[:, 5].tolist() and res.iters.cpu().numpy().tolist() == st[:, 1].tolist()
    assert res.n_problems == 3 and not res.ok.any() and st[:, 0].all()
    for p in range(3):
        rte, rre = eval_pose(res.T_best[p].cpu().numpy(), Ts[p], np.eye(4), 1)
        print("pair %d: ppf RRE %.2f deg, RTE %.4f, %d votes, count %d of %d, winner of rank %d"
              % (p, np.rad2deg(rre), rte, st[p, 1], st[p, 5], off0[p + 1] - off0[p], st[p, 6]))
    sys.stdout.flush()
    # the scene on side 1: the CAD rows vote against the query as the model, and T_ransac is the inverse the library forms
    steps1 = ppf.default_dist_step(q, off0)
    _, Ti1, st1, _, _, _ = ref.ppf_batch(cn, ncn, off1, qn, nqn, off0, [0, 1, 2], [0, 1, 2], steps1, max_corr, 5, 8)
    res1 = R.sym_pose_batch(*args, False, ppf_scene_side=1, **kw)
    assert _bits(res1.T_ransac) == _bits(Ti1.astype(np.float32)) and res1.inliers.cpu().numpy().tolist() == st1[:, 5].tolist()
    # normals that are not given are estimated and oriented away from the centroids: the same bits as the ones made above
    own = R.sym_pose_batch(*args, False, registration="ppf", ppf_ref_step=5, ppf_n_cand=8)
    assert _bits(own.T_ransac) == _bits(res.T_ransac)
    # the ICP options compose: a point-to-plane refinement behind it must not worsen the Chamfer distance
    icp = R.sym_pose_batch(*args, False, icp_max_iter=30, icp_max_dist=2 * voxel, icp_estimation="plane", **kw)
    assert _bits(icp.T_best) == _bits(res.T_best)
    assert (icp.cd_icp.cpu().numpy() <= icp.cd_best.cpu().numpy()).all()
    with pytest.raises(ValueError, match="use_symmetry=False"):
        R.sym_pose_batch(*args, True, **kw)
    with pytest.raises(ValueError, match="normals0 is used by"):          # the refusal stays for the other estimators
        R.sym_pose_batch(torch.zeros((q.shape[0], 33), device=gpu), *args[1:3], torch.zeros((c.shape[0], 33), device=gpu),
                         *args[4:], False, normals0=nq)


def test_defaults_launch_nothing_of_the_family(gpu):
    from corsair_amd import _lib, registration as R, shapenet_eval as SE
    from tests.test_gpu_real_clouds import _real_clouds
    from tests.test_gpu_sc2 import _real as _described

    q, off0, c, off1, Fq, Fc, Ts, voxel = _described()
    args = (Fq, q, off0, Fc, c, off1, [1, 1, 1], 5, 0.2, 0, None, 100, 2000, 0.999, False)
    clouds = [x[:3000] for x in _real_clouds()[:1]]
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        R.sym_pose_batch(*args)
        R.sym_pose_batch(*args, registration="ransac")
        R.sym_pose_batch(*args, registration="fgr")
        R.sym_pose_batch(*args, registration="ransac_fm", fm_iterations=256)
        R.sym_pose_batch(*args, registration="sc2", sc2_seeds=64)
        SE.evaluate(None, clouds, SE.Config(features="fpfh", n_poses_per_model=1, ransac_max_iter=2000))
        torch.cuda.synchronize()
        assert _lib.prof_get("ppf")[1] == 0
        out = SE.evaluate(None, clouds, SE.Config(n_poses_per_model=1, registration="ppf"))
        torch.cuda.synchronize()
        assert _lib.prof_get("ppf")[1] == 1 and len(out) == 1             # the control: the option does launch it, no checkpoint
        assert np.isfinite(out[0]["T_est_ransac"]).all() and out[0]["sym_success"] is False
        print("shapenet_eval ppf, whole copy: RRE %.2f deg, RTE %.4f" % (np.rad2deg(out[0]["rre_ransac"]), out[0]["rte_ransac"]))
        stat = {}
        out = SE.evaluate(None, clouds, SE.Config(n_poses_per_model=1, registration="ppf", partial_view=True, icp_max_iter=30),
                          stat=stat)
        torch.cuda.synchronize()
        assert _lib.prof_get("ppf")[1] == 2 and 0.0 < out[0]["visible_share"] < 1.0 and np.isfinite(out[0]["T_est_icp"]).all()
        print("shapenet_eval ppf, one view (%.0f %% visible): RRE %.2f deg, after 30 ICP updates %.2f deg"
              % (100 * out[0]["visible_share"], np.rad2deg(out[0]["rre_ransac"]), np.rad2deg(out[0]["rre_icp"])))
    finally:
        _lib.prof_enable(False)
