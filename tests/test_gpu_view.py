"""cs_render_views on the device against tests/view_ref.py, bit for bit; the same bits in every schedule and
chunking; the stream contract and the stale-memory schedules through the helpers of tests/stream_cases.py and
tests/stale_cases.py with corsair_amd.views in backend's place; shapenet_eval.evaluate on partial views of bundled clouds;
and that the defaults launch nothing of the family."""
import functools

import numpy as np
import pytest
import torch

from tests import stale_cases as ST
from tests import stream_cases as SC
from tests import view_cases as VC
from tests import view_ref as ref

pytestmark = pytest.mark.gpu


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return (t.detach().contiguous().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).tobytes()


def _same(r, want, what):
    visible, depth, stat = want
    assert _bits(r.stat) == _bits(stat), (what, r.stat.cpu().numpy().tolist(), stat.tolist())
    assert _bits(r.visible) == _bits(visible), (what, int((r.visible.cpu().numpy() != visible).sum()))
    if r.depth is not None:
        assert _bits(r.depth) == _bits(depth), (what, int((r.depth.cpu().numpy() != depth).sum()))


@functools.lru_cache(maxsize=None)
def _want(seed, width, height):
    d = VC.batch(seed)
    return d, ref.render(d["xyz"], VC.OFF, d["cams"], width, height, VC.focal(width), VC.POINT_SIZE, VC.DEPTH_TOL)


def _render(V, x, off, cams, width, height, depth=True):
    return V.render_views(x, off, cams, width, height, VC.focal(width), VC.POINT_SIZE, VC.DEPTH_TOL, return_depth=depth)


@pytest.mark.parametrize("width,height", VC.IMAGES)
def test_bit_equality_with_the_restatement(gpu, width, height):
    from corsair_amd import views as V

    d, want = _want(1, width, height)
    x, cams = _t(gpu, d["xyz"]), _t(gpu, d["cams"])
    _same(_render(V, x, VC.OFF, cams, width, height), want, (width, height))
    assert want[2][0].tolist() == [0, 0, 0, 0] and np.isinf(want[1][0]).all()      # the empty segment
    if width >= 64:
        assert 0 < want[2][-1][2] < want[2][-1][1]                                 # some rows of the large shell are hidden
    mask_only = _render(V, x, VC.OFF, cams, width, height, depth=False)           # NULL d_depth: the same mask and stat
    assert mask_only.depth is None
    _same(mask_only, want, "no depth image")
    # the launch shapes the unit reads from the environment: one segment per chunk, a few, and no read before the atomic
    per_seg = 8 * width * height
    for env in ({"CS_VIEW_CHUNK_BYTES": "1"}, {"CS_VIEW_CHUNK_BYTES": str(3 * per_seg)}, {"CS_VIEW_PRECHECK": "0"},
                {"CS_VIEW_PRECHECK": "0", "CS_VIEW_CHUNK_BYTES": str(2 * per_seg + 5)}):
        with SC.environment(env):
            _same(_render(V, x, VC.OFF, cams, width, height), want, (width, height, env))


def test_defined_cases_on_the_device(gpu):
    from corsair_amd import views as V

    for name, (x, cam, width, height, focal, size, tol) in VC.defined_cases().items():
        vis, z, st = ref.render_one(x, cam, width, height, focal, size, tol)
        with np.errstate(over="ignore"):
            want = (vis, z.astype(np.float32)[None], np.asarray([st], np.int32))
        r = V.render_views(_t(gpu, x), [0, len(x)], _t(gpu, cam.reshape(1, 12)), width, height, focal, size, tol, True)
        _same(r, want, name)
    r = V.render_views(torch.zeros((0, 3), device=gpu), [0], torch.zeros((0, 12), dtype=torch.float64, device=gpu), 8, 8, 8.0,
                       0.1, 0.1, True)
    assert r.visible.shape == (0,) and r.stat.shape == (0, 4) and r.depth.shape == (0, 8, 8)     # n_seg = 0 is legal


def test_the_same_bits_in_every_schedule(gpu):
    from corsair_amd import views as V

    width = height = 64
    d, full = _want(1, width, height)
    a, b = VC.OFF[-2], VC.OFF[-1]
    x, cam = _t(gpu, d["xyz"][a:b]), _t(gpu, d["cams"][-1:])
    want = (full[0][a:b], full[1][-1:], full[2][-1:])
    n = b - a
    _same(_render(V, x, [0, n], cam, width, height), want, "alone")
    twice = _render(V, torch.cat([x, x]), [0, n, 2 * n], torch.cat([cam, cam]), width, height)
    _same(twice, tuple(np.concatenate([w, w]) for w in want), "twice in one call")
    st = torch.cuda.Stream(device=gpu)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other = _render(V, x, [0, n], cam, width, height)
    st.synchronize()
    _same(other, want, "another stream")
    for k in range(2):
        _same(_render(V, x, [0, n], cam, width, height), want, "run %d in a row" % k)
    perm = np.random.default_rng(4).permutation(n)
    permuted = _render(V, _t(gpu, d["xyz"][a:b][perm]), [0, n], cam, width, height)
    _same(permuted, (want[0][perm], want[1], want[2]), "a permuted segment")
    # rows in front of and behind the table are not part of the call: their mask bytes keep what they held
    held = _render(V, torch.cat([x[:7], x, x[:5]]), [7, 7 + n], cam, width, height)
    assert _bits(held.visible[7:7 + n]) == _bits(want[0]) and _bits(held.stat) == _bits(want[2])


# ---- the stream contract and stale memory, with the module in backend's place ------------------------------------------------
def _op_views(B, d):
    return tuple(B.render_views(d["xyz"], VC.OFF, d["cams"], 64, 64, VC.focal(64), VC.POINT_SIZE, VC.DEPTH_TOL, True))


CASES = [SC.Case("render_views", VC.batch, _op_views)]


@pytest.fixture(scope="module")
def plain(gpu):
    from corsair_amd import views as V

    snaps, times = {}, {}
    for case in CASES:
        first, _ = SC.run_plain(V, case, gpu)
        snaps[case.name], times[case.name] = SC.run_plain(V, case, gpu)
        assert SC.first_difference(first, snaps[case.name]) is None, case.name
    delay = SC.Delay(gpu)
    delay_ms = max(SC.MIN_DELAY_MS, 3.0 * max(times.values()))
    assert delay.measure(delay_ms) >= 0.8 * delay_ms, "the delay is shorter than asked for"
    return {"B": V, "snaps": snaps, "delay": delay, "delay_ms": delay_ms}


@pytest.mark.parametrize("kind", ["side", "default"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_late_inputs_give_the_plain_bits(gpu, plain, case, kind):
    """Both inputs arrive late: the rows and the cameras (d_cam is read by the kernels, not by the host)."""
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


# ---- shapenet_eval on partial views --------------------------------------------------------------------------------------
def test_evaluate_on_partial_views_and_the_defaults(gpu):
    from corsair_amd import _lib, shapenet_eval as SE
    from tests.test_gpu_real_clouds import _real_clouds

    clouds = [x[:3000] for x in _real_clouds()[:4]]
    base = dict(features="fpfh", n_poses_per_model=1, ransac_max_iter=2000)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        plain_out = SE.evaluate(None, clouds, SE.Config(**base))
        torch.cuda.synchronize()
        assert _lib.prof_get("view")[1] == 0                               # the default launches nothing of the family
        stat = {}
        out = SE.evaluate(None, clouds, SE.Config(partial_view=True, **base), stat=stat)
        torch.cuda.synchronize()
        assert _lib.prof_get("view")[1] == 1                               # the control: one call per batch
    finally:
        _lib.prof_enable(False)
    assert len(out) == len(plain_out) == 4 and all("visible_share" not in r for r in plain_out)
    shares = [r["visible_share"] for r in out]
    print("visible shares:", [round(s, 3) for s in shares], stat)
    assert all(0.0 < s < 1.0 for s in shares)
    pv = stat["partial_view"]
    assert pv["clouds"] == 4 and pv["rows_in"] == 4 * 3000 and pv["views_skipped"] == 0
    assert pv["rows_visible"] == sum(int(round(s * 3000)) for s in shares) and 0 < pv["rows_visible"] < pv["rows_in"]
    for r, p in zip(out, plain_out):
        assert np.isfinite(r["T_est_ransac"]).all() and np.isfinite(r["T_est_sym"]).all()
        assert _bits(r["pose_gt"]) == _bits(p["pose_gt"])                  # the poses do not see the option
