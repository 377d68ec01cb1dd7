"""cs_icp_scale_batch on the GPU: transforms, scales, fitness, rmse, updates, pair counts and correspondences are BIT-EQUAL to
tests/icp_scale_ref.py for both estimations and on both association paths, the stop rules of the scale leave T and the
scale of before the refused update, and the three rigid entries -- run in the same process -- return what they returned.

`python -m tests.test_gpu_icp_scale OUT.npz` runs the mixed batch of both estimations in a process of its own (the switch
test)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import icp_scale_ref as ref
from tests import test_gpu_icp as pt
from tests.test_gpu_icp_plane import _np_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MAX_DIST = 0.1
_same = pt._same

SIZES_S = (1, 255, 256, 257, 600)           # one association workgroup holds 256 sources
SIZES_T = (1, 511, 512, 513, 3000)          # one LDS stage of the exact kernel holds 512 rows
SCALES = (1.0, 0.9, 0.95, 1.08, 1.15)       # true scale of every source segment
# (source segment, target segment): every size once, then shared target segments
PROBLEMS = ((0, 4), (1, 3), (2, 2), (3, 1), (4, 0), (4, 4), (3, 4), (1, 2), (2, 4))
BOUNDS = (0.5, 2.0)


@functools.lru_cache(maxsize=None)
def _mixed():
    """One synthetic shape: every target segment is a subset of its points, every source segment a jittered subset in
    another pose and shrunk by its true scale; a problem starts at the true rigid pose perturbed by a few degrees."""
    from corsair_amd import synth

    rng = np.random.default_rng(2027)
    cloud = synth.make_cloud(7, 8000)
    Tgt = synth.random_pose(3, max_trans=0.3)
    Tinv = np.linalg.inv(Tgt)
    soff = np.concatenate([[0], np.cumsum(SIZES_S)]).tolist()
    toff = np.concatenate([[0], np.cumsum(SIZES_T)]).tolist()
    tgt = np.concatenate([cloud[rng.choice(len(cloud), n, replace=False)] for n in SIZES_T]).astype(np.float32)
    src = np.concatenate([synth.apply_pose(cloud[rng.choice(len(cloud), n, replace=False)] +
                                           rng.normal(0, 0.003, (n, 3)).astype(np.float32), Tinv) / s
                          for n, s in zip(SIZES_S, SCALES)])
    T0 = np.stack([pt._perturbed(Tgt, 3.0, 0.01, rng) for _ in PROBLEMS])
    nrm = np.concatenate([_np_normals(tgt[toff[t]:toff[t + 1]]) for t in range(len(SIZES_T))])
    return {"src": src.astype(np.float32), "soff": soff, "tgt": tgt, "nrm": nrm, "toff": toff, "T0": T0,
            "sseg": [p[0] for p in PROBLEMS], "tseg": [p[1] for p in PROBLEMS]}


@functools.lru_cache(maxsize=None)
def _mixed_ref(plane, max_iter=2):
    c = _mixed()
    return ref.icp_batch(c["src"], c["soff"], c["tgt"], c["nrm"] if plane else None, c["toff"], c["sseg"], c["tseg"], c["T0"],
                         MAX_DIST, max_iter, scale_bounds=BOUNDS)


def _run(dev, src, soff, tgt, nrm, toff, sseg, tseg, T0, max_dist, max_iter, bounds=BOUNDS, **kw):
    from corsair_amd import backend as B

    to = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shape)).to(dev)
    kw.setdefault("with_scaling", True)
    r = B.icp_batch(to(src, (-1, 3)), soff, to(tgt, (-1, 3)), toff, sseg, tseg, to(T0, (-1, 4, 4)), max_dist, max_iter,
                    return_corr=True, tgt_normals=None if nrm is None else to(nrm, (-1, 3)), scale_bounds=bounds, **kw)
    out = {"T": r.T.cpu().numpy().reshape(-1, 16), "T32": r.T32.cpu().numpy().reshape(-1, 16),
           "fitness": r.fitness.cpu().numpy(), "rmse": r.rmse.cpu().numpy(), "iters": r.iters.cpu().numpy(),
           "ncorr": r.ncorr.cpu().numpy(), "corr": r.corr.cpu().numpy(), "corr_off": np.asarray(r.corr_off, np.int64)}
    if r.scale is not None:
        out["scale"] = r.scale.cpu().numpy()
    if r.wfitness is not None:
        out["wfitness"] = r.wfitness.cpu().numpy()
    return out


def _run_mixed(dev, plane, max_iter=2, **kw):
    c = _mixed()
    return _run(dev, c["src"], c["soff"], c["tgt"], c["nrm"] if plane else None, c["toff"], c["sseg"], c["tseg"], c["T0"],
                MAX_DIST, max_iter, **kw)


def _one(dev, src, tgt, nrm, T0, max_dist, max_iter, bounds=BOUNDS):
    return _run(dev, src, [0, len(src)], tgt, nrm, [0, len(tgt)], [0], [0], np.asarray(T0, np.float32).reshape(1, 4, 4),
                max_dist, max_iter, bounds)


def _check(got, want, what=""):
    pt._check(got, want, what)
    for p, w in enumerate(want):
        assert _same(got["scale"][p], np.float64(w["scale"])), (what, p, got["scale"][p], w["scale"])


def _problem(p):
    c = _mixed()
    s, t = PROBLEMS[p]
    return (c["src"][c["soff"][s]:c["soff"][s + 1]], c["tgt"][c["toff"][t]:c["toff"][t + 1]],
            c["nrm"][c["toff"][t]:c["toff"][t + 1]], c["T0"][p])


def test_mixed_batch_matches_reference_and_the_rigid_entries_are_unchanged(gpu):
    # the three rigid entries first, before this process has made a scaled call
    rigid = {"point": _run_mixed(gpu, False, with_scaling=False), "plane": _run_mixed(gpu, True, with_scaling=False),
             "huber": _run_mixed(gpu, True, with_scaling=False, kernel="huber", kernel_scale=0.02)}
    got = {}
    for plane in (False, True):
        want = _mixed_ref(plane)
        got[plane] = _run_mixed(gpu, plane)
        _check(got[plane], want, "mixed plane" if plane else "mixed point")
        assert max(w["iters"] for w in want) == 2 and any(w["ncorr"] < 3 for w in want)   # both kinds are in the batch
        assert any(w["scale"] > 1.02 for w in want) and any(w["scale"] < 0.98 for w in want)
        again = _run_mixed(gpu, plane)
        assert all(_same(got[plane][k], again[k]) for k in again)                         # two runs: identical bits
    assert any(not _same(got[False]["T"][p], got[True]["T"][p]) for p in range(len(PROBLEMS)))   # two estimations
    after = {"point": _run_mixed(gpu, False, with_scaling=False), "plane": _run_mixed(gpu, True, with_scaling=False),
             "huber": _run_mixed(gpu, True, with_scaling=False, kernel="huber", kernel_scale=0.02)}
    for name in rigid:
        assert "scale" not in rigid[name] and rigid[name].keys() == after[name].keys()
        for k in rigid[name]:
            assert _same(rigid[name][k], after[name][k]), (name, k)
    # ... and they are the rigid restatements: scaling off through this file's loop is icp_ref / icp_plane_ref bit for bit
    # (tests/test_icp_scale_cpu.py), so one reference serves
    c = _mixed()
    for name, nrm in (("point", None), ("plane", c["nrm"])):
        want = ref.icp_batch(c["src"], c["soff"], c["tgt"], nrm, c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST, 2,
                             with_scaling=False)
        pt._check(rigid[name], want, "rigid " + name)


@pytest.mark.parametrize("plane", (False, True))
def test_max_iter_0_1_30_alone_permuted_and_duplicated(gpu, plane):
    src, tgt, nrm, T0 = _problem(5)                 # 600 sources (true scale 1.15) against 3 000 targets
    if not plane:
        nrm = None
    for max_iter in (0, 1, 30):
        want = ref.icp(src, tgt, nrm, T0, MAX_DIST, max_iter, scale_bounds=BOUNDS)
        got = _one(gpu, src, tgt, nrm, T0, MAX_DIST, max_iter)
        _check(got, [want], "max_iter %d" % max_iter)
        assert want["iters"] <= max_iter
    assert 1 < want["iters"] < 30 and abs(want["scale"] - 1.15) < 0.03      # stopped on the convergence rule, near the truth
    # alone = in the batch; a permutation of the source rows changes nothing but the order of the correspondences
    alone = _one(gpu, src, tgt, nrm, T0, MAX_DIST, 2)
    _check(alone, [_mixed_ref(plane)[5]], "alone")
    perm = np.random.default_rng(5).permutation(len(src))
    shuf = _one(gpu, src[perm], tgt, nrm, T0, MAX_DIST, 2)
    for k in ("T", "T32", "scale", "fitness", "rmse", "iters", "ncorr"):
        assert _same(shuf[k], alone[k]), k
    assert np.array_equal(shuf["corr"], alone["corr"][perm])
    # duplicated rows: sources count twice, duplicated targets tie and the smaller row wins
    s2 = np.concatenate([src[:200], src[:57]])
    t2 = np.concatenate([tgt[:700], tgt[:700]])
    n2 = None if nrm is None else np.concatenate([nrm[:700], nrm[:700]])
    want = ref.icp(s2, t2, n2, T0, MAX_DIST, 3, scale_bounds=BOUNDS)
    got = _one(gpu, s2, t2, n2, T0, MAX_DIST, 3)
    _check(got, [want], "duplicates")
    assert got["corr"].max() < 700 and got["iters"][0] >= 1


@pytest.mark.parametrize("plane", (False, True))
def test_out_of_f16_range_takes_the_exact_kernel(gpu, monkeypatch, plane):
    from corsair_amd import backend as B

    src, tgt, nrm, T0 = _problem(3)                 # 257 sources (true scale 1.08) against 511 targets
    tgt = tgt + np.float32([70.0, 0.0, 0.0])        # a coordinate of 70
    T0 = T0.copy()
    T0[0, 3] += 70.0
    nrm = nrm if plane else None
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _one(gpu, src, tgt, nrm, T0, MAX_DIST, 2)
    answered, redone = B.icp_stats(reset=True)
    _check(got, [ref.icp(src, tgt, nrm, T0, MAX_DIST, 2, scale_bounds=BOUNDS)], "coordinate 70")
    assert got["iters"][0] >= 1 and answered == redone == 2 * (got["iters"][0] + 1)     # two workgroups, every round


def _stop_batch(plane):
    """Three problems in one call with a narrow interval: a source 15 % too small (the interval rule), a degenerate
    one (point: every source the same dyadic point -- the denominator is an exact 0; plane: an exactly planar target -- the
    third pivot is an exact 0) and one with a pair fewer than the estimation needs."""
    src_a, tgt_a, nrm_a, T0_a = _problem(5)
    if plane:
        g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) * 0.05
        tgt_b = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
        nrm_b = np.tile(np.float32([0, 0, 1]), (len(tgt_b), 1))
        src_b = (tgt_b[10:100] + np.float32([0.004, -0.003, 0.01])).astype(np.float32)
    else:
        tgt_b = (np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
                 * 0.25).astype(np.float32)
        nrm_b = np.tile(np.float32([0, 0, 1]), (len(tgt_b), 1))
        src_b = np.tile(np.float32([0.375, 0.5, 0.125]), (8, 1))
    few = 6 if plane else 2
    src = np.concatenate([src_a, src_b, src_a[:few]])
    soff = [0, len(src_a), len(src_a) + len(src_b), len(src)]
    tgt, nrm = np.concatenate([tgt_a, tgt_b]), np.concatenate([nrm_a, nrm_b])
    toff = [0, len(tgt_a), len(tgt)]
    T0 = np.stack([T0_a, np.eye(4, dtype=np.float32), T0_a])
    return src, soff, tgt, (nrm if plane else None), toff, [0, 1, 2], [0, 1, 0], T0


@pytest.mark.parametrize("plane", (False, True))
def test_stop_rules_keep_the_state_before_the_refused_update(gpu, plane):
    src, soff, tgt, nrm, toff, sseg, tseg, T0 = _stop_batch(plane)
    # the interval lets at least one update through before it refuses one: the plane fit's accumulated scale goes
    # 1.098, 1.142 on this problem, the point fit's 1.018, 1.040, 1.062 at max_dist 0.25
    bounds = (0.9, 1.12) if plane else (0.95, 1.05)
    md = MAX_DIST if plane else 0.25                # the dyadic sources lie 0.177 from their nearest grid point
    want = ref.icp_batch(src, soff, tgt, nrm, toff, sseg, tseg, T0, md, 30, scale_bounds=bounds)
    got = _run(gpu, src, soff, tgt, nrm, toff, sseg, tseg, T0, md, 30, bounds)
    _check(got, want, "stop rules")
    # the interval: the run ends with the state of a run that was given exactly that many updates, inside the interval,
    # and one more update would have left it
    k = int(got["iters"][0])
    a = (src[soff[0]:soff[1]], tgt[toff[0]:toff[1]], None if nrm is None else nrm[toff[0]:toff[1]], T0[0])
    upto = _one(gpu, *a, md, k, bounds)
    more = _one(gpu, *a, md, k + 1)
    assert 1 <= k < 30 and bounds[0] <= got["scale"][0] <= bounds[1] and got["scale"][0] != 1.0
    assert more["iters"][0] == k + 1 and more["scale"][0] > bounds[1]
    for key in ("T", "T32", "scale", "fitness", "rmse", "iters", "ncorr"):
        assert _same(got[key][:1], upto[key]), key
    # the degenerate problem and the one below the pair minimum: nothing applied
    for p in (1, 2):
        assert got["iters"][p] == 0 and got["scale"][p] == 1.0 and _same(got["T32"][p], T0[p].reshape(16)), p
    assert got["ncorr"][1] == soff[2] - soff[1] and got["ncorr"][2] == (6 if plane else 2)


@pytest.mark.parametrize("plane", (False, True))
def test_empty_segments_and_no_problem(gpu, plane):
    c = _mixed()
    src, tgt, nrm = c["src"][-40:], c["tgt"][-300:], (c["nrm"][-300:] if plane else None)
    T0 = c["T0"][:3]
    soff, toff = [0, 0, 40], [0, 0, 300]
    e = None if nrm is None else nrm[:0]
    want = [ref.icp(src[:0], tgt, nrm, T0[0], MAX_DIST, 3), ref.icp(src, tgt[:0], e, T0[1], MAX_DIST, 3),
            ref.icp(src, tgt, nrm, T0[2], MAX_DIST, 3)]
    got = _run(gpu, src, soff, tgt, nrm, toff, [0, 1, 1], [1, 0, 1], T0, MAX_DIST, 3)
    _check(got, want, "empty")
    for p in (0, 1):
        assert got["fitness"][p] == 0.0 and got["rmse"][p] == 0.0 and got["iters"][p] == 0 and got["scale"][p] == 1.0
        assert _same(got["T"][p], T0[p].reshape(16).astype(np.float64))
    assert got["iters"][2] >= 1
    none = _run(gpu, src, soff, tgt, nrm, toff, [], [], T0[:0], MAX_DIST, 3)
    assert none["T"].shape == (0, 16) and none["corr"].shape == (0,) and none["scale"].shape == (0,)


def test_switch_in_child_processes(gpu, tmp_path):
    """CS_ICP_F16=0 and the default, each in a process of its own under its own time limit: identical bits, equal to this
    process's."""
    res = {}
    for setting in ("default", "0"):
        env = dict(os.environ)
        env.pop("CS_ICP_F16", None)
        env["CS_ICP_STATS"] = "1"
        if setting == "0":
            env["CS_ICP_F16"] = "0"
        path = str(tmp_path / ("out_%s.npz" % setting))
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_icp_scale", path], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[setting] = dict(np.load(path))
    a, b = res["default"], res["0"]
    assert a.keys() == b.keys()
    here = {}
    for plane in (False, True):
        here.update({("plane_" if plane else "point_") + k: v for k, v in _run_mixed(gpu, plane).items()})
    for k in a:
        if k != "stats":
            assert _same(a[k], b[k]) and _same(a[k], here[k]), k
    assert a["stats"][0] > 0 and a["stats"][1] < a["stats"][0] and b["stats"].tolist() == [0, 0]


@pytest.mark.parametrize("plane", (False, True))
def test_fallback_share_on_uniform_clouds(gpu, monkeypatch, plane):
    """tests/test_gpu_icp.py's condition on its fixture: the association is the rigid entries', so is the bar."""
    from corsair_amd import backend as B

    rng = np.random.default_rng(4)
    P, ns, nt = 32, 1000, 5000
    src = rng.uniform(-0.5, 0.5, (P * ns, 3)).astype(np.float32)
    tgt = rng.uniform(-0.5, 0.5, (P * nt, 3)).astype(np.float32)
    nrm = None
    if plane:
        nrm = rng.standard_normal((P * nt, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    T0 = np.stack([np.eye(4, dtype=np.float32)] * P)
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _run(gpu, src, (np.arange(P + 1) * ns).tolist(), tgt, nrm, (np.arange(P + 1) * nt).tolist(), list(range(P)),
               list(range(P)), T0, 0.05, 1)
    answered, redone = B.icp_stats(reset=True)
    print("f16 workgroups answered %d, recomputed %d" % (answered, redone))
    assert answered == P * 4 * 2 and (got["iters"] == 1).all()
    assert redone / answered < 0.10


def test_refused_arguments_launch_nothing(gpu):
    from corsair_amd import _lib, backend as B

    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32, device=gpu)
    buf[:16] = torch.eye(4, device=gpu).reshape(16)
    out = torch.full((64,), -7.0, dtype=torch.float64, device=gpu)
    i64, i32 = ctypes.c_int64 * 2, ctypes.c_int32 * 1
    at = lambda k: ctypes.c_void_p(out.data_ptr() + 8 * k)
    b = ctypes.c_void_p(buf.data_ptr())

    def call(nrm=b, soff=i64(0, 4), max_dist=0.1, max_iter=3, smin=0.5, smax=2.0, T=at(0), scale=at(20)):
        return lib.cs_icp_scale_batch(b, soff, b, nrm, i64(0, 4), i32(0), i32(0), 1, b, max_dist, max_iter, 1e-6, 1e-6, smin,
                                      smax, T, None, at(16), at(17), scale, at(18), at(19), None, None)

    INVALID, UNSUPPORTED = -1, -5
    nan, inf = float("nan"), float("inf")
    for kw in (dict(smin=0.0), dict(smin=-1.0), dict(smin=1.5), dict(smax=0.9), dict(smax=inf), dict(smin=nan),
               dict(smax=nan), dict(scale=None), dict(soff=None), dict(max_dist=0.0), dict(T=None)):
        assert call(**kw) == INVALID, kw
    assert call(smin=1.5) == INVALID and b"scale" in lib.cs_last_error()
    assert call(max_iter=1001) == UNSUPPORTED and call(soff=i64(0, 2 ** 31)) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                # nothing was launched: no output was written
    assert call() == 0 and call(nrm=None) == 0 and call(smin=1.0, smax=1.0) == 0
    torch.cuda.synchronize()
    assert float(out[20]) == 1.0 and float(out[16]) >= 0.0
    x = torch.zeros((4, 3), device=gpu)
    eye = torch.eye(4, device=gpu)[None]
    with pytest.raises(ValueError, match="robust"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, tgt_normals=x, kernel="tukey", kernel_scale=0.1,
                    with_scaling=True)
    with pytest.raises(ValueError, match="scale_bounds"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, with_scaling=True, scale_bounds=(1.2, 2.0))
    torch.cuda.synchronize()


if __name__ == "__main__":
    from corsair_amd import backend as _B

    _B.icp_stats(reset=True)
    _out = {}
    for _plane in (False, True):
        _out.update({("plane_" if _plane else "point_") + k: v
                     for k, v in _run_mixed(torch.device("cuda:0"), _plane).items()})
    _out["stats"] = np.array(_B.icp_stats(), np.int64)
    np.savez(sys.argv[1], **_out)
