"""cs_icp_batch on the GPU: transforms, fitness, rmse, iterations, pair counts and correspondences are BIT-EQUAL to
tests/icp_ref.py on both association paths (f16 matrix-core ranking + strict voucher + exhaustive recomputation, and the
exhaustive kernel alone under CS_ICP_F16=0).

`python -m tests.test_gpu_icp OUT.npz` runs the mixed batch in a process of its own (the switch test)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import icp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES_S = (1, 31, 33, 255, 257, 600)        # lane group, 32-row tile, 256-source workgroup boundaries
SIZES_T = (1, 2, 255, 257, 513, 3000)       # the 256-row stage
# (source segment, target segment): every size once, then shared target segments
PROBLEMS = ((0, 5), (1, 4), (2, 3), (3, 2), (4, 1), (5, 0), (5, 5), (4, 5), (2, 4))
MAX_DIST = 0.1


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _perturbed(T, deg, trans, rng):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    D[:3, 3] = rng.uniform(-trans, trans, 3)
    return (D @ T).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _mixed():
    """One synthetic shape: every target segment is a subset of its points, every source segment a jittered subset in
    another pose; a problem starts at the true pose perturbed by a few degrees."""
    from corsair_amd import synth

    rng = np.random.default_rng(2026)
    cloud = synth.make_cloud(7, 8000)
    Tgt = synth.random_pose(3, max_trans=0.3)
    Tinv = np.linalg.inv(Tgt)
    soff = np.concatenate([[0], np.cumsum(SIZES_S)]).tolist()
    toff = np.concatenate([[0], np.cumsum(SIZES_T)]).tolist()
    tgt = np.concatenate([cloud[rng.choice(len(cloud), n, replace=False)] for n in SIZES_T]).astype(np.float32)
    src = np.concatenate([synth.apply_pose(cloud[rng.choice(len(cloud), n, replace=False)] +
                                           rng.normal(0, 0.003, (n, 3)).astype(np.float32), Tinv) for n in SIZES_S])
    T0 = np.stack([_perturbed(Tgt, 3.0, 0.01, rng) for _ in PROBLEMS])
    return {"src": src.astype(np.float32), "soff": soff, "tgt": tgt, "toff": toff, "T0": T0,
            "sseg": [p[0] for p in PROBLEMS], "tseg": [p[1] for p in PROBLEMS]}


@functools.lru_cache(maxsize=None)
def _mixed_ref(max_iter=2):
    c = _mixed()
    return ref.icp_batch(c["src"], c["soff"], c["tgt"], c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST, max_iter)


def _run(dev, src, soff, tgt, toff, sseg, tseg, T0, max_dist, max_iter, **kw):
    from corsair_amd import backend as B

    r = B.icp_batch(torch.from_numpy(np.ascontiguousarray(src, np.float32).reshape(-1, 3)).to(dev), soff,
                    torch.from_numpy(np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)).to(dev), toff, sseg, tseg,
                    torch.from_numpy(np.ascontiguousarray(T0, np.float32).reshape(-1, 4, 4)).to(dev), max_dist, max_iter,
                    return_corr=True, **kw)
    out = {"T": r.T.cpu().numpy().reshape(-1, 16), "T32": r.T32.cpu().numpy().reshape(-1, 16),
           "fitness": r.fitness.cpu().numpy(), "rmse": r.rmse.cpu().numpy(), "iters": r.iters.cpu().numpy(),
           "ncorr": r.ncorr.cpu().numpy(), "corr": r.corr.cpu().numpy(), "corr_off": np.asarray(r.corr_off, np.int64)}
    return out


def _run_mixed(dev, max_iter=2):
    c = _mixed()
    return _run(dev, c["src"], c["soff"], c["tgt"], c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST, max_iter)


def _check(got, want, what=""):
    """got: _run's dict; want: icp_ref results, one per problem."""
    for p, w in enumerate(want):
        tag = "%s problem %d" % (what, p)
        assert _same(got["T"][p], w["T"]), (tag, got["T"][p], w["T"])
        assert _same(got["T32"][p], w["T32"]), tag
        assert _same(got["fitness"][p], np.float64(w["fitness"])), (tag, got["fitness"][p], w["fitness"])
        assert _same(got["rmse"][p], np.float64(w["rmse"])), (tag, got["rmse"][p], w["rmse"])
        assert got["iters"][p] == w["iters"] and got["ncorr"][p] == w["ncorr"], tag
        assert np.array_equal(got["corr"][got["corr_off"][p]:got["corr_off"][p + 1]], w["corr"]), tag


def test_mixed_batch_matches_reference(gpu):
    want = _mixed_ref()
    got = _run_mixed(gpu)
    _check(got, want, "mixed")
    assert max(w["iters"] for w in want) == 2 and any(w["ncorr"] < 3 for w in want)     # both kinds are in the batch
    # two runs: identical bits
    again = _run_mixed(gpu)
    assert all(_same(got[k], again[k]) for k in got)


def test_problem_alone_and_permuted_sources(gpu):
    c, want = _mixed(), _mixed_ref()
    for p in (6, 2):
        s, t = PROBLEMS[p]
        src = c["src"][c["soff"][s]:c["soff"][s + 1]]
        tgt = c["tgt"][c["toff"][t]:c["toff"][t + 1]]
        alone = _run(gpu, src, [0, len(src)], tgt, [0, len(tgt)], [0], [0], c["T0"][p:p + 1], MAX_DIST, 2)
        _check(alone, [want[p]], "alone")
        perm = np.random.default_rng(5).permutation(len(src))
        shuf = _run(gpu, src[perm], [0, len(src)], tgt, [0, len(tgt)], [0], [0], c["T0"][p:p + 1], MAX_DIST, 2)
        for k in ("T", "T32", "fitness", "rmse", "iters", "ncorr"):
            assert _same(shuf[k], alone[k]), k
        assert np.array_equal(shuf["corr"], alone["corr"][perm])


def _tie_case():
    rng = np.random.default_rng(77)
    tgt = rng.uniform(1.0, 2.0, (600, 3)).astype(np.float32)
    tgt[5] = (0.25, 0.0, 0.0)
    tgt[400] = (-0.25, 0.0, 0.0)            # 395 rows on: another stage of the f16 kernel, another stage of the exact one
    tgt[40] = tgt[10]                       # duplicated row
    tgt[333] = tgt[10]
    # three rows at exactly 0.25 from (0, 3, 0), in three stages and in the SAME lane half (row mod 8 < 4): a lane of the
    # f16 kernel evaluates two tiles at most, so one of the three stays unevaluated and the strict voucher must decline
    tgt[8] = (0.25, 3.0, 0.0)
    tgt[264] = (-0.25, 3.0, 0.0)
    tgt[520] = (0.0, 3.25, 0.0)
    src = np.concatenate([[[0.0, 0.0, 0.0]], tgt[10:11], [[0.0, 3.0, 0.0]],
                          tgt[100:140] + rng.normal(0, 0.01, (40, 3))]).astype(np.float32)
    return src, tgt


def test_ties_go_to_the_smaller_row(gpu, monkeypatch):
    from corsair_amd import backend as B

    src, tgt = _tie_case()
    T0 = np.eye(4, dtype=np.float32)[None]          # the identity poses exactly: the ties are exact
    assert ref.dist2(ref.pose(T0.reshape(16), src[0]), tgt[5]) == ref.dist2(ref.pose(T0.reshape(16), src[0]), tgt[400])
    assert len({ref.dist2(ref.pose(T0.reshape(16), src[2]), tgt[j]) for j in (8, 264, 520)}) == 1
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    for max_iter in (0, 1):
        want = ref.icp(src, tgt, T0, 0.5, max_iter)
        got = _run(gpu, src, [0, len(src)], tgt, [0, len(tgt)], [0], [0], T0, 0.5, max_iter)
        _check(got, [want], "ties")
        if max_iter == 0:
            assert got["corr"][:3].tolist() == [5, 10, 8]
            # rows 5 and 400 sit in different lane halves, both are evaluated and the tie is decided exactly, by row; the
            # three-way tie leaves an unevaluated row level with the result: not vouched for, the workgroup is recomputed
            assert B.icp_stats() == (1, 1)
    answered, redone = B.icp_stats(reset=True)
    assert answered == 3 and 1 <= redone <= answered
    # the same under the exhaustive kernel alone
    monkeypatch.setenv("CS_ICP_F16", "0")
    got = _run(gpu, src, [0, len(src)], tgt, [0, len(tgt)], [0], [0], T0, 0.5, 1)
    _check(got, [ref.icp(src, tgt, T0, 0.5, 1)], "ties, exhaustive")
    assert B.icp_stats() == (0, 0)


def test_max_dist_edges(gpu):
    rng = np.random.default_rng(9)
    tgt = rng.uniform(-0.5, 0.5, (300, 3)).astype(np.float32)
    src = (rng.uniform(-0.5, 0.5, (50, 3)) + 5.0).astype(np.float32)        # far from every target
    src[7] = tgt[20] + np.float32(0.01)
    src[31] = tgt[250] - np.float32(0.01)
    T0 = np.eye(4, dtype=np.float32)[None]
    # below every distance: stops at once with T = T0
    got = _run(gpu, src, [0, 50], tgt, [0, 300], [0], [0], T0, 1e-4, 30)
    _check(got, [ref.icp(src, tgt, T0, 1e-4, 30)], "no pair")
    assert got["ncorr"][0] == 0 and got["iters"][0] == 0 and got["fitness"][0] == 0.0 and got["rmse"][0] == 0.0
    assert _same(got["T"][0], T0.reshape(16).astype(np.float64)) and (got["corr"] == -1).all()
    # exactly two pairs: no fit from fewer than three
    got = _run(gpu, src, [0, 50], tgt, [0, 300], [0], [0], T0, 0.05, 30)
    _check(got, [ref.icp(src, tgt, T0, 0.05, 30)], "two pairs")
    assert got["ncorr"][0] == 2 and got["iters"][0] == 0 and got["fitness"][0] == 2 / 50
    assert sorted(np.nonzero(got["corr"] >= 0)[0].tolist()) == [7, 31]


def test_max_iter_0_1_and_convergence(gpu):
    c = _mixed()
    s, t = 2, 3                                   # 33 sources against 257 targets
    src = c["src"][c["soff"][s]:c["soff"][s + 1]]
    tgt = c["tgt"][c["toff"][t]:c["toff"][t + 1]]
    for max_iter in (0, 1, 30):
        want = ref.icp(src, tgt, c["T0"][2], MAX_DIST, max_iter)
        got = _run(gpu, src, [0, len(src)], tgt, [0, len(tgt)], [0], [0], c["T0"][2:3], MAX_DIST, max_iter)
        _check(got, [want], "max_iter %d" % max_iter)
        assert want["iters"] <= max_iter
    assert 1 < want["iters"] < 30                 # the 30-update run stopped on the convergence rule


def test_empty_segments_and_no_problem(gpu):
    c = _mixed()
    src, tgt = c["src"][:40], c["tgt"][-300:]
    T0 = c["T0"][:3]
    # problem 0: empty source segment; 1: empty target segment; 2: ordinary
    soff, toff = [0, 0, 40], [0, 0, 300]
    want = [ref.icp(src[:0], tgt, T0[0], MAX_DIST, 3), ref.icp(src, tgt[:0], T0[1], MAX_DIST, 3),
            ref.icp(src, tgt, T0[2], MAX_DIST, 3)]
    got = _run(gpu, src, soff, tgt, toff, [0, 1, 1], [1, 0, 1], T0, MAX_DIST, 3)
    _check(got, want, "empty")
    for p in (0, 1):
        assert got["fitness"][p] == 0.0 and got["rmse"][p] == 0.0 and got["iters"][p] == 0
        assert _same(got["T"][p], T0[p].reshape(16).astype(np.float64))
    none = _run(gpu, src, soff, tgt, toff, [], [], T0[:0], MAX_DIST, 3)
    assert none["T"].shape == (0, 16) and none["corr"].shape == (0,)


def test_out_of_f16_range_takes_the_exact_kernel(gpu, monkeypatch):
    from corsair_amd import backend as B

    c = _mixed()
    shift = np.float32([70.0, 0.0, 0.0])
    src = c["src"][c["soff"][3]:c["soff"][4]]
    tgt = c["tgt"][c["toff"][3]:c["toff"][4]] + shift
    T0 = c["T0"][3].copy()
    T0[0, 3] += 70.0
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _run(gpu, src, [0, len(src)], tgt, [0, len(tgt)], [0], [0], T0[None], MAX_DIST, 2)
    answered, redone = B.icp_stats(reset=True)
    _check(got, [ref.icp(src, tgt, T0, MAX_DIST, 2)], "coordinate 70")
    assert got["iters"][0] == 2 and answered == redone == 3


def test_switch_in_child_processes(gpu, tmp_path):
    """CS_ICP_F16=0 and the default, each in a process of its own: identical bits."""
    res = {}
    for setting in ("default", "0"):
        env = dict(os.environ)
        env.pop("CS_ICP_F16", None)
        env["CS_ICP_STATS"] = "1"
        if setting == "0":
            env["CS_ICP_F16"] = "0"
        path = str(tmp_path / ("out_%s.npz" % setting))
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_icp", path], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[setting] = dict(np.load(path))
    a, b = res["default"], res["0"]
    assert a.keys() == b.keys()
    for k in a:
        if k != "stats":
            assert _same(a[k], b[k]), k
    # the switch did select another path
    assert a["stats"][0] > 0 and a["stats"][1] < a["stats"][0] and b["stats"].tolist() == [0, 0]


def _raw_call(lib, **over):
    """cs_icp_batch through ctypes with one valid tiny problem, arguments replaced by `over`."""
    i64, i32 = ctypes.c_int64 * 2, ctypes.c_int32 * 1
    at = lambda k: ctypes.c_void_p(over["out"] + 8 * k)       # disjoint pieces of one f64 buffer
    a = dict(src=over["buf"], soff=i64(0, 4), tgt=over["buf"], toff=i64(0, 4), sseg=i32(0), tseg=i32(0), n=1,
             T0=over["buf"], max_dist=0.1, max_iter=3, rf=1e-6, rr=1e-6, T=at(0), T32=None, fit=at(16), rmse=at(17),
             iters=at(18), ncorr=at(19), corr=None)
    a.update({k: v for k, v in over.items() if k not in ("buf", "out")})
    return lib.cs_icp_batch(a["src"], a["soff"], a["tgt"], a["toff"], a["sseg"], a["tseg"], a["n"], a["T0"], a["max_dist"],
                            a["max_iter"], a["rf"], a["rr"], a["T"], a["T32"], a["fit"], a["rmse"], a["iters"], a["ncorr"],
                            a["corr"], None)


def test_refused_arguments(gpu):
    from corsair_amd import _lib

    lib = _lib.load()
    buf_t = torch.zeros(64, dtype=torch.float32, device=gpu)
    out_t = torch.zeros(64, dtype=torch.float64, device=gpu)
    base = dict(buf=ctypes.c_void_p(buf_t.data_ptr()), out=out_t.data_ptr())
    i64, i32 = ctypes.c_int64 * 2, ctypes.c_int32 * 1
    INVALID, UNSUPPORTED = -1, -5
    assert _raw_call(lib, **base) == 0
    for over, code in ((dict(soff=None), INVALID), (dict(toff=None), INVALID), (dict(sseg=None), INVALID),
                       (dict(tseg=None), INVALID), (dict(sseg=i32(-1)), INVALID), (dict(tseg=i32(-1)), INVALID),
                       (dict(soff=i64(4, 0)), INVALID), (dict(toff=i64(4, 0)), INVALID),
                       (dict(max_dist=0.0), INVALID), (dict(max_dist=-1.0), INVALID),
                       (dict(max_dist=float("inf")), INVALID), (dict(max_dist=float("nan")), INVALID),
                       (dict(max_iter=-1), UNSUPPORTED), (dict(max_iter=1001), UNSUPPORTED),
                       (dict(soff=i64(0, 2 ** 31)), UNSUPPORTED), (dict(toff=i64(0, 2 ** 31)), UNSUPPORTED),
                       (dict(T=None), INVALID), (dict(T0=None), INVALID), (dict(src=None), INVALID)):
        assert _raw_call(lib, **dict(base, **over)) == code, over
        assert lib.cs_last_error()
    torch.cuda.synchronize()
    assert float(out_t.abs().sum()) >= 0.0          # the device is still healthy


def test_fallback_share_on_uniform_clouds(gpu, monkeypatch):
    from corsair_amd import backend as B

    rng = np.random.default_rng(4)
    P, ns, nt = 32, 1000, 5000
    src = rng.uniform(-0.5, 0.5, (P * ns, 3)).astype(np.float32)
    tgt = rng.uniform(-0.5, 0.5, (P * nt, 3)).astype(np.float32)
    T0 = np.stack([np.eye(4, dtype=np.float32)] * P)
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _run(gpu, src, (np.arange(P + 1) * ns).tolist(), tgt, (np.arange(P + 1) * nt).tolist(), list(range(P)),
               list(range(P)), T0, 0.05, 1)
    answered, redone = B.icp_stats(reset=True)
    print("f16 workgroups answered %d, recomputed %d" % (answered, redone))
    assert answered == P * 4 * 2 and (got["iters"] == 1).all()
    assert redone / answered < 0.10


def _pair_batch(dev):
    """Two (query, CAD) pairs of ~150 voxels with made-up 16-d features: a query voxel carries its CAD voxel's feature."""
    from corsair_amd import synth

    rng = np.random.default_rng(21)
    n1 = (180, 160)
    xyz1 = [synth.make_cloud(40 + p, n1[p]) for p in range(2)]
    F1 = [rng.standard_normal((n, 16)).astype(np.float32) for n in n1]
    F1 = [f / np.linalg.norm(f, axis=1, keepdims=True) for f in F1]
    xyz0, F0, Ts = [], [], []
    for p in range(2):
        keep = rng.permutation(n1[p])[:150]
        T = synth.random_pose(60 + p, max_trans=0.2)
        xyz0.append(synth.apply_pose(xyz1[p][keep] + rng.normal(0, 0.002, (150, 3)).astype(np.float32), np.linalg.inv(T)))
        f = F1[p][keep] + rng.normal(0, 0.02, (150, 16)).astype(np.float32)
        F0.append((f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32))
        Ts.append(T)
    to = lambda parts: torch.from_numpy(np.concatenate(parts).astype(np.float32)).to(dev)
    return to(F0), to(xyz0), [0, 150, 300], to(F1), to(xyz1), [0, n1[0], n1[0] + n1[1]], Ts


def test_sym_pose_batch_with_icp(gpu):
    from corsair_amd import backend as B, registration as R

    F0, x0, off0, F1, x1, off1, _ = _pair_batch(gpu)
    kw = dict(k_nn=5, max_corr=0.2, seed=0, max_iter=2000, force_gate=True)
    off = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], **kw)
    on = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_max_iter=5, icp_max_dist=0.06, **kw)
    assert off.T_icp is None and off.cd_icp is None and off.icp_fitness is None and off.icp_rmse is None \
        and off.icp_iters is None
    for name in ("T_best", "cd_best", "T_ransac", "cd_ransac", "iters", "T_all", "cd_all", "inliers"):
        assert _same(getattr(off, name).cpu().numpy(), getattr(on, name).cpu().numpy()), name
    assert np.array_equal(off.ok, on.ok) and np.array_equal(off.best, on.best) and off.n_problems == on.n_problems
    assert off.prob_pair == on.prob_pair and off.prob_cfg == on.prob_cfg
    want = ref.icp_batch(x0.cpu().numpy(), off0, x1.cpu().numpy(), off1, [0, 1], [0, 1], on.T_best.cpu().numpy(), 0.06, 5)
    for p in range(2):
        assert _same(on.T_icp[p].cpu().numpy().reshape(16), want[p]["T32"])
        assert _same(on.icp_fitness[p].cpu().numpy(), np.float64(want[p]["fitness"]))
        assert _same(on.icp_rmse[p].cpu().numpy(), np.float64(want[p]["rmse"]))
        assert int(on.icp_iters[p]) == want[p]["iters"]
    cd = B.chamfer_1dir(x0, off0, x1, off1, [0, 1], [0, 1], on.T_icp)
    assert _same(on.cd_icp.cpu().numpy(), cd.cpu().numpy())
    with pytest.raises(ValueError):
        R.sym_pose_batch(F0, x0, off0, F1, x1, off1, [1, 2], icp_max_iter=5, **kw)


class _Pipe:
    """register_queries needs cfg, device and register: the network is not part of this test."""
    def __init__(self, dev, cfg):
        self.device, self.cfg = dev, cfg

    def register(self, *a, **k):
        from corsair_amd import harness as H

        return H.Pipeline.register(self, *a, **k)


def test_register_queries_returns_the_icp_arrays(gpu):
    from corsair_amd import cache as C, harness as H

    F0, x0, off0, F1, x1, off1, Ts = _pair_batch(gpu)
    desc = torch.zeros((2, 0), dtype=torch.float32, device=gpu)
    qs, cat = H.EmbeddedSet(F0, x0, off0, desc), H.EmbeddedSet(F1, x1, off1, desc)
    args = (np.arange(2), cat, np.arange(2), np.asarray([1, 2]), np.stack(Ts), np.stack([np.eye(4)] * 2))
    plain = H.register_queries(_Pipe(gpu, H.Config(ransac_max_iter=2000)), qs, *args)
    assert set(plain) == set(C.NAMES)
    cfg = H.Config(ransac_max_iter=2000, icp_max_iter=5)
    assert cfg.icp_distance() == 2 * cfg.voxel_size
    got = H.register_queries(_Pipe(gpu, cfg), qs, *args)
    assert set(got) == set(C.NAMES) | set(C.ICP_NAMES)
    for k in C.NAMES:
        assert _same(got[k], plain[k]), k
    for k in C.ICP_NAMES:
        assert got[k].dtype == C.ICP_DTYPES[k] and len(got[k]) == 2, k
    assert got["Ts_est_icp"].shape == (2, 4, 4)
    empty = H.register_queries(_Pipe(gpu, cfg), qs, np.arange(0), *args[1:])
    assert set(empty) == set(C.NAMES) | set(C.ICP_NAMES)
    for k in C.ICP_NAMES:
        assert empty[k].dtype == C.ICP_DTYPES[k] and len(empty[k]) == 0
    assert empty["Ts_est_icp"].shape == (0, 4, 4)
    ev = H.finish_eval({}, got, False)
    assert ev.icp is not None and "rre_mean_deg" in ev.icp and "icp refinement" in ev.report
    assert H.finish_eval({}, plain, False).icp is None


if __name__ == "__main__":
    from corsair_amd import backend as _B

    _B.icp_stats(reset=True)
    _out = _run_mixed(torch.device("cuda:0"))
    _out["stats"] = np.array(_B.icp_stats(), np.int64)
    np.savez(sys.argv[1], **_out)
