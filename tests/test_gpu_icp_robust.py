"""cs_icp_plane_robust_batch on the GPU: transforms, fitness, rmse, wfitness, updates, pair counts and correspondences are
BIT-EQUAL to tests/icp_robust_ref.py for Huber, Cauchy and Tukey on both association paths, and kernel = L2 through the new
entry is cs_icp_plane_batch bit for bit.

`python -m tests.test_gpu_icp_robust OUT.npz` runs the mixed batch with the three kernels in a process of its own (the
switch test)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import icp_plane_ref as plane_ref
from tests import icp_robust_ref as ref
from tests import test_gpu_icp as pt
from tests import test_icp_robust_cpu as cpu
from tests.test_gpu_icp_plane import _np_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MAX_DIST = 0.1
KERNELS = cpu.KERNELS                       # (name, scale): huber 0.01, cauchy 0.01, tukey 0.02
_same = pt._same

SIZES_S = (1, 255, 257, 600, 0)             # both sides of the 256-source workgroup, one segment over three, an empty one
SIZES_T = (1, 513, 1300, 0)                 # both sides of the 512-row LDS stage, an empty one
# (source segment, target segment): target 2 is shared by four problems, target 1 by two; 6 has an empty source, 7 an
# empty target
PROBLEMS = ((0, 2), (1, 1), (2, 2), (3, 2), (3, 1), (1, 0), (4, 2), (2, 3), (0, 0))


@functools.lru_cache(maxsize=None)
def _mixed():
    from corsair_amd import synth

    rng = np.random.default_rng(2027)
    cloud = synth.make_cloud(11, 6000)
    Tgt = synth.random_pose(5, max_trans=0.3)
    Tinv = np.linalg.inv(Tgt)
    soff = np.concatenate([[0], np.cumsum(SIZES_S)]).tolist()
    toff = np.concatenate([[0], np.cumsum(SIZES_T)]).tolist()
    tsegs = [cloud[rng.choice(len(cloud), n, replace=False)].astype(np.float32) for n in SIZES_T]
    src = np.concatenate([synth.apply_pose(cloud[rng.choice(len(cloud), n, replace=False)] +
                                           rng.normal(0, 0.003, (n, 3)).astype(np.float32), Tinv) for n in SIZES_S])
    T0 = np.stack([pt._perturbed(Tgt, 3.0, 0.01, rng) for _ in PROBLEMS])
    return {"src": src.astype(np.float32), "soff": soff, "tgt": np.concatenate(tsegs), "toff": toff, "T0": T0,
            "nrm": np.concatenate([_np_normals(t) for t in tsegs]).astype(np.float32),
            "sseg": [p[0] for p in PROBLEMS], "tseg": [p[1] for p in PROBLEMS]}


@functools.lru_cache(maxsize=None)
def _mixed_ref(kernel, scale, max_iter=1):
    c = _mixed()
    return ref.icp_batch(c["src"], c["soff"], c["tgt"], c["nrm"], c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST, max_iter,
                         kernel=kernel, kernel_scale=scale)


def _result(r):
    out = {"T": r.T.cpu().numpy().reshape(-1, 16), "T32": r.T32.cpu().numpy().reshape(-1, 16),
           "fitness": r.fitness.cpu().numpy(), "rmse": r.rmse.cpu().numpy(), "iters": r.iters.cpu().numpy(),
           "ncorr": r.ncorr.cpu().numpy(), "corr": r.corr.cpu().numpy(), "corr_off": np.asarray(r.corr_off, np.int64)}
    if r.wfitness is not None:
        out["wfitness"] = r.wfitness.cpu().numpy()
    return out


def _run(dev, src, soff, tgt, nrm, toff, sseg, tseg, T0, max_dist, max_iter, kernel, scale):
    from corsair_amd import backend as B

    to = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shape)).to(dev)
    return _result(B.icp_batch(to(src, (-1, 3)), soff, to(tgt, (-1, 3)), toff, sseg, tseg, to(T0, (-1, 4, 4)), max_dist,
                               max_iter, return_corr=True, tgt_normals=to(nrm, (-1, 3)), kernel=kernel, kernel_scale=scale))


def _run_mixed(dev, kernel, scale, max_iter=1):
    c = _mixed()
    return _run(dev, c["src"], c["soff"], c["tgt"], c["nrm"], c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST, max_iter,
                kernel, scale)


def _one(dev, src, tgt, nrm, T0, max_dist, max_iter, kernel, scale):
    return _run(dev, src, [0, len(src)], tgt, nrm, [0, len(tgt)], [0], [0], np.asarray(T0, np.float32).reshape(1, 4, 4),
                max_dist, max_iter, kernel, scale)


def _check(got, want, what=""):
    pt._check(got, want, what)
    for p, w in enumerate(want):
        assert _same(got["wfitness"][p], np.float64(w["wfitness"])), (what, p, got["wfitness"][p], w["wfitness"])


def _problem(p):
    c = _mixed()
    s, t = PROBLEMS[p]
    return (c["src"][c["soff"][s]:c["soff"][s + 1]], c["tgt"][c["toff"][t]:c["toff"][t + 1]],
            c["nrm"][c["toff"][t]:c["toff"][t + 1]], c["T0"][p])


@pytest.mark.parametrize("kernel,scale", KERNELS)
def test_mixed_batch_matches_reference(gpu, kernel, scale):
    want = _mixed_ref(kernel, scale)
    got = _run_mixed(gpu, kernel, scale)
    _check(got, want, "mixed " + kernel)
    assert max(w["iters"] for w in want) == 1 and any(w["ncorr"] < 6 for w in want)     # both kinds are in the batch
    assert any(0.0 < w["wfitness"] < w["fitness"] for w in want)                        # the weights do something
    for p in (6, 7):                                                                    # empty source, empty target
        assert got["fitness"][p] == 0.0 and got["wfitness"][p] == 0.0 and got["iters"][p] == 0
        assert _same(got["T"][p], _mixed()["T0"][p].reshape(16).astype(np.float64))
    again = _run_mixed(gpu, kernel, scale)
    assert got.keys() == again.keys() and all(_same(got[k], again[k]) for k in got)     # two runs: identical bits
    # the weighted estimate is not the unweighted one
    plain = plane_ref.icp(*_problem(3), MAX_DIST, 1)
    assert not _same(got["T"][3], plain["T"])


@pytest.mark.parametrize("kernel,scale", KERNELS)
def test_max_iter_0_1_30_alone_and_permuted(gpu, kernel, scale):
    src, tgt, nrm, T0 = _problem(3)                 # 600 sources against 1 300 targets
    for max_iter in (0, 30):
        want = ref.icp(src, tgt, nrm, T0, MAX_DIST, max_iter, kernel=kernel, kernel_scale=scale)
        got = _one(gpu, src, tgt, nrm, T0, MAX_DIST, max_iter, kernel, scale)
        _check(got, [want], "%s max_iter %d" % (kernel, max_iter))
        assert want["iters"] <= max_iter
    assert want["iters"] > 1
    # alone = in the batch (max_iter 1); a permutation of the source rows changes nothing but the order of the pairs
    alone = _one(gpu, src, tgt, nrm, T0, MAX_DIST, 1, kernel, scale)
    _check(alone, [_mixed_ref(kernel, scale)[3]], "alone")
    perm = np.random.default_rng(5).permutation(len(src))
    shuf = _one(gpu, src[perm], tgt, nrm, T0, MAX_DIST, 1, kernel, scale)
    for k in ("T", "T32", "fitness", "rmse", "wfitness", "iters", "ncorr"):
        assert _same(shuf[k], alone[k]), k
    assert np.array_equal(shuf["corr"], alone["corr"][perm])


def test_residual_equal_to_the_scale_and_all_zero_weights(gpu):
    src, tgt, nrm, eye = cpu.edge_case()            # every residual is exactly 0.25
    for kernel, k, max_iter in (("huber", 0.25, 0), ("tukey", 0.25, 30), ("tukey", 0.5, 0), ("cauchy", 0.25, 0)):
        want = ref.icp(src, tgt, nrm, eye, 0.3, max_iter, kernel=kernel, kernel_scale=k)
        got = _one(gpu, src, tgt, nrm, eye, 0.3, max_iter, kernel, k)
        _check(got, [want], "%s k %g" % (kernel, k))
        assert got["ncorr"][0] == len(src)
        if kernel == "huber":
            assert got["wfitness"][0] == 1.0        # |r| = k: weight 1
        if (kernel, k) == ("tukey", 0.25):          # |r| = k: every weight 0, A = 0, the pivot rule stops it at T0
            assert got["wfitness"][0] == 0.0 and got["iters"][0] == 0 and got["fitness"][0] == 1.0
            assert _same(got["T"][0], eye.reshape(16).astype(np.float64)) and _same(got["T32"][0], eye.reshape(16))
        if (kernel, k) == ("tukey", 0.5):
            assert got["wfitness"][0] == 0.5625
        if kernel == "cauchy":
            assert got["wfitness"][0] == 0.5


def test_out_of_f16_range_takes_the_exact_kernel(gpu, monkeypatch):
    from corsair_amd import backend as B

    src, tgt, nrm, T0 = _problem(1)                 # 255 sources against 513 targets
    tgt = tgt + np.float32([70.0, 0.0, 0.0])        # a coordinate of 70
    T0 = T0.copy()
    T0[0, 3] += 70.0
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _one(gpu, src, tgt, nrm, T0, MAX_DIST, 2, "cauchy", 0.01)
    answered, redone = B.icp_stats(reset=True)
    _check(got, [ref.icp(src, tgt, nrm, T0, MAX_DIST, 2, kernel="cauchy", kernel_scale=0.01)], "coordinate 70")
    assert got["iters"][0] >= 1 and answered == redone == got["iters"][0] + 1


def test_long_normals(gpu):
    src, tgt, nrm, T0 = _problem(2)                 # 257 sources against 1 300 targets
    for kernel, scale in KERNELS:
        want = ref.icp(src, tgt, nrm * np.float32(1e3), T0, MAX_DIST, 3, kernel=kernel, kernel_scale=scale)
        got = _one(gpu, src, tgt, nrm * np.float32(1e3), T0, MAX_DIST, 3, kernel, scale)
        _check(got, [want], kernel + " normals x 1e3")
        assert np.all(np.isfinite(got["T"])) and 0.0 <= got["wfitness"][0] <= got["fitness"][0]


def test_switch_in_child_processes(gpu, tmp_path):
    """CS_ICP_F16=0 and =1, each in a process of its own: identical bits, equal to this process's."""
    res = {}
    for setting in ("1", "0"):
        env = dict(os.environ)
        env["CS_ICP_F16"] = setting
        env["CS_ICP_STATS"] = "1"
        path = str(tmp_path / ("out_%s.npz" % setting))
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_icp_robust", path], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[setting] = dict(np.load(path))
    a, b = res["1"], res["0"]
    assert a.keys() == b.keys()
    for kernel, scale in KERNELS:
        here = _run_mixed(gpu, kernel, scale)
        for k in here:
            assert _same(a[kernel + "_" + k], b[kernel + "_" + k]) and _same(a[kernel + "_" + k], here[k]), (kernel, k)
    assert a["stats"][0] > 0 and a["stats"][1] < a["stats"][0] and b["stats"].tolist() == [0, 0]


def _entry(dev, c, kernel, scale, max_iter, robust=True):
    """The C entries directly: cs_icp_plane_robust_batch (robust) or cs_icp_plane_batch on the mixed batch."""
    from corsair_amd import _lib
    from corsair_amd._lib import i32_array, i64_array, ptr, stream_ptr

    lib = _lib.load()
    n = len(c["sseg"])
    to = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shape)).to(dev)
    src, tgt, nrm, T0 = to(c["src"], (-1, 3)), to(c["tgt"], (-1, 3)), to(c["nrm"], (-1, 3)), to(c["T0"], (-1, 4, 4))
    T = torch.empty((n, 16), dtype=torch.float64, device=dev)
    T32 = torch.empty((n, 16), dtype=torch.float32, device=dev)
    fit, rm, wfit = (torch.full((n,), -1.0, dtype=torch.float64, device=dev) for _ in range(3))
    iters, ncorr = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    lens = [c["soff"][s + 1] - c["soff"][s] for s in c["sseg"]]
    corr = torch.full((sum(lens),), -1, dtype=torch.int32, device=dev)
    head = (ptr(src), i64_array(c["soff"]), ptr(tgt), ptr(nrm), i64_array(c["toff"]), i32_array(c["sseg"]), i32_array(c["tseg"]),
            n, ptr(T0), MAX_DIST, max_iter, 1e-6, 1e-6)
    if robust:
        rc = lib.cs_icp_plane_robust_batch(*head, kernel, scale, ptr(T), ptr(T32), ptr(fit), ptr(rm), ptr(wfit), ptr(iters),
                                           ptr(ncorr), ptr(corr), stream_ptr())
    else:
        rc = lib.cs_icp_plane_batch(*head, ptr(T), ptr(T32), ptr(fit), ptr(rm), ptr(iters), ptr(ncorr), ptr(corr),
                                    stream_ptr())
    assert rc == 0, lib.cs_last_error()
    out = {"T": T, "T32": T32, "fitness": fit, "rmse": rm, "iters": iters, "ncorr": ncorr, "corr": corr}
    if robust:
        out["wfitness"] = wfit
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_l2_through_the_new_entry_is_the_plane_entry(gpu):
    c = _mixed()
    for max_iter in (1, 5):
        plane = _entry(gpu, c, 0, 0.0, max_iter, robust=False)
        for scale in (0.0, float("nan"), 0.02):                    # with L2 the scale is ignored
            l2 = _entry(gpu, c, ref.L2, scale, max_iter)
            for k in plane:
                assert _same(l2[k], plane[k]), (k, scale)
            assert _same(l2["wfitness"], plane["fitness"])         # every weight is 1
    huber = _entry(gpu, c, ref.HUBER, 0.01, 1)                     # and the direct call is what backend.icp_batch returns
    via = _run_mixed(gpu, "huber", 0.01)
    assert all(_same(huber[k], via[k]) for k in huber)
    _check(dict(huber, corr_off=via["corr_off"]), _mixed_ref("huber", 0.01), "direct")


def test_refused_arguments(gpu):
    from corsair_amd import _lib, backend as B

    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32, device=gpu)
    out = torch.zeros(64, dtype=torch.float64, device=gpu)
    i64, i32 = ctypes.c_int64 * 2, ctypes.c_int32 * 1
    at = lambda k: ctypes.c_void_p(out.data_ptr() + 8 * k)
    b = ctypes.c_void_p(buf.data_ptr())

    def call(kernel=ref.TUKEY, scale=0.02, nrm=b, max_dist=0.1, max_iter=3, T=at(0), wfit=at(20)):
        return lib.cs_icp_plane_robust_batch(b, i64(0, 4), b, nrm, i64(0, 4), i32(0), i32(0), 1, b, max_dist, max_iter, 1e-6,
                                             1e-6, kernel, scale, T, None, at(16), at(17), wfit, at(18), at(19), None, None)

    INVALID, UNSUPPORTED = -1, -5
    assert call() == 0 and call(wfit=None) == 0                     # d_wfitness is optional
    for kernel in (-1, 4, 17):
        assert call(kernel=kernel) == INVALID and b"kernel" in lib.cs_last_error()
    for kernel in (ref.HUBER, ref.CAUCHY, ref.TUKEY):
        for scale in (0.0, -0.02, float("inf"), float("nan")):
            assert call(kernel=kernel, scale=scale) == INVALID and b"kernel_scale" in lib.cs_last_error()
    for scale in (0.0, -1.0, float("nan")):
        assert call(kernel=ref.L2, scale=scale) == 0                # with L2 the scale is ignored
    assert call(nrm=None) == INVALID and call(max_dist=0.0) == INVALID and call(T=None) == INVALID
    assert call(max_iter=1001) == UNSUPPORTED
    x = torch.zeros((4, 3), device=gpu)
    eye = torch.eye(4, device=gpu)[None]
    with pytest.raises(ValueError, match="tgt_normals"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, kernel="tukey", kernel_scale=0.02)
    with pytest.raises(ValueError, match="kernel"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, tgt_normals=x, kernel="gm", kernel_scale=0.02)
    with pytest.raises(ValueError, match="kernel_scale"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, tgt_normals=x, kernel="tukey")
    with pytest.raises(_lib.CorsairHipError, match="kernel_scale"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, tgt_normals=x, kernel="tukey", kernel_scale=0.0)
    torch.cuda.synchronize()


def test_clutter_fixture_reaches_the_restatement(gpu):
    """The fixture of tests/test_icp_robust_cpu.py on the GPU: the restatement's bits, and therefore its errors."""
    src, tgt, nrm, T0, Tgt = cpu.clutter_fixture()
    err = {}
    for kernel, scale in KERNELS:
        got = _one(gpu, src, tgt, nrm, T0, cpu.CLUTTER_MAX_DIST, 30, kernel, scale)
        _check(got, [cpu.clutter_ref(kernel, scale)], "clutter " + kernel)
        err[kernel] = cpu.pose_errors(got["T"][0], Tgt)
    from corsair_amd import backend as B

    to = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shape)).to(gpu)
    l2 = B.icp_batch(to(src, (-1, 3)), [0, len(src)], to(tgt, (-1, 3)), [0, len(tgt)], [0], [0], to(T0, (1, 4, 4)),
                     cpu.CLUTTER_MAX_DIST, 30, tgt_normals=to(nrm, (-1, 3)))
    assert l2.wfitness is None
    rte_l2 = cpu.pose_errors(l2.T.cpu().numpy()[0], Tgt)[1]
    print("RTE: L2 %.6f, %s" % (rte_l2, ", ".join("%s %.6f" % (k, e[1]) for k, e in err.items())))
    assert rte_l2 > cpu.pose_errors(T0, Tgt)[1] and err["tukey"][1] < rte_l2 / 10


if __name__ == "__main__":
    from corsair_amd import backend as _B

    _B.icp_stats(reset=True)
    _out = {}
    for _kernel, _scale in KERNELS:
        for _k, _v in _run_mixed(torch.device("cuda:0"), _kernel, _scale).items():
            _out[_kernel + "_" + _k] = _v
    _out["stats"] = np.array(_B.icp_stats(), np.int64)
    np.savez(sys.argv[1], **_out)
