"""cs_icp_gicp_batch on the GPU: transforms, fitness, rmse, Mahalanobis rmse, updates, pair counts and correspondences are
BIT-EQUAL to tests/gicp_ref.py on both association paths, and cs_icp_plane_batch / cs_icp_batch -- run on the same batch in
the same process -- are still bit-equal to their own restatements.

`python -m tests.test_gpu_gicp OUT.npz` runs the mixed batch in a process of its own (the switch test)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gicp_ref as ref
from tests import icp_plane_ref
from tests import icp_ref
from tests import test_gpu_icp as pt
from tests.test_gpu_icp_plane import _np_normals
from tests.test_icp_cpu import _fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MAX_DIST = 0.1
_same = pt._same
# (seed, sources, targets): across the 256-source workgroup and the 512-row stage of the exhaustive kernel, and a small one
SHAPES = ((1, 300, 1400), (2, 257, 513), (3, 64, 40))


@functools.lru_cache(maxsize=None)
def _mixed():
    """Three problems in one batch; the normals of both sides are INPUT data (SciPy's KD-tree and eigh, 8 neighbours)."""
    parts = [_fixture(*s) for s in SHAPES]
    src = np.concatenate([p[0] for p in parts]).astype(np.float32)
    tgt = np.concatenate([p[1] for p in parts]).astype(np.float32)
    soff = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).tolist()
    return {"src": src, "tgt": tgt, "soff": soff, "toff": toff, "sseg": [0, 1, 2], "tseg": [0, 1, 2],
            "snrm": np.concatenate([_np_normals(p[0]) for p in parts]), "tnrm": np.concatenate([_np_normals(p[1]) for p in parts]),
            "T0": np.stack([p[2] for p in parts]).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def _mixed_ref(max_iter=1, epsilon=1e-3):
    c = _mixed()
    return ref.icp_batch(c["src"], c["snrm"], c["soff"], c["tgt"], c["tnrm"], c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST,
                         max_iter, epsilon=epsilon)


def _run(dev, src, snrm, soff, tgt, tnrm, toff, sseg, tseg, T0, max_dist, max_iter, epsilon=1e-3, estimation="gicp"):
    from corsair_amd import backend as B

    to = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shape)).to(dev)
    kw = {}
    if estimation == "gicp":
        kw = dict(estimation="gicp", src_normals=to(snrm, (-1, 3)), gicp_epsilon=epsilon)
    r = B.icp_batch(to(src, (-1, 3)), soff, to(tgt, (-1, 3)), toff, sseg, tseg, to(T0, (-1, 4, 4)), max_dist, max_iter,
                    return_corr=True, tgt_normals=None if estimation == "point" else to(tnrm, (-1, 3)), **kw)
    out = {"T": r.T.cpu().numpy().reshape(-1, 16), "T32": r.T32.cpu().numpy().reshape(-1, 16),
           "fitness": r.fitness.cpu().numpy(), "rmse": r.rmse.cpu().numpy(), "iters": r.iters.cpu().numpy(),
           "ncorr": r.ncorr.cpu().numpy(), "corr": r.corr.cpu().numpy(), "corr_off": np.asarray(r.corr_off, np.int64)}
    if estimation == "gicp":
        out["mrmse"] = r.mrmse.cpu().numpy()
    else:
        assert r.mrmse is None
    return out


def _run_mixed(dev, max_iter=1, epsilon=1e-3, estimation="gicp"):
    c = _mixed()
    return _run(dev, c["src"], c["snrm"], c["soff"], c["tgt"], c["tnrm"], c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST,
                max_iter, epsilon, estimation)


def _one(dev, src, snrm, tgt, tnrm, T0, max_dist, max_iter, epsilon=1e-3):
    return _run(dev, src, snrm, [0, len(src)], tgt, tnrm, [0, len(tgt)], [0], [0], np.asarray(T0, np.float32).reshape(1, 4, 4),
                max_dist, max_iter, epsilon)


def _check(got, want, what=""):
    pt._check(got, want, what)
    for p, w in enumerate(want):
        assert _same(got["mrmse"][p], np.float64(w["mrmse"])), (what, p, got["mrmse"][p], w["mrmse"])


def _problem(p):
    c = _mixed()
    return (c["src"][c["soff"][p]:c["soff"][p + 1]], c["snrm"][c["soff"][p]:c["soff"][p + 1]],
            c["tgt"][c["toff"][p]:c["toff"][p + 1]], c["tnrm"][c["toff"][p]:c["toff"][p + 1]], c["T0"][p])


@pytest.mark.parametrize("max_iter", (0, 1, 30))
def test_mixed_batch_matches_reference(gpu, max_iter):
    want = _mixed_ref(max_iter)
    got = _run_mixed(gpu, max_iter)
    _check(got, want, "mixed, max_iter %d" % max_iter)
    assert all(w["iters"] <= max_iter for w in want)
    if max_iter == 30:
        assert all(1 < w["iters"] < 30 for w in want[:2]) and all(w["mrmse"] >= 0 for w in want)
    again = _run_mixed(gpu, max_iter)
    assert all(_same(got[k], again[k]) for k in got)                    # two runs: identical bits


def test_alone_duplicated_and_permuted(gpu):
    src, snrm, tgt, tnrm, T0 = _problem(0)
    want = _mixed_ref(1)[0]
    alone = _one(gpu, src, snrm, tgt, tnrm, T0, MAX_DIST, 1)
    _check(alone, [want], "alone")
    twice = _run(gpu, src, snrm, [0, len(src)], tgt, tnrm, [0, len(tgt)], [0, 0], [0, 0], np.stack([T0, T0]), MAX_DIST, 1)
    _check(twice, [want, want], "duplicated")
    perm = np.random.default_rng(5).permutation(len(src))
    shuf = _one(gpu, src[perm], snrm[perm], tgt, tnrm, T0, MAX_DIST, 1)
    for k in ("T", "T32", "fitness", "rmse", "mrmse", "iters", "ncorr"):
        assert _same(shuf[k], alone[k]), k
    assert np.array_equal(shuf["corr"], alone["corr"][perm])


def test_switch_in_child_processes(gpu, tmp_path):
    """CS_ICP_F16=0 and the default, each in a process of its own: identical bits, equal to this process's."""
    res = {}
    for setting in ("default", "0"):
        env = dict(os.environ)
        env.pop("CS_ICP_F16", None)
        env["CS_ICP_STATS"] = "1"
        if setting == "0":
            env["CS_ICP_F16"] = "0"
        path = str(tmp_path / ("out_%s.npz" % setting))
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_gicp", path], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[setting] = dict(np.load(path))
    a, b = res["default"], res["0"]
    assert a.keys() == b.keys()
    here = _run_mixed(gpu)
    for k in a:
        if k != "stats":
            assert _same(a[k], b[k]) and _same(a[k], here[k]), k
    assert a["stats"][0] > 0 and a["stats"][1] < a["stats"][0] and b["stats"].tolist() == [0, 0]


def test_out_of_f16_range_takes_the_exact_kernel(gpu, monkeypatch):
    from corsair_amd import backend as B

    src, snrm, tgt, tnrm, T0 = _problem(1)
    tgt = tgt + np.float32([70.0, 0.0, 0.0])        # a coordinate of 70
    T0 = T0.copy()
    T0[0, 3] += 70.0
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _one(gpu, src, snrm, tgt, tnrm, T0, MAX_DIST, 2)
    answered, redone = B.icp_stats(reset=True)
    _check(got, [ref.icp(src, snrm, tgt, tnrm, T0, MAX_DIST, 2)], "coordinate 70")
    assert got["iters"][0] >= 1 and answered == redone == 2 * (got["iters"][0] + 1)       # two workgroups per round


def test_edge_shapes(gpu):
    src, snrm, tgt, tnrm, T0 = _problem(1)
    s, sn, t, tn = src[:40], snrm[:40], tgt[-300:], tnrm[-300:]
    T3 = np.stack([T0, T0, T0])
    soff, toff = [0, 0, 40], [0, 0, 300]
    want = [ref.icp(s[:0], sn[:0], t, tn, T0, MAX_DIST, 3), ref.icp(s, sn, t[:0], tn[:0], T0, MAX_DIST, 3),
            ref.icp(s, sn, t, tn, T0, MAX_DIST, 3)]
    got = _run(gpu, s, sn, soff, t, tn, toff, [0, 1, 1], [1, 0, 1], T3, MAX_DIST, 3)
    _check(got, want, "empty")
    for p in (0, 1):
        assert got["fitness"][p] == 0.0 and got["rmse"][p] == 0.0 and got["mrmse"][p] == 0.0 and got["iters"][p] == 0
        assert _same(got["T"][p], T0.reshape(16).astype(np.float64))
    none = _run(gpu, s, sn, soff, t, tn, toff, [], [], T3[:0], MAX_DIST, 3)
    assert none["T"].shape == (0, 16) and none["corr"].shape == (0,) and none["mrmse"].shape == (0,)
    src, snrm, tgt, tnrm, T0 = _problem(0)
    for n in (5, 6, 40):
        _check(_one(gpu, src[:n], snrm[:n], tgt, tnrm, T0, MAX_DIST, 30), [ref.icp(src[:n], snrm[:n], tgt, tnrm, T0, MAX_DIST, 30)],
               "%d sources" % n)
    five = _one(gpu, src[:5], snrm[:5], tgt, tnrm, T0, MAX_DIST, 30)
    assert five["ncorr"][0] == 5 and five["iters"][0] == 0 and _same(five["T32"][0], T0.reshape(16))


def test_bad_normals_on_both_sides(gpu):
    src, snrm, tgt, tnrm, T0 = _problem(1)
    bs, bt = snrm.copy(), tnrm.copy()
    bs[::5], bs[1::5], bs[2::5] = 0.0, np.nan, bs[2::5] * np.float32(-40.0)
    bt[::7], bt[1::7], bt[2::7] = np.nan, 0.0, bt[2::7] * np.float32(1e3)
    bt[3::7, 0] = np.inf
    want = ref.icp(src, bs, tgt, bt, T0, MAX_DIST, 3)
    got = _one(gpu, src, bs, tgt, bt, T0, MAX_DIST, 3)
    _check(got, [want], "bad normals")
    assert np.all(np.isfinite(got["T"])) and got["iters"][0] == 3
    # every normal bad: every pair is weighted by I / 2 (the sums keep epsilon's scales, so the bits are not epsilon = 1's)
    zero, nan = np.zeros_like(snrm), np.full_like(tnrm, np.nan)
    _check(_one(gpu, src, zero, tgt, nan, T0, MAX_DIST, 3), [ref.icp(src, zero, tgt, nan, T0, MAX_DIST, 3)], "all bad")


@pytest.mark.parametrize("epsilon", (2.0 ** -10, 1.0))
def test_epsilon_at_both_ends(gpu, epsilon):
    src, snrm, tgt, tnrm, T0 = _problem(1)
    want = ref.icp(src, snrm, tgt, tnrm, T0, MAX_DIST, 3, epsilon=epsilon)
    _check(_one(gpu, src, snrm, tgt, tnrm, T0, MAX_DIST, 3, epsilon), [want], "epsilon %g" % epsilon)
    assert want["iters"] == 3 and want["mrmse"] > 0


def test_similarity_start(gpu):
    src, snrm, tgt, tnrm, T0 = _problem(1)
    T0 = T0.copy()
    T0[:3, :3] *= np.float32(1.1)                   # the source covariance is rotated, not scaled: m is normalised
    src = (src / np.float32(1.1)).astype(np.float32)
    want = ref.icp(src, snrm, tgt, tnrm, T0, MAX_DIST, 3)
    _check(_one(gpu, src, snrm, tgt, tnrm, T0, MAX_DIST, 3), [want], "scale 1.1")
    assert want["iters"] >= 1 and want["ncorr"] > 100


def test_refused_arguments(gpu):
    from corsair_amd import _lib, backend as B

    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32, device=gpu)
    out = torch.zeros(64, dtype=torch.float64, device=gpu)
    i64, i32 = ctypes.c_int64 * 2, ctypes.c_int32 * 1
    at = lambda k: ctypes.c_void_p(out.data_ptr() + 8 * k)
    b = ctypes.c_void_p(buf.data_ptr())

    def call(snrm=b, tnrm=b, soff=i64(0, 4), max_dist=0.1, max_iter=3, T=at(0), eps=1e-3, mrmse=at(20)):
        return lib.cs_icp_gicp_batch(b, snrm, soff, b, tnrm, i64(0, 4), i32(0), i32(0), 1, b, max_dist, max_iter, 1e-6, 1e-6,
                                     eps, T, None, at(16), at(17), mrmse, at(18), at(19), None, None)

    INVALID, UNSUPPORTED = -1, -5
    assert call() == 0 and call(mrmse=None) == 0 and call(eps=1.0) == 0 and call(eps=2.0 ** -10) == 0
    assert call(snrm=None) == INVALID and b"source normal" in lib.cs_last_error()
    assert call(tnrm=None) == INVALID and b"target normal" in lib.cs_last_error()
    assert call(snrm=None, soff=i64(0, 0)) == 0                          # no source row: the array is not needed
    for eps in (0.0, 2.0 ** -11, 1.0000001, -1e-3, float("nan"), float("inf")):
        assert call(eps=eps) == INVALID and b"epsilon" in lib.cs_last_error(), eps
    assert call(soff=None) == INVALID and call(max_dist=0.0) == INVALID and call(T=None) == INVALID
    assert call(max_iter=1001) == UNSUPPORTED and call(soff=i64(0, 2 ** 31)) == UNSUPPORTED
    x = torch.zeros((4, 3), device=gpu)
    eye = torch.eye(4, device=gpu)[None]
    with pytest.raises(ValueError, match="src_normals"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, tgt_normals=x, estimation="gicp")
    with pytest.raises(ValueError, match="src_normals"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, tgt_normals=x, estimation="gicp", src_normals=x[:3])
    with pytest.raises(ValueError, match="gicp_epsilon"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, tgt_normals=x, estimation="gicp", src_normals=x, gicp_epsilon=0.0)
    with pytest.raises(ValueError, match="estimation"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], eye, 0.1, 1, tgt_normals=x, estimation="plane2plane", src_normals=x)
    torch.cuda.synchronize()


def test_plane_and_point_calls_are_unchanged(gpu):
    """cs_icp_plane_batch and cs_icp_batch on the same batch, before and after a GICP call, against their own
    restatements."""
    c = _mixed()
    plane_want = icp_plane_ref.icp_batch(c["src"], c["soff"], c["tgt"], c["tnrm"], c["toff"], c["sseg"], c["tseg"], c["T0"],
                                         MAX_DIST, 2)
    point_want = icp_ref.icp_batch(c["src"], c["soff"], c["tgt"], c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST, 2)
    for turn in range(2):
        pt._check(_run_mixed(gpu, 2, estimation="plane"), plane_want, "plane, turn %d" % turn)
        pt._check(_run_mixed(gpu, 2, estimation="point"), point_want, "point, turn %d" % turn)
        gicp = _run_mixed(gpu, 1)
    assert any(not _same(gicp["T"][p], np.asarray(plane_want[p]["T"])) for p in range(3))      # another estimation


if __name__ == "__main__":
    from corsair_amd import backend as _B

    _B.icp_stats(reset=True)
    _out = _run_mixed(torch.device("cuda:0"))
    _out["stats"] = np.array(_B.icp_stats(), np.int64)
    np.savez(sys.argv[1], **_out)
