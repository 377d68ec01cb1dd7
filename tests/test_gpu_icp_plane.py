"""cs_icp_plane_batch on the GPU: transforms, fitness, rmse, updates, pair counts and correspondences are BIT-EQUAL to
tests/icp_plane_ref.py on both association paths, and cs_icp_batch -- run on the same problems in the same process -- is
still bit-equal to tests/icp_ref.py.

`python -m tests.test_gpu_icp_plane OUT.npz` runs the mixed batch in a process of its own (the switch test)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import icp_plane_ref as ref
from tests import icp_ref
from tests import test_gpu_icp as pt          # the point test's mixed batch (sources of 1-600 rows, targets of 1-3 000 rows,
                                              # shared targets) and its comparison helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MAX_DIST = pt.MAX_DIST
_same = pt._same


def _np_normals(seg, k=8):
    """Unit normals of one target segment from SciPy's KD-tree and eigh: INPUT data of these tests (any f32 rows would do)."""
    from scipy.spatial import cKDTree

    seg = np.asarray(seg, np.float64)
    if len(seg) < 3:
        return np.tile(np.float32([0, 0, 1]), (len(seg), 1))
    _, idx = cKDTree(seg).query(seg, min(k, len(seg)))
    nb = seg[idx] - seg[idx].mean(1, keepdims=True)
    _, v = np.linalg.eigh(np.einsum("nka,nkb->nab", nb, nb))
    return v[:, :, 0].astype(np.float32)


@functools.lru_cache(maxsize=None)
def _mixed():
    c = dict(pt._mixed())
    c["nrm"] = np.concatenate([_np_normals(c["tgt"][c["toff"][t]:c["toff"][t + 1]]) for t in range(len(c["toff"]) - 1)])
    return c


@functools.lru_cache(maxsize=None)
def _mixed_ref(max_iter=1):
    c = _mixed()
    return ref.icp_batch(c["src"], c["soff"], c["tgt"], c["nrm"], c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST, max_iter)


def _run(dev, src, soff, tgt, nrm, toff, sseg, tseg, T0, max_dist, max_iter):
    from corsair_amd import backend as B

    to = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shape)).to(dev)
    r = B.icp_batch(to(src, (-1, 3)), soff, to(tgt, (-1, 3)), toff, sseg, tseg, to(T0, (-1, 4, 4)), max_dist, max_iter,
                    return_corr=True, tgt_normals=None if nrm is None else to(nrm, (-1, 3)))
    return {"T": r.T.cpu().numpy().reshape(-1, 16), "T32": r.T32.cpu().numpy().reshape(-1, 16),
            "fitness": r.fitness.cpu().numpy(), "rmse": r.rmse.cpu().numpy(), "iters": r.iters.cpu().numpy(),
            "ncorr": r.ncorr.cpu().numpy(), "corr": r.corr.cpu().numpy(), "corr_off": np.asarray(r.corr_off, np.int64)}


def _run_mixed(dev, max_iter=1, plane=True):
    c = _mixed()
    return _run(dev, c["src"], c["soff"], c["tgt"], c["nrm"] if plane else None, c["toff"], c["sseg"], c["tseg"], c["T0"],
                MAX_DIST, max_iter)


def _one(dev, src, tgt, nrm, T0, max_dist, max_iter):
    return _run(dev, src, [0, len(src)], tgt, nrm, [0, len(tgt)], [0], [0], np.asarray(T0, np.float32).reshape(1, 4, 4),
                max_dist, max_iter)


_check = pt._check


def test_mixed_batch_matches_reference_and_the_point_path_is_unchanged(gpu):
    want = _mixed_ref()
    got = _run_mixed(gpu)
    _check(got, want, "mixed plane")
    assert max(w["iters"] for w in want) == 1 and any(w["ncorr"] < 6 for w in want)     # both kinds are in the batch
    again = _run_mixed(gpu)
    assert all(_same(got[k], again[k]) for k in got)                                    # two runs: identical bits
    # the same problems through cs_icp_batch, in this process, before and after a plane call
    point_want = pt._mixed_ref()
    _check(_run_mixed(gpu, 2, plane=False), point_want, "mixed point")
    _run_mixed(gpu)
    _check(_run_mixed(gpu, 2, plane=False), point_want, "mixed point again")
    assert any(not _same(got["T"][p], np.asarray(point_want[p]["T"])) for p in range(len(want)))   # two estimations


def _problem(p):
    c = _mixed()
    s, t = pt.PROBLEMS[p]
    return (c["src"][c["soff"][s]:c["soff"][s + 1]], c["tgt"][c["toff"][t]:c["toff"][t + 1]],
            c["nrm"][c["toff"][t]:c["toff"][t + 1]], c["T0"][p])


def test_max_iter_0_1_30_alone_and_permuted(gpu):
    src, tgt, nrm, T0 = _problem(6)                 # 600 sources against 3 000 targets
    for max_iter in (0, 30):
        want = ref.icp(src, tgt, nrm, T0, MAX_DIST, max_iter)
        got = _one(gpu, src, tgt, nrm, T0, MAX_DIST, max_iter)
        _check(got, [want], "max_iter %d" % max_iter)
        assert want["iters"] <= max_iter
    assert 1 < want["iters"] < 30                   # the 30-update run stopped on the convergence rule
    # alone = in the batch; a permutation of the source rows changes nothing but the order of the correspondences
    alone = _one(gpu, src, tgt, nrm, T0, MAX_DIST, 1)
    _check(alone, [_mixed_ref()[6]], "alone")
    perm = np.random.default_rng(5).permutation(len(src))
    shuf = _one(gpu, src[perm], tgt, nrm, T0, MAX_DIST, 1)
    for k in ("T", "T32", "fitness", "rmse", "iters", "ncorr"):
        assert _same(shuf[k], alone[k]), k
    assert np.array_equal(shuf["corr"], alone["corr"][perm])


def test_max_dist_edges_and_fewer_than_six_pairs(gpu):
    eye = np.eye(4, dtype=np.float32)
    s1, t1, n1 = np.float32([[2.0, 0.0, 0.0]]), np.float32([[2.25, 0.0, 0.0]]), np.float32([[1.0, 0.0, 0.0]])
    for md, n in ((0.25, 0), (0.2500001, 1)):       # the threshold is strict
        got = _one(gpu, s1, t1, n1, eye, md, 0)
        _check(got, [ref.icp(s1, t1, n1, eye, md, 0)], "edge")
        assert got["ncorr"][0] == n
    src, tgt, nrm, T0 = _problem(6)
    got = _one(gpu, src, tgt, nrm, T0, 1e-4, 30)    # below every distance: stops at once with T = T0
    _check(got, [ref.icp(src, tgt, nrm, T0, 1e-4, 30)], "no pair")
    assert got["ncorr"][0] == 0 and got["iters"][0] == 0 and (got["corr"] == -1).all()
    for n in (5, 6, 40):
        want = ref.icp(src[:n], tgt, nrm, T0, MAX_DIST, 30)
        got = _one(gpu, src[:n], tgt, nrm, T0, MAX_DIST, 30)
        _check(got, [want], "%d sources" % n)
    five = _one(gpu, src[:5], tgt, nrm, T0, MAX_DIST, 30)
    assert five["ncorr"][0] == 5 and five["iters"][0] == 0 and _same(five["T32"][0], T0.reshape(16))
    assert got["iters"][0] >= 1


def test_empty_segments_and_no_problem(gpu):
    c = _mixed()
    src, tgt, nrm = c["src"][:40], c["tgt"][-300:], c["nrm"][-300:]
    T0 = c["T0"][:3]
    soff, toff = [0, 0, 40], [0, 0, 300]
    want = [ref.icp(src[:0], tgt, nrm, T0[0], MAX_DIST, 3), ref.icp(src, tgt[:0], nrm[:0], T0[1], MAX_DIST, 3),
            ref.icp(src, tgt, nrm, T0[2], MAX_DIST, 3)]
    got = _run(gpu, src, soff, tgt, nrm, toff, [0, 1, 1], [1, 0, 1], T0, MAX_DIST, 3)
    _check(got, want, "empty")
    for p in (0, 1):
        assert got["fitness"][p] == 0.0 and got["rmse"][p] == 0.0 and got["iters"][p] == 0
        assert _same(got["T"][p], T0[p].reshape(16).astype(np.float64))
    none = _run(gpu, src, soff, tgt, nrm, toff, [], [], T0[:0], MAX_DIST, 3)
    assert none["T"].shape == (0, 16) and none["corr"].shape == (0,)


def test_exact_plane_stops_with_the_initial_transform(gpu):
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2) * 0.05
    tgt = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(tgt), 1))
    src = (tgt[10:100] + np.float32([0.004, -0.003, 0.01])).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)
    want = ref.icp(src, tgt, nrm, eye, 0.1, 30)
    got = _one(gpu, src, tgt, nrm, eye, 0.1, 30)
    _check(got, [want], "singular plane")
    assert got["iters"][0] == 0 and got["ncorr"][0] == len(src) and _same(got["T32"][0], eye.reshape(16))
    assert got["rmse"][0] > 0.01


def test_non_unit_and_non_finite_normals(gpu):
    src, tgt, nrm, T0 = _problem(7)                 # 257 sources against 3 000 targets
    bad = nrm.copy()
    bad[::7] = np.nan
    for name, n in (("x 1e3", nrm * np.float32(1e3)), ("x 0.5", nrm * np.float32(0.5)), ("NaN rows", bad)):
        want = ref.icp(src, tgt, n, T0, MAX_DIST, 3)
        got = _one(gpu, src, tgt, n, T0, MAX_DIST, 3)
        _check(got, [want], name)
        assert np.all(np.isfinite(got["T"]))


def test_out_of_f16_range_takes_the_exact_kernel(gpu, monkeypatch):
    from corsair_amd import backend as B

    src, tgt, nrm, T0 = _problem(3)
    tgt = tgt + np.float32([70.0, 0.0, 0.0])        # a coordinate of 70
    T0 = T0.copy()
    T0[0, 3] += 70.0
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _one(gpu, src, tgt, nrm, T0, MAX_DIST, 2)
    answered, redone = B.icp_stats(reset=True)
    _check(got, [ref.icp(src, tgt, nrm, T0, MAX_DIST, 2)], "coordinate 70")
    assert got["iters"][0] >= 1 and answered == redone == got["iters"][0] + 1


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
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_icp_plane", path], cwd=ROOT, env=env, capture_output=True,
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


def test_refused_arguments(gpu):
    from corsair_amd import _lib, backend as B

    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32, device=gpu)
    out = torch.zeros(64, dtype=torch.float64, device=gpu)
    i64, i32 = ctypes.c_int64 * 2, ctypes.c_int32 * 1
    at = lambda k: ctypes.c_void_p(out.data_ptr() + 8 * k)
    b = ctypes.c_void_p(buf.data_ptr())

    def call(nrm=b, soff=i64(0, 4), max_dist=0.1, max_iter=3, T=at(0)):
        return lib.cs_icp_plane_batch(b, soff, b, nrm, i64(0, 4), i32(0), i32(0), 1, b, max_dist, max_iter, 1e-6, 1e-6, T,
                                      None, at(16), at(17), at(18), at(19), None, None)

    INVALID, UNSUPPORTED = -1, -5
    assert call() == 0
    assert call(nrm=None) == INVALID and b"normal" in lib.cs_last_error()
    assert call(soff=None) == INVALID and call(max_dist=0.0) == INVALID and call(T=None) == INVALID
    assert call(max_iter=1001) == UNSUPPORTED and call(soff=i64(0, 2 ** 31)) == UNSUPPORTED
    x = torch.zeros((4, 3), device=gpu)
    with pytest.raises(ValueError, match="tgt_normals"):
        B.icp_batch(x, [0, 4], x, [0, 4], [0], [0], torch.eye(4, device=gpu)[None], 0.1, 1, tgt_normals=x[:3])
    torch.cuda.synchronize()


if __name__ == "__main__":
    from corsair_amd import backend as _B

    _B.icp_stats(reset=True)
    _out = _run_mixed(torch.device("cuda:0"))
    _out["stats"] = np.array(_B.icp_stats(), np.int64)
    np.savez(sys.argv[1], **_out)
