"""The six ICP estimations through the ONE host driver (corsair_amd/csrc/icp.hip), interleaved in one process:
every call is BIT-EQUAL to its own restatement (tests/icp_ref.py, icp_plane_ref.py, icp_robust_ref.py, icp_scale_ref.py,
gicp_ref.py) and to the same call made earlier, whatever estimation ran in between -- nothing of a call (the number of sums,
the plane frame, the scale or the Mahalanobis output) survives into the next one.  The statistics counters sit behind the
sums of every layout, and the launch functions take the exhaustive path alone under CS_ICP_F16=0.

`python -m tests.test_gpu_icp_units OUT.npz` makes the first six calls in a process of its own (the switch test)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gicp_ref
from tests import icp_plane_ref
from tests import icp_ref
from tests import icp_robust_ref
from tests import icp_scale_ref
from tests import test_gpu_icp as pt
from tests.test_icp_cpu import _fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MAX_DIST = 0.1
MAX_ITER = 3
EPSILON = 1e-3
HUBER_SCALE = 0.02
_same = pt._same
# (seed, sources, targets): 257 sources are two association workgroups, the second with ONE source, and 513 targets two LDS
# stages of the exhaustive kernel, the second with one row; the other problem is small on both sides
SHAPES = ((2, 257, 513), (3, 33, 40))
ORDER = ("point", "gicp", "plane", "point_s", "robust", "plane_s", "point", "gicp")
EXTRA = {"gicp": "mrmse", "robust": "wfitness", "point_s": "scale", "plane_s": "scale"}


@functools.lru_cache(maxsize=None)
def _batch(dev):
    """Both problems in one batch; the normals of both sides come from backend.estimate_normals and are INPUT data of the
    calls and of the restatements alike."""
    from corsair_amd import backend as B

    parts = [_fixture(*s) for s in SHAPES]
    c = {"src": np.concatenate([p[0] for p in parts]).astype(np.float32),
         "tgt": np.concatenate([p[1] for p in parts]).astype(np.float32),
         "soff": np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).tolist(),
         "toff": np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).tolist(),
         "sseg": [0, 1], "tseg": [0, 1], "T0": np.stack([p[2] for p in parts]).astype(np.float32)}
    c["snrm"] = B.estimate_normals(torch.from_numpy(c["src"]).to(dev), c["soff"]).cpu().numpy()
    c["tnrm"] = B.estimate_normals(torch.from_numpy(c["tgt"]).to(dev), c["toff"]).cpu().numpy()
    assert c["snrm"].shape == c["src"].shape and c["tnrm"].shape == c["tgt"].shape
    return c


@functools.lru_cache(maxsize=None)
def _want(dev, name):
    """The restatement's results for estimation `name` on the batch, computed once."""
    c = _batch(dev)
    tail = (c["toff"], c["sseg"], c["tseg"], c["T0"], MAX_DIST, MAX_ITER)
    if name == "point":
        return icp_ref.icp_batch(c["src"], c["soff"], c["tgt"], *tail)
    if name == "plane":
        return icp_plane_ref.icp_batch(c["src"], c["soff"], c["tgt"], c["tnrm"], *tail)
    if name == "robust":
        return icp_robust_ref.icp_batch(c["src"], c["soff"], c["tgt"], c["tnrm"], *tail, kernel=icp_robust_ref.HUBER,
                                        kernel_scale=HUBER_SCALE)
    if name == "point_s":
        return icp_scale_ref.icp_batch(c["src"], c["soff"], c["tgt"], None, *tail)
    if name == "plane_s":
        return icp_scale_ref.icp_batch(c["src"], c["soff"], c["tgt"], c["tnrm"], *tail)
    assert name == "gicp"
    return gicp_ref.icp_batch(c["src"], c["snrm"], c["soff"], c["tgt"], c["tnrm"], *tail, epsilon=EPSILON)


def _call(dev, name, sseg=None, tseg=None, max_iter=MAX_ITER, **kw):
    """One backend.icp_batch call of estimation `name`: every output tensor, as NumPy arrays."""
    from corsair_amd import backend as B

    c = _batch(dev)
    to = lambda a: torch.from_numpy(a).to(dev)
    sseg, tseg = c["sseg"] if sseg is None else sseg, c["tseg"] if tseg is None else tseg
    if name != "point" and name != "point_s":
        kw["tgt_normals"] = to(c["tnrm"])
    if name == "robust":
        kw.update(kernel="huber", kernel_scale=HUBER_SCALE)
    if name in ("point_s", "plane_s"):
        kw["with_scaling"] = True
    if name == "gicp":
        kw.update(estimation="gicp", src_normals=to(c["snrm"]), gicp_epsilon=EPSILON)
    r = B.icp_batch(to(c["src"]), c["soff"], to(c["tgt"]), c["toff"], sseg, tseg, to(c["T0"][:len(sseg)]), MAX_DIST, max_iter,
                    return_corr=True, **kw)
    out = {"T": r.T.cpu().numpy().reshape(-1, 16), "T32": r.T32.cpu().numpy().reshape(-1, 16),
           "fitness": r.fitness.cpu().numpy(), "rmse": r.rmse.cpu().numpy(), "iters": r.iters.cpu().numpy(),
           "ncorr": r.ncorr.cpu().numpy(), "corr": r.corr.cpu().numpy(), "corr_off": np.asarray(r.corr_off, np.int64)}
    for k in ("wfitness", "scale", "mrmse"):
        v = getattr(r, k, None)
        assert (v is not None) == (EXTRA.get(name) == k), (name, k)     # an output of a neighbour does not appear
        if v is not None:
            out[k] = v.cpu().numpy()
    return out


def _check(got, want, name, what):
    pt._check(got, want, what)
    k = EXTRA.get(name)
    for p, w in enumerate(want):
        if k:
            assert _same(got[k][p], np.float64(w[k])), (what, p, got[k][p], w[k])


def _first_six(dev):
    return [_call(dev, name) for name in ORDER[:6]]


def test_interleaved_estimations(gpu, monkeypatch):
    monkeypatch.delenv("CS_ICP_F16", raising=False)
    first = {}
    for i, name in enumerate(ORDER):
        got = _call(gpu, name)
        what = "call %d (%s)" % (i, name)
        _check(got, _want(gpu, name), name, what)
        if name in first:
            assert got.keys() == first[name].keys() and all(_same(got[k], first[name][k]) for k in got), what
        first.setdefault(name, got)
    assert len(first) == 6
    # the calls did work: every estimation updated both problems (the restatements: 3 and 2 or 3 updates)
    for name, got in first.items():
        assert (got["iters"] >= 1).all() and (got["ncorr"] > 0).all(), name


@pytest.mark.parametrize("name", ORDER[:6])
def test_statistics_sit_behind_every_sum_layout(gpu, monkeypatch, name):
    """The two counters of CS_ICP_STATS are allocated behind n_prob * NS sums, NS = 17 / 30 / 29 / 18 / 30 / 37: three rounds
    of the two workgroups of the 257-source problem, counted exactly, with an offset from a neighbour's NS they would be a
    sum's bits or stay zero."""
    from corsair_amd import backend as B

    monkeypatch.delenv("CS_ICP_F16", raising=False)
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _call(gpu, name, sseg=[0], tseg=[0], max_iter=2, relative_fitness=0.0, relative_rmse=0.0)
    answered, redone = B.icp_stats(reset=True)
    assert got["iters"].tolist() == [2]
    assert answered == 3 * 2 and redone <= answered


def test_exhaustive_path_in_a_child_process(gpu, tmp_path, monkeypatch):
    """CS_ICP_F16=0 in a process of its own: the launch functions enqueue k_icp_exact alone, and the bits are this process's."""
    monkeypatch.delenv("CS_ICP_F16", raising=False)
    env = dict(os.environ)
    env["CS_ICP_F16"] = "0"
    env["CS_ICP_STATS"] = "1"
    path = str(tmp_path / "exact.npz")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_icp_units", path], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    child = dict(np.load(path))
    assert child.pop("stats").tolist() == [0, 0]                    # the f16 kernel did not run there
    here = {"%d_%s_%s" % (i, name, k): v for i, (name, got) in enumerate(zip(ORDER[:6], _first_six(gpu))) for k, v in got.items()}
    assert child.keys() == here.keys()
    for k in here:
        assert _same(child[k], here[k]), k


if __name__ == "__main__":
    from corsair_amd import backend as _B

    _dev = torch.device("cuda:0")
    _B.icp_stats(reset=True)
    _out = {"%d_%s_%s" % (i, name, k): v for i, (name, got) in enumerate(zip(ORDER[:6], _first_six(_dev))) for k, v in got.items()}
    _out["stats"] = np.array(_B.icp_stats(), np.int64)
    np.savez(sys.argv[1], **_out)
