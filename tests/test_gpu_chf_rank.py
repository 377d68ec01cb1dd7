"""The boundaries of the f16 ranking scan (corsair_amd/csrc/chf_rank.h) through both of its callers, k_chamfer_f16 and
k_icp_f16: target segments of one row, around one 32-row tile (31, 32, 33), at the last size where every tile is evaluated and
the first where the third tile minimum matters (64, 65), around one 256-row stage (255, 256, 257), a stage that ends on a
tile boundary (288) and 513 rows, each against 1 source and against 257 (two workgroups, the second with one source).  All
problems are one batch, so a segment's last stage reads on into the next problem's rows and the last one into the image's
padding.  The default path must equal the exhaustive one bit for bit -- and, since that holds as well when every workgroup
falls back, the statistics must show that the f16 kernels answered."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import rot_y_pose

pytestmark = pytest.mark.gpu
TARGETS = (1, 31, 32, 33, 64, 65, 255, 256, 257, 288, 513)
SOURCES = (1, 257)
MAX_DIST = 4.0     # beyond the diameter of the cube: every source with a target keeps its pair
MAX_ITER = 2
ICP_FIELDS = ("T", "T32", "fitness", "rmse", "iters", "ncorr", "corr")


@pytest.fixture(scope="module")
def batch():
    """Problem p = (TARGETS[p // 2] targets, SOURCES[p % 2] sources), uniform in [-0.8, 0.8]^3, under a small pose of its own."""
    rng = np.random.default_rng(20)
    shapes = [(tn, sn) for tn in TARGETS for sn in SOURCES]
    c = {"shapes": shapes,
         "src": rng.uniform(-0.8, 0.8, (sum(s for _, s in shapes), 3)).astype(np.float32),
         "tgt": rng.uniform(-0.8, 0.8, (sum(t for t, _ in shapes), 3)).astype(np.float32),
         "soff": np.concatenate([[0], np.cumsum([s for _, s in shapes])]).tolist(),
         "toff": np.concatenate([[0], np.cumsum([t for t, _ in shapes])]).tolist(),
         "T": np.stack([rot_y_pose(2.0 + p) for p in range(len(shapes))]).astype(np.float32)}
    nrm = rng.standard_normal(c["tgt"].shape)
    c["tnrm"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return c


def _chamfer(dev, c, probs, hausdorff):
    from corsair_amd import backend as B

    fn = B.hausdorff_1dir if hausdorff else B.chamfer_1dir
    to = lambda a: torch.from_numpy(a).to(dev)
    return fn(to(c["src"]), c["soff"], to(c["tgt"]), c["toff"], probs, probs, to(c["T"][probs])).cpu().numpy()


def _icp(dev, c, probs, plane):
    from corsair_amd import backend as B

    to = lambda a: torch.from_numpy(a).to(dev)
    r = B.icp_batch(to(c["src"]), c["soff"], to(c["tgt"]), c["toff"], probs, probs, to(c["T"][probs]), MAX_DIST, MAX_ITER,
                    return_corr=True, tgt_normals=to(c["tnrm"]) if plane else None)
    return {k: getattr(r, k).cpu().numpy() for k in ICP_FIELDS}


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("hausdorff", (False, True), ids=("chamfer", "hausdorff"))
def test_chamfer_default_equals_exhaustive(gpu, batch, monkeypatch, hausdorff):
    from corsair_amd import _lib

    probs = list(range(len(batch["shapes"])))
    small = [p for p in probs if batch["shapes"][p][0] <= 64]
    lib, st = _lib.load(), (ctypes.c_uint64 * 2)()
    monkeypatch.delenv("CS_CHAMFER_F16", raising=False)
    monkeypatch.setenv("CS_CHAMFER_MFMA", "0")
    want = _chamfer(gpu, batch, probs, hausdorff)
    monkeypatch.delenv("CS_CHAMFER_MFMA")
    monkeypatch.setenv("CS_CHAMFER_STATS", "1")
    lib.cs_chamfer_f16_stats(st, 1)
    got = _chamfer(gpu, batch, probs, hausdorff)
    lib.cs_chamfer_f16_stats(st, 1)
    answered, redone = int(st[0]), int(st[1])
    got_small = _chamfer(gpu, batch, small, hausdorff)
    lib.cs_chamfer_f16_stats(st, 1)
    print("chamfer f16 stats, hausdorff=%d: batch %d answered, %d recomputed; <= 64 targets %d answered, %d recomputed"
          % (hausdorff, answered, redone, int(st[0]), int(st[1])))
    assert np.isfinite(want).all() and (want > 0).all()
    assert np.array_equal(got, want)
    assert np.array_equal(got_small, want[small])
    # a workgroup per 256 sources: 1 or 2 per problem
    assert answered == sum(-(-sn // 256) for _, sn in batch["shapes"])
    assert redone < answered, (answered, redone)
    # at most two tiles: both get evaluated and the bound of the unevaluated rows is +inf, so every workgroup is vouched for
    assert (int(st[0]), int(st[1])) == (sum(-(-batch["shapes"][p][1] // 256) for p in small), 0)


@pytest.mark.parametrize("plane", (False, True), ids=("point", "plane"))
def test_icp_default_equals_exhaustive(gpu, batch, monkeypatch, plane):
    from corsair_amd import backend as B

    probs = list(range(len(batch["shapes"])))
    small = [p for p in probs if batch["shapes"][p][0] <= 64]
    monkeypatch.setenv("CS_ICP_F16", "0")
    want = _icp(gpu, batch, probs, plane)
    want_small = _icp(gpu, batch, small, plane)
    monkeypatch.delenv("CS_ICP_F16")
    monkeypatch.setenv("CS_ICP_STATS", "1")
    B.icp_stats(reset=True)
    got = _icp(gpu, batch, probs, plane)
    answered, redone = B.icp_stats(reset=True)
    got_small = _icp(gpu, batch, small, plane)
    answered_small, redone_small = B.icp_stats(reset=True)
    print("icp f16 stats, plane=%d: batch %d answered, %d recomputed; <= 64 targets %d answered, %d recomputed"
          % (plane, answered, redone, answered_small, redone_small))
    # the comparison is about real pairs (max_dist spans the cube) and real updates
    full = [p for p in probs if batch["shapes"][p][0] >= 31 and batch["shapes"][p][1] == 257]
    assert (want["ncorr"][full] > 0).all() and (want["iters"][full] >= 1).all()
    for k in ICP_FIELDS:
        assert _bits_equal(got[k], want[k]), k
        assert _bits_equal(got_small[k], want_small[k]), k
    assert 0 < answered and redone < answered, (answered, redone)
    # at most two tiles: both get evaluated and the bound of the unevaluated rows is +inf, so every workgroup is vouched for
    assert answered_small > 0 and redone_small == 0, (answered_small, redone_small)
