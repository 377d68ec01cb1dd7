"""cs_estimate_normals on the cell grid: segments of 1025 rows or more are ranked in the 27 cells around each
row, a list is accepted only with the voucher of normals.hip, everything else is recomputed by the exhaustive scan -- and
every normal is BIT-EQUAL to tests/normals_ref.py and to the CS_NORMALS_GRID=0 path."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import normals_ref as ref
from tests import test_gpu_normals as knn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_MIN = 1025        # the smallest segment that may take the grid path (NRM_KNN_GRID_MIN, normals.hip)
VOXEL = 0.03
_bits_equal = knn._bits_equal


def _assert_bits(got, want, what=""):
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(1))[0]
    assert not len(bad), (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


def _voxelised(dev, cloud_ids):
    """synth.make_cloud(c, 15000)[:10000] voxelised at 0.03, packed: (f32 [n,3] host, offsets)."""
    from corsair_amd import backend as B, synth

    clouds = [synth.make_cloud(c, 15000)[:10000] for c in cloud_ids]
    xyz = torch.from_numpy(np.concatenate(clouds)).to(dev)
    keep, _, off = B.voxelize(xyz, (np.arange(len(clouds) + 1) * 10000).tolist(), VOXEL)
    return xyz[keep].cpu().numpy(), [int(o) for o in off]


def _run_with_stats(dev, xyz, off, k):
    """(normals, (rows answered by the grid, of those recomputed)); CS_NORMALS_STATS must be set."""
    from corsair_amd import backend as B

    B.normals_stats(reset=True)
    got = knn._run(dev, xyz, off, k)
    return got, B.normals_stats(reset=True)


def test_voxelised_cloud_matches_reference(gpu, monkeypatch):
    monkeypatch.setenv("CS_NORMALS_STATS", "1")
    xyz, off = _voxelised(gpu, [0])
    assert off == [0, 5176]
    got, (answered, redone) = _run_with_stats(gpu, xyz, off, 16)
    print("grid rows %d, recomputed %d" % (answered, redone))
    assert answered == 5176 and redone < answered            # fails if the grid never ran
    _assert_bits(got, ref.estimate_normals(xyz, off, 16))
    assert _bits_equal(knn._run(gpu, xyz, off, 16), got)     # two runs: identical bits
    monkeypatch.setenv("CS_NORMALS_GRID", "0")               # read per call
    again, stats = _run_with_stats(gpu, xyz, off, 16)
    assert stats == (0, 0) and _bits_equal(again, got)


def _run_switch_cases(dev):
    from corsair_amd import backend as B

    xyz, off = _voxelised(dev, [0, 3, 9])
    out = {"rows": np.array(off, np.int64)}
    for k in (8, 16, 32):
        B.normals_stats(reset=True)
        out["normals%d" % k] = knn._run(dev, xyz, off, k)
        out["stats%d" % k] = np.array(B.normals_stats(reset=True), np.int64)
    return out


def test_three_clouds_against_the_switch_in_child_processes(gpu, tmp_path):
    """Clouds 0, 3 and 9 in one call at k = 8, 16, 32: CS_NORMALS_GRID=0 and the default, each in a process of its own,
    give identical bits, and at most 0.10 of the grid's rows are recomputed (the bar DESIGN 12 set for a fallback share).
    Measured on an MI355X: 0, 0 and 5 of 12 816 rows (k = 8, 16, 32)."""
    res = {}
    for setting in ("default", "0"):
        env = dict(os.environ)
        env.pop("CS_NORMALS_GRID", None)
        env["CS_NORMALS_STATS"] = "1"
        if setting == "0":
            env["CS_NORMALS_GRID"] = "0"
        path = str(tmp_path / ("out_%s.npz" % setting))
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_normals_grid", path], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[setting] = dict(np.load(path))
    a, b = res["default"], res["0"]
    assert a.keys() == b.keys() and np.diff(a["rows"]).min() >= GRID_MIN
    for k in (8, 16, 32):
        assert _bits_equal(a["normals%d" % k], b["normals%d" % k]), k
        answered, redone = a["stats%d" % k].tolist()
        print("k = %d: grid rows %d, recomputed %d (%.5f)" % (k, answered, redone, redone / max(answered, 1)))
        assert answered == a["rows"][-1] and redone <= 0.10 * answered, k
        assert b["stats%d" % k].tolist() == [0, 0]


def _sphere(n, seed, radius=0.5):
    rng = np.random.default_rng(seed)
    sph = rng.standard_normal((n, 3))
    return (radius * sph / np.linalg.norm(sph, axis=1, keepdims=True)).astype(np.float32)


def test_a_cluster_the_voucher_must_refuse(gpu, monkeypatch):
    """Twelve rows 5 units from a 3000-row cluster at k = 16: their 13th to 16th neighbours lie 5 units away, outside
    any 27 cells; the voucher refuses them and the exhaustive scan answers."""
    monkeypatch.setenv("CS_NORMALS_STATS", "1")
    rng = np.random.default_rng(12)
    far = (rng.uniform(-0.03, 0.03, (12, 3)) + [5.0, 0.0, 0.0]).astype(np.float32)
    xyz = np.concatenate([_sphere(1500, 1), far[:5], _sphere(1500, 2), far[5:]])          # the twelve are not one block
    got, (answered, redone) = _run_with_stats(gpu, xyz, [0, 3012], 16)
    print("grid rows %d, recomputed %d" % (answered, redone))
    assert answered == 3012 and 12 <= redone < 3012 // 2
    _assert_bits(got, ref.estimate_normals(xyz, [0, 3012], 16))


def test_segments_that_never_reach_the_grid(gpu, monkeypatch):
    monkeypatch.setenv("CS_NORMALS_STATS", "1")
    n = 1100
    rng = np.random.default_rng(4)
    point = np.tile(np.float32([[0.3, -0.2, 0.9]]), (n, 1))            # a box of size zero
    single = np.float32([[0.1, 0.2, 0.3]])
    nan = _sphere(n, 5)
    nan[77, 1] = np.nan                                                # a box that is not finite
    inf = _sphere(n, 6)
    inf[3, 0] = np.inf
    line = np.zeros((n, 3), np.float32)                                # a box of area zero
    line[:, 0] = rng.uniform(-1, 1, n).astype(np.float32)
    flat = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), np.full((n, 1), 0.25)], 1).astype(np.float32)   # area > 0
    out_there = _sphere(n, 7) + np.float32([1.0e6, 0.0, 0.0])          # a cell index would reach the clamp
    seventy = _sphere(n, 8) + np.float32([70.0, -70.0, 0.0])
    parts = [point, single, nan, inf, line, flat, out_there, seventy]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    got, (answered, redone) = _run_with_stats(gpu, xyz, off, 8)
    print("grid rows %d, recomputed %d" % (answered, redone))
    assert answered == 2 * n                                            # the flat segment and the sphere at 70
    # the defined answers: copies of one point, a single row, the NaN and inf rows themselves
    assert np.array_equal(got[off[0]:off[1]], np.tile(np.float32([1, 0, 0]), (n, 1)))
    assert np.array_equal(got[off[1]], np.float32([0, 0, 1]))
    assert np.array_equal(got[off[2] + 77], np.float32([0, 0, 1])) and np.array_equal(got[off[3] + 3], np.float32([0, 0, 1]))
    assert np.array_equal(got[off[5]:off[6]], np.tile(np.float32([0, 0, 1]), (n, 1)))       # rows of the plane z = 0.25
    want = ref.estimate_normals(xyz[off[1]:], [o - off[1] for o in off[1:]], 8)
    _assert_bits(got[off[1]:], want)
    small = ref.estimate_normals(point[:40], [0, 40], 8)
    assert np.array_equal(small, got[:40])


def test_segments_around_the_grid_threshold(gpu, monkeypatch):
    monkeypatch.setenv("CS_NORMALS_STATS", "1")
    from corsair_amd import synth

    cloud = synth.make_cloud(3, 4000)
    rng = np.random.default_rng(9)
    parts = [cloud[rng.choice(len(cloud), m, replace=False)] for m in (GRID_MIN - 1, GRID_MIN)]
    xyz = np.concatenate(parts).astype(np.float32)
    off = [0, GRID_MIN - 1, 2 * GRID_MIN - 1]
    for k in (3, 32):
        got, (answered, redone) = _run_with_stats(gpu, xyz, off, k)
        print("k = %d: grid rows %d, recomputed %d" % (k, answered, redone))
        assert answered == GRID_MIN
        _assert_bits(got, ref.estimate_normals(xyz, off, k), k)
        swapped = knn._run(gpu, np.concatenate(parts[::-1]).astype(np.float32), [0, GRID_MIN, 2 * GRID_MIN - 1], k)
        assert _bits_equal(swapped[:GRID_MIN], got[GRID_MIN - 1:]) and _bits_equal(swapped[GRID_MIN:], got[:GRID_MIN - 1])


if __name__ == "__main__":
    np.savez(sys.argv[1], **_run_switch_cases(torch.device("cuda:0")))
