"""cs_estimate_normals on the GPU: every normal is BIT-EQUAL to tests/normals_ref.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import normals_ref as ref

pytestmark = pytest.mark.gpu

STAGE = 512     # segment rows per LDS stage of k_normals
KS = (3, 8, 16, 17, 32)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _run(dev, xyz, off, k):
    from corsair_amd import backend as B

    x = torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)).to(dev)
    return B.estimate_normals(x, off, k).cpu().numpy()


def _sizes(k):
    """0, 1, 2, 3, k-1, k, k+1, one more than the LDS stage holds, in one call (300 too for k = 16); an empty segment in
    the middle and at the end."""
    return [0, 1, 2, 3, k - 1, 0, k, k + 1] + ([300] if k == 16 else []) + [STAGE + 1, 0]


@functools.lru_cache(maxsize=None)
def _mixed(k):
    from corsair_amd import synth

    rng = np.random.default_rng(100 + k)
    cloud = synth.make_cloud(9, 4000)
    sizes = _sizes(k)
    xyz = np.concatenate([cloud[rng.choice(len(cloud), n, replace=False)] for n in sizes]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return xyz, off, ref.estimate_normals(xyz, off, k)


@pytest.mark.parametrize("k", KS)
def test_mixed_segments_match_reference(gpu, k):
    xyz, off, want = _mixed(k)
    got = _run(gpu, xyz, off, k)
    bad = np.nonzero((got.view(np.int32) != want.view(np.int32)).any(1))[0]
    assert not len(bad), (k, bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-6
    # two runs: identical bits
    assert _bits_equal(_run(gpu, xyz, off, k), got)


def test_batch_neighbours_do_not_matter(gpu):
    xyz, off, want = _mixed(16)
    for s in (4, 8, 9):                       # k - 1 rows, 300 rows, STAGE + 1 rows
        seg = xyz[off[s]:off[s + 1]]
        alone = _run(gpu, seg, [0, len(seg)], 16)
        assert _bits_equal(alone, want[off[s]:off[s + 1]]), s
    # the same segments in another order, with other neighbours
    order = [9, 1, 8, 4, 3]
    sh = np.concatenate([xyz[off[s]:off[s + 1]] for s in order])
    soff = np.concatenate([[0], np.cumsum([off[s + 1] - off[s] for s in order])]).tolist()
    got = _run(gpu, sh, soff, 16)
    for i, s in enumerate(order):
        assert _bits_equal(got[soff[i]:soff[i + 1]], want[off[s]:off[s + 1]]), s


def _ties_case():
    g = np.stack(np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(6)
    cont = rng.uniform(-1, 1, (90, 3)).astype(np.float32)
    dup = np.concatenate([cont, cont[:40], cont[10:30]])            # duplicated rows: zero distances that tie
    return np.concatenate([g, dup]), [0, len(g), len(g) + len(dup)]


@pytest.mark.parametrize("k", (8, 17))
def test_integer_grid_and_duplicated_rows(gpu, k):
    xyz, off = _ties_case()
    assert _bits_equal(_run(gpu, xyz, off, k), ref.estimate_normals(xyz, off, k))


def test_exact_plane_line_nan_and_coordinate_70(gpu):
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    plane = np.concatenate([g, np.full((len(g), 1), 0.75, np.float32)], 1)
    line = np.zeros((9, 3), np.float32)
    line[:, 0] = np.arange(9) * 0.5
    rng = np.random.default_rng(3)
    sph = rng.standard_normal((200, 3))
    sph = (0.5 * sph / np.linalg.norm(sph, axis=1, keepdims=True)).astype(np.float32)
    nan = sph[:80].copy()
    nan[17, 1] = np.nan
    nan[40, 0] = np.inf
    far = sph + np.float32([70.0, -70.0, 0.0])                      # a coordinate of 70
    point = np.tile(np.float32([[0.3, -0.2, 0.9]]), (6, 1))
    parts = [plane, line, nan, far, point]
    xyz = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    got = _run(gpu, xyz, off, 8)
    assert _bits_equal(got, ref.estimate_normals(xyz, off, 8))
    # the defined answers of the header comment
    assert np.array_equal(got[off[0]:off[1]], np.tile(np.float32([0, 0, 1]), (len(plane), 1)))
    assert np.array_equal(got[off[1]:off[2]], np.tile(np.float32([0, 1, 0]), (len(line), 1)))
    assert np.array_equal(got[off[2] + 17], np.float32([0, 0, 1])) and np.array_equal(got[off[2] + 40], np.float32([0, 0, 1]))
    assert np.array_equal(got[off[4]:off[5]], np.tile(np.float32([1, 0, 0]), (6, 1)))
    # the far sphere: the normal of a sphere is radial, to the sampling density
    radial = sph / np.linalg.norm(sph, axis=1, keepdims=True)
    assert np.abs(np.abs((got[off[3]:off[4]] * radial).sum(1)) - 1).max() < 0.05


def test_refused_arguments_and_empty_calls(gpu):
    from corsair_amd import _lib, backend as B

    x = torch.zeros((10, 3), device=gpu)
    for k in (2, 33, 0, -1):
        with pytest.raises(_lib.CorsairHipError, match="k outside"):
            B.estimate_normals(x, [0, 10], k)
    with pytest.raises(ValueError):
        B.estimate_normals(x, [0, 11], 8)
    with pytest.raises(ValueError):
        B.estimate_normals(x.reshape(-1), [0, 10], 8)
    with pytest.raises(_lib.CorsairHipError, match="bad segment"):
        B.estimate_normals(x, [0, 7, 5], 8)
    with pytest.raises(TypeError):
        B.estimate_normals(x.double(), [0, 10], 8)
    lib = _lib.load()
    off = (ctypes.c_int64 * 2)(0, 10)
    out = torch.empty_like(x)
    assert lib.cs_estimate_normals(None, off, 1, 8, _lib.ptr(out), None) < 0
    assert lib.cs_estimate_normals(_lib.ptr(x), off, 1, 8, None, None) < 0
    assert lib.cs_estimate_normals(_lib.ptr(x), None, 1, 8, _lib.ptr(out), None) < 0
    assert lib.cs_estimate_normals(_lib.ptr(x), off, -1, 8, _lib.ptr(out), None) < 0
    # n_seg = 0 and empty segments are legal
    assert B.estimate_normals(x[:0], [0], 8).shape == (0, 3)
    assert B.estimate_normals(x[:0], [0, 0, 0], 8).shape == (0, 3)


def test_profile_family(gpu):
    from corsair_amd import _lib

    xyz, off, _ = _mixed(3)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        _run(gpu, xyz, off, 3)
        torch.cuda.synchronize()
        ms, n, flop = _lib.prof_get("normals")
    finally:
        _lib.prof_enable(False)
    assert n == 1 and ms > 0 and flop > 0
