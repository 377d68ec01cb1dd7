"""cs_segment_plane on the GPU against tests/plane_ref.py, bit for bit: segments around every boundary of the launch shape
(the 256-hypothesis tile, the slices, the LDS stage), the independence statements of the header, its defined cases and
refusals, the fixture's table through backend, and the harness step on random weights."""
import os

import numpy as np
import pytest
import torch

from tests import outlier_cases as OC
from tests import plane_cases as PC
from tests import plane_ref as ref
from tests.test_plane_cpu import TABLE, defined_cases

pytestmark = pytest.mark.gpu

V = PC.VOXEL
SIZES = (0, 1, 2, 3, 5, 64, 257, 513, 1500)    # 257: two workgroups of the row passes; 513: one LDS stage and a row
ITERS = (1, 255, 256, 257, 1024)               # around the 256-hypothesis tile
SEEDS = (0, 0x9E3779B97F4A7C15)
SLICES = (None, 64, 513)                       # CS_PLANE_SLICE: the default, many slices per segment, a stage and a tail
_cache = {}


def _box_on_slab(n, seed):
    """n rows at one per voxel: about half on the surface of a box, the rest on a noisy slab under it."""
    if n == 0:
        return np.zeros((0, 3), np.float32)
    rng = np.random.default_rng(seed)
    side = max(np.sqrt(0.65 * n * V * V / 6.0), 2 * V)
    p = rng.uniform(-0.5, 0.5, (20 * n + 100, 3))
    face = rng.integers(0, 6, len(p))
    p[np.arange(len(p)), face % 3] = np.where(face < 3, -0.5, 0.5)
    q = rng.uniform(-0.9, 0.9, (20 * n + 100, 3))
    q[:, 2] = -0.5 - (0.5 + rng.uniform(-0.3, 0.3, len(q))) * V / side
    both = np.concatenate([p, q])[rng.permutation(2 * len(p))]
    both = (both * side).astype(np.float32)
    _, idx = np.unique(np.floor(both.astype(np.float64) / V).astype(np.int64), axis=0, return_index=True)
    both = both[np.sort(idx)]
    assert len(both) >= n
    return np.ascontiguousarray(both[:n])


def _mixed():
    if "mixed" not in _cache:
        parts = [_box_on_slab(n, 40 + k) for k, n in enumerate(SIZES)] + [PC.floor_cloud(0)[0]]
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
        _cache["mixed"] = (np.concatenate(parts), off)
    return _cache["mixed"]


def _want(xyz, off, dist, iters, seed, tag):
    """the restatement per segment; the counts of the largest iters serve every smaller one (a prefix)"""
    inl = np.zeros(len(xyz), bool)
    plane = np.zeros((len(off) - 1, 4))
    stat = np.zeros((len(off) - 1, 8), np.int32)
    for p, (a, b) in enumerate(zip(off[:-1], off[1:])):
        key = (tag, p, seed)
        if key not in _cache:
            _cache[key] = ref.counts(xyz[a:b], dist, max(ITERS), seed)
        plane[p], stat[p], inl[a:b] = ref.segment_plane_one(xyz[a:b], dist, iters, seed, count=_cache[key])
    return inl, plane, stat


def _call(dev, xyz, off, dist, iters, seed=0, slice_rows=None):
    from corsair_amd import backend as B

    if slice_rows is not None:
        os.environ["CS_PLANE_SLICE"] = str(slice_rows)       # read per call
    try:
        inl, plane, stat = B.segment_plane(torch.from_numpy(np.ascontiguousarray(xyz)).to(dev), off, dist, iters, seed)
    finally:
        os.environ.pop("CS_PLANE_SLICE", None)
    return inl.cpu().numpy(), plane.cpu().numpy(), stat.cpu().numpy()


def _assert_bits(got, want, what=""):
    inl, plane, stat = got
    winl, wplane, wstat = want
    assert stat.tolist() == np.asarray(wstat).tolist(), what
    assert np.array_equal(plane.view(np.uint64), np.asarray(wplane, np.float64).view(np.uint64)), (what, plane, wplane)
    assert np.array_equal(inl, winl), what


@pytest.mark.parametrize("slice_rows", SLICES)
def test_mixed_segments_match_the_restatement(gpu, slice_rows):
    xyz, off = _mixed()
    seen = set()
    for seed in SEEDS:
        for iters in ITERS:
            want = _want(xyz, off, V, iters, seed, "mixed")
            _assert_bits(_call(gpu, xyz, off, V, iters, seed, slice_rows), want, (seed, iters, slice_rows))
            seen |= {tuple(r[[0, 3]]) for r in want[2]}
            assert want[2][:3, 0].tolist() == [0, 0, 0] and want[2][:3, 7].tolist() == [0, 1, 2]   # 0, 1, 2 rows: NO PLANE
    assert (1, 1) in seen and (0, 0) in seen               # refitted planes and segments without one were both compared
    assert _want(xyz, off, V, 1024, 0, "mixed")[2][-1].tolist() == TABLE[0][0]


def test_independence(gpu):
    from corsair_amd import backend as B

    xyz, off = _mixed()
    big = PC.floor_cloud(0)[0]
    mid = xyz[off[-3]:off[-2]]                             # the 1 500-row segment
    alone = _call(gpu, big, [0, len(big)], V, 300, 5)
    again = _call(gpu, big, [0, len(big)], V, 300, 5)
    _assert_bits(again, alone, "run twice")
    pack = np.concatenate([mid, big, mid[:700], big])
    poff = [0, 1500, 1500 + len(big), 2200 + len(big), 2200 + 2 * len(big)]
    inl, plane, stat = _call(gpu, pack, poff, V, 300, 5)
    for p in (1, 3):                                       # the same segment twice in one call, and among others
        _assert_bits((inl[poff[p]:poff[p + 1]], plane[p:p + 1], stat[p:p + 1]), alone, "segment %d of the pack" % p)
    assert stat[0, 0] == 1 and stat[2, 0] == 1
    x = torch.from_numpy(big).to(gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        got = B.segment_plane(x, [0, len(big)], V, 300, 5)
    side.synchronize()
    _assert_bits(tuple(t.cpu().numpy() for t in got), alone, "another stream")
    _assert_bits(_call(gpu, big, [0, len(big)], V, 300, 5, slice_rows=100), alone, "another launch shape")


def test_defined_cases(gpu):
    cases = defined_cases()
    for name, (rows, dist, iters, seed) in cases.items():
        want = ref.segment_plane(rows, [0, len(rows)], dist, iters, seed)
        _assert_bits(_call(gpu, rows, [0, len(rows)], dist, iters, seed), want, name)
    # and in one call where the parameters agree: empty segments between the others
    names = ("rows0", "lattice", "rows0", "copies", "collinear", "rows1", "rows2")
    parts = [cases[k][0] for k in names]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    xyz = np.concatenate(parts)
    want = ref.segment_plane(xyz, off, 0.1, 32, 0)
    assert want[2][:, 0].tolist() == [0, 1, 0, 0, 0, 0, 0]
    _assert_bits(_call(gpu, xyz, off, 0.1, 32, 0), want, "one call")


def test_refusals(gpu):
    from corsair_amd import _lib, backend as B
    from corsair_amd._lib import CorsairHipError, i64_array, ptr, stream_ptr

    x = torch.zeros((8, 3), device=gpu)
    for dist in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CorsairHipError, match="dist"):
            B.segment_plane(x, [0, 8], dist)
    for iters in (0, -1, 65537):
        with pytest.raises(CorsairHipError, match="iters"):
            B.segment_plane(x, [0, 8], 0.1, iters)
    with pytest.raises(CorsairHipError, match="bad segment"):
        B.segment_plane(x, [0, 5, 3, 8], 0.1)
    with pytest.raises(ValueError, match="offset table"):
        B.segment_plane(x, [0, 9], 0.1)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        B.segment_plane(torch.zeros((8, 2), device=gpu), [0, 8], 0.1)
    lib = _lib.load()
    plane = torch.zeros((2, 4), dtype=torch.float64, device=gpu)
    stat = torch.full((2, 8), 7, dtype=torch.int32, device=gpu)
    inl = torch.zeros(8, dtype=torch.uint8, device=gpu)
    f = lib.cs_segment_plane
    one = i64_array([0, 8])
    assert f(ptr(x), None, 1, 0.1, 8, 0, ptr(plane), ptr(stat), ptr(inl), stream_ptr()) < 0
    assert b"NULL offset table" in lib.cs_last_error()
    assert f(ptr(x), one, -1, 0.1, 8, 0, ptr(plane), ptr(stat), ptr(inl), stream_ptr()) < 0
    assert f(None, one, 1, 0.1, 8, 0, ptr(plane), ptr(stat), ptr(inl), stream_ptr()) < 0
    assert b"NULL" in lib.cs_last_error()
    assert f(ptr(x), one, 1, 0.1, 8, 0, ptr(plane), ptr(stat), None, stream_ptr()) < 0
    assert f(ptr(x), one, 1, 0.1, 8, 0, None, ptr(stat), ptr(inl), stream_ptr()) < 0
    assert f(ptr(x), one, 1, 0.1, 8, 0, ptr(plane), None, ptr(inl), stream_ptr()) < 0
    assert f(ptr(x), i64_array([0, 1 << 31]), 1, 0.1, 8, 0, ptr(plane), ptr(stat), ptr(inl), stream_ptr()) == -5
    assert b"2^31" in lib.cs_last_error()
    assert f(None, i64_array([0]), 0, 0.1, 8, 0, None, None, None, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert stat.tolist() == [[7] * 8] * 2                                     # a refused call writes nothing
    assert f(None, i64_array([0, 0, 0]), 2, 0.1, 8, 0, ptr(plane), ptr(stat), None, stream_ptr()) == 0     # empty segments
    torch.cuda.synchronize()
    assert stat.tolist() == [[0, -1, 0, 0, 0, 0, 0, 0]] * 2 and not plane.any()
    assert f(ptr(x), one, 1, 0.1, 65536, 2 ** 64 - 1, ptr(plane), ptr(stat), ptr(inl), stream_ptr()) == 0   # copies of the origin
    torch.cuda.synchronize()
    assert stat[0].tolist() == [0, -1, 0, 0, 0, 0, 0, 8]


def test_fixture_through_backend(gpu):
    """The three floor clouds in one call: the table of tests/test_plane_cpu.py, and one profile scope per call."""
    from corsair_amd import _lib, backend as B, harness as H

    xyz, off, kind = PC.packed()
    x = torch.from_numpy(xyz).to(gpu)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        inl, plane, stat = B.segment_plane(x, off, V)
        torch.cuda.synchronize()
        ms, n, units = _lib.prof_get("plane")
        assert _lib.prof_get("cluster")[1] == 0 and _lib.prof_get("outlier")[1] == 0
    finally:
        _lib.prof_enable(False)
    assert n == 1 and ms > 0 and units == 10.0 * len(xyz) * 1024
    assert inl.dtype == torch.bool and plane.dtype == torch.float64 and stat.dtype == torch.int32
    inl, plane, stat = inl.cpu().numpy(), plane.cpu().numpy(), stat.cpu().numpy()
    _assert_bits((inl, plane, stat), _want(xyz, off, V, 1024, 0, "packed"))
    for p, i in enumerate(PC.CLOUDS):
        seg = slice(off[p], off[p + 1])
        assert stat[p].tolist() == TABLE[i][0]
        assert (int(((kind[seg] == PC.REAL) & inl[seg]).sum()), int(((kind[seg] == PC.CLUTTER) & inl[seg]).sum())) == TABLE[i][1:]
        assert H.is_support_plane(stat[p].tolist(), plane[p].tolist(), H.Config())
    assert inl[kind == PC.FLOOR].all()


def _rows(a):
    return {r.tobytes() for r in np.ascontiguousarray(a, np.float32)}


def test_harness_removes_the_support_plane_only_when_configured(gpu):
    from corsair_amd import _lib, harness, synth

    sd, emb = synth.make_state_dicts(31)
    clouds = [PC.floor_cloud(i)[0].astype(np.float64) for i in PC.CLOUDS]      # f64, as posed queries arrive
    kinds = [PC.floor_cloud(i)[1] for i in PC.CLOUDS]
    vox = harness.Config().voxel_size
    assert vox == V
    plain = harness.Pipeline(sd, emb, device=gpu)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        base = plain.embed_clouds(clouds)
        same = plain.embed_clouds(clouds, scan_filter=True)          # the default Config names no step
        torch.cuda.synchronize()
        assert _lib.prof_get("plane")[1] == 0 and _lib.prof_get("cluster")[1] == 0 and _lib.prof_get("outlier")[1] == 0
    finally:
        _lib.prof_enable(False)
    assert same.offsets == base.offsets and torch.equal(same.F, base.F) and torch.equal(same.desc, base.desc)
    assert plain.scan_filter_stat == {"rows_in": 0, "rows_kept": 0, "clouds_skipped": 0}
    assert plain.scan_plane_stat == {"clouds": 0, "planes_removed": 0, "rows_removed": 0}
    cfg = harness.Config(scan_plane="remove")
    pipe = harness.Pipeline(sd, emb, device=gpu, config=cfg)
    untouched = pipe.embed_clouds(clouds)                             # the catalog's call: scan_filter stays False
    assert untouched.offsets == base.offsets and torch.equal(untouched.F, base.F)
    got = pipe.embed_clouds(clouds, scan_filter=True)
    origin = got.origin.cpu().numpy()
    removed = 0
    for p, (c, k) in enumerate(zip(clouds, kinds)):
        seg = origin[got.offsets[p]:got.offsets[p + 1]]
        seen = base.origin[base.offsets[p]:base.offsets[p + 1]].cpu().numpy()       # the first row of every voxel
        plane, stat, inl = ref.segment_plane_one(seen, 1.0 * vox, 1024, 0)
        assert harness.is_support_plane(stat, plane, cfg)
        assert np.array_equal(seg, seen[~inl]), "the rows the restatement keeps, in their order"
        assert not (_rows(seg) & _rows(c[k == PC.FLOOR])), "a floor row reached the network"
        removed += int(inl.sum())
    assert removed > 2500
    assert got.offsets[-1] == base.offsets[-1] - removed == got.F.shape[0] and got.desc.shape[0] == 3
    assert pipe.scan_plane_stat == {"clouds": 3, "planes_removed": 3, "rows_removed": removed}
    assert pipe.scan_filter_stat == {"rows_in": 0, "rows_kept": 0, "clouds_skipped": 0}
    # a cloud of 12 rows, nine of them in a plane: the plane is a support plane, and the cloud keeps all of its rows
    g = 4.0 * np.array([[x, y, 0] for x in range(3) for y in range(3)] + [[0, 0, 3], [2, 1, 5], [1, 2, 4]], np.float64)
    tiny = ((g + 0.5) * vox).astype(np.float32).astype(np.float64)
    plane, stat, inl = ref.segment_plane_one(tiny, vox, 1024, 0)
    assert stat[4] == 9 and harness.is_support_plane(stat, plane, cfg)
    pipe.scan_plane_stat = {"clouds": 0, "planes_removed": 0, "rows_removed": 0}
    got = pipe.embed_clouds([tiny], scan_filter=True)
    assert got.offsets == [0, 12] and _rows(got.origin.cpu().numpy()) == _rows(tiny)
    assert pipe.scan_plane_stat == {"clouds": 1, "planes_removed": 0, "rows_removed": 0}


def test_harness_plane_then_cluster_and_the_up_hint(gpu):
    from corsair_amd import harness, synth
    from tests import dbscan_ref

    sd, emb = synth.make_state_dicts(31)
    vox = harness.Config().voxel_size
    clouds = [PC.floor_patch_cloud(i)[0].astype(np.float64) for i in PC.CLOUDS]
    kinds = [PC.floor_patch_cloud(i)[1] for i in PC.CLOUDS]
    base = harness.Pipeline(sd, emb, device=gpu).embed_clouds(clouds)
    # the cluster filter alone keeps every floor and patch row it is shown ...
    alone = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(scan_filter="cluster"))
    got = alone.embed_clouds(clouds, scan_filter=True)
    for p, (c, k) in enumerate(zip(clouds, kinds)):
        seg = _rows(got.origin[got.offsets[p]:got.offsets[p + 1]].cpu().numpy())
        seen = _rows(base.origin[base.offsets[p]:base.offsets[p + 1]].cpu().numpy())
        assert seen & _rows(c[k == PC.FLOOR]) <= seg and seen & _rows(c[k == PC.PATCH]) <= seg
    # ... and after the plane step none of them, nor clutter
    pipe = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(scan_plane="remove", scan_filter="cluster"))
    got = pipe.embed_clouds(clouds, scan_filter=True)
    rows_in = 0
    for p, (c, k) in enumerate(zip(clouds, kinds)):
        seg = got.origin[got.offsets[p]:got.offsets[p + 1]].cpu().numpy()
        seen = base.origin[base.offsets[p]:base.offsets[p + 1]].cpu().numpy()
        _, _, inl = ref.segment_plane_one(seen, vox, 1024, 0)
        rest = seen[~inl]
        rows_in += len(rest)
        label, _, _ = dbscan_ref.dbscan(rest, [0, len(rest)], 2.5 * vox, 5)
        keep, _ = dbscan_ref.cluster_largest(label, [0, len(rest)])
        assert np.array_equal(seg, rest[keep])
        assert not (_rows(seg) & _rows(c[k != PC.REAL])), "a floor, patch or clutter row reached the network"
        assert len(seg) >= 0.85 * (k == PC.REAL).sum()
    assert pipe.scan_plane_stat["planes_removed"] == 3
    assert pipe.scan_filter_stat == {"rows_in": rows_in, "rows_kept": got.offsets[-1], "clouds_skipped": 0}   # three keys
    # THE LIMIT: the bare table loses its top without a hint of what is up, and keeps it with one
    table = [OC.clutter_cloud(5)[0].astype(np.float64)]
    bare = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(scan_plane="remove"))
    hint = harness.Pipeline(sd, emb, device=gpu, config=harness.Config(scan_plane="remove", scan_plane_up=(0.0, 0.0, 1.0)))
    full = bare.embed_clouds(table)
    lost = bare.embed_clouds(table, scan_filter=True)
    kept = hint.embed_clouds(table, scan_filter=True)
    assert full.offsets[-1] - lost.offsets[-1] > 400 and bare.scan_plane_stat["planes_removed"] == 1
    assert kept.offsets == full.offsets and torch.equal(kept.origin, full.origin) and torch.equal(kept.F, full.F)
    assert hint.scan_plane_stat == {"clouds": 1, "planes_removed": 0, "rows_removed": 0}


if __name__ == "__main__":
    import sys

    sys.exit(pytest.main([__file__, "-q"] + sys.argv[1:]))
