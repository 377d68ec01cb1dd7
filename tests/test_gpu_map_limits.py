"""Coordinate maps and kernel maps AT the limits of their documented ranges (include/corsair_hip.h): the corners of the
16-bit coordinate fields and the last batch index, the floor of negative coordinates next to -32768, the row limits of the
three LDS tables of k_level_maps, the 10-bit box fields of its keys, and the 21-bit counters of the pyramid's packed scan.

The reference is tests/maps_ref.py (tuples in a dict, no packed keys: tests/test_maps_ref_cpu.py).  Everything is exact
integer equality: coordinates, neighbour tables, exported triples and pair counts.  Every batch is built twice (create +
chained stride(2), and pyramid) and every kernel map twice (the level kernel with its LDS tables, and CS_KMAP_GLOBAL=1).
No map of this file is given to a convolution."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import maps_ref as mref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS_ERR_RANGE = -3


def _specs(c):
    """Every kernel map of the levels c[0..n): submanifold, strided and transposed -- (in, out, transposed) level indices."""
    out = []
    for l in range(len(c)):
        out.append((l, l, False))
        if l + 1 < len(c):
            out.append((l, l + 1, False))
            out.append((l + 1, l, True))
    return out


def _reference(rows, n_levels, ts, specs):
    levels = mref.chain(rows, n_levels, ts)
    assert all(mref.all_in_range(c) for c, _ in levels)
    maps = []
    for i, o, tr in specs:
        nbr = mref.kernel_map(levels[i][0], levels[i][1], levels[o][0], levels[o][1], transposed=tr)
        maps.append((nbr, mref.triples(nbr)))
    return levels, maps


def _build_both_ways(gpu, rows, n_levels, hint, ts=1):
    from corsair_amd import backend as B

    g = torch.from_numpy(np.array(rows, dtype=np.int32)).to(gpu)       # (a copy: the cached batches are read-only)
    chain = [B.CoordMap.create(g, ts)]
    for _ in range(1, n_levels):
        chain.append(chain[-1].stride(2))
    return chain, B.CoordMap.pyramid(g, n_levels, hint, tensor_stride=ts)


def _check(gpu, monkeypatch, rows, n_levels, hint, ts=1, specs=None, ref=None):
    """Both ways of building the levels and both ways of building the kernel maps against the reference."""
    from corsair_amd import backend as B

    specs = _specs(range(n_levels)) if specs is None else specs
    levels, maps = ref if ref is not None else _reference(rows, n_levels, ts, specs)
    chain, pyr = _build_both_ways(gpu, rows, n_levels, hint, ts)
    for how, c in (("chain", chain), ("pyramid", pyr)):
        for l, (want, stride) in enumerate(levels):
            assert c[l].n == len(want) and c[l].tensor_stride == stride, (how, l)
            assert np.array_equal(c[l].coords.cpu().numpy(), want), (how, l)
        for mode in ("lds", "global"):
            if mode == "global":
                monkeypatch.setenv("CS_KMAP_GLOBAL", "1")
            try:
                kms = B.KernelMap.build_many([(c[i], c[o], 3, tr) for i, o, tr in specs])
            finally:
                monkeypatch.delenv("CS_KMAP_GLOBAL", raising=False)
            for (i, o, tr), km, (nbr, (wk, wi, wo)) in zip(specs, kms, maps):
                what = (how, mode, i, o, tr)
                t = km.table().cpu().numpy()
                assert t.shape == nbr.shape, what
                assert t.min(initial=-1) >= -1 and t.max(initial=-1) < max(c[i].n, 1), what   # nothing outside [-1, n_in)
                assert np.array_equal(t, nbr), what
                assert km.num_pairs == len(wk), what
                k, ii, oo = (x.cpu().numpy() for x in km.export())
                assert np.array_equal(k, wk) and np.array_equal(ii, wi) and np.array_equal(oo, wo), what
    return chain, pyr


def _with_batch(b, xyz):
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([np.full((len(xyz), 1), b, np.int64), xyz], 1)


def _unique(xyz):
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    _, first = np.unique(xyz, axis=0, return_index=True)
    return xyz[np.sort(first)]


# ---- the corners of the coordinate range, the last batch index ---------------------------------------------------------------
LAST_BATCH = 65534          # 0 <= batch < 65535


def _corner_cluster(rng, sign, n=300, depth=8):
    """The corner voxel sign * 32767, the part of its 3x3x3 neighbourhood that is in range (a 2x2x2 block), and n voxels
    drawn from the depth^3 cells behind the corner."""
    block = np.array([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)])
    r = _unique(np.concatenate([block, rng.integers(0, depth, (n, 3))]))
    return np.asarray(sign) * (32767 - r)


CORNERS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]


@functools.lru_cache(maxsize=None)
def _corner_batch():
    """Batch index 0 and the last one hold all eight corners each (more than 1 280 rows in a box of 65 534 cells: the level
    kernel probes them in the global table); batch indices 1..8 hold one corner each, a few hundred rows (an LDS table
    whose box ends at the edge of the range)."""
    rng = np.random.default_rng(61)
    parts = [_with_batch(0, np.concatenate([_corner_cluster(rng, s) for s in CORNERS]))]
    parts += [_with_batch(1 + j, _corner_cluster(rng, s)) for j, s in enumerate(CORNERS)]
    parts.append(_with_batch(LAST_BATCH, np.concatenate([_corner_cluster(rng, s) for s in CORNERS])))
    rows = np.concatenate(parts).astype(np.int32)
    for s in CORNERS:                                          # the corner voxels themselves are rows
        assert (rows[rows[:, 0] == 0, 1:] == 32767 * np.array(s)).all(1).any()
        assert (rows[rows[:, 0] == LAST_BATCH, 1:] == 32767 * np.array(s)).all(1).any()
    rows.setflags(write=False)
    return rows


@pytest.mark.parametrize("shuffled", [False, True])
def test_corners_of_the_coordinate_range_and_the_last_batch_index(gpu, monkeypatch, shuffled):
    """Submanifold map at stride 1 (the floor cell of -32767 is out of range at any stride).  The segment tables have 65 535
    entries, nearly all empty; the level kernel runs 65 535 workgroups.  Probes that leave the range are -1."""
    rows = _corner_batch()
    if shuffled:
        rows = rows[np.random.default_rng(62).permutation(len(rows))]       # not grouped: the global kernel serves the map
    per_sample = np.bincount(rows[:, 0])
    assert (per_sample[1:9] >= 200).all() and (per_sample[1:9] <= 1280).all() and len(rows) < 8000
    chain, _ = _check(gpu, monkeypatch, rows, 1, LAST_BATCH + 1)
    # the corner rows by hand: 8 of the 27 probes stay in range, and those find the 2x2x2 block
    from corsair_amd import backend as B

    t = B.KernelMap.build(chain[0], chain[0]).table().cpu().numpy()
    for b in (0, 3, LAST_BATCH):
        for s in CORNERS if b != 3 else [CORNERS[2]]:
            o = int(np.flatnonzero((rows == np.array((b,) + tuple(32767 * v for v in s))).all(1))[0])
            for k, d in enumerate(mref.OFFSETS):
                inside = all(dv * sv <= 0 for dv, sv in zip(d, s))
                assert (t[o, k] >= 0) == inside, (b, s, k)
                if inside:
                    assert rows[t[o, k]].tolist() == [b] + [32767 * sv + dv for dv, sv in zip(d, s)]


def test_the_positive_corner_through_every_level(gpu, monkeypatch):
    """The (+, +, +) corner can be strided (its floor cells stay in range): four levels and all ten maps for batch indices 0,
    3 and the last one; a level-8 probe from cell 32760 reaches 32768 and finds nothing."""
    rng = np.random.default_rng(63)
    rows = np.concatenate([_with_batch(b, _corner_cluster(rng, (1, 1, 1), n=400, depth=12)) for b in (0, 3, LAST_BATCH)])
    rows = rows.astype(np.int32)
    ref = _reference(rows, 4, 1, _specs(range(4)))
    _check(gpu, monkeypatch, rows, 4, LAST_BATCH + 1, ref=ref)
    _check(gpu, monkeypatch, rows, 4, 0, ref=ref)              # no announcement: segments on first use


def test_batch_index_65535_is_refused(gpu):
    """(65535, 32767, 32767, 32767) would pack to the hash tables' empty marker: the batch range ends at 65534."""
    from corsair_amd import _lib, backend as B

    for xyz in ((1, 2, 3), (32767, 32767, 32767)):
        for also in ([], [[0, 5, 5, 5]], [[65534, 32766, 32766, 32766]]):
            bad = torch.tensor(also + [[65535, *xyz]], dtype=torch.int32, device=gpu)
            with pytest.raises(_lib.CorsairHipError, match="range"):
                B.CoordMap.create(bad, 1)
            for n_levels, hint in ((1, 0), (4, 0), (4, 65535), (4, 65536)):
                outs = (ctypes.c_void_p * n_levels)(*([1] * n_levels))
                rc = _lib.load().cs_coordmap_pyramid(_lib.ptr(bad), len(bad), 1, n_levels, hint, _lib.stream_ptr(), outs)
                assert rc == CS_ERR_RANGE and all(h is None for h in outs)
                with pytest.raises(_lib.CorsairHipError, match="range"):
                    B.CoordMap.pyramid(bad, n_levels, hint)
    # the same thread goes on working
    good = torch.tensor([[65534, 32767, 32767, 32767], [65534, 32766, 32767, 32767]], dtype=torch.int32, device=gpu)
    for c in (B.CoordMap.create(good, 1), B.CoordMap.pyramid(good, 1, 65535)[0]):
        assert c.n == 2 and torch.equal(c.coords, good)
        t = B.KernelMap.build(c, c).table().cpu().numpy()
        assert t[0].tolist() == [-1] * 12 + [1, 0] + [-1] * 13 and t[1].tolist() == [-1] * 13 + [1, 0] + [-1] * 12


# ---- the floor of negative coordinates at a stride -----------------------------------------------------------------------------
def _floor_rows(rng, lowest, unit=1, n=250):
    """Three samples: one in the corner whose lowest coordinate is `lowest` on every axis, one around the origin, one on both
    sides of it far out; coordinates are multiples of `unit`."""
    def cloud(lo, span):
        return _unique(np.concatenate([[[0, 0, 0]], rng.integers(0, span, (n, 3))])) * unit + lo
    rows = np.concatenate([_with_batch(0, cloud(lowest, 8)), _with_batch(1, cloud(-4 * unit, 8)),
                           _with_batch(3, np.concatenate([cloud(-3000 * unit, 6), cloud(9000 * unit, 6)]))]).astype(np.int32)
    assert (rows[:, 1:].min(0) == lowest).all()
    return rows


def test_floor_of_negative_coordinates_down_to_the_last_cell(gpu, monkeypatch):
    """-32760 is the lowest coordinate whose cells at 2, 4 and 8 are in range (it is its own cell at all three)."""
    rows = _floor_rows(np.random.default_rng(64), -32760)
    _check(gpu, monkeypatch, rows, 4, 4)


def _refused(fn):
    from corsair_amd import _lib

    with pytest.raises(_lib.CorsairHipError, match="range"):
        fn()


def _pyramid_rc(rows_dev, n_levels, hint, ts=1):
    from corsair_amd import _lib

    outs = (ctypes.c_void_p * n_levels)(*([1] * n_levels))
    rc = _lib.load().cs_coordmap_pyramid(_lib.ptr(rows_dev), len(rows_dev), ts, n_levels, hint, _lib.stream_ptr(), outs)
    handles = [h for h in outs]
    for h in handles:
        if rc == 0 and h:
            _lib.load().cs_coordmap_free(ctypes.c_void_p(h))
    return rc, handles


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_floor_cell_that_leaves_the_range_is_refused(gpu, monkeypatch, axis):
    """The cells of -32761 are -32762, -32764 and -32768: levels 1 and 2 accept the row, level 3 refuses it.  -32767 is
    refused by the first stride(2).  The pyramid refuses exactly when the chain does and then returns no map at all."""
    from corsair_amd import backend as B

    base = _floor_rows(np.random.default_rng(65 + axis), -32760, n=120)
    for low, ok_levels in ((-32761, 3), (-32767, 1), (-32765, 2), (-32763, 3), (-32762, 3), (-32764, 3), (-32766, 2)):
        extra = [7, 7, 7]
        extra[axis] = low
        rows = np.concatenate([base[base[:, 0] == 0], [[0] + extra], base[base[:, 0] != 0]]).astype(np.int32)
        g = torch.from_numpy(rows).to(gpu)
        # what the reference says about it
        levels = mref.chain(rows, 4)
        assert [mref.all_in_range(c) for c, _ in levels] == [l < ok_levels for l in range(4)]
        # the chain: ok_levels maps, then CS_ERR_RANGE
        c = [B.CoordMap.create(g, 1)]
        for l in range(1, ok_levels):
            c.append(c[-1].stride(2))
            assert np.array_equal(c[l].coords.cpu().numpy(), levels[l][0]), (low, l)
        _refused(lambda: c[-1].stride(2))
        # the pyramid: every n_levels the chain can make, and nothing beyond
        for n_levels in range(1, 5):
            for hint in (0, 4):
                rc, handles = _pyramid_rc(g, n_levels, hint)
                if n_levels <= ok_levels:
                    assert rc == 0 and all(handles), (low, n_levels, hint)
                else:
                    assert rc == CS_ERR_RANGE and not any(handles), (low, n_levels, hint)
        # a call on the same thread afterwards works: the levels that exist, and their maps, against the reference
        if low in (-32761, -32767):
            _check(gpu, monkeypatch, rows, ok_levels, 4)


def test_floor_of_negative_coordinates_of_a_stride_3_tensor(gpu, monkeypatch):
    """Tensor stride 3 takes floor_div (cells of 6 are no mask) and the global table.  -32766 = -5461 * 6 is the lowest
    multiple of 3 whose cell of 6 is in range; -32766 at cell 12 is -32772, so a third level is refused."""
    from corsair_amd import backend as B

    rows = _floor_rows(np.random.default_rng(68), -32766, unit=3)
    assert (rows[:, 1:] % 3 == 0).all() and (rows[:, 1:] < 0).any()
    assert int((rows[:, 1:] % 6 != 0).sum()) > 100 and int(((rows[:, 1:] % 6 != 0) & (rows[:, 1:] < 0)).sum()) > 100
    _check(gpu, monkeypatch, rows, 2, 4, ts=3)
    assert not mref.all_in_range(mref.chain(rows, 3, 3)[2][0])
    g = torch.from_numpy(rows).to(gpu)
    c = B.CoordMap.create(g, 3).stride(2)
    _refused(lambda: c.stride(2))
    rc, handles = _pyramid_rc(g, 3, 4, ts=3)
    assert rc == CS_ERR_RANGE and not any(handles)
    # one step lower on one axis: -32769 is no coordinate at all, -32767 (not a multiple of 3, still a valid row) floors to -32772
    low = np.concatenate([rows, [[3, -32767, 0, 0]]]).astype(np.int32)
    gl = torch.from_numpy(low).to(gpu)
    _refused(lambda: B.CoordMap.create(gl, 3).stride(2))
    rc, handles = _pyramid_rc(gl, 2, 4, ts=3)
    assert rc == CS_ERR_RANGE and not any(handles)


# ---- the row limits of the three LDS tables ---------------------------------------------------------------------------------
# k_level_maps<SLOTS>: MAX_ROWS = SLOTS / 8 * 5 rows of one sample fit the table (load factor 0.625)
LDS_SLOTS = (2048, 8192, 24576)
MAX_ROWS = {2048: 1280, 8192: 5120, 24576: 15360}
N_SMALL = {2048: 4, 8192: 4, 24576: 1}       # small samples (40 rows each) that bring the mean to the instantiation wanted


def _slots_for(n, n_batch):
    """launch_level's choice: 2.5 x the mean rows per batch index against the row limits of the two smaller tables."""
    need = (n // n_batch) * 5 // 2
    return 2048 if need <= 1280 else 8192 if need <= 5120 else 24576


@functools.lru_cache(maxsize=None)
def _row_limit_batch(slots):
    """Samples of exactly MAX_ROWS rows (the table is as full as it gets), MAX_ROWS + 1 rows (the same workgroups probe the
    global table), one row, none, and the small ones.  The counts hold at tensor stride 1 AND 2: the cells of 2 are drawn
    first, and every cell gets exactly one stride-1 voxel -- so the level that serves a submanifold, a strided and a
    transposed job in one launch (stride 2) has them too."""
    assert all(MAX_ROWS[s] == s // 8 * 5 for s in LDS_SLOTS)
    rng = np.random.default_rng(slots)
    sizes = [MAX_ROWS[slots], MAX_ROWS[slots] + 1, 1, 0] + [40] * N_SMALL[slots]
    parts = []
    for b, m in enumerate(sizes):
        side = max(2, int(np.ceil((3 * m) ** (1 / 3))))                     # a cube of cells about one third full
        assert side < 1023 and side ** 3 >= m
        cells = np.stack(np.unravel_index(rng.choice(side ** 3, m, replace=False), (side,) * 3), 1)
        origin = rng.integers(-2000, 2000, 3) // 2 * 2
        parts.append(_with_batch(b, 2 * cells + origin + rng.integers(0, 2, (m, 3))))
    rows = np.concatenate(parts).astype(np.int32)
    # the arithmetic of the choice, for both levels of that size
    n, nb = len(rows), len(sizes)
    assert n == sum(sizes) and _slots_for(n, nb) == slots
    if slots == 2048:
        assert (n, nb, n // nb) == (2722, 8, 340) and 340 * 5 // 2 == 850 <= 1280
    elif slots == 8192:
        assert (n, nb, n // nb) == (10402, 8, 1300) and 1280 < 1300 * 5 // 2 == 3250 <= 5120
    else:
        assert (n, nb, n // nb) == (30762, 5, 6152) and 6152 * 5 // 2 == 15380 > 5120
    rows.setflags(write=False)
    return rows, tuple(sizes)


ROW_LIMIT_SPECS = [(0, 0, False), (0, 1, False), (1, 1, False), (1, 2, False), (1, 0, True)]


@pytest.mark.parametrize("slots", LDS_SLOTS)
def test_lds_table_row_limits(gpu, monkeypatch, slots):
    rows, sizes = _row_limit_batch(slots)
    ref = _reference(rows, 3, 1, ROW_LIMIT_SPECS)
    for l in (0, 1):                                            # both levels have the sample sizes asked for
        assert np.bincount(ref[0][l][0][:, 0], minlength=len(sizes)).tolist() == list(sizes)
    _check(gpu, monkeypatch, rows, 3, len(sizes), specs=ROW_LIMIT_SPECS, ref=ref)


def _run_row_limit_batches(dev):
    """The three batches through the level kernel (the child process of the test below)."""
    from corsair_amd import backend as B

    pairs = []
    for slots in LDS_SLOTS:
        rows, sizes = _row_limit_batch(slots)
        c = B.CoordMap.pyramid(torch.from_numpy(np.array(rows)).to(dev), 3, len(sizes))
        kms = B.KernelMap.build_many([(c[i], c[o], 3, tr) for i, o, tr in ROW_LIMIT_SPECS])
        pairs.append([km.num_pairs for km in kms])
    return pairs


def test_lds_table_row_limits_use_the_three_instantiations(gpu):
    """CS_KMAP_TRACE=1 (read once per process: a child) reports the table of every level launch.  The two levels that hold
    the boundary samples must be served by the instantiation whose limit they sit on -- else the cases above would pass on
    another table."""
    env = dict(os.environ)
    env["CS_KMAP_TRACE"] = "1"
    env.pop("CS_KMAP_GLOBAL", None)
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_map_limits"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = [(int(m.group(1)), int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"\[kmap trace\] level n_in (\d+), (\d+) samples x \d+ slices, (\d+) slots", r.stderr)]
    for slots in LDS_SLOTS:
        rows, sizes = _row_limit_batch(slots)
        got = [s for n, nb, s in seen if n == len(rows) and nb == len(sizes)]
        assert got == [slots, slots], (slots, seen)             # stride 1 and stride 2
    assert {s for _, _, s in seen} == set(LDS_SLOTS)


# ---- the 10-bit box fields of the LDS keys ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _box_batch(unit):
    """Seven samples whose bounding boxes AT TENSOR STRIDE `unit` are, in cells of that level: 1023 wide on x (the key field is
    all ones: still the LDS table) / 1024 wide on x (the global arm) / the same on y / on z / 1023 wide on all three axes.
    Every sample is two clusters, one on each face of its box, so probes at -1 and at extent + 1 happen."""
    rng = np.random.default_rng(70 + unit)
    parts, extents = [], []
    cases = [(ax, e) for ax in range(3) for e in (1023, 1024)] + [(None, 1023)]
    for b, (ax, e) in enumerate(cases):
        ext = np.array([e if ax is None or a == ax else 4 for a in range(3)])
        lo_hi = []
        for face in (0, 1):
            # three cells deep behind the face on the long axes, the whole width on the short ones; the face corner itself
            depth = np.where(ext > 4, 3, 5)
            cells = _unique(np.concatenate([[[0, 0, 0]], rng.integers(0, depth, (40, 3))]))
            lo_hi.append(cells if face == 0 else ext - cells)
        cells = np.concatenate(lo_hi)
        origin = rng.integers(-600, -400, 3) * 8                             # a multiple of every unit, negative
        fine = []
        for c in cells:                                                      # one or two stride-1 voxels inside every cell
            offs = _unique(rng.integers(0, unit, (int(rng.integers(1, 3)), 3)))
            fine.append(origin + unit * c + offs)
        parts.append(_with_batch(b, np.concatenate(fine)))
        extents.append(ext)
    rows = np.concatenate(parts).astype(np.int32)
    rows.setflags(write=False)
    return rows, extents


@pytest.mark.parametrize("unit", [1, 2, 4, 8])
def test_box_extents_of_1023_and_1024_cells(gpu, monkeypatch, unit):
    rows, extents = _box_batch(unit)
    n_levels = 4
    level = {1: 0, 2: 1, 4: 2, 8: 3}[unit]
    specs = _specs(range(n_levels))
    ref = _reference(rows, n_levels, 1, specs)
    cu, stride = ref[0][level]
    assert stride == unit
    for b, ext in enumerate(extents):                          # the boxes of that level are what the case is about
        s = cu[cu[:, 0] == b, 1:].astype(np.int64)
        assert ((s.max(0) - s.min(0)) == ext * unit).all(), (b, ext)
    assert len(rows) < 2000
    _check(gpu, monkeypatch, rows, n_levels, len(extents), specs=specs, ref=ref)


# ---- the 21-bit counters of the pyramid's packed scan ---------------------------------------------------------------------------
def test_pyramid_at_the_last_row_count_of_its_packed_scan(gpu, monkeypatch):
    """2^21 - 1 rows on the lattice 8 (i, j, k): every row is its own cell at strides 2, 4 and 8, so each of the three 21-bit
    counters of the packed scan ends at its maximum 2^21 - 1 (one more row and cs_coordmap_pyramid takes the chained calls:
    test_coordmap_pyramid_beyond_its_packed_scan_limit).  Closed form instead of the CPU reference: every level has all n
    rows with the input's coordinates; the stride-8 submanifold map is the 27-neighbourhood of the lattice inside a sample;
    maps between two levels find the centre only."""
    from corsair_amd import backend as B

    side = 128
    n = side ** 3 - 1
    assert n == (1 << 21) - 1
    idx = np.arange(n, dtype=np.int64)
    rows = np.empty((n, 4), np.int32)
    rows[:, 0] = idx * 3 // n                                 # three samples, grouped
    i, j, k = np.unravel_index(idx, (side, side, side))
    rows[:, 1], rows[:, 2], rows[:, 3] = 8 * i - 512, 8 * j - 512, 8 * k - 512
    assert rows[:, 0].max() == 2 and rows[0, 0] == 0
    g = torch.from_numpy(rows).to(gpu)
    chain = [B.CoordMap.create(g, 1)]
    for _ in range(3):
        chain.append(chain[-1].stride(2))
    pyr = B.CoordMap.pyramid(g, 4, 3)
    for c in (chain, pyr):
        for l in range(4):
            assert c[l].n == n and c[l].tensor_stride == 1 << l
            assert torch.equal(c[l].coords, g)
    # closed forms, on the device: row o = (i, j, k) -> i * side^2 + j * side + k
    o = torch.arange(n, device=gpu, dtype=torch.int64)
    gi, gj, gk = o // (side * side), (o // side) % side, o % side
    gb = o * 3 // n
    want = torch.full((n, 27), -1, dtype=torch.int32, device=gpu)
    for kk, (dx, dy, dz) in enumerate(mref.OFFSETS):
        ni, nj, nk = gi + dx, gj + dy, gk + dz
        q = ni * side * side + nj * side + nk
        ok = (ni >= 0) & (ni < side) & (nj >= 0) & (nj < side) & (nk >= 0) & (nk < side) & (q < n) & (q >= 0)
        ok &= (q.clamp(0, n - 1) * 3 // n) == gb
        want[:, kk] = torch.where(ok, q, torch.full_like(q, -1)).to(torch.int32)
    centre = torch.full((n, 27), -1, dtype=torch.int32, device=gpu)
    centre[:, 13] = o.to(torch.int32)
    specs = lambda c: [(c[3], c[3]), (c[2], c[3]), (c[3], c[2], 3, True), (c[0], c[0])]
    wants = [want, centre, centre, centre]
    built = [B.KernelMap.build_many(specs(chain)), B.KernelMap.build_many(specs(pyr))]
    monkeypatch.setenv("CS_KMAP_GLOBAL", "1")
    try:
        built.append(B.KernelMap.build_many(specs(pyr)))
    finally:
        monkeypatch.delenv("CS_KMAP_GLOBAL", raising=False)
    for kms in built:
        for km, w in zip(kms, wants):
            assert torch.equal(km.table(), w)
            assert km.num_pairs == int((w >= 0).sum())


if __name__ == "__main__":
    print(_run_row_limit_batches(torch.device("cuda:0")))
