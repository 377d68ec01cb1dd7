"""Independent reference of the coordinate maps and kernel maps (include/corsair_hip.h): plain Python / NumPy that never
packs a coordinate into a key.  TEST INFRASTRUCTURE ONLY.

oracle/sparse.py packs its keys exactly as pack_key (csrc/common.h) does, so an error of the packing contract itself -- a
valid coordinate whose key is the empty marker, a field that wraps -- is shared by the library and the oracle.  Here a
coordinate is the tuple (b, x, y, z) in a dict, cells come from Python's floor division, and the documented range is one
comparison per number.  tests/test_maps_ref_cpu.py pins this module to the oracle on ordinary batches and to hand-written
cases at the edges.
"""
from itertools import repeat

import numpy as np

COORD_LIMIT = 32768      # |x|, |y|, |z| < COORD_LIMIT
BATCH_LIMIT = 65535      # 0 <= batch < BATCH_LIMIT

# delta_k for k = (dx+1) + 3(dy+1) + 9(dz+1)
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _rows(coords):
    c = np.asarray(coords)
    assert c.ndim == 2 and c.shape[1] == 4
    return [tuple(r) for r in c.tolist()]


def in_range(b, x, y, z):
    return 0 <= b < BATCH_LIMIT and -COORD_LIMIT < x < COORD_LIMIT and -COORD_LIMIT < y < COORD_LIMIT and \
        -COORD_LIMIT < z < COORD_LIMIT


def all_in_range(coords):
    return all(in_range(*r) for r in _rows(coords))


def row_index(coords):
    """dict (b, x, y, z) -> row; the rows must be unique."""
    rows = _rows(coords)
    d = {r: i for i, r in enumerate(rows)}
    assert len(d) == len(rows), "duplicate coordinate rows"
    return d


def coordmap_stride(coords, tensor_stride, stride=2):
    """(cells int32 [m,4], cell size): unique rows of floor(c / cell) * cell, cell = stride * tensor_stride, in the order of
    their first occurrence.  The cells are returned as they fall, in range or not (all_in_range tells)."""
    cell = int(tensor_stride) * int(stride)
    seen = {}
    for b, x, y, z in _rows(coords):
        seen.setdefault((b, (x // cell) * cell, (y // cell) * cell, (z // cell) * cell), None)   # (dicts keep insertion order)
    return np.array(list(seen), dtype=np.int32).reshape(-1, 4), cell


def chain(coords, n_levels, tensor_stride=1):
    """[(coords, tensor stride)] of create + (n_levels - 1) chained stride(2)."""
    out = [(np.asarray(coords, dtype=np.int32), int(tensor_stride))]
    for _ in range(1, n_levels):
        out.append(coordmap_stride(out[-1][0], out[-1][1], 2))
    return out


def kernel_map(in_coords, in_stride, out_coords, out_stride, transposed=False):
    """int32 [n_out, 27]: the in row that feeds out row o through offset k, or -1.
       normal:     in coordinate = o + delta_k * in_stride    (out_stride in {in_stride, 2 in_stride})
       transposed: in coordinate = o - delta_k * out_stride   (in_stride == 2 out_stride)
    A probe outside the documented range finds nothing."""
    if transposed:
        assert in_stride == 2 * out_stride
        step = -out_stride
    else:
        assert out_stride in (in_stride, 2 * in_stride)
        step = in_stride
    get = row_index(in_coords).get
    oc = np.asarray(out_coords, dtype=np.int64).reshape(-1, 4)
    nbr = np.full((len(oc), 27), -1, dtype=np.int32)
    if len(oc) == 0:
        return nbr
    b = oc[:, 0].tolist()
    for k, (dx, dy, dz) in enumerate(OFFSETS):
        q = oc[:, 1:] + np.array([dx, dy, dz], dtype=np.int64) * step
        # (the dict holds only rows of the in map; the range is still tested on the probe itself, as the header words it)
        ok = (np.abs(q) < COORD_LIMIT).all(axis=1)
        hit = np.fromiter(map(get, zip(b, q[:, 0].tolist(), q[:, 1].tolist(), q[:, 2].tolist()), repeat(-1)), dtype=np.int32,
                          count=len(oc))
        nbr[:, k] = np.where(ok, hit, -1)
    return nbr


def triples(nbr):
    """(k, in_row, out_row) int32, sorted by (k, out_row)."""
    kk, oo = np.nonzero(nbr.T >= 0)          # (nonzero walks [27, n_out] row by row: k ascending, then out_row)
    return kk.astype(np.int32), nbr[oo, kk].astype(np.int32), oo.astype(np.int32)
