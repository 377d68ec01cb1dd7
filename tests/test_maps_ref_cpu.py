"""tests/maps_ref.py (the reference of tests/test_gpu_map_limits.py) checked two ways: it equals oracle/sparse.py on
ordinary batches, and it is right on hand-written cases at the edges of the documented range."""
import numpy as np
import pytest

from oracle import sparse as osp
from tests import maps_ref as mref
from tests.helpers import make_batch


def _equal_to_oracle(coords, ts):
    levels = mref.chain(coords, 3, ts)
    c = [coords]
    for l in (1, 2):
        want, cell = osp.coordmap_stride(c[-1], ts * 2 ** (l - 1), 2)
        assert cell == levels[l][1] == ts * 2 ** l
        assert levels[l][0].dtype == np.int32 and np.array_equal(levels[l][0], want)
        c.append(want)
    (c0, s0), (c1, s1), (c2, s2) = levels
    for args, tr in (((c0, s0, c0, s0), False), ((c0, s0, c1, s1), False), ((c1, s1, c1, s1), False), ((c1, s1, c2, s2), False),
                     ((c1, s1, c0, s0), True), ((c2, s2, c1, s1), True)):
        got, want = mref.kernel_map(*args, transposed=tr), osp.kernel_map(*args, transposed=tr)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert (got >= 0).any()
        for a, b in zip(mref.triples(got), osp.kernel_map_triples(want)):
            assert a.dtype == np.int32 and np.array_equal(a, b)


def test_equals_the_oracle_on_ordinary_batches():
    coords, _, _, _ = make_batch([41, 42, 43], n_points=2500)
    assert (coords[:, 1:] < 0).any() and mref.all_in_range(coords)
    _equal_to_oracle(coords, 1)
    rng = np.random.default_rng(3)
    _equal_to_oracle(np.ascontiguousarray(coords[rng.permutation(len(coords))]), 1)     # rows not grouped by sample


def test_equals_the_oracle_on_a_stride_3_tensor():
    coords, _, _, _ = make_batch([44, 45], n_points=2000)
    c3 = coords.copy()
    c3[:, 1:] *= 3
    assert (c3[:, 1:] < 0).any()
    _equal_to_oracle(c3, 3)


def test_floor_cells_by_hand():
    rows = np.array([[0, -1, 0, 1], [0, -2, 1, 0], [0, 3, -3, -4], [1, -1, 0, 1], [0, 2, -4, -3]], np.int32)
    got, cell = mref.coordmap_stride(rows, 1, 2)
    # -1 // 2 = -1: the cell of -1 is -2, not 0; rows 0 and 1 share a cell, so do rows 2 and 4; row 3 is another sample
    assert cell == 2
    assert got.tolist() == [[0, -2, 0, 0], [0, 2, -4, -4], [1, -2, 0, 0]]
    got, cell = mref.coordmap_stride(np.array([[0, -7, 7, -6]], np.int32), 3, 2)
    assert cell == 6 and got.tolist() == [[0, -12, 6, -6]]
    # the lower edge: -32767 at cell 2 lands on -32768, which is outside the range; -32766 stays inside
    edge = np.array([[0, -32767, 5, 5], [0, -32766, 5, 5]], np.int32)
    assert mref.all_in_range(edge)
    got, _ = mref.coordmap_stride(edge, 1, 2)
    assert got.tolist() == [[0, -32768, 4, 4], [0, -32766, 4, 4]]
    assert not mref.all_in_range(got) and mref.all_in_range(got[1:])
    # -32761 at cells 2, 4, 8: -32762, -32764, -32768; -32760 stays at -32760
    lv = mref.chain(np.array([[0, -32761, 0, 0], [0, -32760, 8, 0]], np.int32), 4)
    assert [c[:, 1].tolist() for c, _ in lv] == [[-32761, -32760], [-32762, -32760], [-32764, -32760], [-32768, -32760]]
    assert [s for _, s in lv] == [1, 2, 4, 8]
    assert [mref.all_in_range(c) for c, _ in lv] == [True, True, True, False]


def test_range_by_hand():
    assert mref.in_range(0, 32767, -32767, 0) and mref.in_range(65534, 32767, 32767, 32767)
    assert not mref.in_range(65535, 0, 0, 0) and not mref.in_range(-1, 0, 0, 0)
    assert not mref.in_range(0, 32768, 0, 0) and not mref.in_range(0, 0, -32768, 0) and not mref.in_range(0, 0, 0, 32768)


def test_a_corner_voxel_and_its_27_neighbours_by_hand():
    # row i of a sample: the corner minus bit 0 / 1 / 2 of i along x / y / z -- the corner itself is row 0, the 2x2x2 block
    # is all of its 3x3x3 neighbourhood that is in range
    block = [[32767 - (i & 1), 32767 - ((i >> 1) & 1), 32767 - ((i >> 2) & 1)] for i in range(8)]
    rows = np.array([[0] + p for p in block] + [[65534] + p for p in block], np.int32)
    nbr = mref.kernel_map(rows, 1, rows, 1)
    want = [7, 6, -1, 5, 4, -1, -1, -1, -1,          # dz = -1: (dx, dy) = (-1,-1) (0,-1) (1,-1) (-1,0) (0,0) (1,0) (.,1)
            3, 2, -1, 1, 0, -1, -1, -1, -1,          # dz = 0
            -1, -1, -1, -1, -1, -1, -1, -1, -1]      # dz = +1: outside the range
    assert nbr[0].tolist() == want
    assert nbr[8].tolist() == [v + 8 if v >= 0 else -1 for v in want]       # the other sample finds its own rows only
    # the opposite corner of the block sees all eight rows, through the mirrored offsets
    assert nbr[7, 13] == 7 and nbr[7, 26] == 0 and nbr[7, 14] == 6 and int((nbr[7] >= 0).sum()) == 8
    assert int((nbr >= 0).sum()) == 2 * 64           # any two rows of a 2x2x2 block are neighbours: 8 x 8 pairs per sample
    k, i, o = mref.triples(nbr)
    assert len(k) == 128 and k.tolist() == sorted(k.tolist())
    assert all(nbr[oo, kk] == ii for kk, ii, oo in zip(k.tolist(), i.tolist(), o.tolist()))
    assert all(o[j] < o[j + 1] for j in range(127) if k[j] == k[j + 1])
    # the negative corner, mirrored
    neg = rows.copy()
    neg[:, 1:] = -neg[:, 1:]
    nn = mref.kernel_map(neg, 1, neg, 1)
    assert nn[0].tolist() == [want[26 - kk] for kk in range(27)]


def test_strided_and_transposed_senses_by_hand():
    fine = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 1, 1], [0, -1, 0, 0], [0, 2, 0, 0]], np.int32)
    coarse, cell = mref.coordmap_stride(fine, 1, 2)
    assert cell == 2 and coarse.tolist() == [[0, 0, 0, 0], [0, -2, 0, 0], [0, 2, 0, 0]]
    s = mref.kernel_map(fine, 1, coarse, 2)                     # out row o gathers fine rows at o + delta
    assert {kk: int(v) for kk, v in enumerate(s[0]) if v >= 0} == {13: 0, 14: 1, 26: 2, 12: 3}
    assert {kk: int(v) for kk, v in enumerate(s[1]) if v >= 0} == {14: 3}
    assert {kk: int(v) for kk, v in enumerate(s[2]) if v >= 0} == {13: 4, 12: 1, 24: 2}
    t = mref.kernel_map(coarse, 2, fine, 1, transposed=True)    # the same pairs with in / out swapped, the same k
    pairs_s = {(kk, int(s[o, kk]), o) for o in range(3) for kk in range(27) if s[o, kk] >= 0}
    pairs_t = {(kk, o, int(t[o, kk])) for o in range(5) for kk in range(27) if t[o, kk] >= 0}
    assert pairs_s == pairs_t and len(pairs_s) == 8
    with pytest.raises(AssertionError):
        mref.kernel_map(fine, 1, coarse, 2, transposed=True)
    with pytest.raises(AssertionError):
        mref.row_index(np.array([[0, 1, 2, 3], [0, 1, 2, 3]], np.int32))
