"""Pins of the oracle functions that the operator-level GPU tests (test_gpu_operator_contract.py) trust, at odd
shapes, against plain NumPy definitions written here: the epilogue of include/corsair_hip.h (oracle.native.affine_act
and the tail of oracle.native.conv_fwd), oracle.native.row_l2_normalize and oracle.sparse.segmented_max."""
import numpy as np
import pytest

from oracle import sparse as osp
from tests.helpers import EPILOGUES, epilogue_args

CHANNELS = [1, 3, 17, 65, 200]
U = 2.0 ** -24   # f32 unit roundoff


def _fma_f32(a, b, c):
    """round_f32(a * b + c) with ONE rounding, for f32 arrays.  The f64 product of two f32 values is exact (48 bits);
    the f64 sum is rounded to ODD when inexact (TwoSum gives the sign of what was lost), and a value rounded to odd at
    53 bits rounds to f32 exactly as the infinitely precise one does (no double rounding)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def _epilogue(v, scale, shift, residual, relu):
    """The header's formula, every step one f32 operation: v = scale ? fma(v, scale, shift) : (shift ? v + shift : v);
    v = residual ? v + residual : v; v = relu ? max(v, 0) : v."""
    v = v.astype(np.float32)
    if scale is not None:
        v = _fma_f32(v, scale[None, :], shift[None, :])
    elif shift is not None:
        v = v + shift[None, :]
    if residual is not None:
        v = v + residual
    if relu:
        v = np.maximum(v, np.float32(0))
    assert v.dtype == np.float32
    return v


def test_fma_helper_is_a_single_rounding():
    """A case where rounding the f64 sum to nearest first would round twice (a * b = 1 + 2^-11 + 2^-24 is the midpoint
    of two f32 values, c = 2^-60 lifts it above the midpoint by less than the f64 spacing), and random triples against
    exact rational arithmetic."""
    from fractions import Fraction

    rng = np.random.default_rng(1)
    a = np.concatenate([[1 + 2.0 ** -12], rng.standard_normal(500)]).astype(np.float32)
    b = np.concatenate([[1 + 2.0 ** -12], rng.standard_normal(500)]).astype(np.float32)
    c = np.concatenate([[2.0 ** -60], rng.standard_normal(500) * 10.0 ** rng.integers(-9, 3, 500)]).astype(np.float32)
    got = _fma_f32(a, b, c)
    assert got[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert np.float32(np.float64(a[0]) * np.float64(b[0]) + np.float64(c[0])) != got[0]   # the naive f64 route is wrong here
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        mid = np.float32(float(exact))
        cands = [np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf))]
        errs = [abs(Fraction(float(f)) - exact) for f in cands]
        assert abs(Fraction(float(got[i])) - exact) == min(errs), i   # a nearest f32 (ties do not occur in this data)


@pytest.mark.parametrize("c", CHANNELS)
def test_affine_act_is_the_header_epilogue(oracle_native, c):
    rng = np.random.default_rng(100 + c)
    n = 7
    x = rng.standard_normal((n, c)).astype(np.float32)
    for combo in EPILOGUES:
        scale, shift, residual, relu = epilogue_args(rng, n, c, combo)
        want = _epilogue(x, scale, shift, residual, relu)
        got = oracle_native.affine_act(x, scale, shift, residual, relu)
        assert got.dtype == np.float32 and np.array_equal(got, want), (c, combo)


@pytest.mark.parametrize("cin,cout", [(1, 3), (3, 17), (17, 65), (65, 200), (200, 1)])
def test_conv_fwd_epilogue_and_chain(oracle_native, cin, cout):
    """conv_fwd with an epilogue == the header's epilogue applied to conv_fwd without one (equality), for a 27-offset
    table with absent neighbours and for the 1x1 form; and the plain accumulation against f64: one f32 fma chain of
    L = (present offsets) * cin terms is off by at most L u sum|x||w| (each partial sum is bounded by the sum of the
    absolute terms and is rounded once)."""
    rng = np.random.default_rng(cin * 1000 + cout)
    n_in, n_out = 9, 6
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = rng.standard_normal((27, cin, cout)).astype(np.float32)
    nbr = rng.integers(-1, n_in, (n_out, 27)).astype(np.int32)
    nbr[0] = -1                                               # a row without any neighbour: exact zeros
    for table, xi, wi, rows in ((nbr, x, w, n_out), (None, x, w[13], n_in)):
        acc = oracle_native.conv_fwd(table, xi, wi)
        x64, w64 = xi.astype(np.float64), wi.astype(np.float64).reshape(-1, cin, cout)
        tab = table if table is not None else np.arange(n_in, dtype=np.int32)[:, None]
        ref = np.zeros((rows, cout))
        mag = np.zeros((rows, cout))
        for o in range(rows):
            for k in range(tab.shape[1]):
                if tab[o, k] >= 0:
                    ref[o] += x64[tab[o, k]] @ w64[k]
                    mag[o] += np.abs(x64[tab[o, k]]) @ np.abs(w64[k])
        terms = (tab >= 0).sum(1, keepdims=True) * cin
        assert np.all(np.abs(acc - ref) <= terms * U * mag)
        if table is not None:
            assert np.all(acc[0] == 0)
        for combo in EPILOGUES:
            scale, shift, residual, relu = epilogue_args(rng, rows, cout, combo)
            want = _epilogue(acc, scale, shift, residual, relu)
            got = oracle_native.conv_fwd(table, xi, wi, scale, shift, residual, relu)
            assert np.array_equal(got, want), (cin, cout, combo)


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("eps", [0.0, 1e-12])
def test_row_l2_normalize(oracle_native, c, eps):
    """out = x / max(||x||, eps) against f64.  Bound: the sum of c non-negative squares, in ANY order, rounds each
    product and each partial sum once, so no term passes through more than c roundings: relative error <= c u.  The
    square root halves it and rounds once, the division rounds once: (c / 2 + 2) u, plus one u for the second-order
    terms and the rounding of the f64 reference itself."""
    rng = np.random.default_rng(300 + c)
    x = rng.standard_normal((6, c)).astype(np.float32)
    x[1] *= 1e3
    x[2] *= 1e-3
    x[3] = 0.0                                                # zero row
    x[4] = np.float32(1e-20) * (1 + np.arange(c) % 3)         # norm far below eps = 1e-12 (f32 squares underflow)
    got = oracle_native.row_l2_normalize(x, eps)
    assert got.dtype == np.float32
    e32 = np.float64(np.float32(eps))
    x64 = x.astype(np.float64)
    nrm = np.maximum(np.sqrt((x64 * x64).sum(1, keepdims=True)), e32)
    live = [0, 1, 2, 5] + ([4] if eps > 0 else [])
    ref = x64[live] / nrm[live]
    bound = (c / 2 + 3) * U * np.abs(ref)
    assert np.all(np.abs(got[live] - ref) <= bound), float((np.abs(got[live] - ref) / np.maximum(bound, 1e-300)).max())
    if eps > 0:
        assert np.all(got[3] == 0)                            # 0 / eps
        assert np.array_equal(got[4], x[4] / np.float32(eps))  # clamped: one f32 division
    else:
        assert np.all(np.isnan(got[3]))                       # 0 / 0
    # unit rows: the property the network relies on
    assert np.all(np.abs(np.sqrt((got[[0, 1, 2, 5]].astype(np.float64) ** 2).sum(1)) - 1) <= (c / 2 + 3) * U * 2)


@pytest.mark.parametrize("c", CHANNELS)
def test_segmented_max(c):
    """Per-sample column max, rows not grouped by sample, an absent sample (-inf), exact ties, ids that name no sample.
    max is one exact operation: equality."""
    rng = np.random.default_rng(400 + c)
    n, nb = 41, 5
    x = rng.standard_normal((n, c)).astype(np.float32)
    x[7] = x[3]                                               # duplicated rows: exact ties
    batch = rng.integers(0, nb, n)
    batch[batch == 2] = 4                                     # sample 2 is absent
    batch[7] = batch[3]
    batch[[11, 19]] = [-1, nb]                                # out of range: contribute nowhere
    x[[11, 19]] = 1e9
    got = osp.segmented_max(x, batch, nb)
    want = np.full((nb, c), -np.inf)
    for r in range(n):
        if 0 <= batch[r] < nb:
            want[batch[r]] = np.maximum(want[batch[r]], x[r].astype(np.float64))
    assert got.dtype == np.float32 and got.shape == (nb, c)
    assert np.array_equal(got.astype(np.float64), want)
    assert np.all(np.isneginf(got[2])) and np.all(np.isfinite(got[[0, 1, 3, 4]]))
