"""Operator-level contract of the sparse-convolution entry points and the row operators: every kernel the dispatchers
can choose is reached BY ARGUMENTS (channel divisibility, pointer alignment, leading dimension, NULL epilogue pointers;
never by environment variables) and compared bit for bit (np.array_equal) with the CPU oracle evaluated on contiguous
copies of the same values.  Column views live in buffers pre-filled with a NaN sentinel: nothing outside an output
view may change, nothing outside an input view may reach a result.

Kernel each conv test is written to reach, by the dispatch conditions of cs_conv_fwd in conv.hip (equal bits cannot
tell kernels apart: which kernel ran is a matter for a kernel trace of this module, not for these assertions):
  k_conv_generic   test_conv_generic_by_channels, test_conv_alignment_fallback, test_conv_views[generic],
                   test_conv_epilogues[generic]
  k_conv_mfma      test_conv_register_staged_mfma, test_conv_views[mfma], test_conv_epilogues[mfma]
  k_conv_dma       test_conv_lds_dma (gathered and 1x1 forms), test_conv_alignment_fallback (its contiguous calls),
                   test_conv_views[dma, 1x1], test_conv_epilogues[dma, 1x1]
  k_conv_stem      test_conv_stem_reads_a_column, test_conv_views[stem]
and cs_conv_wgrad (conv_bwd.hip): k_wgrad_mfma by the (64, 64) cases, k_wgrad_valu by the (48, 20) cases of
test_wgrad_slices_and_odd_leading_dimensions / test_wgrad_chunk_boundaries."""
import zlib

import numpy as np
import pytest
import torch

from corsair_amd import _lib, backend as B
from oracle import sparse as osp
from tests.helpers import (EPILOGUES, column_view, epilogue_args, make_batch, outside_view_untouched, sentinel_buffer)
from tests.test_gpu_conv_backward import _ref_wgrad

pytestmark = pytest.mark.gpu

CONV_ENV = ("CS_CONV_DMA", "CS_CONV_CFG", "CS_CONV_FWD_ORDER", "CS_CONV_TRACE")
FULL = ("scale+shift", True, True)


@pytest.fixture(autouse=True)
def _default_dispatch(monkeypatch):
    for name in CONV_ENV:
        monkeypatch.delenv(name, raising=False)


class _Batch:
    pass


@pytest.fixture(scope="module")
def batch(gpu):
    """One collated batch with an empty sample (index 2) and ragged last tiles (rows not a multiple of 32), its
    stride-1, strided and transposed maps on the device and the oracle's tables of the same maps."""
    coords, _, _, _ = make_batch([3, 4, 5], n_points=1200)
    coords[coords[:, 0] == 2, 0] = 3
    c2, _ = osp.coordmap_stride(coords, 1, 2)
    n1, n2 = len(coords), len(c2)
    assert n1 % 32 and n1 % 128 and n2 % 32 and n1 < 5000
    ct = torch.from_numpy(coords).to(gpu)
    m1, m2 = B.CoordMap.pyramid(ct, 2, 0)
    kms = B.KernelMap.build_many([(m1, m1), (m1, m2), (m2, m1, 3, True)])
    tables = [osp.kernel_map(coords, 1, coords, 1), osp.kernel_map(coords, 1, c2, 2),
              osp.kernel_map(c2, 2, coords, 1, transposed=True)]
    b = _Batch()
    b.gpu, b.coords, b.n1, b.n2 = gpu, coords, n1, n2
    b.maps = {"1x1": (None, None, n1, n1)}
    for name, km, t in zip(("s1", "s1_s2", "s2_s1_T"), kms, tables):
        assert np.array_equal(km.table().cpu().numpy(), t), name
        b.maps[name] = (km, t, km.n_in, km.n_out)
    return b


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(a).to(gpu)


def _conv_values(batch, kind, cin, cout, combo, seed=0):
    _, _, n_in, n_out = batch.maps[kind]
    rng = np.random.default_rng([seed, cin, cout, zlib.crc32(kind.encode())])
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = (rng.standard_normal((cin, cout) if kind == "1x1" else (27, cin, cout)) * 0.1).astype(np.float32)
    return (x, w) + epilogue_args(rng, n_out, cout, combo)


def _conv_check(batch, oracle_native, kind, cin, cout, combo=FULL, views=(None,), seed=0):
    """cs_conv_fwd against the oracle for every entry of `views`: None (contiguous tensors) or a dict with optional
    keys x / out / res = (first column, leading dimension).  Returns the results (all equal to the oracle's)."""
    gpu = batch.gpu
    km, table, n_in, n_out = batch.maps[kind]
    x, w, scale, shift, res, relu = _conv_values(batch, kind, cin, cout, combo, seed)
    want = oracle_native.conv_fwd(table, x, w, scale, shift, res, relu)
    assert want.shape == (n_out, cout) and not np.isnan(want).any()
    wd, sd, hd = _dev(w, gpu), _dev(scale, gpu), _dev(shift, gpu)
    got_all = []
    for view in views:
        view = view or {}
        _, xv = column_view(x, gpu, *view.get("x", (0, None)))
        rv = None
        if res is not None:
            _, rv = column_view(res, gpu, *view.get("res", (0, None)))
        ow = ov = None
        if "out" in view:
            c0, ld = view["out"]
            ow = sentinel_buffer(n_out, ld, gpu)
            ov = ow[:, c0:c0 + cout]
        got = B.conv_fwd(km, xv, wd, sd, hd, rv, relu, out=ov)
        if ov is not None:
            assert got.data_ptr() == ov.data_ptr() and got.stride(0) == ld
            assert outside_view_untouched(ow, c0, cout), (kind, cin, cout, combo, view)
        got = got.cpu().numpy()
        assert not np.isnan(got).any(), (kind, cin, cout, combo, view)
        assert np.array_equal(got, want), (kind, cin, cout, combo, view, float(np.abs(got - want).max()))
        got_all.append(got)
    return got_all


KINDS = ["s1", "s1_s2", "s2_s1_T", "1x1"]


# ---- cs_conv_fwd: one kernel per set of arguments ----------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(3, 5), (8, 8), (17, 33), (48, 32), (1, 16), (1, 32)])
def test_conv_generic_by_channels(batch, oracle_native, cin, cout):
    """cin % 32 != 0 or cout % 4 != 0 -> k_conv_generic.  (1, 32) is the stem's shape: only its 1x1 form (km None,
    kernel volume 1) is not the stem kernel's, so that is the form run for it."""
    for kind in (["1x1"] if (cin, cout) == (1, 32) else KINDS):
        _conv_check(batch, oracle_native, kind, cin, cout)


@pytest.mark.parametrize("cin,cout", [(32, 4), (64, 48), (32, 100)])
def test_conv_register_staged_mfma(batch, oracle_native, cin, cout):
    """cin % 32 == 0, cout % 4 == 0, cout % 32 != 0 -> k_conv_mfma (a ragged last column tile at cout 4, 48, 100)."""
    for kind in KINDS:
        _conv_check(batch, oracle_native, kind, cin, cout)


@pytest.mark.parametrize("kind,cin,cout", [("s1", 32, 32), ("s1_s2", 32, 32), ("s2_s1_T", 32, 32), ("s1", 64, 128),
                                           ("s1_s2", 64, 128), ("s2_s1_T", 64, 128), ("1x1", 128, 64)])
def test_conv_lds_dma(batch, oracle_native, kind, cin, cout):
    """cin % 32 == 0 and cout % 32 == 0, aligned -> k_conv_dma (4x1x1 tiles at cout 32, 1x4x1 at 128, 2x2x1 at 64;
    the 1x1 form is its GATHER = false instantiation)."""
    _conv_check(batch, oracle_native, kind, cin, cout)


@pytest.mark.parametrize("kind", ["s1", "s1_s2", "s2_s1_T"])
def test_conv_stem_reads_a_column(batch, oracle_native, kind):
    """(1, 32) with a 27-offset map -> k_conv_stem; the single input channel is column 0, 2 or 6 of a wider buffer
    (ld_in 1, 3, 7) whose other columns hold NaN."""
    got = _conv_check(batch, oracle_native, kind, 1, 32,
                      views=[None, {"x": (0, 3)}, {"x": (2, 3)}, {"x": (6, 7), "out": (5, 41), "res": (1, 35)}])
    assert all(np.array_equal(g, got[0]) for g in got[1:])


@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("kind", ["s1", "s2_s1_T", "1x1"])
def test_conv_alignment_fallback(batch, oracle_native, kind, cin):
    """An MFMA-shaped layer whose input is not 16-byte aligned (a column slice starting at column 1, 2 or 3) or whose
    rows are not (ld_in = cin + 1, cin + 3 at the 4-aligned column 0: the only one such a buffer has room for) must
    give the contiguous call's bits.  The dispatcher's alignment terms are expected to send these to the scalar kernel;
    equal bits cannot tell which kernel ran."""
    views = [None] + [{"x": (c0, cin + 8)} for c0 in (1, 2, 3)] + [{"x": (0, cin + 1)}, {"x": (0, cin + 3)}]
    got = _conv_check(batch, oracle_native, kind, cin, cin, views=views)
    assert all(np.array_equal(g, got[0]) for g in got[1:])


KERNEL_SHAPES = {"generic": ("s1_s2", 8, 8), "mfma": ("s2_s1_T", 64, 48), "dma": ("s1", 32, 32), "1x1": ("1x1", 128, 64)}


@pytest.mark.parametrize("which", list(KERNEL_SHAPES) + ["stem"])
def test_conv_views(batch, oracle_native, which):
    """out as a slice at column 0 and at column 5 (not 16-byte aligned) with ld_out > cout, residual as a slice with
    ld_res != ld_out, input a slice too: the bits of the contiguous call, and not one element outside the output view
    written."""
    kind, cin, cout = KERNEL_SHAPES.get(which, ("s1", 1, 32))
    xin = (4, cin + 12) if which in ("mfma", "dma", "1x1") else (3, cin + 5)   # (4-aligned: stays on the MFMA kernels)
    views = [None,
             {"out": (0, cout + 7), "res": (2, cout + 3)},
             {"out": (5, cout + 9), "res": (0, cout + 1), "x": xin},
             {"out": (5, cout + 5), "res": (7, 2 * cout + 8), "x": xin}]
    got = _conv_check(batch, oracle_native, kind, cin, cout, views=views)
    assert all(np.array_equal(g, got[0]) for g in got[1:])


@pytest.mark.parametrize("combo", EPILOGUES, ids=lambda c: "%s-res%d-relu%d" % (c[0], c[1], c[2]))
@pytest.mark.parametrize("which", list(KERNEL_SHAPES))
def test_conv_epilogues(batch, oracle_native, which, combo):
    """scale+shift | shift | none  x  residual  x  relu on each kernel (NULL pointers select the branch); the residual
    is a slice so that the early residual loads of the DMA kernel use their own leading dimension."""
    kind, cin, cout = KERNEL_SHAPES[which]
    _conv_check(batch, oracle_native, kind, cin, cout, combo, views=[{"res": (1, cout + 6), "out": (0, cout + 2)}], seed=1)


def test_conv_refusals(batch):
    """Bad arguments: negative status, a cs_last_error text that names the entry point, output untouched."""
    gpu = batch.gpu
    lib = _lib.load()
    km, _, n_in, n_out = batch.maps["s1"]
    cin = cout = 32
    x = torch.zeros((n_in + 1, cin), device=gpu)
    w = torch.zeros((27, cin, cout), device=gpu)
    v = torch.ones(cout, device=gpu)
    res = torch.zeros((n_out, cout), device=gpu)
    out = sentinel_buffer(n_out, cout, gpu)
    p = _lib.ptr

    def call(km_=km, n_in_=n_in, n_out_=n_out, ld_in=cin, scale=None, shift=None, residual=None, ld_res=0, ld_out=cout):
        return lib.cs_conv_fwd(km_._h if km_ is not None else None, n_in_, n_out_, p(x), ld_in, cin, p(w), cout, p(scale),
                               p(shift), p(residual), ld_res, 1, p(out), ld_out, _lib.stream_ptr())

    cases = [("ld_in < cin", dict(ld_in=cin - 1), "leading dimension"),
             ("ld_out < cout", dict(ld_out=cout - 1), "leading dimension"),
             ("ld_res < cout", dict(residual=res, ld_res=cout - 1), "residual"),
             ("scale without shift", dict(scale=v), "scale without shift"),
             ("map rows != tensor rows (in)", dict(n_in_=n_in + 1), "kernel map is for"),
             ("map rows != tensor rows (out)", dict(n_out_=n_out - 1), "kernel map is for"),
             ("1x1 with n_in != n_out", dict(km_=None, n_in_=n_in, n_out_=n_in - 1), "n_in == n_out")]
    for what, kw, text in cases:
        rc = call(**kw)
        msg = lib.cs_last_error().decode()
        assert rc < 0, what
        assert "cs_conv_fwd" in msg and text in msg, (what, msg)
        with pytest.raises(_lib.CorsairHipError, match="cs_conv_fwd"):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert outside_view_untouched(out, 0, 0)
    assert call(shift=v) == 0                                   # the same arguments, legal: the call goes through
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()


# ---- cs_conv_wgrad ------------------------------------------------------------------------------------------
def _wgrad_check(gpu, km, x, g, views):
    """f64 restatement with the 4e-5 sum|x||g| bound of test_gpu_conv_backward.py for the contiguous call; every view
    (x first column, x ld, g first column, g ld) bit-identical to it (the header: fixed summation order, whatever the
    layout)."""
    ref, sc, counts = _ref_wgrad(km, x, g)
    base = B.conv_wgrad(km, _dev(x, gpu), _dev(g, gpu))
    got = base.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= 4e-5 * sc + 1e-30), float(np.max(np.abs(got - ref) - 4e-5 * sc))
    if counts is not None:
        assert np.all(got[counts == 0] == 0.0)
    for xc, xld, gc, gld in views:
        _, xv = column_view(x, gpu, xc, xld)
        _, gv = column_view(g, gpu, gc, gld)
        again = B.conv_wgrad(km, xv, gv)
        assert not torch.isnan(again).any()
        assert torch.equal(again, base), (xc, xld, gc, gld)


@pytest.mark.parametrize("cin,cout", [(64, 64), (48, 20)])
@pytest.mark.parametrize("kind", KINDS)
def test_wgrad_slices_and_odd_leading_dimensions(batch, kind, cin, cout):
    """(64, 64) -> k_wgrad_mfma, chosen from the channel counts alone; (48, 20) -> k_wgrad_valu.  x and g as slices
    at columns 1 and 3 (pointers that are not 16-byte aligned) and with odd leading dimensions."""
    km, _, n_in, n_out = batch.maps[kind]
    rng = np.random.default_rng([cin, cout, zlib.crc32(kind.encode())])
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    g = rng.standard_normal((n_out, cout)).astype(np.float32)
    _wgrad_check(batch.gpu, km, x, g, [(1, cin + 8, 3, cout + 8), (3, cin + 3, 1, cout + 1), (0, cin + 1, 0, cout + 3),
                                       (1, cin + 5, 0, None)])


@pytest.mark.parametrize("cin,cout", [(64, 64), (48, 20)])
@pytest.mark.parametrize("n", [100, 128, 256, 257])
def test_wgrad_chunk_boundaries(gpu, n, cin, cout):
    """Row chunks of cs_conv_wgrad: ceil(n / 128) chunks of ceil32(n / chunks) rows.  n = 100 and 128: one chunk (ragged /
    full); 256: exactly two chunks of 128; 257: three chunks of 96 rows, the last with 65.  Stride-1 map of the first n
    cells of a 7^3 block (every offset present), and the 1x1 form (chunk masks from the table scan)."""
    cells = np.stack(np.unravel_index(np.arange(n), (7, 7, 7)), 1)
    coords = np.concatenate([np.zeros((n, 1), np.int64), cells], 1).astype(np.int32)
    m = B.CoordMap.create(torch.from_numpy(coords).to(gpu))
    km = B.KernelMap.build(m, m, 3)
    assert km.n_out == n
    rng = np.random.default_rng([n, cin, cout])
    x = rng.standard_normal((n, cin)).astype(np.float32)
    g = rng.standard_normal((n, cout)).astype(np.float32)
    for k in (km, None):
        _wgrad_check(gpu, k, x, g, [(1, cin + 4, 3, cout + 5)])


# ---- cs_affine_act ------------------------------------------------------------------------------------------
def _affine_check(gpu, oracle_native, n, c, combo, rng, sliced):
    x = rng.standard_normal((n, c)).astype(np.float32)
    scale, shift, res, relu = epilogue_args(rng, n, c, combo)
    want = oracle_native.affine_act(x, scale, shift, res, relu)
    sd, hd = _dev(scale, gpu), _dev(shift, gpu)
    if not sliced:
        got = B.affine_act(_dev(x, gpu), sd, hd, _dev(res, gpu), relu).cpu().numpy()
        assert np.array_equal(got, want), (n, c, combo)
        xa = _dev(x, gpu)                                       # out aliasing in (SparseTensor.__iadd__ does this)
        B.affine_act(xa, sd, hd, _dev(res, gpu), relu, out=xa)
        assert np.array_equal(xa.cpu().numpy(), want), ("alias", n, c, combo)
        return
    _, xv = column_view(x, gpu, 3, c + 5)
    rv = column_view(res, gpu, 1, c + 2)[1] if res is not None else None
    ow = sentinel_buffer(n, c + 9, gpu)
    got = B.affine_act(xv, sd, hd, rv, relu, out=ow[:, 5:5 + c])
    assert outside_view_untouched(ow, 5, c)
    assert np.array_equal(got.cpu().numpy(), want), ("sliced", n, c, combo)
    xw, xv = column_view(x, gpu, 2, c + 3)                      # sliced and aliased
    B.affine_act(xv, sd, hd, rv, relu, out=xv)
    assert outside_view_untouched(xw, 2, c)
    assert np.array_equal(xv.cpu().numpy(), want), ("sliced alias", n, c, combo)


@pytest.mark.parametrize("c", [1, 3, 16, 17, 64, 100, 257])
def test_affine_act(gpu, oracle_native, c):
    rng = np.random.default_rng(500 + c)
    for n in (1, 255, 257):
        for combo in EPILOGUES:
            _affine_check(gpu, oracle_native, n, c, combo, rng, sliced=False)
            _affine_check(gpu, oracle_native, n, c, combo, rng, sliced=True)


@pytest.mark.parametrize("combo", [FULL, ("shift", False, True), ("none", True, False)])
def test_affine_act_grid_stride(gpu, oracle_native, combo):
    """n * c above the 4096 x 256 threads of the largest launch: the grid-stride loop takes a second trip."""
    n, c = 4100, 257
    assert n * c > 4096 * 256
    rng = np.random.default_rng(77)
    _affine_check(gpu, oracle_native, n, c, combo, rng, sliced=False)
    _affine_check(gpu, oracle_native, n, c, combo, rng, sliced=True)


def test_affine_act_refusals(gpu):
    lib = _lib.load()
    x = torch.zeros((4, 8), device=gpu)
    out = sentinel_buffer(4, 8, gpu)
    v = torch.ones(8, device=gpu)
    p = _lib.ptr
    for ld_in, ld_out, scale in ((7, 8, None), (8, 7, None), (8, 8, v)):
        rc = lib.cs_affine_act(4, 8, p(x), ld_in, p(scale), None, None, 0, 0, p(out), ld_out, _lib.stream_ptr())
        assert rc < 0 and "cs_affine_act" in lib.cs_last_error().decode()
    torch.cuda.synchronize()
    assert outside_view_untouched(out, 0, 0)


# ---- cs_row_l2_normalize ------------------------------------------------------------------------------------
def _equal_with_nan(got, want):
    """np.array_equal where both are numbers, NaN exactly where the oracle has NaN (0 / 0 of a zero row at eps = 0:
    the payload of that NaN is not part of the contract)."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


@pytest.mark.parametrize("eps", [0.0, 1e-12])
@pytest.mark.parametrize("c", [1, 3, 15, 16, 17, 32, 63, 64, 65, 128, 200, 256])
def test_row_l2_normalize(gpu, oracle_native, c, eps):
    """c <= 16: k_row_l2norm16 (16 lanes per row); above: k_row_l2norm (one wave per row; above 64 a lane adds several
    squares before the butterfly).  Both match the same oracle, so at c = 16 they agree with each other as the source
    comment claims.  Row counts that fill neither 4 rows per workgroup nor 16.  A zero row (NaN at eps = 0, zeros
    otherwise) and a row whose norm is below eps (all values normal f32 numbers, squares included)."""
    rng = np.random.default_rng(600 + c)
    for n in (1, 3, 37):
        x = rng.standard_normal((n, c)).astype(np.float32)
        if n == 37:
            x[5] = 0.0
            x[9] = np.float32(1e-14) * (1 + np.arange(c) % 3)   # norm <= 4.8e-13 < 1e-12
            x[20] *= 1e4
        want = oracle_native.row_l2_normalize(x, eps)
        if n == 37:
            assert np.isnan(want[5]).all() if eps == 0 else (want[5] == 0).all()
            if eps > 0:
                assert np.array_equal(want[9], x[9] / np.float32(eps))
        got = B.row_l2_normalize(_dev(x, gpu), eps).cpu().numpy()
        assert _equal_with_nan(got, want), (n, c, eps)
        _, xv = column_view(x, gpu, 1, c + 3)
        ow = sentinel_buffer(n, c + 6, gpu)
        got = B.row_l2_normalize(xv, eps, out=ow[:, 5:5 + c])
        assert outside_view_untouched(ow, 5, c)
        assert _equal_with_nan(got.cpu().numpy(), want), ("sliced", n, c, eps)


# ---- cs_segmented_max ---------------------------------------------------------------------------------------
# Finite inputs only: for NaN and for -0 against +0 the kernel orders the bit patterns (a total order), which differs
# from torch's max by design; that policy is not part of this contract.
@pytest.mark.parametrize("c", [1, 16, 256, 257, 300])
def test_segmented_max(gpu, c):
    """Sample boundaries at rows 31, 32, 33 and 64 (around the kernel's 32-row runs), an absent sample (-inf), exact ties,
    then the same rows shuffled (not grouped by sample) and rows whose batch id is < 0 or >= n_batch (they hold the
    largest values and must contribute nowhere).  The batch column is read from a coords tensor with batch_ld = 4, and
    once from a plain vector (batch_ld = 1); the input once as a slice.  c > 256: the second grid dimension."""
    rng = np.random.default_rng(700 + c)
    n, nb = 100, 6
    batch = np.repeat([0, 1, 2, 3, 5], [31, 1, 1, 31, 36])     # sample 4 is absent
    assert len(batch) == n
    x = np.round(rng.standard_normal((n, c)) * 2).astype(np.float32) / 2   # a coarse grid of values: many exact ties
    x[40] = x[35]
    x[70:75] = x[64]
    perm = rng.permutation(n)
    wild = batch.copy()
    wild[[0, 31, 32, 50, 64, 99]] = [-1, nb, -7, nb + 3, -1, nb]
    xw = x.copy()
    xw[[0, 31, 32, 50, 64, 99]] = 1e6
    for name, xs, bs in (("grouped", x, batch), ("shuffled", x[perm], batch[perm]), ("out-of-range ids", xw, wild),
                         ("out-of-range ids, shuffled", xw[perm], wild[perm])):
        want = osp.segmented_max(xs, bs, nb)
        assert np.isneginf(want[4]).all() and (want < 1e6).all()
        coords = np.zeros((n, 4), np.int32)
        coords[:, 0] = bs
        coords[:, 1:] = rng.integers(-50, 50, (n, 3))
        ct = torch.from_numpy(coords).to(gpu)
        got = B.segmented_max(_dev(xs, gpu), ct, nb).cpu().numpy()
        assert np.array_equal(got, want), (name, c)
        _, xv = column_view(xs, gpu, 3, c + 4)
        got = B.segmented_max(xv, ct[:, :1].contiguous(), nb).cpu().numpy()
        assert np.array_equal(got, want), (name, c, "sliced input, batch_ld 1")


# ---- cs_instance_norm ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 32, 257])
def test_instance_norm(gpu, c):
    """Sample lengths 255, 1, 0, 256, 513, 257 in one batch (around the 256-row chunks of the fixed summation order; the
    empty sample in the middle, a one-row sample whose variance is 0), weight and bias each present or NULL, contiguous
    and as slices; bit for bit against oracle.sparse.instance_norm.  c = 257: the second channel block of the grid."""
    rng = np.random.default_rng(800 + c)
    lens = [255, 1, 0, 256, 513, 257]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n = int(seg[-1])
    x = (rng.standard_normal((n, c)) * rng.uniform(0.5, 3, c) + rng.uniform(-2, 2, c)).astype(np.float32)
    sd = torch.from_numpy(seg).to(gpu)
    for has_w in (True, False):
        for has_b in (True, False):
            w = rng.uniform(0.5, 1.5, c).astype(np.float32) if has_w else None
            b = rng.standard_normal(c).astype(np.float32) if has_b else None
            want = osp.instance_norm(x, seg, w, b, 1e-8)
            got = B.instance_norm(_dev(x, gpu), sd, _dev(w, gpu), _dev(b, gpu), 1e-8).cpu().numpy()
            assert np.array_equal(got, want), (c, has_w, has_b)
            _, xv = column_view(x, gpu, 1, c + 2)
            ow = sentinel_buffer(n, c + 7, gpu)
            got = B.instance_norm(xv, sd, _dev(w, gpu), _dev(b, gpu), 1e-8, out=ow[:, 5:5 + c])
            assert outside_view_untouched(ow, 5, c)
            got = got.cpu().numpy()
            assert np.array_equal(got, want), ("sliced", c, has_w, has_b)
            assert np.all(got[255] == (b if has_b else 0))      # the one-row sample: (x - x) * inv_std * weight + bias
