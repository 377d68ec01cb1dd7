"""Sparse convolution backward: cs_conv_wgrad (weight gradient) and the data gradient through cs_conv_fwd on the
reverse kernel map, against f64 restatements over the exported kernel-map triples and against a dense conv3d."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.helpers import make_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CHANNELS = [(1, 32), (32, 32), (32, 64), (64, 64), (64, 128), (256, 128), (96, 64), (64, 16)]
STRIDED = [("s1_s2", "s2_s1_T"), ("s2_s4", "s4_s2_T"), ("s4_s8", "s8_s4_T")]
# map of each case -> its reverse map (the data gradient's map); None = 1x1
CASES = {"s1": "s1", "s1_s2": "s2_s1_T", "s2_s1_T": "s1_s2", "1x1": None}


@pytest.fixture(scope="module")
def maps(gpu):
    from corsair_amd import engine

    coords, _, _, _ = make_batch([0, 1, 2], 6000)
    return engine.BatchMaps(torch.from_numpy(coords).to(gpu))


def _triples(km):
    k, i, o = km.export()
    return k.cpu().numpy().astype(np.int64), i.cpu().numpy().astype(np.int64), o.cpu().numpy().astype(np.int64)


def _sizes(maps, name):
    if name == "1x1":
        return maps.c1.n, maps.c1.n
    km = getattr(maps, name)
    return km.n_in, km.n_out


def _ref_wgrad(km, x, g):
    """f64 dW and the per-element scale sum |x||g| over the exported triples (identity pairs for 1x1)."""
    x, g = x.astype(np.float64), g.astype(np.float64)
    if km is None:
        return x.T @ g, np.abs(x).T @ np.abs(g), None
    k, i, o = _triples(km)
    dw = np.zeros((km.kvol, x.shape[1], g.shape[1]))
    sc = np.zeros_like(dw)
    for kk in range(km.kvol):
        sel = k == kk
        dw[kk] = x[i[sel]].T @ g[o[sel]]
        sc[kk] = np.abs(x[i[sel]]).T @ np.abs(g[o[sel]])
    if km.kvol == 1:   # kernel size 1: the kernel is [cin, cout]
        return dw[0], sc[0], None
    return dw, sc, np.bincount(k, minlength=27)


def _ref_dgrad(km, g, w, n_in):
    g, w = g.astype(np.float64), w.astype(np.float64)
    if km is None:
        return g @ w.T, np.abs(g) @ np.abs(w).T
    k, i, o = _triples(km)
    w = w.reshape(km.kvol, w.shape[-2], w.shape[-1])
    dx = np.zeros((n_in, w.shape[1]))
    sc = np.zeros_like(dx)
    for kk in range(km.kvol):
        sel = k == kk
        np.add.at(dx, i[sel], g[o[sel]] @ w[kk].T)
        np.add.at(sc, i[sel], np.abs(g[o[sel]]) @ np.abs(w[kk]).T)
    return dx, sc


def test_reverse_map_identities(maps):
    """Strided map == its transposed map with in/out swapped (same k); stride-1 tables are their own reverse."""
    for fwd, tr in STRIDED:
        a, b = getattr(maps, fwd), getattr(maps, tr)
        ka, ia, oa = _triples(a)
        kb, ib, ob = _triples(b)
        assert len(ka) == len(kb) > 0
        sa = np.lexsort((ia, oa, ka))
        sb = np.lexsort((ob, ib, kb))
        assert np.array_equal(ka[sa], kb[sb]) and np.array_equal(ia[sa], ob[sb]) and np.array_equal(oa[sa], ib[sb])
    for name in ("s1", "s2", "s4", "s8"):
        t = getattr(maps, name).table().cpu().numpy()
        o, k = np.nonzero(t >= 0)
        assert np.array_equal(t[t[o, k], 26 - k], o), name


def _wgrad_case(gpu, maps, name, cin, cout, seed, slices=False):
    from corsair_amd import backend as B

    rng = np.random.default_rng(seed)
    km = None if name == "1x1" else getattr(maps, name)
    n_in, n_out = _sizes(maps, name)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    g = rng.standard_normal((n_out, cout)).astype(np.float32)
    if slices:   # column slices of wider buffers (the decoder inputs are slices of the concat buffers)
        xw = torch.zeros((n_in, cin + 40), device=gpu)
        gw = torch.zeros((n_out, cout + 24), device=gpu)
        xw[:, 8:8 + cin] = torch.from_numpy(x).to(gpu)
        gw[:, 16:16 + cout] = torch.from_numpy(g).to(gpu)
        xt, gt = xw[:, 8:8 + cin], gw[:, 16:16 + cout]
    else:
        xt, gt = torch.from_numpy(x).to(gpu), torch.from_numpy(g).to(gpu)
    got = B.conv_wgrad(km, xt, gt)
    again = B.conv_wgrad(km, xt, gt)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "wgrad is not bit-identical run to run"
    ref, sc, counts = _ref_wgrad(km, x, g)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= 4e-5 * sc + 1e-30), (name, cin, cout, np.max(np.abs(got - ref) - 4e-5 * sc))
    if counts is not None:
        empty = counts == 0
        assert np.all(got[empty] == 0.0)
    return x, g


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_matches_f64(gpu, maps, name, cin, cout):
    _wgrad_case(gpu, maps, name, cin, cout, seed=cin * 1000 + cout)


@pytest.mark.parametrize("name", ["s1", "s2_s1_T"])
def test_wgrad_column_slices(gpu, maps, name):
    _wgrad_case(gpu, maps, name, 64, 64, seed=5, slices=True)


def test_wgrad_empty_offsets_are_zero(gpu, maps):
    """A transposed map leaves most offsets of most rows empty; a one-cloud 1-row map leaves all but k = 13 empty."""
    from corsair_amd import backend as B

    c = torch.tensor([[0, 0, 0, 0]], dtype=torch.int32, device=gpu)
    m = B.CoordMap.create(c)
    km = B.KernelMap.build(m, m, 3)
    dw = B.conv_wgrad(km, torch.ones((1, 32), device=gpu), torch.full((1, 32), 2.0, device=gpu)).cpu()
    assert torch.all(dw[13] == 2.0) and int((dw != 0).sum()) == 32 * 32


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("name", list(CASES))
def test_dgrad_matches_f64(gpu, maps, name, cin, cout):
    from corsair_amd import backend as B

    rng = np.random.default_rng(7 + cin * 1000 + cout)
    km = None if name == "1x1" else getattr(maps, name)
    rev = None if CASES[name] is None else getattr(maps, CASES[name])
    n_in, n_out = _sizes(maps, name)
    g = rng.standard_normal((n_out, cout)).astype(np.float32)
    w = rng.standard_normal((cin, cout) if km is None else (27, cin, cout)).astype(np.float32)
    got = B.conv_dgrad(km, rev, torch.from_numpy(g).to(gpu), torch.from_numpy(w).to(gpu))
    again = B.conv_dgrad(km, rev, torch.from_numpy(g).to(gpu), torch.from_numpy(w).to(gpu))
    assert torch.equal(got, again)
    ref, sc = _ref_dgrad(km, g, w, n_in)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == (n_in, cin)
    assert np.all(np.abs(got - ref) <= 4e-5 * sc + 1e-30), (name, cin, cout)


def _shim():
    sys.path.insert(0, os.path.join(ROOT, "shim"))
    import MinkowskiEngine as ME

    return ME


@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 32), (96, 64), (64, 16)])
def test_shim_backward_matches_f64(gpu, cin, cout):
    """loss.backward() through shim modules: stride-1, stride-2, transposed and 1x1 (with bias) convolutions; input and
    weight gradients against the f64 restatement over the manager's own maps."""
    ME = _shim()
    coords, _, _, _ = make_batch([3, 4], 5000)
    rng = np.random.default_rng(cin + cout)
    ct = torch.from_numpy(coords).to(gpu)
    cm = ME.CoordinateManager()
    torch.manual_seed(cin * 7 + cout)
    convs = [ME.MinkowskiConvolution(cin, cout, kernel_size=3, stride=1, dimension=3),
             ME.MinkowskiConvolution(cin, cout, kernel_size=3, stride=2, dimension=3),
             None,
             ME.MinkowskiConvolution(cin, cout, kernel_size=1, stride=1, bias=True, dimension=3)]
    x0 = ME.SparseTensor(torch.zeros((len(coords), cin), device=gpu), ct, coordinate_manager=cm)
    coarse = ME.MinkowskiConvolution(cin, cin, kernel_size=3, stride=2, dimension=3).to(gpu)
    with torch.no_grad():
        xc = coarse(x0)   # makes the stride-2 map, the transposed convolution's input
    convs[2] = ME.MinkowskiConvolutionTranspose(cin, cout, kernel_size=3, stride=2, dimension=3)
    for j, conv in enumerate(convs):
        conv = conv.to(gpu)
        base = xc if j == 2 else x0
        f = rng.standard_normal((base.F.shape[0], cin)).astype(np.float32)
        ft = torch.from_numpy(f).to(gpu).requires_grad_(True)
        x = ME.SparseTensor(ft, coordinate_map_key=base.coordinate_map_key, coordinate_manager=cm)
        y = conv(x)
        r = rng.standard_normal(tuple(y.F.shape)).astype(np.float32)
        (y.F * torch.from_numpy(r).to(gpu)).sum().backward()
        w = conv.kernel.detach().cpu().numpy()
        if j == 3:
            km = None
        elif j == 2:
            km = cm.kernel_map(x.coordinate_map_key, y.coordinate_map_key, 3, True)
        else:
            km = cm.kernel_map(x.coordinate_map_key, y.coordinate_map_key, 3, False)
        ref_dw, sc_w, _ = _ref_wgrad(km, f, r)
        ref_dx, sc_x = _ref_dgrad(km, r, w, f.shape[0])
        gw = conv.kernel.grad.cpu().numpy().astype(np.float64)
        gx = ft.grad.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(gw - ref_dw) <= 4e-5 * sc_w + 1e-30), j
        assert np.all(np.abs(gx - ref_dx) <= 4e-5 * sc_x + 1e-30), j
        if conv.bias is not None:
            assert np.allclose(conv.bias.grad.cpu().numpy().reshape(-1), r.astype(np.float64).sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_matches_dense_conv3d(gpu, stride):
    """Independent of the kernel-map builder: a random occupied subset of an 8^3 grid, MinkowskiConvolution against
    CPU f64 conv3d (padding 1, zero-filled grid) sampled at the active sites, forward and backward."""
    ME = _shim()
    rng = np.random.default_rng(11 + stride)
    cin, cout = 32, 32
    occ = np.argwhere(rng.random((8, 8, 8)) < 0.35)
    coords = np.concatenate([np.zeros((len(occ), 1), np.int64), occ], 1).astype(np.int32)
    f = rng.standard_normal((len(occ), cin)).astype(np.float32)
    torch.manual_seed(stride)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=3, stride=stride, dimension=3).to(gpu)
    ft = torch.from_numpy(f).to(gpu).requires_grad_(True)
    x = ME.SparseTensor(ft, torch.from_numpy(coords).to(gpu))
    y = conv(x)
    out_c = y.C.cpu().numpy()
    r = rng.standard_normal(tuple(y.F.shape)).astype(np.float32)
    (y.F * torch.from_numpy(r).to(gpu)).sum().backward()

    fd = torch.from_numpy(f).double().requires_grad_(True)
    W = torch.from_numpy(conv.kernel.detach().cpu().numpy()).double().requires_grad_(True)   # [27, cin, cout]
    # k = (dx+1) + 3(dy+1) + 9(dz+1)  ->  dense weight [cout, cin, dx, dy, dz] over a grid indexed [x, y, z]
    Wd = W.reshape(3, 3, 3, cin, cout).permute(4, 3, 2, 1, 0)
    X = torch.zeros((cin, 8, 8, 8), dtype=torch.float64)
    X[:, occ[:, 0], occ[:, 1], occ[:, 2]] = fd.T
    Y = torch.nn.functional.conv3d(X.unsqueeze(0), Wd, stride=stride, padding=1)[0]
    p = torch.from_numpy(out_c[:, 1:] // stride).long()
    yd = Y[:, p[:, 0], p[:, 1], p[:, 2]].T
    (yd * torch.from_numpy(r).double()).sum().backward()
    assert np.allclose(y.F.detach().cpu().numpy(), yd.detach().numpy(), rtol=1e-5, atol=1e-5)
    assert np.allclose(ft.grad.cpu().numpy(), fd.grad.numpy(), rtol=1e-4, atol=1e-4)
    assert np.allclose(conv.kernel.grad.cpu().numpy(), W.grad.numpy(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("transposed", [False, True])
def test_shim_kernel1_stride2_backward_matches_f64(gpu, transposed):
    """Kernel size 1 with stride 2 (plain: fine -> coarse, transposed: coarse -> fine) runs on a strided map of kernel
    volume 1: the kernel is [cin, cout], the data gradient uses the opposite map with W^T."""
    ME = _shim()
    coords, _, _, _ = make_batch([5, 6], 4000)
    rng = np.random.default_rng(21 + transposed)
    cm = ME.CoordinateManager()
    cin, cout = 64, 32
    x0 = ME.SparseTensor(torch.zeros((len(coords), cin), device=gpu), torch.from_numpy(coords).to(gpu),
                         coordinate_manager=cm)
    torch.manual_seed(3)
    down = ME.MinkowskiConvolution(cin, cin, kernel_size=1, stride=2, dimension=3).to(gpu)
    base = x0
    if transposed:
        with torch.no_grad():
            base = down(x0)   # the coarse map is the transposed convolution's input
        conv = ME.MinkowskiConvolutionTranspose(cin, cout, kernel_size=1, stride=2, dimension=3).to(gpu)
    else:
        conv = ME.MinkowskiConvolution(cin, cout, kernel_size=1, stride=2, dimension=3).to(gpu)
    f = rng.standard_normal((base.F.shape[0], cin)).astype(np.float32)
    ft = torch.from_numpy(f).to(gpu).requires_grad_(True)
    x = ME.SparseTensor(ft, coordinate_map_key=base.coordinate_map_key, coordinate_manager=cm)
    y = conv(x)
    r = rng.standard_normal(tuple(y.F.shape)).astype(np.float32)
    (y.F * torch.from_numpy(r).to(gpu)).sum().backward()
    km = cm.kernel_map(x.coordinate_map_key, y.coordinate_map_key, 1, transposed)
    assert km.kvol == 1 and km.num_pairs > 0
    w = conv.kernel.detach().cpu().numpy()
    ref_dw, sc_w, _ = _ref_wgrad(km, f, r)
    ref_dx, sc_x = _ref_dgrad(km, r, w, f.shape[0])
    assert conv.kernel.grad.shape == conv.kernel.shape == (cin, cout)
    assert np.all(np.abs(conv.kernel.grad.cpu().numpy() - ref_dw) <= 4e-5 * sc_w + 1e-30)
    assert np.all(np.abs(ft.grad.cpu().numpy() - ref_dx) <= 4e-5 * sc_x + 1e-30)


def test_broadcast_output_gradient(gpu):
    """An output gradient that is a broadcast view (row stride 0, from `.sum(0)`) is made row-major before the HIP
    entry points see it."""
    ME = _shim()
    coords, _, _, _ = make_batch([7], 3000)
    rng = np.random.default_rng(4)
    f = rng.standard_normal((len(coords), 32)).astype(np.float32)
    ft = torch.from_numpy(f).to(gpu).requires_grad_(True)
    x = ME.SparseTensor(ft, torch.from_numpy(coords).to(gpu))
    torch.manual_seed(4)
    conv = ME.MinkowskiConvolution(32, 32, kernel_size=3, stride=1, dimension=3).to(gpu)
    y = conv(x)
    y.F.sum(0).sum().backward()
    km = x.coordinate_manager.kernel_map(x.coordinate_map_key, y.coordinate_map_key, 3, False)
    ones = np.ones(tuple(y.F.shape), np.float32)
    ref_dw, sc_w, _ = _ref_wgrad(km, f, ones)
    ref_dx, sc_x = _ref_dgrad(km, ones, conv.kernel.detach().cpu().numpy(), f.shape[0])
    assert np.all(np.abs(conv.kernel.grad.cpu().numpy() - ref_dw) <= 4e-5 * sc_w + 1e-30)
    assert np.all(np.abs(ft.grad.cpu().numpy() - ref_dx) <= 4e-5 * sc_x + 1e-30)
