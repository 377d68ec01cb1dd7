"""The hand-written backwards of corsair_amd/autograd.py, one operator at a time, against torch CPU f64 autograd of the
operator's plain definition written here.  Selections (max, ReLU, add) are compared with torch.equal.  For the others the
tolerance is not picked: the same definition is evaluated by torch CPU autograd in f32, its worst error against the f64
result relative to the absolute-value scale sum|terms| of each gradient element (the convention of
test_gpu_conv_backward.py) is the measured value, and the operator may be off by 4x that (its expressions may associate
differently; a wrong formula is off by orders of magnitude).  Every backward runs under
torch.use_deterministic_algorithms(True), twice, with equal bits."""
import numpy as np
import pytest
import torch

from corsair_amd import autograd as AG, backend as B, minkowski as ME
from tests.helpers import make_batch

pytestmark = pytest.mark.gpu


def _twice_deterministic(run):
    """run() -> tuple of tensors, evaluated twice under deterministic algorithms: equal bits (NaN = NaN)."""
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a, b = run(), run()
    finally:
        torch.use_deterministic_algorithms(prev)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "backward is not bit-identical run to run"
    return [t.detach().cpu() for t in a]


def _ratio(got, ref, scale):
    got, ref, scale = (np.asarray(t, dtype=np.float64) for t in (got, ref, scale))
    assert got.shape == ref.shape == scale.shape
    err = np.abs(got - ref)
    assert np.all(err[scale == 0] == 0)          # no terms: the element is exactly the reference's
    live = scale > 0
    return float((err[live] / scale[live]).max()) if live.any() else 0.0


def _within_4x(name, got, f32, f64, scale):
    measured = _ratio(f32, f64, scale)
    worst = _ratio(got, f64, scale)
    print(f"{name}: f32 CPU autograd is off by {measured:.3e} of sum|terms|, bound {4 * measured:.3e}, operator {worst:.3e}")
    assert worst <= 4 * measured, (name, worst, measured)


def _line_coords(n, gpu, batch=None):
    c = np.zeros((n, 4), np.int32)
    c[:, 1] = np.arange(n)
    if batch is not None:
        c[:, 0] = batch
    return torch.from_numpy(c).to(gpu)


# ---- SegmentedMaxFunction -----------------------------------------------------------------------------------
def _first_argmax(x, batch, nb):
    idx = np.full((nb, x.shape[1]), -1, np.int64)
    for b in range(nb):
        rows = np.nonzero(batch == b)[0]
        if len(rows):
            idx[b] = rows[np.argmax(x[rows], axis=0)]           # np.argmax: the first maximal row
    return idx


@pytest.mark.parametrize("c", [1, 16, 33])
@pytest.mark.parametrize("order", ["grouped", "shuffled", "out-of-range ids"])
def test_segmented_max_gradient_goes_to_the_first_maximal_row(gpu, c, order):
    """Definition: out[b, ch] = x[first row of sample b in row order that attains the column maximum, ch] (a gather; -inf
    for a sample without rows).  A ReLU'd matrix (its zeros tie) with duplicated rows; sample 2 is empty."""
    rng = np.random.default_rng(c * 10 + len(order))
    n, nb = 200, 5
    x = np.maximum(rng.standard_normal((n, c)), 0).astype(np.float32)
    x[50:60] = x[40:50]
    x[150] = x[3]
    batch = np.sort(rng.integers(0, nb, n))
    batch[batch == 2] = 3
    if order != "grouped":
        p = rng.permutation(n)
        x, batch = x[p], batch[p]
    if order == "out-of-range ids":
        bad = rng.choice(n, 12, replace=False)
        batch[bad] = np.resize([-1, nb, -3, nb + 2], 12)
        x[bad] = 50.0
    g = rng.standard_normal((nb, c)).astype(np.float32)
    idx = _first_argmax(x, batch, nb)
    live = torch.from_numpy(idx >= 0)
    assert not live[2].any() and live[[0, 1, 3, 4]].all()
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    out64 = x64[torch.from_numpy(np.maximum(idx, 0)), torch.arange(c).expand(nb, c)]
    (out64 * torch.from_numpy(g).double())[live].sum().backward()
    want_out = torch.where(live, out64.detach(), torch.full_like(out64, float("-inf"))).float()
    coords = _line_coords(n, gpu, batch)

    def run():
        xg = torch.from_numpy(x).to(gpu).requires_grad_(True)
        out = B.segmented_max(xg, coords, nb)
        assert out.grad_fn is not None
        out.backward(torch.from_numpy(g).to(gpu))
        return xg.grad, out.detach()

    gx, out = _twice_deterministic(run)
    assert torch.equal(out, want_out)
    assert torch.equal(gx, x64.grad.float()), order               # g[b, ch] at the first maximal row, exact 0 elsewhere
    assert int((gx != 0).sum()) <= 4 * c


# ---- AffineFunction: eval-mode batch norm with frozen statistics -------------------------------------------
@pytest.mark.parametrize("c", [16, 33])
def test_eval_batch_norm_backward(gpu, c):
    rng = np.random.default_rng(40 + c)
    n = 1000
    x = (rng.standard_normal((n, c)) * 2 + 1).astype(np.float32)
    r = rng.standard_normal((n, c)).astype(np.float32)
    gamma = rng.uniform(-1.5, 1.5, c).astype(np.float32)
    beta = rng.standard_normal(c).astype(np.float32)
    mean = rng.standard_normal(c).astype(np.float32)
    var = rng.uniform(0.3, 3.0, c).astype(np.float32)
    eps = 1e-5

    def cpu(dtype):
        t = [torch.from_numpy(a).to(dtype) for a in (x, gamma, beta)]
        for a in t:
            a.requires_grad_(True)
        y = torch.nn.functional.batch_norm(t[0], torch.from_numpy(mean).to(dtype), torch.from_numpy(var).to(dtype), t[1],
                                           t[2], training=False, eps=eps)
        (y * torch.from_numpy(r).to(dtype)).sum().backward()
        return [a.grad.numpy() for a in t], y.detach().numpy()

    (g64, _), (g32, _) = cpu(torch.float64), cpu(torch.float32)
    coords = _line_coords(n, gpu)

    def run():
        bn = ME.MinkowskiBatchNorm(c, eps=eps).to(gpu)
        with torch.no_grad():
            bn.bn.weight.copy_(torch.from_numpy(gamma))
            bn.bn.bias.copy_(torch.from_numpy(beta))
            bn.bn.running_mean.copy_(torch.from_numpy(mean))
            bn.bn.running_var.copy_(torch.from_numpy(var))
        bn.eval()
        xg = torch.from_numpy(x).to(gpu).requires_grad_(True)
        y = bn(ME.SparseTensor(xg, coords)).F
        assert type(y.grad_fn).__name__.startswith("AffineFunction")
        (y * torch.from_numpy(r).to(gpu)).sum().backward()
        return xg.grad, bn.bn.weight.grad, bn.bn.bias.grad, y.detach()

    gx, gg, gb, y = _twice_deterministic(run)
    a = lambda t: np.abs(t.astype(np.float64))                    # noqa: E731
    inv = 1.0 / np.sqrt(var.astype(np.float64) + eps)
    # measured on an MI355X (c = 16 / 33), as a fraction of sum|terms|: f32 CPU autograd 1.33e-7 / 1.48e-7 (gx), 1.09e-8 /
    # 1.51e-8 (ggamma), 1.04e-8 / 9.82e-9 (gbeta) -> bounds 5.3e-7 / 5.9e-7, 4.4e-8 / 6.0e-8, 4.1e-8 / 3.9e-8; the operator
    # was off by 1.64e-7 / 1.33e-7, 9.7e-9 / 1.36e-8, 6.7e-9 / 8.5e-9
    _within_4x("eval BN gx", gx.numpy(), g32[0], g64[0], a(r) * a(gamma) * inv)
    _within_4x("eval BN ggamma", gg.numpy(), g32[1], g64[1], (a(r) * (a(x) + a(mean)) * inv).sum(0))
    _within_4x("eval BN gbeta", gb.numpy(), g32[2], g64[2], a(r).sum(0))


# ---- RowL2NormalizeFunction ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [16, 32, 100])
@pytest.mark.parametrize("eps", [0.0, 1e-12, 0.5])
def test_row_l2_normalize_backward(gpu, c, eps):
    """y = x / max(||x||, eps).  Rows of norm 2 (above eps = 0.5), 0.5 (1 +- 1e-3) (near it on either side) and 0.1
    (below it: there the forward is x / eps and the Jacobian I / eps, not the projection); eps = 0 and 1e-12 see the same
    rows above their clamp."""
    rng = np.random.default_rng(60 + c)
    n = 64
    x = rng.standard_normal((n, c))
    target = np.resize([2.0, 0.5 * (1 + 1e-3), 0.5 * (1 - 1e-3), 0.1, 1.0, 30.0], n)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True) * target[:, None]).astype(np.float32)
    r = rng.standard_normal((n, c)).astype(np.float32)
    e32 = float(np.float32(eps))

    def cpu(dtype):
        t = torch.from_numpy(x).to(dtype).requires_grad_(True)
        y = t / torch.linalg.vector_norm(t, dim=1, keepdim=True).clamp_min(e32)
        (y * torch.from_numpy(r).to(dtype)).sum().backward()
        return t.grad.numpy(), y.detach().numpy()

    (g64, y64), (g32, _) = cpu(torch.float64), cpu(torch.float32)

    def run():
        xg = torch.from_numpy(x).to(gpu).requires_grad_(True)
        y = B.row_l2_normalize(xg, eps)
        assert type(y.grad_fn).__name__.startswith("RowL2NormalizeFunction")
        (y * torch.from_numpy(r).to(gpu)).sum().backward()
        return xg.grad, y.detach()

    gx, y = _twice_deterministic(run)
    assert torch.equal(y, B.row_l2_normalize(torch.from_numpy(x).to(gpu), eps).cpu())   # same kernel as without grad
    nrm = np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    clamped = nrm < e32
    assert clamped.sum() == ((target < 0.5).sum() if eps == 0.5 else 0)
    ya, ra = np.abs(y64), np.abs(r.astype(np.float64))
    scale = (ra + np.where(clamped, 0.0, ya * (ya * ra).sum(1, keepdims=True))) / np.maximum(nrm, e32)
    # measured (c = 16 / 32 / 100, the same for every eps: the worst row is not a clamped one): f32 CPU autograd 2.50e-7 /
    # 1.57e-7 / 1.53e-7 of sum|terms| -> bounds 1.0e-6 / 6.3e-7 / 6.1e-7; the operator was off by 1.56e-7 / 1.48e-7 / 1.49e-7.
    # (The projection formula applied below the clamp, as before this test existed, is off by about |y (y . g)| / eps: of
    # the order of the scale itself.)
    _within_4x(f"row L2 normalize gx (eps {eps})", gx.numpy(), g32, g64, scale)


# ---- InstanceNormFunction -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 32])
def test_instance_norm_backward(gpu, c):
    """Samples of 1 row (variance 0: the gradient to that row is 0), 0 rows (in the middle), 257 rows (one row more than a
    chunk of the forward's summation order) and 40 rows."""
    rng = np.random.default_rng(80 + c)
    lens = [1, 0, 257, 40, 1]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n, eps = int(seg[-1]), 1e-8
    x = (rng.standard_normal((n, c)) * rng.uniform(0.5, 2, c) + rng.uniform(-1, 1, c)).astype(np.float32)
    r = rng.standard_normal((n, c)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, (1, c)).astype(np.float32)
    b = rng.standard_normal((1, c)).astype(np.float32)

    def cpu(dtype):
        t = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (x, w, b)]
        parts = []
        for s in range(len(lens)):
            xs = t[0][seg[s]:seg[s + 1]]
            if len(xs):
                d = xs - xs.mean(0, keepdim=True)
                parts.append(d / torch.sqrt((d * d).mean(0, keepdim=True) + eps) * t[1] + t[2])
        y = torch.cat(parts, 0)
        (y * torch.from_numpy(r).to(dtype)).sum().backward()
        return [a.grad.numpy() for a in t]

    g64, g32 = cpu(torch.float64), cpu(torch.float32)
    segd = torch.from_numpy(seg).to(gpu)

    def run():
        t = [torch.from_numpy(a).to(gpu).requires_grad_(True) for a in (x, w, b)]
        y = AG.InstanceNormFunction.apply(t[0], t[1], t[2], segd, eps)
        assert torch.equal(y, B.instance_norm(t[0].detach(), segd, t[1].detach(), t[2].detach(), eps))
        (y * torch.from_numpy(r).to(gpu)).sum().backward()
        return tuple(a.grad for a in t)

    gx, gw, gb = _twice_deterministic(run)
    assert gw.shape == (1, c) and gb.shape == (1, c)
    # scales: gx = inv (dy - mean(dy) - xhat mean(dy xhat)), gw = sum g xhat, gb = sum g, every term in absolute value
    x64, r64, w64 = x.astype(np.float64), np.abs(r.astype(np.float64)), np.abs(w.astype(np.float64))
    sx, sw = np.zeros((n, c)), np.zeros((1, c))
    for s in range(len(lens)):
        a0, a1 = seg[s], seg[s + 1]
        if a1 > a0:
            d = x64[a0:a1] - x64[a0:a1].mean(0)
            inv = 1.0 / np.sqrt((d * d).mean(0) + eps)
            xh, dy = np.abs(d) * inv, r64[a0:a1] * w64
            sx[a0:a1] = inv * (dy + dy.mean(0) + xh * (dy * xh).mean(0))
            sw += (r64[a0:a1] * xh).sum(0)
    # measured (c = 1 / 32): f32 CPU autograd 9.7e-8 / 1.69e-7 (gx), 1.14e-8 / 2.36e-8 (gweight), 4.6e-9 / 2.24e-8 (gbias) of
    # sum|terms| -> bounds 3.9e-7 / 6.8e-7, 4.5e-8 / 9.4e-8, 1.8e-8 / 8.9e-8; the operator (f64 inside) was off by 3.4e-8 /
    # 4.7e-8, 1.6e-9 / 4.3e-9, 2.9e-9 / 4.3e-9
    _within_4x("instance norm gx", gx.numpy(), g32[0], g64[0], sx)
    _within_4x("instance norm gweight", gw.numpy(), g32[1], g64[1], sw)
    _within_4x("instance norm gbias", gb.numpy(), g32[2], g64[2], r64.sum(0, keepdims=True))
    assert np.all(g64[0][[0, n - 1]] == 0)                        # the one-row samples: d/dx of (x - x) * inv_std


# ---- ReLUFunction, AddFunction, the bias gradient of ConvFunction ------------------------------------------
def test_relu_backward_at_zero(gpu):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((300, 17)).astype(np.float32)
    x[::3] = 0.0
    x[1::7] = -0.0
    r = rng.standard_normal(x.shape).astype(np.float32)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    (torch.relu(x64) * torch.from_numpy(r).double()).sum().backward()

    def run():
        xg = torch.from_numpy(x).to(gpu).requires_grad_(True)
        y = AG.ReLUFunction.apply(xg)
        (y * torch.from_numpy(r).to(gpu)).sum().backward()
        return xg.grad, y.detach()

    gx, y = _twice_deterministic(run)
    assert torch.equal(y, torch.relu(torch.from_numpy(x)))
    assert torch.equal(gx, x64.grad.float())                    # g where x > 0, exact 0 at 0, -0 and below
    assert np.all(gx.numpy()[x == 0] == 0)


def test_add_backward(gpu):
    rng = np.random.default_rng(6)
    a, b, r = (rng.standard_normal((257, 33)).astype(np.float32) for _ in range(3))

    def run():
        t = [torch.from_numpy(v).to(gpu).requires_grad_(True) for v in (a, b)]
        y = AG.AddFunction.apply(t[0], t[1])
        (y * torch.from_numpy(r).to(gpu)).sum().backward()
        return t[0].grad, t[1].grad, y.detach()

    ga, gb, y = _twice_deterministic(run)
    assert torch.equal(y, torch.from_numpy(a + b))
    assert torch.equal(ga, torch.from_numpy(r)) and torch.equal(gb, torch.from_numpy(r))


@pytest.mark.parametrize("kernel_size,cin,cout", [(1, 32, 48), (3, 32, 32), (3, 3, 5)])
def test_conv_bias_gradient(gpu, kernel_size, cin, cout):
    """gbias = sum over rows of the output gradient, shape [1, cout]; the forward adds the bias (one f32 addition on top
    of the bias-free convolution)."""
    coords, _, _, _ = make_batch([7], 1500)
    n = len(coords)
    rng = np.random.default_rng(90 + cin + cout)
    f = rng.standard_normal((n, cin)).astype(np.float32)
    r = rng.standard_normal((n, cout)).astype(np.float32)
    ct = torch.from_numpy(coords).to(gpu)
    torch.manual_seed(kernel_size)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=kernel_size, stride=1, bias=True, dimension=3).to(gpu)

    def run():
        conv.zero_grad(set_to_none=True)
        ft = torch.from_numpy(f).to(gpu).requires_grad_(True)
        y = conv(ME.SparseTensor(ft, ct)).F
        (y * torch.from_numpy(r).to(gpu)).sum().backward()
        return conv.bias.grad, conv.kernel.grad, ft.grad, y.detach()

    gb, _, _, y = _twice_deterministic(run)
    assert gb.shape == (1, cout)
    with torch.no_grad():
        x0 = ME.SparseTensor(torch.from_numpy(f).to(gpu), ct)
        kmap = None if kernel_size == 1 else x0.coordinate_manager.kernel_map(x0.coordinate_map_key, x0.coordinate_map_key, 3)
        plain = B.conv_fwd(kmap, x0.F, conv.kernel.detach())
    assert torch.equal(y, (plain + conv.bias.detach()).cpu())
    sums = lambda dt: torch.from_numpy(r).to(dt).sum(0, keepdim=True).numpy()   # noqa: E731
    # measured (the three cases): f32 CPU sum 1.49e-8 / 1.26e-8 / 6.3e-9 of sum|g| -> bounds 6.0e-8 / 5.0e-8 / 2.5e-8; the
    # operator was off by 9.6e-9 / 7.3e-9 / 6.5e-9
    _within_4x("conv gbias", gb.numpy(), sums(torch.float32), sums(torch.float64), np.abs(r.astype(np.float64)).sum(0, keepdims=True))
