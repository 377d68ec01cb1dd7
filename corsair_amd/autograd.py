"""torch.autograd.Function wrappers of the shim's operators (training through corsair_amd.minkowski).

Every forward calls the same HIP entry point as the inference path, so forward values with grad enabled are
bit-identical to the torch.no_grad() forward.  The backward of the convolution is HIP (cs_conv_wgrad for the
weights, cs_conv_fwd on the reverse kernel map for the input); the backward of the small row ops is a few dense
torch expressions.  Nothing here accumulates with atomics or index_add_: every backward is deterministic and
runs under torch.use_deterministic_algorithms(True).
"""
from __future__ import annotations

import torch

from . import backend as B


def _rowmajor(t):
    """t itself when its rows are contiguous and do not overlap (a usable leading dimension), else a copy: an output
    gradient may be a broadcast view (e.g. of conv(x).F.sum(0)) with row stride 0."""
    ok = t.dim() == 2 and t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
    return t if ok else t.contiguous()


class ConvFunction(torch.autograd.Function):
    """out = conv_fwd(kmap, x, weight) + bias.  `rev` is a callable returning the reverse kernel map (called only
    when the input gradient is needed, so the maps come from the coordinate manager's cache)."""

    @staticmethod
    def forward(ctx, x, weight, bias, kmap, rev):
        ctx.kmap, ctx.rev = kmap, rev
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight)
        b = bias.detach().reshape(-1) if bias is not None else None
        return B.conv_fwd(kmap, x.detach(), weight.detach(), None, b, None, False)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = _rowmajor(g)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            rev = ctx.rev() if ctx.kmap is not None and not ctx.kmap.stride1 else None
            gx = B.conv_dgrad(ctx.kmap, rev, g, weight.detach())
        if ctx.needs_input_grad[1]:
            gw = B.conv_wgrad(ctx.kmap, x.detach(), g).reshape(weight.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = g.sum(0, keepdim=True)
        return gx, gw, gb, None, None


class AffineFunction(torch.autograd.Function):
    """Eval-mode batch norm with grad (frozen statistics): out = x * scale + shift (cs_affine_act), scale and
    shift folded from gamma, beta and the running statistics."""

    @staticmethod
    def forward(ctx, x, gamma, beta, scale, shift, mean, inv_std):
        ctx.save_for_backward(x, scale, mean, inv_std)
        return B.affine_act(x.detach(), scale, shift, None, False)

    @staticmethod
    def backward(ctx, g):
        x, scale, mean, inv_std = ctx.saved_tensors
        gx = g * scale if ctx.needs_input_grad[0] else None
        ggamma = (g * ((x - mean) * inv_std)).sum(0) if ctx.needs_input_grad[1] else None
        gbeta = g.sum(0) if ctx.needs_input_grad[2] else None
        return gx, ggamma, gbeta, None, None, None, None


class ReLUFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = B.affine_act(x.detach(), None, None, None, True)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return torch.where(y > 0, g, torch.zeros_like(g))


class AddFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return B.affine_act(a.detach(), None, None, b.detach(), False)

    @staticmethod
    def backward(ctx, g):
        return g, g


class RowL2NormalizeFunction(torch.autograd.Function):
    """y = x / max(||x||, eps) per row (eps = 0: model/resunet.py:260-262).  ||x|| >= eps: dx = (g - y (y . g)) / ||x||;
    below the clamp the forward is x / eps and dx = g / eps."""

    @staticmethod
    def forward(ctx, x, eps):
        y = B.row_l2_normalize(x.detach(), eps)
        ctx.eps = eps
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        # eps as the kernel sees it (an f32 argument).  The kernel clamps its own f32 sum of squares; within a few ulp of
        # eps this norm may fall on the other side of the clamp -- at the kink, where no gradient is defined
        eps = torch.tensor(ctx.eps, dtype=x.dtype, device=x.device)
        nrm = torch.linalg.vector_norm(x, dim=1, keepdim=True)
        gx = (g - y * (y * g).sum(1, keepdim=True)) / torch.maximum(nrm, eps)
        if ctx.eps > 0:
            gx = torch.where(nrm < eps, g / eps, gx)
        return gx, None


def _seg_sum(v, seg):
    """Per-segment column sums [n_seg, c] of v [n, c] over the row ranges seg [n_seg + 1] (device int64): differences
    of one f64 prefix sum (a scan: fixed order, no atomics, no host wait)."""
    s = torch.cat([torch.zeros((1, v.shape[1]), dtype=torch.float64, device=v.device), v.double().cumsum(0)], 0)
    return s[seg[1:]] - s[seg[:-1]]


class SegmentedMaxFunction(torch.autograd.Function):
    """Per-sample column max (cs_segmented_max).  The gradient of out[b, c] goes to the FIRST row of sample b in row
    order that attains the maximum -- the row `feat.max(0)` picks in the reference's model/fc.py.  With the rows
    grouped by sample (stably sorted when they are not), that row is a reversed cumulative min of candidate row
    indices read at the start of the sample's rows: one pass over [n, c], a gather (no scatter)."""

    @staticmethod
    def forward(ctx, x, coords, n_batch):
        out = B.segmented_max(x.detach(), coords, n_batch)
        ctx.save_for_backward(x, coords, out)
        ctx.n_batch = n_batch
        return out

    @staticmethod
    def backward(ctx, g):
        x, coords, out = ctx.saved_tensors
        n, c = x.shape
        nb = ctx.n_batch
        batch = coords[:, 0].long()
        perm = None
        if n > 1 and not bool((batch[1:] >= batch[:-1]).all()):
            perm = torch.sort(batch, stable=True).indices
            batch, x = batch[perm], x[perm]
        valid = ((batch >= 0) & (batch < nb)).unsqueeze(1)
        bi = batch.clamp(0, max(nb - 1, 0))
        start = torch.searchsorted(batch, batch)                # first row of the row's sample
        end = torch.searchsorted(batch, batch, right=True)      # one past its last row
        rows = torch.arange(n, device=x.device).unsqueeze(1)
        hit = (x == out[bi]) & valid
        # a row without a hit stands for its sample's end: every later sample's candidates are >= that end, so the
        # reversed running min at a sample's first row is its first hit (or its end: no gradient)
        cand = torch.where(hit, rows.expand(n, c), end.unsqueeze(1).expand(n, c))
        first = cand.flip(0).cummin(0).values.flip(0)[start]
        gx = torch.where(rows == first, g[bi], torch.zeros((), dtype=g.dtype, device=g.device))
        if perm is not None:
            gx = gx[torch.argsort(perm)]
        return gx, None, None


class InstanceNormFunction(torch.autograd.Function):
    """MinkowskiInstanceNorm: forward cs_instance_norm; backward the standard instance-norm formula per sample and
    channel (biased variance, eps inside the root), in f64 with segment sums over the device row offsets."""

    @staticmethod
    def forward(ctx, x, weight, bias, seg, eps):
        out = B.instance_norm(x.detach(), seg, weight.detach(), bias.detach(), eps)
        ctx.save_for_backward(x, weight, seg)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, seg = ctx.saved_tensors
        seg = seg.long()
        n = x.shape[0]
        w = weight.reshape(1, -1).double()
        g = g.double()
        cnt = (seg[1:] - seg[:-1]).clamp_min(1).double().unsqueeze(1)
        bi = torch.searchsorted(seg[1:], torch.arange(n, device=x.device), right=True).clamp_max(seg.numel() - 2)
        mean = _seg_sum(x, seg) / cnt
        d = x.double() - mean[bi]
        inv = torch.rsqrt(_seg_sum(d * d, seg) / cnt + ctx.eps)
        xhat = d * inv[bi]
        dy = g * w
        gx = inv[bi] * (dy - (_seg_sum(dy, seg) / cnt)[bi] - xhat * (_seg_sum(dy * xhat, seg) / cnt)[bi])
        gw = (g * xhat).sum(0)
        gb = g.sum(0)
        return (gx.to(x.dtype), gw.to(weight.dtype).reshape(weight.shape), gb.to(weight.dtype).reshape(weight.shape),
                None, None)


class PairLossFunction(torch.autograd.Function):
    """total, term_losses = PairLossFunction.apply(terms, *mats): cs_pair_loss_fwd / cs_pair_loss_bwd.
    mats are the distinct feature matrices (f32 [n, C]; `out.F` of the shim as it comes, views with a leading
    dimension included), terms a list of (a, b, pairs int32 [P, 2], kind, margin, weight) with a, b indices into
    mats.  total is the f32 scalar, term_losses f64 [T] (for logging: not differentiable).  The backward returns one
    gradient per matrix, all terms summed into it with integer accumulators: bit-identical from run to run."""

    @staticmethod
    def forward(ctx, terms, *mats):
        mats = [_rowmajor(m.detach()) for m in mats]
        ctx.terms = [(int(t[0]), int(t[1]), t[2].detach(), int(t[3]), float(t[4]), float(t[5])) for t in terms]
        ctx.save_for_backward(*mats)
        term_losses, total = B.pair_loss_fwd(mats, ctx.terms)
        ctx.mark_non_differentiable(term_losses)
        return total.reshape(()), term_losses

    @staticmethod
    def backward(ctx, g, _g_terms):
        mats = list(ctx.saved_tensors)
        grads = B.pair_loss_bwd(mats, ctx.terms, g.reshape(1).float().contiguous())
        return (None,) + tuple(gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[1:]))
