"""cs_pair_loss_fwd / cs_pair_loss_bwd against the NumPy restatement tests/pair_loss_ref.py: value and
gradients bit for bit, independence of the pair order, the autograd wrapper on a real shim forward, and refusals."""
import os
import sys

import numpy as np
import pytest
import torch

from corsair_amd import _lib, backend as B
from tests import pair_loss_ref as PL
from tests.test_pair_loss_cpu import make_case, torch_f64, unit_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _dev_mats(mats, gpu, ld=None):
    """Device copies; ld = a leading dimension above C: the matrix is a column view of a wider buffer filled with
    NaN elsewhere (nothing outside the view may be read into a result)."""
    out = []
    for k, m in enumerate(mats):
        t = torch.from_numpy(m).to(gpu)
        if ld is not None:
            wide = torch.full((m.shape[0], ld), float("nan"), dtype=torch.float32, device=gpu)
            c0 = (5 * k) % (ld - m.shape[1] + 1)
            wide[:, c0:c0 + m.shape[1]] = t
            t = wide[:, c0:c0 + m.shape[1]]
            assert t.stride(0) == ld
        out.append(t)
    return out


def _dev_terms(terms, gpu):
    return [(a, b, torch.from_numpy(np.ascontiguousarray(p)).to(gpu), k, m, w) for a, b, p, k, m, w in terms]


def _run(mats, terms, gpu, g=0.37, ld=None):
    dm, dt = _dev_mats(mats, gpu, ld), _dev_terms(terms, gpu)
    L, total = B.pair_loss_fwd(dm, dt)
    grads = B.pair_loss_bwd(dm, dt, torch.tensor([g], dtype=torch.float32, device=gpu))
    return L.cpu().numpy(), total.cpu().numpy()[0], [x.cpu().numpy() for x in grads]


def _check_bits(mats, terms, gpu, g=0.37, ld=None):
    L, total, grads = _run(mats, terms, gpu, g, ld)
    wL, wtotal = PL.forward(mats, terms)
    wgrads = PL.backward(mats, terms, np.float32(g))
    assert np.array_equal(L, wL), (L, wL)
    assert total == wtotal and total.dtype == np.float32
    for k, (got, want) in enumerate(zip(grads, wgrads)):
        assert got.dtype == np.float32 and np.array_equal(got, want), (k, float(np.abs(got - want).max()))
    return L, total, grads


@pytest.mark.parametrize("ld", [None, 48])
def test_three_terms_c16_bit_equal(gpu, ld):
    mats, terms = make_case()                          # 30 - 33 k pairs per term, shared base, repeats, d = 0
    _, _, grads = _check_bits(mats, terms, gpu, ld=ld)
    assert all(np.abs(g).max() > 0 for g in grads)


def test_production_size_and_repeated_row(gpu):
    mats, terms = make_case(seed=2, n=(60000, 58000, 59000), P=(1024 * 32,) * 3)
    assert np.bincount(terms[2][2][:, 0]).max() >= 500  # one base row in 500 pairs
    _check_bits(mats, terms, gpu)


@pytest.mark.parametrize("C", [3, 256])
def test_other_widths_bit_equal(gpu, C):
    rng = np.random.default_rng(C)
    a, b = unit_rows(rng, 300, C), unit_rows(rng, 280, C)
    b[:100] = (a[:100] + 0.02 * rng.standard_normal((100, C))).astype(np.float32)
    pull = np.stack([rng.integers(0, 100, 2000)] * 2, 1).astype(np.int32)
    push = np.stack([rng.integers(0, 300, 3000), rng.integers(0, 280, 3000)], 1).astype(np.int32)
    _check_bits([a, b], [(0, 1, pull, PL.PULL, 0.1, 1.0), (0, 1, push, PL.PUSH, 1.4, 1.0)], gpu, g=1.0)
    _check_bits([a, b], [(0, 1, pull, PL.PULL, 0.0, 3.0)], gpu, ld=C + 7)


@pytest.mark.parametrize("P", [1, 31])
def test_small_terms_and_empty_term(gpu, P):
    rng = np.random.default_rng(P)
    a, b, c = unit_rows(rng, 40), unit_rows(rng, 50), unit_rows(rng, 45)
    pr = np.stack([rng.integers(0, 40, P), rng.integers(0, 50, P)], 1).astype(np.int32)
    none = np.zeros((0, 2), np.int32)
    terms = [(0, 1, pr, PL.PULL, 0.1, 1.0), (0, 1, none, PL.PUSH, 1.4, 1.0), (0, 2, pr[:, ::-1] % 40, PL.PUSH, 1.4, 1.0)]
    L, total, grads = _check_bits([a, b, c], terms, gpu, g=1.0)
    assert L[1] == 0.0
    # only empty terms: value 0, gradients written as zeros
    L, total, grads = _check_bits([a, b], [(0, 1, none, PL.PUSH, 1.4, 1.0)], gpu)
    assert total == 0.0 and not grads[0].any() and not grads[1].any()
    # a term of one matrix against itself (A and B the same matrix): both sides land in the one output
    self_pairs = np.stack([rng.integers(0, 40, 64), rng.integers(0, 40, 64)], 1).astype(np.int32)
    _check_bits([a], [(0, 0, self_pairs, PL.PUSH, 1.4, 1.0)], gpu)


def test_permutation_invariance(gpu):
    mats, terms = make_case(seed=4)
    rng = np.random.default_rng(1)
    shuffled = [(a, b, p[rng.permutation(len(p))], k, m, w) for a, b, p, k, m, w in terms]
    L0, t0, g0 = _run(mats, terms, gpu)
    L1, t1, g1 = _run(mats, shuffled, gpu)
    assert np.array_equal(L0, L1) and t0 == t1
    for x, y in zip(g0, g1):
        assert np.array_equal(x, y)
    L2, t2, g2 = _run(mats, terms, gpu)                # and from run to run
    assert np.array_equal(L0, L2) and t0 == t2 and all(np.array_equal(x, y) for x, y in zip(g0, g2))


def test_out_of_precondition_rows_do_not_fault(gpu):
    rng = np.random.default_rng(0)
    a, b = unit_rows(rng, 64), unit_rows(rng, 64)
    a[0] = np.inf
    a[1] = np.nan
    a[2] *= 1e30
    b[3] = -np.inf
    pr = np.stack([np.arange(64), np.arange(64)[::-1]], 1).astype(np.int32)
    pr[:8, 1] = np.arange(8)
    L, total, grads = _run([a, b], [(0, 1, pr, PL.PULL, 0.1, 1024.0), (0, 1, pr, PL.PUSH, 16.0, 1024.0)], gpu)
    assert L.shape == (2,) and grads[0].shape == (64, 16)     # numbers may be meaningless; the call completes
    torch.cuda.synchronize()


def _shim_forward(gpu):
    sys.path.insert(0, os.path.join(ROOT, "shim"))
    import MinkowskiEngine as ME
    from corsair_amd import synth
    from corsair_amd.model import load_model
    from tests.helpers import make_batch

    sd, _ = synth.make_state_dicts(31)
    model = load_model("ResUNetBN2C")(1, 16, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=3, D=3).to(gpu)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model.train()
    outs = []
    for ids, poses in (([0, 1], None), ([0, 1], [3, 4]), ([2, 3], None)):
        coords, feats, _, _ = make_batch(ids, 3000, pose_ids=poses)
        out, _ = model(ME.SparseTensor(torch.from_numpy(feats).to(gpu), torch.from_numpy(coords).to(gpu)))
        outs.append(out.F)
    return outs


def test_autograd_function_on_shim_output(gpu):
    from corsair_amd import losses
    from corsair_amd.autograd import PairLossFunction

    outs = _shim_forward(gpu)
    assert all(o.requires_grad for o in outs)
    rng = np.random.default_rng(8)
    n = [o.shape[0] for o in outs]

    def pairs(na, nb, p):
        return np.stack([rng.integers(0, na, p), rng.integers(0, nb, p)], 1).astype(np.int32)

    data = {"PiP_pairs": pairs(n[0], n[1], 2000), "PiN_pairs": pairs(n[0], n[1], 2100), "NiN_pairs": pairs(n[0], n[2], 1900)}
    ddata = {k: torch.from_numpy(v).to(gpu) for k, v in data.items()}
    leaves = [o.detach().clone().requires_grad_(True) for o in outs]
    feats = dict(zip(("base", "pos", "neg"), leaves))
    loss, parts = losses.pair_contrastive(feats, ddata, return_parts=True)
    (loss * 0.37).backward()                                         # upstream gradient != 1
    terms = [(0, 1, data["PiP_pairs"], PL.PULL, 0.1, 1.0), (0, 1, data["PiN_pairs"], PL.PUSH, 1.4, 1.0),
             (0, 2, data["NiN_pairs"], PL.PUSH, 1.4, 1.0)]
    # equals the backend called directly
    dt = _dev_terms(terms, gpu)
    L, total = B.pair_loss_fwd([x.detach() for x in leaves], dt)
    g = B.pair_loss_bwd([x.detach() for x in leaves], dt, torch.tensor([0.37], dtype=torch.float32, device=gpu))
    assert torch.equal(loss.detach().reshape(1), total) and torch.equal(parts, L)
    for x, want in zip(leaves, g):
        assert torch.equal(x.grad, want)
    # ... and the restatement, and torch f64 autograd within the CPU test's tolerance
    mats = [x.detach().cpu().numpy() for x in leaves]
    wgrads = PL.backward(mats, terms, np.float32(0.37))
    fL, ftotal, fgrads = torch_f64(mats, terms, float(np.float32(0.37)))
    assert abs(float(loss.detach()) - ftotal) <= 1e-6 * abs(ftotal)
    step = PL.grad_step(mats, terms, 0.37)
    for x, w, f in zip(leaves, wgrads, fgrads):
        assert np.array_equal(x.grad.cpu().numpy(), w)
        top = float(np.abs(f).max())
        assert float(np.abs(x.grad.cpu().numpy().astype(np.float64) - f).max()) <= 1e-6 * top + step
    # attached to the graph of the network (out.F as it comes, not a leaf): the same gradient arrives at out.F
    o = _shim_forward(gpu)
    model_loss = PairLossFunction.apply(dt, *o)[0]
    for gr, want in zip(torch.autograd.grad(model_loss * 0.37, o), g):
        assert torch.equal(gr, want)           # out.F has the same values as the detached leaves


def test_refusals_leave_outputs_untouched(gpu):
    rng = np.random.default_rng(0)
    a, b = unit_rows(rng, 20), unit_rows(rng, 20)
    pr = np.stack([rng.integers(0, 20, 10), rng.integers(0, 20, 10)], 1).astype(np.int32)
    dm = _dev_mats([a, b], gpu)
    dp = torch.from_numpy(pr).to(gpu)
    sentinel = -7.25
    bad = {
        "margin": [(0, 1, dp, PL.PULL, 16.5, 1.0)], "margin ": [(0, 1, dp, PL.PUSH, -0.1, 1.0)],
        "weight": [(0, 1, dp, PL.PULL, 0.1, 1025.0)], "weight ": [(0, 1, dp, PL.PULL, 0.1, -1.0)],
        "kind": [(0, 1, dp, 2, 0.1, 1.0)], "matrix": [(0, 2, dp, PL.PULL, 0.1, 1.0)],
        "terms": [(0, 1, dp, PL.PULL, 0.1, 1.0)] * 9,
    }
    for what, terms in bad.items():
        out = (torch.full((9,), sentinel, dtype=torch.float64, device=gpu),
               torch.full((1,), sentinel, dtype=torch.float32, device=gpu))
        with pytest.raises(_lib.CorsairHipError, match=what.strip()):
            B.pair_loss_fwd(dm, terms, out=out)
        assert what.strip() in _lib.load().cs_last_error().decode()
        gout = [torch.full((20, 16), sentinel, dtype=torch.float32, device=gpu) for _ in dm]
        with pytest.raises(_lib.CorsairHipError):
            B.pair_loss_bwd(dm, terms, torch.ones(1, device=gpu), out=gout)
        torch.cuda.synchronize()
        assert bool((out[0] == sentinel).all()) and bool((out[1] == sentinel).all())
        assert all(bool((x == sentinel).all()) for x in gout)
    # C out of range, ld < C (an overlapping-row view handed to the library as it is), too many pairs
    wide = torch.zeros((4, 257), dtype=torch.float32, device=gpu)
    with pytest.raises(_lib.CorsairHipError, match="C <= 256"):
        B.pair_loss_fwd([wide, wide], [(0, 1, dp[:1] * 0, PL.PULL, 0.1, 1.0)])
    lib = _lib.load()
    from ctypes import c_double, c_float, c_void_p

    m = dm[0]
    vp = (c_void_p * 1)(m.data_ptr())
    pp = (c_void_p * 1)(dp.data_ptr())
    out = (torch.full((1,), sentinel, dtype=torch.float64, device=gpu), torch.full((1,), sentinel, device=gpu))

    def call(ld, npairs):
        return lib.cs_pair_loss_fwd(1, vp, _lib.i64_array([20]), _lib.i32_array([ld]), 16, 1, _lib.i32_array([0]),
                                    _lib.i32_array([0]), _lib.i32_array([0]), (c_float * 1)(0.1), (c_double * 1)(1.0),
                                    pp, _lib.i64_array([npairs]), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.stream_ptr())

    assert call(15, 10) < 0 and "leading dimension" in lib.cs_last_error().decode()
    assert call(16, (1 << 22) + 1) < 0 and "2^22" in lib.cs_last_error().decode()
    assert call(16, 10) == 0
    torch.cuda.synchronize()
    assert float(out[1]) != sentinel
