"""The yardstick of the pair loss: the NumPy restatement of the library's fixed-point arithmetic
(tests/pair_loss_ref.py) against torch autograd in f64 on the same inputs, plus the host logic of the trainer that
needs no device (epoch_batches, step seeds, the parser's defaults)."""
import dataclasses

import numpy as np
import torch

from tests import pair_loss_ref as PL


def unit_rows(rng, n, c=16):
    x = rng.standard_normal((n, c))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def make_case(seed=0, n=(4000, 3500, 3000), P=(30000, 33000, 31000), c=16):
    """Three terms sharing the base matrix: PULL on (base, pos), PUSH on (base, pos) with about half the pairs beyond
    the margin, PUSH on (base, neg); pairs with repeats; one pair of identical rows (d = 0) in the PULL term."""
    rng = np.random.default_rng(seed)
    base, pos, neg = (unit_rows(rng, k, c) for k in n)
    pos[:1000] = (base[:1000] + 0.05 * rng.standard_normal((1000, c))).astype(np.float32)   # near pairs for PULL
    pos[7] = base[5]                                            # identical rows: d = 0 exactly

    def pairs(na, nb, p):
        return np.stack([rng.integers(0, na, p), rng.integers(0, nb, p)], 1).astype(np.int32)

    pip = pairs(1000, 1000, P[0])
    pip[:, 1] = pip[:, 0]
    pip[::3] = pairs(n[0], n[1], len(pip[::3]))                 # a third of them far apart
    pip[11] = (5, 7)
    pin = pairs(n[0], n[1], P[1])                               # random unit rows: d around sqrt(2), margin 1.4
    nin = pairs(n[0], n[2], P[2])
    nin[:500, 0] = 3                                            # one base row in 500 pairs
    mats = [base, pos, neg]
    terms = [(0, 1, pip, PL.PULL, 0.1, 1.0), (0, 1, pin, PL.PUSH, 1.4, 1.0), (0, 2, nin, PL.PUSH, 1.4, 0.5)]
    return mats, terms


def torch_f64(mats, terms, g):
    """(term losses, total, gradients) of the same loss by torch autograd in f64 (gather, norm, hinge, mean)."""
    xs = [torch.from_numpy(m.astype(np.float64)).requires_grad_(True) for m in mats]
    Ls = []
    for a, b, pairs, kind, margin, weight in terms:
        if len(pairs) == 0:
            Ls.append(torch.zeros((), dtype=torch.float64))
            continue
        p = torch.from_numpy(pairs.astype(np.int64))
        diff = xs[a][p[:, 0]] - xs[b][p[:, 1]]
        s = (diff * diff).sum(1)
        d = torch.sqrt(torch.where(s > 0, s, torch.ones_like(s))) * (s > 0)   # d = 0 pairs: no gradient, as specified
        m = float(np.float32(margin))
        h = torch.relu(d - m if kind == PL.PULL else m - d)
        Ls.append(weight * (h * h).mean())
    total = torch.stack(Ls).sum()
    (total * g).backward()
    grads = [x.grad.numpy() if x.grad is not None else np.zeros(x.shape) for x in xs]
    return np.array([float(v.detach()) for v in Ls]), float(total.detach()), grads


def check_against_f64(mats, terms, g):
    L, total = PL.forward(mats, terms)
    grads = PL.backward(mats, terms, np.float32(g))
    wL, wtotal, wgrads = torch_f64(mats, terms, float(np.float32(g)))
    assert abs(float(total) - wtotal) <= 1e-6 * abs(wtotal), (float(total), wtotal)
    for t in range(len(terms)):
        assert abs(L[t] - wL[t]) <= 1e-6 * abs(wL[t]) + 1e-300, (t, L[t], wL[t])
    step = PL.grad_step(mats, terms, g)
    for got, want in zip(grads, wgrads):
        top = float(np.abs(want).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("gradient error / largest magnitude:", err / top if top else err)
        assert err <= 1e-6 * top + step, (err, top, step)


def test_restatement_matches_torch_f64():
    mats, terms = make_case()
    check_against_f64(mats, terms, 0.37)
    # half of the PUSH pairs are beyond the margin (contribute nothing), the rest are active
    _, d, h = PL._chain(mats[0], mats[1], terms[1][2], PL.PUSH, 1.4)
    share = float((h > 0).mean())
    assert 0.25 < share < 0.75, share
    _, d, _ = PL._chain(mats[0], mats[1], terms[0][2], PL.PULL, 0.1)
    assert d[11] == 0.0


def test_restatement_small_and_empty_terms():
    rng = np.random.default_rng(3)
    a, b = unit_rows(rng, 40, 3), unit_rows(rng, 50, 3)
    one = np.array([[4, 9]], np.int32)
    none = np.zeros((0, 2), np.int32)
    many = np.stack([rng.integers(0, 40, 31), rng.integers(0, 50, 31)], 1).astype(np.int32)
    terms = [(0, 1, one, PL.PULL, 0.1, 1.0), (0, 1, none, PL.PUSH, 1.4, 1.0), (0, 1, many, PL.PUSH, 1.4, 2.0)]
    L, total = PL.forward([a, b], terms)
    assert L[1] == 0.0
    check_against_f64([a, b], terms, 1.0)
    g = PL.backward([a, b], [terms[1]], np.float32(1.0))
    assert not g[0].any() and not g[1].any()


def test_restatement_is_order_free():
    mats, terms = make_case(seed=1, P=(3000, 3300, 3100))
    rng = np.random.default_rng(9)
    shuffled = [(a, b, p[rng.permutation(len(p))], k, m, w) for a, b, p, k, m, w in terms]
    L0, t0 = PL.forward(mats, terms)
    L1, t1 = PL.forward(mats, shuffled)
    assert np.array_equal(L0, L1) and t0 == t1
    for x, y in zip(PL.backward(mats, terms, np.float32(0.37)), PL.backward(mats, shuffled, np.float32(0.37))):
        assert np.array_equal(x, y)


# ---- host logic of the trainer ----------------------------------------------------------------------------------
def test_epoch_batches():
    from corsair_amd.train import epoch_batches, step_seed

    b = epoch_batches(37, 8, 5, 0)
    assert [len(x) for x in b] == [8, 8, 8, 8, 5]                       # the short last batch is kept
    flat = [i for x in b for i in x]
    assert sorted(flat) == list(range(37))                              # a permutation: every anchor once
    assert b == epoch_batches(37, 8, 5, 0)                              # equal keys, equal batches
    assert b != epoch_batches(37, 8, 5, 1) and b != epoch_batches(37, 8, 6, 0)
    assert epoch_batches(0, 8, 5, 0) == []
    state = np.random.get_state()[1].copy(), torch.random.get_rng_state().clone()
    epoch_batches(100, 7, 1, 2)
    assert np.array_equal(state[0], np.random.get_state()[1]) and torch.equal(state[1], torch.random.get_rng_state())
    seeds = {step_seed(5, e, s) for e in range(10) for s in range(10)}
    assert len(seeds) == 100 and all(0 <= v < 2 ** 63 for v in seeds)
    assert step_seed(5, 3, 4) == step_seed(5, 3, 4) != step_seed(6, 3, 4)


def test_val_poses_fixed():
    from corsair_amd.train import val_poses

    a, b = val_poses(5, 31), val_poses(5, 31)
    assert a.shape == (5, 3, 4, 4) and np.array_equal(a, b) and not np.array_equal(a, val_poses(5, 32))
    R = a[:, :, :3, :3]
    assert np.allclose(R @ R.transpose(0, 1, 3, 2), np.eye(3), atol=1e-12)


def test_parser_defaults_equal_config():
    from corsair_amd.train import TrainConfig, build_parser, config_from_args

    a = build_parser().parse_args(["--clouds-dir", "x", "--out", "y"])
    assert config_from_args(a) == TrainConfig()
    for f in dataclasses.fields(TrainConfig):
        assert hasattr(a, f.name), f.name
    b = build_parser().parse_args(["--clouds-dir", "x", "--out", "y", "--lr", "0.5", "--pair-weights", "1", "2", "3",
                                   "--batch-size", "4", "--resume", "c.pth"])
    cfg = config_from_args(b)
    assert cfg.lr == 0.5 and cfg.pair_weights == (1.0, 2.0, 3.0) and cfg.batch_size == 4 and b.resume == "c.pth"
