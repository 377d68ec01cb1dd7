"""NumPy restatement of cs_pair_loss_fwd / cs_pair_loss_bwd (include/corsair_hip.h): the canonical
arithmetic, operation by operation.  NumPy's f32 `-`, `*`, `+`, `/` and np.sqrt are the same correctly rounded IEEE
operations the kernels use; the sums are exact 64-bit integer sums, so neither side depends on an order."""
import numpy as np

PULL, PUSH = 0, 1
F = np.float32


def _chain(A, B, pairs, kind, margin):
    """(diff [P, C], d [P], h [P]) of a term, all f32."""
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    diff = A[i].astype(F) - B[j].astype(F)
    s = np.zeros(len(pairs), F)
    for k in range(diff.shape[1]):               # k ascending: product rounded, then the sum rounded
        s = s + diff[:, k] * diff[:, k]
    d = np.sqrt(s)
    m = F(margin)
    h = np.maximum(d - m if kind == PULL else m - d, F(0))
    assert s.dtype == F and d.dtype == F and h.dtype == F
    return diff, d, h


def forward(mats, terms):
    """mats: list of f32 [n, C] arrays; terms: list of (a, b, pairs int [P, 2], kind, margin, weight).
    Returns (term losses f64 [T], total f32)."""
    L = np.zeros(len(terms), np.float64)
    for t, (a, b, pairs, kind, margin, weight) in enumerate(terms):
        P = len(pairs)
        if P == 0:
            continue
        _, _, h = _chain(mats[a], mats[b], pairs, kind, margin)
        l = h * h
        S = int((l.astype(np.float64) * 2.0 ** 32).astype(np.uint64).sum(dtype=np.uint64))   # cast truncates
        L[t] = np.float64(weight) * np.float64(S) * 2.0 ** -32 / np.float64(P)
    total = np.float64(0)
    for v in L:
        total = total + v
    return L, F(total)


def backward(mats, terms, g):
    """The gradient of every matrix (f32 [n, C]), upstream scalar g (f32)."""
    C = mats[0].shape[1]
    acc = [np.zeros((m.shape[0], C), np.int64) for m in mats]
    for a, b, pairs, kind, margin, weight in terms:
        P = len(pairs)
        if P == 0:
            continue
        diff, d, h = _chain(mats[a], mats[b], pairs, kind, margin)
        r = F(np.float64(weight) / np.float64(P))
        on = (h > 0) & (d > 0)
        diff, d, h, pr = diff[on], d[on], h[on], pairs[on]
        c = (h + h) * r
        u = diff / d[:, None]
        e = c[:, None] * u
        if kind == PUSH:
            e = -e
        assert e.dtype == F
        q = (e.astype(np.float64) * 2.0 ** 44).astype(np.int64)   # truncates toward zero
        np.add.at(acc[a], pr[:, 0].astype(np.int64), q)
        np.add.at(acc[b], pr[:, 1].astype(np.int64), -q)
    return [(x.astype(np.float64) * 2.0 ** -44).astype(F) * F(g) for x in acc]


def grad_step(mats, terms, g):
    """Largest error the fixed-point truncation can add to a gradient element: below one unit of 2^-44 per
    contribution to the element's row, times |g| (the additive part of the tolerance against torch autograd)."""
    hits = [np.zeros(m.shape[0], np.int64) for m in mats]
    for a, b, pairs, *_ in terms:
        hits[a] += np.bincount(pairs[:, 0], minlength=len(hits[a]))
        hits[b] += np.bincount(pairs[:, 1], minlength=len(hits[b]))
    return int(max(h.max() for h in hits)) * 2.0 ** -44 * abs(float(g))
