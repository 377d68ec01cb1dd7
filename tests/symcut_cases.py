"""Seeded inputs of the part-cut tests (tests/test_symcut_cpu.py, tests/test_gpu_symcut.py): the CPU file states on the
oracle's branch census (oracle.native.symcut_census) which Lloyd branch each case takes, the GPU file compares the
kernels with the oracle on the very same arrays.  Every builder returns (feat f32 [n, dim], xyz f32 [n, 3], anchors
int32 [n_anchor]); tie_blocks returns a TieCase that also names the rows the selection must return."""
from collections import namedtuple

import numpy as np

N_ANCHOR = 24


def _unit_rows(rng, n, dim):
    f = rng.standard_normal((n, dim))
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def _anchors(rng, n, n_anchor):
    return rng.choice(n, n_anchor, replace=False).astype(np.int32)


def uniform(n=600, dim=16, n_anchor=N_ANCHOR, seed=0):
    """Unit-norm normal features, xyz uniform in [-0.5, 0.5]^3: the ordinary cloud (every restart stops on repeated
    labels; some later restarts replace the best one)."""
    rng = np.random.default_rng([seed, n, dim])
    f = _unit_rows(rng, n, dim)
    x = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    return f, x, _anchors(rng, n, n_anchor)


def three_positions(n=600, seed=1):
    """xyz takes 3 distinct values: with K = 4 one cluster is empty in every restart and is relocated."""
    rng = np.random.default_rng([seed, n])
    pos = np.array([[0.3, 0.1, -0.2], [-0.25, 0.2, 0.15], [0.05, -0.35, 0.3]], np.float32)
    x = pos[rng.integers(0, 3, n)]
    return _unit_rows(rng, n, 16), np.ascontiguousarray(x), _anchors(rng, n, N_ANCHOR)


def identical(n=600, seed=2):
    """Every xyz is the same point (4 anchors): K - 1 clusters are relocated per restart, the variance and so tol are
    0, and at the final assignment every point goes to centre 0 -- the other clusters have no member."""
    rng = np.random.default_rng([seed, n])
    x = np.tile(np.array([[0.125, -0.25, 0.375]], np.float32), (n, 1))
    return _unit_rows(rng, n, 16), x, _anchors(rng, n, 4)


def blobs(n=600, sd=1e-3, seed=3):
    """Four tight blobs at the corners of a 0.4 square, normal noise of standard deviation sd.  Lloyd is at its fixed
    point after one update; whether that update already moved the centres by no more than tol = 1e-4 mean(var) =
    2.7e-6 decides between the two stops: the expected squared shift is about 11 sd^2, so at sd = 1e-3 nearly every
    restart still stops on repeated labels and at sd = 3e-4 nearly every one stops on shift <= tol."""
    rng = np.random.default_rng([seed, n])
    corners = np.array([[0.2, 0.2, 0.0], [-0.2, 0.2, 0.0], [-0.2, -0.2, 0.0], [0.2, -0.2, 0.0]])
    x = (corners[rng.integers(0, 4, n)] + rng.normal(0.0, sd, (n, 3))).astype(np.float32)
    return _unit_rows(rng, n, 16), x, _anchors(rng, n, N_ANCHOR)


def ring_and_core(seed=11443968):
    """24 distinct points, half on a ring of radius 0.4 and half in a core of radius 0.05, all with ONE feature (any n_nn
    >= 24 selects the whole cloud).  Found by a search with the oracle over 12 million such sets: in restart 0 of K = 4 a
    cluster loses all its members to its neighbours' new means and is relocated to a point that is NOT a duplicate of a
    centre -- the one known input on which dropping the relocation changes the result (with n_init = 1, where restart 0
    is the model).  Relocations between duplicates (three_positions, identical) move a point onto a centre that is
    already there and change no mean."""
    rng = np.random.default_rng(seed)
    m = int(rng.integers(6, 51))
    th = rng.uniform(0, 2 * np.pi, m)
    r = np.where(rng.random(m) < 0.5, 0.4, rng.uniform(0, 0.05, m))
    x = np.stack([r * np.cos(th), r * np.sin(th), np.zeros(m)], 1).astype(np.float32)
    assert m == 24 and len(np.unique(x, axis=0)) == m
    f = np.zeros((m, 16), np.float32)
    f[:, 0] = 1.0
    return f, x, np.zeros(1, np.int32)


def exactly_K(K, seed=4):
    """A cloud of K rows, every row an anchor: each point is its own cluster."""
    rng = np.random.default_rng([seed, K])
    x = rng.uniform(-0.5, 0.5, (K, 3)).astype(np.float32)
    return _unit_rows(rng, K, 16), x, np.arange(K, dtype=np.int32)


def wave_quarter(n):
    """Rows per wave of the ordered compaction of k_symcut_select: q = ceil(ceil(n / 4) / 64) * 64."""
    return ((n + 3) // 4 + 63) // 64 * 64


TieCase = namedtuple("TieCase", "feat xyz anchors rows block closer")

# (rows strictly closer than the tie block, anchor included; tie rows in quarter 0 up to its end, in quarter 1 from
# its start, inside quarter 2, inside quarter 3) per (n_nn, variant).  Budget of ties = n_nn - closer:
#   "q2": spent inside quarter 2 (quarters 0 and 1 are taken whole, quarter 3 gets nothing)
#   "q1": spent inside quarter 1 (quarters 2 and 3 hold ties and get nothing)
TIE_LAYOUTS = {(50, "q2"): (10, 12, 12, 30, 10), (50, "q1"): (10, 25, 25, 10, 10),
               (20, "q2"): (6, 4, 4, 10, 6), (20, "q1"): (6, 8, 10, 10, 6)}


def tie_blocks(n, n_nn, variant="q2", n_anchor=12, seed=5):
    """Selection ties laid out against the four wave quarters.  Anchor 0 has a feature of its own; `closer` rows
    (itself included) are strictly nearer to it than a block of bit-identical rows that straddles the boundary of
    quarters 0 and 1, continues in quarter 2 and ends in quarter 3; every other row is farther.  The n_nn nearest
    are therefore the closer rows plus the first n_nn - closer block rows in row order (TieCase.rows).  Anchor 1 is
    the LAST block row: all its ties are at distance zero and the budget is spent in whatever quarter n_nn falls."""
    n_closer, b0, b1, b2, b3 = TIE_LAYOUTS[(n_nn, variant)]
    q = wave_quarter(n)
    assert 3 * q < n <= 4 * q, "all four waves must own rows"
    rng = np.random.default_rng([seed, n, n_nn, variant == "q1"])
    o2, o3 = 5, 7                                      # offsets inside quarters 2 and 3 (not lane-aligned)
    block = np.concatenate([np.arange(q - b0, q + b1), 2 * q + o2 + np.arange(b2), 3 * q + o3 + np.arange(b3)])
    assert block.max() < n and len(np.unique(block)) == b0 + b1 + b2 + b3
    free = np.setdiff1d(np.arange(n), block)
    closer = np.sort(rng.choice(free, n_closer, replace=False))
    anchor = int(closer[n_closer // 2])
    f = _unit_rows(rng, n, 16).astype(np.float64)
    a = f[anchor].copy()
    u = _unit_rows(rng, 1, 16)[0].astype(np.float64)
    tie = a + 0.5 * u
    tie /= np.linalg.norm(tie)
    near = a[None] + 0.1 * _unit_rows(rng, n_closer, 16)
    f[closer] = near / np.linalg.norm(near, axis=1, keepdims=True)
    f[anchor] = a
    f[block] = tie
    f = f.astype(np.float32)
    x = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    # the layout, by construction
    assert all(np.array_equal(f[r], f[block[0]]) for r in block)
    d = ((f.astype(np.float64) - f[anchor].astype(np.float64)) ** 2).sum(1)
    d_tie = d[block[0]]
    others = np.setdiff1d(free, closer)
    assert d[closer].max() < 0.5 * d_tie and d[others].min() > 1.5 * d_tie
    assert not np.isin(anchor, block) and d[anchor] == 0.0
    assert block[0] < q <= block[b0] and block[b0 - 1] == q - 1 and block[b0] == q          # straddles quarters 0 | 1
    assert ((block >= 2 * q) & (block < 3 * q)).sum() == b2 and (block >= 3 * q).sum() == b3
    need_eq = n_nn - n_closer
    assert 0 < need_eq < len(block) - b3
    if variant == "q1":
        assert b0 < need_eq < b0 + b1                  # spent inside quarter 1
    else:
        assert b0 + b1 < need_eq < b0 + b1 + b2        # spent inside quarter 2
    rows = np.sort(np.concatenate([closer, block[:need_eq]])).astype(np.int32)
    assert len(rows) == n_nn and not np.isin(block[-b3:], rows).any()
    anchors = _anchors(rng, n, n_anchor)
    anchors[0] = anchor
    anchors[1] = block[-1]
    return TieCase(f, x, anchors, rows, block, closer)


def wide_keys(n=600, n_anchor=12, seed=6):
    """Features that are NOT normalised: row norms from about 1e-15 to 1e15, so the squared distances to an anchor span
    some 200 binades and the first radix passes see many occupied bins.  Rows n // 2 .. n // 2 + 4 are copies of the
    row of anchor 0 (distance exactly zero).  Every value is finite, in f32 and squared in f64."""
    rng = np.random.default_rng([seed, n])
    scale = 10.0 ** rng.uniform(-15.0, 15.0, (n, 1))
    f = (rng.standard_normal((n, 16)) * scale).astype(np.float32)
    x = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    anchors = _anchors(rng, n, n_anchor)
    copies = np.setdiff1d(np.arange(n // 2, n // 2 + 6), anchors)[:5]
    f[copies] = f[anchors[0]]
    norms = np.linalg.norm(f.astype(np.float64), axis=1)
    assert np.isfinite(f).all() and norms.min() < 1e-13 and norms.max() > 1e13
    return f, x, anchors
