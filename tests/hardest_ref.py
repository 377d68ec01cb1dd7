"""NumPy restatement of cs_hardest_negatives (include/corsair_hip.h): exact f64 admissibility, the canonical f64 fma
chain over the feature columns, ties to the smaller row.

fma: this interpreter has no math.fma, so fma(a, b, c) is float(Fraction(a) * Fraction(b) + Fraction(c)): rational
arithmetic is exact and int / int true division (Fraction.__float__) rounds correctly to nearest-even, which is the
definition of the fused operation.  The exact chain is only run on the rows that can win: a vectorised plain
multiply-add chain d~ ranks all rows first.  Both chains sum C non-negative terms, so each is within (1 + 2^-53)^(C + 2)
- 1 < 3e-14 (C <= 256) of the true sum, and a row whose fma chain is minimal has d~ within 6e-14 relative of the
smallest d~; every admissible row with d~ <= min d~ * (1 + 1e-12) gets the exact chain, the rest cannot win or tie.
"""
import math
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def chain(q, t):
    """The canonical squared distance of two f32 rows: d = fma(diff, diff, d), columns ascending, diff in f64."""
    d = 0.0
    for qc, tc in zip(q, t):
        diff = float(qc) - float(tc)
        d = fma(diff, diff, d)
    return d


def admissible(qxyz, txyz, radius):
    """bool [nq, nt]: NOT ((dx dx + dy dy) + dz dz) < r r in f64; radius <= 0 admits everything."""
    nq, nt = len(qxyz), len(txyz)
    if not radius > 0:
        return np.ones((nq, nt), bool)
    q = np.asarray(qxyz, np.float32).astype(np.float64)
    t = np.asarray(txyz, np.float32).astype(np.float64)
    dx = q[:, None, 0] - t[None, :, 0]
    dy = q[:, None, 1] - t[None, :, 1]
    dz = q[:, None, 2] - t[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    return ~(d2 < np.float64(radius) * np.float64(radius))


def hardest(qf, qxyz, tf, txyz, radius, chunk=128):
    """One problem: for every query row the admissible target row of smallest chain distance.  Returns (idx int32
    [nq] or -1, dist f64 [nq] = sqrt(d) or +inf)."""
    qf = np.asarray(qf, np.float32)
    tf = np.asarray(tf, np.float32)
    nq, nt = len(qf), len(tf)
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, np.inf, np.float64)
    if nt == 0:
        return idx, dist
    t64 = tf.astype(np.float64)
    for i0 in range(0, nq, chunk):
        q64 = qf[i0:i0 + chunk].astype(np.float64)
        adm = admissible(qxyz[i0:i0 + chunk], txyz, radius)
        approx = np.zeros((len(q64), nt))
        for c in range(qf.shape[1]):
            diff = q64[:, c:c + 1] - t64[None, :, c]
            approx += diff * diff
        approx[~adm] = np.inf
        for k in range(len(q64)):
            m = approx[k].min()
            if not np.isfinite(m):
                continue
            best = None
            for j in np.nonzero(approx[k] <= m * (1 + 1e-12))[0]:
                d = chain(qf[i0 + k], tf[j])
                if best is None or d < best[0]:       # j ascends: strict < keeps the smaller row
                    best = (d, int(j))
            idx[i0 + k] = best[1]
            dist[i0 + k] = math.sqrt(best[0])
    return idx, dist


def hardest_batch(qf, qxyz, qoff, tf, txyz, toff, anchors, radius, qseg=None, tseg=None):
    """The whole call: anchors are global query rows; an anchor in no problem's segment gets -1 / +inf."""
    if qseg is None:
        qseg, tseg = list(range(len(qoff) - 1)), list(range(len(toff) - 1))
    anchors = np.asarray(anchors, np.int64)
    idx = np.full(len(anchors), -1, np.int32)
    dist = np.full(len(anchors), np.inf, np.float64)
    for qs, ts in zip(qseg, tseg):
        sel = np.nonzero((anchors >= qoff[qs]) & (anchors < qoff[qs + 1]))[0]
        if len(sel) == 0:
            continue
        rows = anchors[sel]
        t0, t1 = int(toff[ts]), int(toff[ts + 1])
        i, d = hardest(qf[rows], qxyz[rows], tf[t0:t1], txyz[t0:t1], radius)
        idx[sel], dist[sel] = i, d
    return idx, dist
