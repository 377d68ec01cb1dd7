"""NumPy / Python restatement of cs_sc2_batch (include/corsair_hip.h), bit for bit: the compatibility matrix, the
degrees and the seed ranks, the second-order counts, the consensus sets, the fit (tests/featmatch_ref.fit: the Horn fit of
cs_ransac_fm_batch at any n), the counts, the tie rules and the fixed-point rmse.

Every plain Python float operation is one IEEE f64 operation; fma is the exact form of tests/gicp_ref.py.  The exact chains
only run where they can matter (tests/featmatch_ref.py's habit): an unfused vectorised chain classifies every pair of rows
first.  Both squared lengths are sums of three squares, so the fused and the unfused chain lie within a relative 2^-50 of the
true sum; the bounds below take 2^-48, and whatever lies within them of a threshold, underflows, overflows or is not finite
takes the exact chain.  Everything else is integer work (NumPy sorts with the header's keys, a float32 matrix product for the
second-order counts, exact below 2^24).
"""
import math
import types

import numpy as np

from tests import featmatch_ref as fm
from tests import icp_ref
from tests.gicp_ref import fma


def _rebound(fn, **names):
    """fn with some of its module's globals replaced: the same operation sequence, other helpers."""
    return types.FunctionType(fn.__code__, {**fn.__globals__, **names}, fn.__name__, fn.__defaults__)


# tests/icp_ref.py's solver with the four times faster exact fma of tests/gicp_ref.py (tests/test_gicp_cpu.py compares the two
# fmas; tests/test_sc2_cpu.py compares the two fits): a call with n_seeds = 0 fits every row of a problem
fit = _rebound(fm.fit, horn_qcp=_rebound(icp_ref.horn_qcp, fma=fma))

IDENTITY = fm.IDENTITY
E48 = 2.0 ** -48
TINY = 1e-280
BLOCK = 512


def _len2(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return fma(dz, dz, fma(dy, dy, dx * dx))


def compat_exact(si, qi, sj, qj, tau2):
    """c_ij of two rows (lists of three floats each) by the header's chain."""
    if not all(math.isfinite(v) for v in (*si, *qi, *sj, *qj)):
        return False
    ls2, lt2 = _len2(si, sj), _len2(qi, qj)
    a = (ls2 + lt2) - tau2
    return ls2 > 0.0 and lt2 > 0.0 and (a < 0.0 or a * a < 4.0 * (ls2 * lt2))


def compat_matrix(s64, q64, tau2):
    """bool [m,m]: the compatibility matrix, and the number of pairs of rows that took the exact chain."""
    m = len(s64)
    C = np.zeros((m, m), bool)
    n_exact = 0
    if m == 0:
        return C, n_exact
    fin = np.isfinite(s64).all(1) & np.isfinite(q64).all(1)
    with np.errstate(all="ignore"):
        for r0 in range(0, m, BLOCK):
            r1 = min(m, r0 + BLOCK)
            e = s64[r0:r1, None, :] - s64[None, :, :]
            f = q64[r0:r1, None, :] - q64[None, :, :]
            ls2 = (e * e).sum(2)
            lt2 = (f * f).sum(2)
            zero = (e == 0.0).all(2) | (f == 0.0).all(2)          # an exact zero length in either chain
            both = fin[r0:r1, None] & fin[None, :]
            a = (ls2 + lt2) - tau2
            ea = 4.0 * E48 * (ls2 + lt2 + (tau2 if math.isfinite(tau2) else 0.0))
            rhs = 4.0 * (ls2 * lt2)
            lo, hi = np.maximum(np.abs(a) - ea, 0.0), np.abs(a) + ea
            sure_yes = (a < -ea) | ((hi * hi) * (1 + 8 * E48) < rhs * (1 - 8 * E48))
            sure_no = (a > ea) & ((lo * lo) * (1 - 8 * E48) > rhs * (1 + 8 * E48))
            safe = (ls2 > TINY) & (lt2 > TINY) & (rhs > TINY) & np.isfinite(hi * hi) & np.isfinite(rhs) & np.isfinite(a)
            known = ~both | zero | (safe & (sure_yes | sure_no))
            C[r0:r1] = both & ~zero & safe & sure_yes
            for i, j in zip(*np.nonzero(~known)):
                n_exact += 1
                C[r0 + i, j] = compat_exact([float(v) for v in s64[r0 + i]], [float(v) for v in q64[r0 + i]],
                                            [float(v) for v in s64[j]], [float(v) for v in q64[j]], tau2)
    return C, n_exact


def seed_order(deg):
    """The rows in the order of their ranks: the largest key (deg << 32) | ~row first."""
    m = len(deg)
    return np.lexsort((np.arange(m), -deg.astype(np.int64)))


class Graph:
    """Everything about one problem that the parameters n_seeds and K do not change: the matrix, the degrees, the rank
    order; per seed rank the second-order counts; per (rank, K) the consensus set, the fit and the count."""

    def __init__(self, src, tgt, compat_dist, max_corr):
        self.s32 = np.asarray(src, np.float32).reshape(-1, 3)
        self.q32 = np.asarray(tgt, np.float32).reshape(-1, 3)
        self.s64, self.q64 = self.s32.astype(np.float64), self.q32.astype(np.float64)
        self.m = len(self.s64)
        self.tau2 = float(compat_dist) * float(compat_dist)
        self.thr2 = float(max_corr) * float(max_corr)
        self.C, self.n_exact = compat_matrix(self.s64, self.q64, self.tau2)
        self.deg = self.C.sum(1).astype(np.int64)
        self.order = seed_order(self.deg)
        self._Cf = None
        self._sc = {}
        self._hyp = {}

    def n_seeds(self, n_seeds):
        return self.m if n_seeds == 0 else min(int(n_seeds), self.m)

    def scores(self, ranks):
        """Second-order counts of the seeds of the given ranks against every row (int64 [len(ranks), m])."""
        need = [r for r in ranks if r not in self._sc]
        if need:
            if self._Cf is None:
                self._Cf = self.C.astype(np.float32)
            sc = np.rint(self._Cf[self.order[need]] @ self._Cf).astype(np.int64)
            for k, r in enumerate(need):
                self._sc[r] = sc[k]
        return [self._sc[r] for r in ranks]

    def consensus(self, r, K):
        """A_s of the seed of rank r in ascending row index (None: fewer than three rows)."""
        s = int(self.order[r])
        cand = np.nonzero(self.C[s])[0]
        sc = self.scores([r])[0][cand]
        take = cand[np.lexsort((cand, -sc))[:K]]
        A = sorted([s] + [int(j) for j in take])
        return A if len(A) >= 3 else None

    def hypothesis(self, r, K):
        """(A, R | t or None, count, mask) of the seed of rank r."""
        if (r, K) not in self._hyp:
            A = self.consensus(r, K)
            R = None
            if A is not None:
                R = fit([[float(v) for v in self.s64[i]] for i in A], [[float(v) for v in self.q64[i]] for i in A])
            if R is None:
                self._hyp[(r, K)] = (A, None, 0, None)
            else:
                inl, _ = fm.classify(self.s64, self.q64, R, self.thr2)
                self._hyp[(r, K)] = (A, R, int(inl.sum()), inl)
        return self._hyp[(r, K)]

    def result(self, n_seeds=1024, K=20):
        """(T 16 floats, stat [found, row, count, n_valid, rank, deg], rmse, inlier bool [m])."""
        S = self.n_seeds(n_seeds)
        self.scores(list(range(S)))
        best, r_best, n_valid = 0, -1, 0
        for r in range(S):                                 # ascending rank: a later equal count does not replace the first
            _, R, count, _ = self.hypothesis(r, K)
            if R is None:
                continue
            n_valid += 1
            if count > best:
                best, r_best = count, r
        if self.m < 3 or best < 3:
            return list(IDENTITY), [0, -1, 0, n_valid, -1, 0], 0.0, np.zeros(self.m, bool)
        _, R, _, inl = self.hypothesis(r_best, K)
        eM = 0 if self.m <= 1 else (self.m - 1).bit_length()
        ex = 1024
        if self.thr2 < math.inf:
            ex = max(math.frexp(self.thr2)[1], -900)
        k2 = 61 - eM - ex
        scale = math.ldexp(1.0, k2)
        E = 0
        for i in np.nonzero(inl)[0]:
            d2 = fm.dist2(R, [float(x) for x in self.s64[i]], [float(x) for x in self.q64[i]])
            assert d2 < self.thr2
            E += int(d2 * scale)
        assert E < 1 << 63
        rmse = math.sqrt((float(E) * math.ldexp(1.0, -k2)) / float(best))
        row = int(self.order[r_best])
        return R + [0.0, 0.0, 0.0, 1.0], [1, row, best, n_valid, r_best, int(self.deg[row])], rmse, inl


def sc2_one(src, tgt, max_corr, compat_dist, n_seeds=1024, k_consensus=20):
    return Graph(src, tgt, compat_dist, max_corr).result(n_seeds, k_consensus)


def sc2_batch(src, tgt, offsets, max_corr, compat_dist, m=None, n_seeds=1024, k_consensus=20):
    """(T f64 [P,4,4], stat int32 [P,6], rmse f64 [P], mask u8 [offsets[-1]]): cs_sc2_batch."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    P = len(offsets) - 1
    T = np.zeros((P, 4, 4), np.float64)
    stat = np.zeros((P, 6), np.int32)
    rmse = np.zeros(P, np.float64)
    mask = np.zeros(int(offsets[-1]), np.uint8)
    for p in range(P):
        a, b = int(offsets[p]), int(offsets[p + 1])
        k = b - a if m is None else min(max(int(m[p]), 0), b - a)
        Tp, stat[p], rmse[p], inl = sc2_one(src[a:a + k], tgt[a:a + k], max_corr, compat_dist, n_seeds, k_consensus)
        T[p] = np.asarray(Tp).reshape(4, 4)
        mask[a:a + k] = inl
    return T, stat, rmse, mask
