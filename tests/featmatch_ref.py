"""NumPy / Python restatement of cs_corr_mutual and cs_ransac_fm_batch (include/corsair_hip.h), bit for bit: the mutual filter
with its fallback and stable compaction, the draws of common.h's generator, the edge-length checker, the Horn fit (horn_qcp
and Horn's matrix of tests/icp_ref.py, the operation sequence of corsair_amd/csrc/horn.h), the distance checker, the counts,
the tie rule and the fixed-point rmse.

Every plain Python float operation is one IEEE f64 operation; fma is the exact form of tests/gicp_ref.py.  The exact chains
only run where they can matter: unfused vectorised chains classify first, with an error bound that covers both chains
(each rounds a sum of a few terms once per operation, so both lie within a few 2^-53 of the sum of the terms' magnitudes;
the bounds below take 2^-48), and whatever lies within the bound or a relative 1e-12 of a threshold takes the exact chain.
The rmse needs the exact d2 of every inlier of the best hypothesis (the truncation sees every bit).
"""
import math

import numpy as np

from tests.gicp_ref import fma
from tests.icp_ref import horn_matrix, horn_qcp
from tests.plane_ref import rng_index

IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
E48 = 2.0 ** -48


# ---- cs_corr_mutual ----------------------------------------------------------------------------------------------------
def mutual(nn_fwd, nn_bwd, xyz0, off0, xyz1, off1, ransac_n=3, mutual=True):
    """(src f32 [N0,3], tgt f32 [N0,3], m int32 [P], stat int32 [P,2]); the slots past m[p] are zero."""
    xyz0 = np.asarray(xyz0, np.float32).reshape(-1, 3)
    xyz1 = np.asarray(xyz1, np.float32).reshape(-1, 3)
    fwd = np.asarray(nn_fwd, np.int64).reshape(-1)
    bwd = None if nn_bwd is None else np.asarray(nn_bwd, np.int64).reshape(-1)
    P = len(off0) - 1
    src = np.zeros((len(xyz0), 3), np.float32)
    tgt = np.zeros((len(xyz0), 3), np.float32)
    m = np.zeros(P, np.int32)
    stat = np.zeros((P, 2), np.int32)
    for p in range(P):
        a0, a1, b0, b1 = int(off0[p]), int(off0[p + 1]), int(off1[p]), int(off1[p + 1])
        n1 = b1 - b0
        valid, mut = [], []
        for i in range(a1 - a0):
            j = int(fwd[a0 + i])
            if 0 <= j < n1:
                valid.append(i)
                if mutual and int(bwd[b0 + j]) == i:
                    mut.append(i)
        use_mut = bool(mutual) and len(mut) >= 3 * ransac_n
        kept = mut if use_mut else valid
        for s, i in enumerate(kept):
            src[a0 + s] = xyz0[a0 + i]
            tgt[a0 + s] = xyz1[b0 + int(fwd[a0 + i])]
        m[p] = len(kept)
        stat[p] = (len(mut) if mutual else len(valid), 1 if (mutual and not use_mut) else 0)
    return src, tgt, m, stat


# ---- cs_ransac_fm_batch ------------------------------------------------------------------------------------------------
def draws(seed, t, n, m):
    return [rng_index(seed, t, j, m) for j in range(n)]


def _len2(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return fma(dz, dz, fma(dy, dy, dx * dx))


def edge_exact(S, Q, sim2):
    """The edge-length checker on the sampled rows S, Q (lists of three floats each)."""
    n = len(S)
    for a in range(n):
        for b in range(a + 1, n):
            ls2, lt2 = _len2(S[a], S[b]), _len2(Q[a], Q[b])
            if not (ls2 >= sim2 * lt2 and lt2 >= sim2 * ls2):
                return False
    return True


def dist2(R, s, q):
    """The canonical chain of the posed source: R = 12 floats (4a+b = R[a][b], 4a+3 = t[a])."""
    d = [fma(R[4 * c + 2], s[2], fma(R[4 * c + 1], s[1], fma(R[4 * c], s[0], R[4 * c + 3]))) - q[c] for c in range(3)]
    return fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0]))


def _div(a, b):
    """a / b as IEEE divides (Python raises on a zero divisor)."""
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def fit(S, Q):
    """R | t (12 floats) of the sampled rows, None when horn_qcp declines or a value is not finite."""
    n = len(S)
    dn = float(n)
    cs, ct = [0.0] * 3, [0.0] * 3
    for j in range(n):
        for c in range(3):
            cs[c] = cs[c] + S[j][c]
            ct[c] = ct[c] + Q[j][c]
    cs = [v / dn for v in cs]
    ct = [v / dn for v in ct]
    M = [[0.0] * 3 for _ in range(3)]
    for j in range(n):
        ds = [S[j][c] - cs[c] for c in range(3)]
        dt = [Q[j][c] - ct[c] for c in range(3)]
        for x in range(3):
            for y in range(3):
                M[x][y] = fma(ds[x], dt[y], M[x][y])
    q = horn_qcp(M, horn_matrix(M))
    if q is None:
        return None
    qw, qx, qy, qz = q
    s = qw * qw + qx * qx + qy * qy + qz * qz
    qn = math.sqrt(s) if s >= 0.0 else math.nan
    qw, qx, qy, qz = _div(qw, qn), _div(qx, qn), _div(qy, qn), _div(qz, qn)
    R = [0.0] * 12
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz)
    R[1] = 2.0 * (qx * qy - qw * qz)
    R[2] = 2.0 * (qx * qz + qw * qy)
    R[4] = 2.0 * (qx * qy + qw * qz)
    R[5] = 1.0 - 2.0 * (qx * qx + qz * qz)
    R[6] = 2.0 * (qy * qz - qw * qx)
    R[8] = 2.0 * (qx * qz - qw * qy)
    R[9] = 2.0 * (qy * qz + qw * qx)
    R[10] = 1.0 - 2.0 * (qx * qx + qy * qy)
    for a in range(3):
        R[4 * a + 3] = ct[a] - (R[4 * a] * cs[0] + R[4 * a + 1] * cs[1] + R[4 * a + 2] * cs[2])
    if not all(math.isfinite(v) for v in R):
        return None
    return R


def hypothesis(s64, q64, idx, sim2, thr2, check_distance=True, edge_known=None):
    """R | t of the hypothesis that samples the rows idx, None when it is not valid.  edge_known: the edge checker's answer
    when the vectorised screen was sure of it."""
    S = [[float(v) for v in s64[i]] for i in idx]
    Q = [[float(v) for v in q64[i]] for i in idx]
    if sim2 > 0.0:
        ok = edge_exact(S, Q, sim2) if edge_known is None else edge_known
        if not ok:
            return None
    R = fit(S, Q)
    if R is None:
        return None
    if check_distance and not all(dist2(R, S[j], Q[j]) < thr2 for j in range(len(S))):
        return None
    return R


def edge_screen(s64, q64, I, sim2):
    """Vectorised edge checker over the draws I [K,n]: int8 [K], 1 = passes for sure, 0 = fails for sure, -1 = exact chain."""
    K, n = I.shape
    sure_ok = np.ones(K, bool)
    sure_no = np.zeros(K, bool)
    with np.errstate(all="ignore"):
        for a in range(n):
            for b in range(a + 1, n):
                ls2 = ((s64[I[:, a]] - s64[I[:, b]]) ** 2).sum(1)
                lt2 = ((q64[I[:, a]] - q64[I[:, b]]) ** 2).sum(1)
                for x, y in ((ls2, lt2), (lt2, ls2)):
                    lo, hi = x * (1 - 1e-12), x * (1 + 1e-12)
                    r = sim2 * y
                    sure_ok &= lo >= r * (1 + 1e-12)
                    sure_no |= (hi < r * (1 - 1e-12)) & np.isfinite(x) & np.isfinite(r)
        finite = np.isfinite(s64[I]).all((1, 2)) & np.isfinite(q64[I]).all((1, 2))   # a NaN or inf sample: the exact chain
    return np.where(~finite, -1, np.where(sure_no, 0, np.where(sure_ok, 1, -1))).astype(np.int8)


def classify(s64, q64, R, thr2):
    """(inlier bool [m], exact d2 of the rows that needed the exact chain: dict row -> d2)."""
    m = len(s64)
    exact = {}
    if m == 0 or not thr2 > 0.0:
        return np.zeros(m, bool), exact
    with np.errstate(all="ignore"):
        d2 = np.zeros(m)
        err = np.zeros(m)
        for c in range(3):
            t0, t1, t2 = R[4 * c] * s64[:, 0], R[4 * c + 1] * s64[:, 1], R[4 * c + 2] * s64[:, 2]
            d = (t0 + t1 + t2 + R[4 * c + 3]) - q64[:, c]
            e = E48 * (np.abs(t0) + np.abs(t1) + np.abs(t2) + abs(R[4 * c + 3]) + np.abs(q64[:, c]))
            d2 = d2 + d * d
            err = err + 2.0 * np.abs(d) * e + e * e
        err = err + E48 * d2
        sure_in = d2 + err < thr2 * (1 - 1e-12)
        sure_out = (d2 - err > thr2 * (1 + 1e-12)) & np.isfinite(d2) & np.isfinite(err)
    inl = sure_in.copy()
    for i in np.nonzero(~(sure_in | sure_out))[0]:
        v = dist2(R, [float(x) for x in s64[i]], [float(x) for x in q64[i]])
        exact[int(i)] = v
        inl[i] = v < thr2
    return inl, exact


class Table:
    """Everything about the first `iterations` hypotheses of one problem: valid t -> R, t -> count."""

    def __init__(self, src, tgt, max_corr, ransac_n=3, edge_similarity=0.9, check_distance=True, iterations=1, seed=0):
        self.s32 = np.asarray(src, np.float32).reshape(-1, 3)
        self.q32 = np.asarray(tgt, np.float32).reshape(-1, 3)
        self.s64, self.q64 = self.s32.astype(np.float64), self.q32.astype(np.float64)
        self.m, self.n, self.iterations, self.seed = len(self.s64), int(ransac_n), int(iterations), int(seed)
        self.thr2 = float(max_corr) * float(max_corr)
        self.sim2 = float(edge_similarity) * float(edge_similarity)
        self.R, self.count, self.masks = {}, {}, {}
        if self.m < self.n:
            return
        I = np.asarray([draws(self.seed, t, self.n, self.m) for t in range(self.iterations)], np.int64).reshape(-1, self.n)
        screen = edge_screen(self.s64, self.q64, I, self.sim2) if self.sim2 > 0.0 else np.full(len(I), 1, np.int8)
        for t in np.nonzero(screen != 0)[0]:
            known = None if screen[t] < 0 else True
            R = hypothesis(self.s64, self.q64, I[t], self.sim2, self.thr2, check_distance, known)
            if R is not None:
                inl, _ = classify(self.s64, self.q64, R, self.thr2)
                self.R[int(t)], self.count[int(t)], self.masks[int(t)] = R, int(inl.sum()), inl

    def valid(self, iterations=None):
        k = self.iterations if iterations is None else iterations
        return sorted(t for t in self.R if t < k)

    def result(self, iterations=None):
        """(T 16 floats, stat [found, t_best, inliers, n_valid], rmse, inlier bool [m]) of the first `iterations` hypotheses."""
        k = self.iterations if iterations is None else iterations
        assert 1 <= k <= self.iterations
        valid = self.valid(k)
        best, t_best = 0, -1
        for t in valid:                               # ascending t: a later equal count does not replace the first
            if self.count[t] > best:
                best, t_best = self.count[t], t
        if self.m < self.n or best < self.n:
            return list(IDENTITY), [0, -1, 0, len(valid)], 0.0, np.zeros(self.m, bool)
        R, inl = self.R[t_best], self.masks[t_best]
        eM = 0 if self.m <= 1 else (self.m - 1).bit_length()
        ex = 1024
        if self.thr2 < math.inf:
            ex = max(math.frexp(self.thr2)[1], -900)
        k2 = 61 - eM - ex
        scale = math.ldexp(1.0, k2)
        E = 0
        for i in np.nonzero(inl)[0]:
            d2 = dist2(R, [float(x) for x in self.s64[i]], [float(x) for x in self.q64[i]])
            assert d2 < self.thr2
            E += int(d2 * scale)
        assert E < 1 << 63
        rmse = math.sqrt((float(E) * math.ldexp(1.0, -k2)) / float(best))
        return R + [0.0, 0.0, 0.0, 1.0], [1, t_best, best, len(valid)], rmse, inl


def ransac_fm_one(src, tgt, max_corr, ransac_n=3, edge_similarity=0.9, check_distance=True, iterations=100000, seed=0):
    return Table(src, tgt, max_corr, ransac_n, edge_similarity, check_distance, iterations, seed).result()


def ransac_fm_batch(src, tgt, offsets, max_corr, m=None, ransac_n=3, edge_similarity=0.9, check_distance=True,
                    iterations=100000, seed=0):
    """(T f64 [P,4,4], stat int32 [P,4], rmse f64 [P]): cs_ransac_fm_batch."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    P = len(offsets) - 1
    T = np.zeros((P, 4, 4), np.float64)
    stat = np.zeros((P, 4), np.int32)
    rmse = np.zeros(P, np.float64)
    for p in range(P):
        a, b = int(offsets[p]), int(offsets[p + 1])
        k = b - a if m is None else min(max(int(m[p]), 0), b - a)
        Tp, stat[p], rmse[p], _ = ransac_fm_one(src[a:a + k], tgt[a:a + k], max_corr, ransac_n, edge_similarity,
                                                check_distance, iterations, seed)
        T[p] = np.asarray(Tp).reshape(4, 4)
    return T, stat, rmse
