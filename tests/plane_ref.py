"""NumPy / Python restatement of cs_segment_plane (include/corsair_hip.h), bit for bit: the draws of common.h's generator, the
hypotheses operation by operation, Python integers for the nine sums and the 128-bit covariance, jacobi3 of
tests/normals_ref.py, the selection, the orientation.

Every plain Python float operation is one IEEE f64 operation; fma is the exact form of tests/gicp_ref.py.  The exact chain
s = fma(u_z, n_z, fma(u_y, n_y, u_x * n_x)) only runs where it can matter: an unfused vectorised chain s~ classifies all rows
first.  Both chains lie within 3 * 2^-53 * T of the true sum, T = |u_x n_x| + |u_y n_y| + |u_z n_z|, so with err = 2^-49 T a row
with (|s~| + err)^2 < bound (1 - 1e-12) is an inlier, one with (|s~| - err)^2 > bound (1 + 1e-12), |s~| > err, is none and has
the sign of s~; every other row (a non-finite one among them) takes the exact chain.
"""
import math

import numpy as np

from tests.gicp_ref import fma
from tests.normals_ref import jacobi3

MAX_ITERS = 65536
MASK = (1 << 64) - 1
NO_PLANE = (0, -1, 0, 0, 0, 0, 0)


def rng_u64(seed, itr, j):
    x = (seed + 0x9E3779B97F4A7C15 * (itr * 64 + j + 1)) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def rng_index(seed, itr, j, m):
    return (((rng_u64(seed, itr, j) >> 32) * m) >> 32) & 0xFFFFFFFF


def triple(seed, t, m):
    return tuple(rng_index(seed, t, j, m) for j in range(3))


def hypothesis(s64, tri, thr2):
    """(o, n, nn, bound) of the rows `tri`; bound = 0.0 for a hypothesis that is not valid."""
    p0, p1, p2 = ([float(v) for v in s64[i]] for i in tri)
    with np.errstate(all="ignore"):
        e1 = [p1[a] - p0[a] for a in range(3)]
        e2 = [p2[a] - p0[a] for a in range(3)]
        n = [fma(e1[1], e2[2], -(e1[2] * e2[1])), fma(e1[2], e2[0], -(e1[0] * e2[2])), fma(e1[0], e2[1], -(e1[1] * e2[0]))]
        nn = fma(n[2], n[2], fma(n[1], n[1], n[0] * n[0]))
        bound = thr2 * nn
    valid = 0.0 < nn < math.inf and 0.0 < bound < math.inf
    return p0, n, nn, (bound if valid else 0.0)


def s_exact(row, c, n):
    ux, uy, uz = float(row[0]) - c[0], float(row[1]) - c[1], float(row[2]) - c[2]
    return fma(uz, n[2], fma(uy, n[1], ux * n[0]))


def classify(s64, c, n, bound):
    """(inlier bool [m], side int8 [m]: the sign of s for the rows that are no inliers) against s * s < bound."""
    m = len(s64)
    if not bound > 0.0:
        return np.zeros(m, bool), np.zeros(m, np.int8)
    with np.errstate(all="ignore"):
        ux, uy, uz = s64[:, 0] - c[0], s64[:, 1] - c[1], s64[:, 2] - c[2]
        tx, ty, tz = ux * n[0], uy * n[1], uz * n[2]
        approx = tx + ty + tz
        err = (np.abs(tx) + np.abs(ty) + np.abs(tz)) * 2.0 ** -49
        a = np.abs(approx)
        hi, lo = a + err, a - err
        sure_in = hi * hi < bound * (1 - 1e-12)
        sure_out = (lo > 0.0) & (lo * lo > bound * (1 + 1e-12)) & np.isfinite(approx)
    inl = sure_in.copy()
    side = np.where(sure_out, np.sign(approx), 0).astype(np.int8)
    for q in np.nonzero(~(sure_in | sure_out))[0]:
        with np.errstate(all="ignore"):
            s = s_exact(s64[q], c, n)
            inl[q] = s * s < bound
        side[q] = 0 if inl[q] else (1 if s > 0.0 else (-1 if s < 0.0 else 0))
    return inl, side


def counts(seg, dist, iters, seed):
    """count_t for t < iters (int64 [iters]); a prefix of the counts of a larger iters."""
    s64 = np.asarray(seg, np.float32).reshape(-1, 3).astype(np.float64)
    m = len(s64)
    out = np.zeros(iters, np.int64)
    thr2 = float(dist) * float(dist)
    for t in range(iters if m else 0):
        o, n, _, bound = hypothesis(s64, triple(seed, t, m), thr2)
        if bound > 0.0:
            out[t] = int(classify(s64, o, n, bound)[0].sum())
    return out


def shift_of(M):
    return min(15 - math.frexp(M)[1], 1023)


def cov_to_float(c):
    mag = abs(c)
    d = float(mag >> 64) * 18446744073709551616.0 + float(mag & MASK)
    return -d if c < 0 else d


def refit(s64, inl, o, n_s, nn):
    """(n, c, refit) of stage 2 over the rows `inl` (bool), about o; the sampled plane (n_s, nn) where it is skipped."""
    A = s64[inl]
    U = [[float(r[a]) - o[a] for a in range(3)] for r in A]
    M = max((abs(v) for u in U for v in u), default=0.0)
    e = None
    if M > 0.0:
        sh = shift_of(M)
        Q = [[int(np.rint(math.ldexp(v, sh))) for v in u] for u in U]
        assert all(abs(v) <= 1 << 15 for q in Q for v in q)
        S = [sum(q[a] for q in Q) for a in range(3)]
        S2 = {(a, b): sum(q[a] * q[b] for q in Q) for a in range(3) for b in range(a, 3)}
        assert max(abs(v) for v in list(S2.values()) + S) < 1 << 62
        cnt = len(Q)
        C = [[0.0] * 3 for _ in range(3)]
        for (a, b), sab in S2.items():
            c = cnt * sab - S[a] * S[b]
            assert abs(c) < 1 << 93
            C[a][b] = C[b][a] = cov_to_float(c)
        v = jacobi3(C)
        best, col = C[0][0], 0
        for k in (1, 2):
            if C[k][k] < best:
                best, col = C[k][k], k
        e = [v[0][col], v[1][col], v[2][col]]
        len2 = fma(e[2], e[2], fma(e[1], e[1], e[0] * e[0]))
        if not 0.0 < len2 < math.inf:
            e = None
    if e is None:
        ln = math.sqrt(nn)
        return [n_s[0] / ln, n_s[1] / ln, n_s[2] / ln], list(o), 0
    ln = math.sqrt(len2)
    c = [o[a] + math.ldexp(float(S[a]) / float(cnt), -sh) for a in range(3)]
    return [e[0] / ln, e[1] / ln, e[2] / ln], c, 1


def segment_plane_one(seg, dist, iters, seed, count=None):
    """(plane 4 floats, stat 8 ints, inlier bool [m]) of one segment; count: counts(seg, dist, >= iters, seed) if at hand."""
    assert 1 <= iters <= MAX_ITERS and 0.0 < float(dist) < math.inf
    s32 = np.asarray(seg, np.float32).reshape(-1, 3)
    s64 = s32.astype(np.float64)
    m = len(s64)
    finite = np.isfinite(s64).all(1)
    none = ([0.0] * 4, list(NO_PLANE) + [int(finite.sum())], np.zeros(m, bool))
    if m == 0:
        return none
    thr2 = float(dist) * float(dist)
    count = counts(s32, dist, iters, seed) if count is None else np.asarray(count)[:iters]
    t = int(np.argmax(count))                      # the first of the largest
    if count[t] < 3:
        return none
    o, n_s, nn, bound = hypothesis(s64, triple(seed, t, m), thr2)
    inl1 = classify(s64, o, n_s, bound)[0]
    assert int(inl1.sum()) == int(count[t])
    n, c, did = refit(s64, inl1, o, n_s, nn)
    inl, side = classify(s64, c, n, thr2)
    inl &= finite
    n_pos = int(((side > 0) & finite & ~inl).sum())
    n_neg = int(((side < 0) & finite & ~inl).sum())
    flip = n_neg > n_pos
    if n_neg == n_pos:
        big, lead = abs(n[0]), n[0]
        for k in (1, 2):
            if abs(n[k]) > big:
                big, lead = abs(n[k]), n[k]
        flip = lead < 0.0
    if flip:
        n = [-n[0], -n[1], -n[2]]
        n_pos, n_neg = n_neg, n_pos
    d = -fma(c[2], n[2], fma(c[1], n[1], c[0] * n[0]))
    return n + [d], [1, t, int(count[t]), did, int(inl.sum()), n_pos, n_neg, int(finite.sum())], inl


def segment_plane(xyz, offsets, dist, iters=1024, seed=0):
    """(inlier bool [n], plane f64 [n_seg,4], stat int32 [n_seg,8]): cs_segment_plane."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n_seg = len(offsets) - 1
    inlier = np.zeros(len(xyz), bool)
    plane = np.zeros((n_seg, 4), np.float64)
    stat = np.zeros((n_seg, 8), np.int32)
    for p, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        plane[p], stat[p], inlier[a:b] = segment_plane_one(xyz[a:b], dist, iters, seed)
    return inlier, plane, stat
