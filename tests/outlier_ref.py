"""NumPy / Python restatement of cs_knn_mean_dist, cs_outlier_statistical and cs_outlier_radius (include/corsair_hip.h),
bit for bit: NumPy for the distance chains, Python integers for the three sums, the finishing sequence operation by
operation.

Every plain Python float operation is one IEEE f64 operation; fma is the exact form of tests/gicp_ref.py.  As in
tests/normals_ref.py the exact distance chain only runs where it can matter: an unfused vectorised chain d~ ranks all rows
first, and both chains are within 4 * 2^-53 relative of the true sum of the same three squares, so a row outside
d~ <= (k-th smallest d~) * (1 + 1e-12) cannot enter or tie the list, and a pair outside |d~ - r2| <= 1e-12 r2 is on the
side of the radius that d~ says.
"""
import math

import numpy as np

from tests.gicp_ref import fma

K_MIN, K_MAX = 2, 32
NAN = float(np.float64(np.nan))


def _approx(s64, i):
    """d~ of row i to every row of the segment; +inf where it is not finite."""
    with np.errstate(all="ignore"):
        dx, dy, dz = s64[:, 0] - s64[i, 0], s64[:, 1] - s64[i, 1], s64[:, 2] - s64[i, 2]
        a = dx * dx + dy * dy + dz * dz
    return np.where(np.isfinite(a), a, np.inf)


def d2_exact(s64, i, j):
    ux, uy, uz = float(s64[j, 0]) - float(s64[i, 0]), float(s64[j, 1]) - float(s64[i, 1]), float(s64[j, 2]) - float(s64[i, 2])
    return fma(uz, uz, fma(uy, uy, ux * ux))


def nearest_d2(seg, i, k):
    """The min(k, found) smallest finite d2 of row i of `seg` (f32 [n,3]), ascending; itself included."""
    s64 = np.asarray(seg, np.float32).astype(np.float64)
    n = len(s64)
    if n == 0:
        return []
    approx = _approx(s64, i)
    m = min(k, n)
    kth = np.partition(approx, m - 1)[m - 1]
    cand = np.nonzero(approx <= kth * (1 + 1e-12))[0] if math.isfinite(kth) else np.nonzero(np.isfinite(approx))[0]
    out = []
    for j in cand:
        d = d2_exact(s64, i, j)
        if math.isfinite(d):
            out.append(d)
    out.sort()
    return out[:k]


def mean_of(d2s):
    """(((+0 + sqrt(d2_0)) + sqrt(d2_1)) + ...) / c; NaN for an empty list."""
    if not d2s:
        return NAN
    s = 0.0
    for d in d2s:
        s = s + math.sqrt(d)
    return s / float(len(d2s))


def knn_mean_dist(xyz, offsets, k):
    """f64 [n]: cs_knn_mean_dist."""
    assert K_MIN <= k <= K_MAX
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.full(len(xyz), np.nan, np.float64)
    for a, b in zip(offsets[:-1], offsets[1:]):
        seg = xyz[a:b]
        for i in range(b - a):
            out[a + i] = mean_of(nearest_d2(seg, i, k))
    return out


def shift_of(M):
    """s = min(31 - e, 1023) for M = f 2^e, f in [0.5, 1); 31 for M = 0."""
    e = math.frexp(M)[1] if M > 0.0 else 0
    return min(31 - e, 1023)


def quantise(means):
    """(n_valid, M, s, [q_i] as Python integers) of one segment's means."""
    valid = [float(m) for m in means if 0.0 <= float(m) < math.inf]          # False for NaN
    M = max(valid) if valid else 0.0
    s = shift_of(M)
    q = [int(np.rint(math.ldexp(m, s))) for m in valid]                      # rint: round to nearest even
    return len(valid), M, s, q


def finish(n, M, s, q, std_ratio):
    """(n_valid, mu, sigma, tau) from the integer sums, the header's sequence."""
    S1 = sum(q)
    S2lo = sum((v * v) & 0xFFFFFFFF for v in q)
    S2hi = sum((v * v) >> 32 for v in q)
    assert max(S1, S2lo, S2hi) < 1 << 63
    mu = sigma = 0.0
    if n >= 1 and M > 0.0:
        mu = math.ldexp(float(S1) / float(n), -s)                            # int -> float rounds to nearest even
    if n >= 2 and M > 0.0:
        S2 = (S2hi << 32) + S2lo
        D = n * S2 - S1 * S1
        assert 0 <= D < 1 << 124
        dhi, dlo = D >> 64, D & ((1 << 64) - 1)
        dd = float(dhi) * 18446744073709551616.0 + float(dlo)
        den = float(n) * float(n - 1)
        sigma = math.ldexp(math.sqrt(dd / den), -s)
    return float(n), mu, sigma, fma(std_ratio, sigma, mu)


def outlier_statistical(means, offsets, std_ratio):
    """(keep bool [n], stat f64 [n_seg,4]): cs_outlier_statistical on the means of cs_knn_mean_dist."""
    means = np.asarray(means, np.float64)
    keep = np.zeros(len(means), bool)
    stat = np.zeros((len(offsets) - 1, 4), np.float64)
    for p, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        n, M, s, q = quantise(means[a:b])
        stat[p] = finish(n, M, s, q, float(std_ratio))
        tau = float(stat[p, 3])
        keep[a:b] = [float(m) > 0.0 and float(m) < tau for m in means[a:b]]
    return keep, stat


def radius_count(xyz, offsets, radius):
    """int32 [n]: the rows of the row's segment, itself included, with d2 < radius * radius."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    r2 = float(radius) * float(radius)
    out = np.zeros(len(xyz), np.int32)
    for a, b in zip(offsets[:-1], offsets[1:]):
        s64 = xyz[a:b].astype(np.float64)
        for i in range(b - a):
            raw = _approx(s64, i)
            sure = raw < r2 * (1 - 1e-12)
            near = np.nonzero(~sure & (raw <= r2 * (1 + 1e-12)))[0] if math.isfinite(r2) else np.nonzero(np.isfinite(raw))[0]
            c = int(sure.sum()) if math.isfinite(r2) else 0
            for j in near:
                c += d2_exact(s64, i, j) < r2
            out[a + i] = c
    return out


def outlier_radius(xyz, offsets, radius, nb_points):
    """(keep bool [n], count int32 [n]): cs_outlier_radius."""
    count = radius_count(xyz, offsets, radius)
    return count > nb_points, count
