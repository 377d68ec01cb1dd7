"""NumPy / Python restatement of cs_orient_normals and cs_fpfh (include/corsair_hip.h), bit for bit.

Everything the header writes as single f64 operations is a NumPy f64 operation here, in the same order (NumPy's + - * /
sqrt floor are correctly rounded and never contracted).  The fused operations:
  * the distance chain d2 = fma(dz, dz, fma(dy, dy, dx * dx)) -- as in tests/normals_hybrid_ref.py the exact chain only
    runs on the rows that can be in the list (an unfused vectorised chain ranks all rows first; both chains are within
    4 * 2^-53 relative of the true sum of the same three squares).  The fused steps are exact_fma below: Dekker's product
    a * b = p + e exactly, then math.fsum((p, e, c)), which rounds the exact sum once -- tests.icp_ref.fma (rationals)
    wherever the product could leave Dekker's range, and test_fpfh_cpu.py holds the two against each other;
  * the angle boundaries t_m = fma(c_m, y, -(s_m * x)): only the sign is used, decided by the same exact sum;
  * cs_orient_normals' s: tests.icp_ref.fma.
The boundary directions are read from corsair_amd/csrc/fpfh_bounds.h, the table the kernel compiles.
"""
import math
import os
import re

import numpy as np

from tests.icp_ref import fma

MAX_NN_MIN, MAX_NN_MAX, BINS = 4, 128, 33
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "corsair_amd", "csrc", "fpfh_bounds.h")


def bounds():
    """[(cos theta_m, sin theta_m)] for m = 1..10, from the generated header."""
    with open(_HEADER) as f:
        text = f.read()
    pairs = re.findall(r"\{(-?0x[0-9a-f.]+p[-+]?\d+), (-?0x[0-9a-f.]+p[-+]?\d+)\}", text)
    assert len(pairs) == 10
    return [(float.fromhex(c), float.fromhex(s)) for c, s in pairs]


BOUNDS = bounds()
_SPLIT = 134217729.0   # 2^27 + 1


def _two_prod(a, b):
    """a * b = p + e exactly (Veltkamp / Dekker), for |a * b| well inside the normal range."""
    p = a * b
    ta = _SPLIT * a
    ah = ta - (ta - a)
    al = a - ah
    tb = _SPLIT * b
    bh = tb - (tb - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_fma(a, b, c):
    a, b, c = float(a), float(b), float(c)
    p = a * b
    if not (math.isfinite(p) and math.isfinite(c)) or not (p == 0.0 or 1e-250 < abs(p) < 1e250) or \
            abs(a) > 1e150 or abs(b) > 1e150:
        return fma(a, b, c)
    if p == 0.0:
        return p + c
    p, e = _two_prod(a, b)
    return math.fsum((p, e, c))


def neighbours(seg, i, radius, max_nn):
    """Rows j != i of `seg` (f32 [n,3]) with d2 < radius^2, the max_nn - 1 smallest by (d2, j): [(d2, j)] ascending."""
    r2 = float(radius) * float(radius)
    keep = max_nn - 1
    s64 = seg.astype(np.float64)
    x = s64[i]
    with np.errstate(all="ignore"):
        dx, dy, dz = s64[:, 0] - x[0], s64[:, 1] - x[1], s64[:, 2] - x[2]
        approx = dx * dx + dy * dy + dz * dz
    approx = np.where(np.isfinite(approx), approx, np.inf)
    approx[i] = np.inf
    lim = r2
    if len(seg) > keep:
        lim = min(lim, float(np.partition(approx, keep - 1)[keep - 1]))
    cand = np.nonzero(approx <= lim * (1 + 1e-12))[0]
    out = []
    for j in cand:
        ux, uy, uz = float(dx[j]), float(dy[j]), float(dz[j])
        d = exact_fma(uz, uz, exact_fma(uy, uy, ux * ux))
        if math.isfinite(d) and d < r2:
            out.append((d, int(j)))
    out.sort()
    return out[:keep]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _bin11(f):
    t = np.floor((11.0 * (f + 1.0)) * 0.5)
    return np.clip(t, 0.0, 10.0).astype(np.int64)


def _bin_angle(x, y):
    """The header's rule on arrays of finite x, y."""
    out = np.zeros(len(x), np.int64)
    lower = y < 0.0
    out[~lower] = 5
    for m in range(10):
        c, s = BOUNDS[m]
        q = s * x
        p, e = _two_prod(np.full_like(y, c), y)
        t = (p - q) + e
        ge = t >= 0.0
        # the sign of the exact c * y - q where the float estimate is too close to call
        close = np.abs(t) <= 1e-13 * (np.abs(p) + np.abs(q))
        for k in np.nonzero(close)[0]:
            if abs(float(p[k])) < 1e-250:
                ge[k] = fma(c, float(y[k]), -float(q[k])) >= 0.0
            else:
                ge[k] = math.fsum((float(p[k]), float(e[k]), -float(q[k]))) >= 0.0
        out += (ge & (lower if m < 5 else ~lower)).astype(np.int64)
    out[(x == 0.0) & (y == 0.0)] = 5
    return out


def pair_bins(pi, ni, pj, nj, d2):
    """Bins (b0, b1, b2) of the pairs (i, j): arrays [P,3] of f64 rows and normals, d2 [P] the canonical distances."""
    with np.errstate(all="ignore"):
        dp = [pj[:, c] - pi[:, c] for c in range(3)]
        ni = [ni[:, c] for c in range(3)]
        nj = [nj[:, c] for c in range(3)]
        ln = np.sqrt(d2)
        a1 = _dot(ni, dp) / ln
        a2 = _dot(nj, dp) / ln
        sw = np.abs(a1) < np.abs(a2)
        n1 = [np.where(sw, nj[c], ni[c]) for c in range(3)]
        n2 = [np.where(sw, ni[c], nj[c]) for c in range(3)]
        dp = [np.where(sw, -dp[c], dp[c]) for c in range(3)]
        f2 = np.where(sw, -a2, a1)
        v = _cross(dp, n1)
        vl = np.sqrt(_dot(v, v))
        v = [v[c] / vl for c in range(3)]
        w = _cross(n1, v)
        f1 = _dot(v, n2)
        x = _dot(n1, n2)
        y = _dot(w, n2)
        good = (ln > 0.0) & (vl > 0.0) & np.isfinite(vl) & np.isfinite(f1) & np.isfinite(f2) & np.isfinite(x) & np.isfinite(y)
        z = np.zeros_like(x)
        b0 = np.where(good, _bin_angle(np.where(good, x, z), np.where(good, y, z)), 5)
        b1 = np.where(good, _bin11(np.where(good, f1, z)), 5)
        b2 = np.where(good, _bin11(np.where(good, f2, z)), 5)
    return b0, b1, b2


def spfh_counts(seg, nrm, lists):
    """Integer SPFH counts [n,33] and neighbour counts [n] of one segment from its neighbour lists."""
    n = len(seg)
    I = np.asarray([i for i in range(n) for _ in lists[i]], np.int64)
    J = np.asarray([j for i in range(n) for _, j in lists[i]], np.int64)
    D = np.asarray([d for i in range(n) for d, _ in lists[i]], np.float64)
    counts = np.zeros((n, BINS), np.int64)
    m = np.asarray([len(l) for l in lists], np.int64)
    if len(I):
        p64, n64 = seg.astype(np.float64), nrm.astype(np.float64)
        b0, b1, b2 = pair_bins(p64[I], n64[I], p64[J], n64[J], D)
        np.add.at(counts, (I, b0), 1)
        np.add.at(counts, (I, 11 + b1), 1)
        np.add.at(counts, (I, 22 + b2), 1)
    return counts, m


def fpfh_segment(seg, nrm, radius, max_nn, lists=None, cast=True):
    """f32 [n,33] of one segment (f32 rows and normals); cast=False: the f64 values before the one cast."""
    n = len(seg)
    if lists is None:
        lists = [neighbours(seg, i, radius, max_nn) for i in range(n)]
    counts, m = spfh_counts(seg, nrm, lists)
    with np.errstate(all="ignore"):
        spfh = np.where(m[:, None] > 0, counts.astype(np.float64) * (100.0 / np.maximum(m, 1).astype(np.float64))[:, None],
                        0.0)
        keep = max(max_nn - 1, 1)
        Jp = np.zeros((n, keep), np.int64)
        Dp = np.zeros((n, keep), np.float64)     # 0 = skipped: padding and true d2 == 0 alike
        for i, l in enumerate(lists):
            for t, (d, j) in enumerate(l):
                Jp[i, t], Dp[i, t] = j, d
        acc = np.zeros((n, BINS))
        sums = np.zeros((n, 3))
        for t in range(keep):
            d2 = Dp[:, t]
            on = d2 != 0.0
            if not on.any():
                continue
            val = spfh[Jp[:, t]] / np.where(on, d2, 1.0)[:, None]
            acc = np.where(on[:, None], acc + val, acc)
            for g in range(3):
                sg = sums[:, g]
                for k in range(11):
                    sg = sg + val[:, 11 * g + k]
                sums[:, g] = np.where(on, sg, sums[:, g])
        sb = np.repeat(sums, 11, axis=1)
        out = np.where(sb != 0.0, acc * (100.0 / sb), acc)
        out = out + spfh
        return out.astype(np.float32) if cast else out


def fpfh(xyz, normals, offsets, radius, max_nn):
    """The whole call: f32 [n,33]."""
    assert MAX_NN_MIN <= max_nn <= MAX_NN_MAX and math.isfinite(radius) and radius > 0
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    out = np.zeros((len(xyz), BINS), np.float32)
    for s in range(len(offsets) - 1):
        a, b = offsets[s], offsets[s + 1]
        if b > a:
            out[a:b] = fpfh_segment(xyz[a:b], normals[a:b], radius, max_nn)
    return out


OR_SCALE, OR_LIMIT = 65536.0, 32768.0


def centroid(seg):
    """cs_orient_normals' centroid of a segment (f32 [n,3]): (x, y, z) f64, or None when no row qualifies."""
    seg = np.asarray(seg, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ok = (np.abs(seg) < np.float32(OR_LIMIT)).all(axis=1)
    rows = seg[ok].astype(np.float64)
    if not len(rows):
        return None
    q = np.rint(rows * OR_SCALE).astype(np.int64)
    S = [int(v) for v in q.sum(axis=0)]             # Python integers: exact
    dc = float(len(rows))
    return [(float(S[c]) / dc) * (1.0 / OR_SCALE) for c in range(3)]


def orient_normals(xyz, offsets, normals, view=None, away=True):
    """The whole call: a new f32 [n,3]."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.array(normals, np.float32).reshape(-1, 3)
    for s in range(len(offsets) - 1):
        a, b = offsets[s], offsets[s + 1]
        v = centroid(xyz[a:b]) if view is None else [float(t) for t in np.asarray(view, np.float64)[s]]
        if v is None:
            continue
        for r in range(a, b):
            d = [float(xyz[r, c]) - v[c] for c in range(3)]
            nx, ny, nz = (float(out[r, c]) for c in range(3))
            sdot = fma(nz, d[2], fma(ny, d[1], nx * d[0]))
            if (sdot < 0.0) if away else (sdot > 0.0):
                out[r] = -out[r]
    return out
