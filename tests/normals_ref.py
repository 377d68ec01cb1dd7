"""NumPy / Python restatement of cs_estimate_normals (include/corsair_hip.h), bit for bit: the neighbours by (canonical
distance, row), the scatter matrix about the query row summed in neighbour order, the fixed-sweep cyclic Jacobi of
corsair_amd/csrc/horn.h (jacobi3), the selection, normalisation and sign rules.

Every plain Python float operation is one IEEE f64 operation; fma is the exact form of tests/icp_ref.py.  As there, the
exact distance chain only runs on the rows that can be among the m nearest: an unfused vectorised chain d~ ranks all rows
first, and both chains are within 4 * 2^-53 relative of the true sum of the same three squares, so a row outside
d~ <= (m-th smallest d~) * (1 + 1e-12) cannot enter or tie the list.
"""
import math

import numpy as np

from tests.icp_ref import fma

K_MIN, K_MAX, SWEEPS = 3, 32, 5


def neighbours(seg, i, k):
    """Rows of `seg` (f32 [n,3]) nearest to row i: the min(k, n) smallest (d2, row) with finite d2, ascending."""
    n = len(seg)
    m = min(k, n)
    s64 = seg.astype(np.float64)
    x = s64[i]
    with np.errstate(all="ignore"):
        dx, dy, dz = s64[:, 0] - x[0], s64[:, 1] - x[1], s64[:, 2] - x[2]
        approx = dx * dx + dy * dy + dz * dz
    approx = np.where(np.isfinite(approx), approx, np.inf)
    kth = np.partition(approx, m - 1)[m - 1]
    cand = np.nonzero(approx <= kth * (1 + 1e-12))[0] if math.isfinite(kth) else np.nonzero(np.isfinite(approx))[0]
    out = []
    for j in cand:
        ux, uy, uz = float(s64[j, 0]) - float(x[0]), float(s64[j, 1]) - float(x[1]), float(s64[j, 2]) - float(x[2])
        d = fma(uz, uz, fma(uy, uy, ux * ux))
        if math.isfinite(d):
            out.append((d, int(j)))
    out.sort()
    return out[:m]


def scatter(seg, i, nbr):
    """S (3x3 list, symmetric) about row i over the neighbour rows in the given order."""
    x = [float(v) for v in seg[i]]
    s = [0.0, 0.0, 0.0]
    C = [[0.0] * 3 for _ in range(3)]
    for j in nbr:
        u = [float(seg[j][c]) - x[c] for c in range(3)]
        for a in range(3):
            s[a] = s[a] + u[a]
        for a in range(3):
            for b in range(a, 3):
                C[a][b] = fma(u[a], u[b], C[a][b])
    m = float(len(nbr))
    S = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            S[a][b] = fma(-(s[a] / m), s[b], C[a][b])
            S[b][a] = S[a][b]
    return S


def jacobi3(a, sweeps=SWEEPS):
    """Cyclic Jacobi on the symmetric 3x3 `a` (list of lists, modified); returns the eigenvector matrix (columns)."""
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(sweeps):
        for p in range(2):
            for q in range(p + 1, 3):
                r = 3 - p - q
                apq = a[p][q]
                if apq != 0.0:
                    h = 0.5 * (a[q][q] - a[p][p])
                    den = abs(h) + math.sqrt(h * h + apq * apq)
                    sg = 1.0 if (h == 0.0 or ((h > 0.0) == (apq > 0.0))) else -1.0
                    t = sg * abs(apq) / den if den > 0.0 else sg
                    c = 1.0 / math.sqrt(t * t + 1.0)
                    s = t * c
                    a[p][p] = a[p][p] - t * apq
                    a[q][q] = a[q][q] + t * apq
                    a[p][q] = 0.0
                    a[q][p] = 0.0
                    arp, arq = a[r][p], a[r][q]
                    nrp = c * arp - s * arq
                    nrq = s * arp + c * arq
                    a[r][p] = nrp
                    a[p][r] = nrp
                    a[r][q] = nrq
                    a[q][r] = nrq
                    for i in range(3):
                        vip, viq = v[i][p], v[i][q]
                        v[i][p] = c * vip - s * viq
                        v[i][q] = s * vip + c * viq
    return v


def normal_of(S, sweeps=SWEEPS):
    """The unit normal (3 floats, f64) of scatter matrix S by the selection, normalisation and sign rules."""
    a = [row[:] for row in S]
    if not all(math.isfinite(x) for row in a for x in row):
        return [0.0, 0.0, 1.0]
    v = jacobi3(a, sweeps)
    best, col = a[0][0], 0
    for c in (1, 2):
        if a[c][c] < best:
            best, col = a[c][c], c
    n = [v[0][col], v[1][col], v[2][col]]
    ln = math.sqrt(fma(n[2], n[2], fma(n[1], n[1], n[0] * n[0])))
    if not (math.isfinite(ln) and ln > 0.0):
        return [0.0, 0.0, 1.0]
    n = [n[0] / ln, n[1] / ln, n[2] / ln]
    big, at = abs(n[0]), 0
    for c in (1, 2):
        if abs(n[c]) > big:
            big, at = abs(n[c]), c
    if n[at] < 0.0:
        n = [-n[0], -n[1], -n[2]]
    if not all(math.isfinite(x) for x in n):
        return [0.0, 0.0, 1.0]
    return n


def estimate_normals(xyz, offsets, k):
    """The whole call: f32 [n,3]."""
    assert K_MIN <= k <= K_MAX
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros((len(xyz), 3), np.float32)
    for s in range(len(offsets) - 1):
        seg = xyz[offsets[s]:offsets[s + 1]]
        for i in range(len(seg)):
            nbr = neighbours(seg, i, k) if len(seg) else []
            if len(nbr) < 3:
                out[offsets[s] + i] = (0.0, 0.0, 1.0)
                continue
            out[offsets[s] + i] = np.asarray(normal_of(scatter(seg, i, [j for _, j in nbr])), np.float64).astype(np.float32)
    return out
