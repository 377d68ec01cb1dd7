"""NumPy / Python restatement of cs_icp_batch (include/corsair_hip.h), bit for bit: the pose and distance fma chains, the
association with ties to the smaller row, the 17 fixed-point sums as Python ints, the Horn solve with its fallback (the
operation sequence of corsair_amd/csrc/horn.h) and the stop rule.

Every plain Python float operation is one IEEE f64 operation, which is what the library's kernels execute (they are built
without contraction); fma is the exact rational form of tests/hardest_ref.py.  The exact chain only runs on the rows that
can win: a vectorised unfused chain d~ ranks all rows first.  Both chains sum three non-negative terms of the SAME
differences, so each is within 4 * 2^-53 relative of the true sum and a row whose fma chain is minimal has d~ within 1e-15
relative of the smallest d~; every row with d~ <= min d~ * (1 + 1e-12) gets the exact chain, the rest cannot win or tie.
"""
import math
from fractions import Fraction

import numpy as np

EM_MIN, EM_MAX, SUM_BITS = -100, 400, 61


def fma(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def pose(T, s):
    """p_c = fma(T_c0, x, fma(T_c1, y, fma(T_c2, z, T_c3))); T: 16 floats row-major, s: f32 row."""
    x, y, z = float(s[0]), float(s[1]), float(s[2])
    return [fma(T[4 * c], x, fma(T[4 * c + 1], y, fma(T[4 * c + 2], z, T[4 * c + 3]))) for c in range(3)]


def dist2(p, t):
    dx, dy, dz = p[0] - float(t[0]), p[1] - float(t[1]), p[2] - float(t[2])
    return fma(dz, dz, fma(dy, dy, dx * dx))


def frame(tgt, n_src, max_dist):
    """Origin and scales of the fixed-point sums of one problem (k_icp_frame)."""
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    o = [0.0, 0.0, 0.0]
    h = 0.0
    if len(tgt):
        with np.errstate(all="ignore"):
            lo = [float(np.fmin.reduce(tgt[:, c])) for c in range(3)]     # fminf / fmaxf: NaN loses
            hi = [float(np.fmax.reduce(tgt[:, c])) for c in range(3)]
            oo = [0.5 * (lo[c] + hi[c]) for c in range(3)]
            hh = [0.5 * (hi[c] - lo[c]) for c in range(3)]
        if all(math.isfinite(v) for v in oo + hh):
            o, h = oo, max(0.0, hh[0], hh[1], hh[2])
    M = h + float(max_dist)
    eM = math.frexp(M)[1] if math.isfinite(M) else EM_MAX
    eM = min(max(eM, EM_MIN), EM_MAX)
    eN = 0 if n_src <= 1 else (int(n_src) - 1).bit_length()
    s1, s2 = SUM_BITS - eN - eM, SUM_BITS - eN - 2 * eM
    return {"o": o, "sc1": math.ldexp(1.0, s1), "inv1": math.ldexp(1.0, -s1), "sc2": math.ldexp(1.0, s2),
            "inv2": math.ldexp(1.0, -s2), "clamp": math.ldexp(1.0, SUM_BITS - eN), "s1": s1, "s2": s2, "eN": eN, "eM": eM}


def fix(v, scale, clamp):
    x = v * scale
    x = -clamp if x != x else min(max(x, -clamp), clamp)
    return int(x)                                   # truncates toward zero


def associate(T, src, tgt, thr2):
    """Nearest target row of every posed source by (canonical distance, row); returns (corr int32 [-1 = no pair], posed
    points, d2 of every source's nearest row)."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    t64 = tgt.astype(np.float64)
    corr = np.full(len(src), -1, np.int32)
    P, D = [], []
    for i, s in enumerate(src):
        p = pose(T, s)
        P.append(p)
        best = None
        if len(tgt):
            with np.errstate(all="ignore"):
                dx, dy, dz = p[0] - t64[:, 0], p[1] - t64[:, 1], p[2] - t64[:, 2]
                approx = dx * dx + dy * dy + dz * dz
                approx = np.where(np.isnan(approx), np.inf, approx)
                m = approx.min()
            if math.isfinite(m):
                for j in np.nonzero(approx <= m * (1 + 1e-12))[0]:
                    d = dist2(p, tgt[j])
                    if best is None or d < best[0]:        # j ascends: strict < keeps the smaller row
                        best = (d, int(j))
        D.append(best[0] if best else math.inf)
        if best is not None and best[0] < thr2:
            corr[i] = best[1]
    return corr, P, D


def sums_of(corr, P, D, tgt, fr):
    """The 17 integer sums over the kept pairs (any order: Python ints)."""
    S = [0] * 17
    o = fr["o"]
    for i, j in enumerate(corr):
        if j < 0:
            continue
        p = [P[i][c] - o[c] for c in range(3)]
        q = [float(tgt[j][c]) - o[c] for c in range(3)]
        S[0] += 1
        for c in range(3):
            S[1 + c] += fix(p[c], fr["sc1"], fr["clamp"])
            S[4 + c] += fix(q[c], fr["sc1"], fr["clamp"])
        for a in range(3):
            for b in range(3):
                S[7 + 3 * a + b] += fix(p[a] * q[b], fr["sc2"], fr["clamp"])
        S[16] += fix(D[i], fr["sc2"], fr["clamp"])
    assert all(abs(v) < 2 ** 62 for v in S)
    return S


# ---- corsair_amd/csrc/horn.h -----------------------------------------------------------------------------------------
def jacobi4(a):
    """Cyclic Jacobi, 5 sweeps, on the symmetric 4x4 `a` (list of lists, modified); returns the eigenvector matrix."""
    v = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(5):
        for p in range(3):
            for q in range(p + 1, 4):
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
                    for r in range(4):
                        if r != p and r != q:
                            arp, arq = a[r][p], a[r][q]
                            nrp = c * arp - s * arq
                            nrq = s * arp + c * arq
                            a[r][p] = nrp
                            a[p][r] = nrp
                            a[r][q] = nrq
                            a[q][r] = nrq
                    for r in range(4):
                        vrp, vrq = v[r][p], v[r][q]
                        v[r][p] = c * vrp - s * vrq
                        v[r][q] = s * vrp + c * vrq
    return v


def horn_qcp(S, N):
    """Largest eigenvector of Horn's N from the characteristic polynomial; None when the solver declines."""
    f2 = 0.0
    for a in range(3):
        for b in range(3):
            f2 = fma(S[a][b], S[a][b], f2)
    c2 = -2.0 * f2
    detS = (S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) -
            S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0]) +
            S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0]))
    c1 = -8.0 * detS
    u5 = N[0][2] * N[1][3] - N[0][3] * N[1][2]
    w0 = N[2][0] * N[3][1] - N[2][1] * N[3][0]
    u0 = N[0][0] * N[1][1] - N[0][1] * N[1][0]
    u1 = N[0][0] * N[1][2] - N[0][2] * N[1][0]
    u2 = N[0][0] * N[1][3] - N[0][3] * N[1][0]
    u3 = N[0][1] * N[1][2] - N[0][2] * N[1][1]
    u4 = N[0][1] * N[1][3] - N[0][3] * N[1][1]
    w1 = N[2][0] * N[3][2] - N[2][2] * N[3][0]
    w2 = N[2][0] * N[3][3] - N[2][3] * N[3][0]
    w3 = N[2][1] * N[3][2] - N[2][2] * N[3][1]
    w4 = N[2][1] * N[3][3] - N[2][3] * N[3][1]
    w5 = N[2][2] * N[3][3] - N[2][3] * N[3][2]
    c0 = u0 * w5 - u1 * w4 + u2 * w3 + u3 * w2 - u4 * w1 + u5 * w0
    lam = math.sqrt(3.0 * f2)
    conv = False
    it = 0
    while it < 8 and not conv:
        l2 = lam * lam
        P = fma(fma(l2 + c2, lam, c1), lam, c0)
        dP = fma(fma(4.0, l2, 2.0 * c2), lam, c1)
        ddP = fma(12.0, l2, 2.0 * c2)
        den = fma(2.0 * dP, dP, -(P * ddP))
        num = 2.0 * P * dP
        if den == 0.0:
            d = math.nan if (num == 0.0 or num != num) else math.copysign(math.inf, num) * math.copysign(1.0, den)
        else:
            d = num / den
        lam = lam - d
        conv = abs(d) <= 1e-6 * lam
        it += 1
    l2 = lam * lam
    dP = fma(fma(4.0, l2, 2.0 * c2), lam, c1)
    if not (conv and dP >= 0.02 * (l2 * lam)):
        return None
    m00, m11, m22, m33 = N[0][0] - lam, N[1][1] - lam, N[2][2] - lam, N[3][3] - lam
    m01, m02, m03, m12, m13, m23 = N[0][1], N[0][2], N[0][3], N[1][2], N[1][3], N[2][3]
    u0 = m00 * m11 - m01 * m01
    u1 = m00 * m12 - m02 * m01
    u2 = m00 * m13 - m03 * m01
    u3 = m01 * m12 - m02 * m11
    u4 = m01 * m13 - m03 * m11
    w1 = m02 * m23 - m22 * m03
    w2 = m02 * m33 - m23 * m03
    w3 = m12 * m23 - m22 * m13
    w4 = m12 * m33 - m23 * m13
    w5 = m22 * m33 - m23 * m23
    a00 = m11 * w5 - m12 * w4 + m13 * w3
    a01 = -m01 * w5 + m02 * w4 - m03 * w3
    a02 = m13 * u5 - m23 * u4 + m33 * u3
    a03 = -m12 * u5 + m22 * u4 - m23 * u3
    a11 = m00 * w5 - m02 * w2 + m03 * w1
    a12 = -m03 * u5 + m23 * u2 - m33 * u1
    a13 = m02 * u5 - m22 * u2 + m23 * u1
    a22 = m03 * u4 - m13 * u2 + m33 * u0
    a23 = -m02 * u4 + m12 * u2 - m23 * u0
    a33 = m02 * u3 - m12 * u1 + m22 * u0
    best, q = abs(a00), [a00, a01, a02, a03]
    if abs(a11) > best:
        best, q = abs(a11), [a01, a11, a12, a13]
    if abs(a22) > best:
        best, q = abs(a22), [a02, a12, a22, a23]
    if abs(a33) > best:
        best, q = abs(a33), [a03, a13, a23, a33]
    return q if best > 0.0 else None


def horn_matrix(S):
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = S[0][0] + S[1][1] + S[2][2]
    N[0][1] = S[1][2] - S[2][1]
    N[0][2] = S[2][0] - S[0][2]
    N[0][3] = S[0][1] - S[1][0]
    N[1][1] = S[0][0] - S[1][1] - S[2][2]
    N[1][2] = S[0][1] + S[1][0]
    N[1][3] = S[2][0] + S[0][2]
    N[2][2] = -S[0][0] + S[1][1] - S[2][2]
    N[2][3] = S[1][2] + S[2][1]
    N[3][3] = -S[0][0] - S[1][1] + S[2][2]
    for i in range(4):
        for j in range(i):
            N[i][j] = N[j][i]
    return N


def rotation_of(S, force_jacobi=False):
    """R (3x3 list) of the cross-covariance S (source index first), by the RANSAC's solver and selection rules."""
    N = horn_matrix(S)
    q = None if force_jacobi else horn_qcp(S, N)
    if q is None:
        V = jacobi4(N)
        best, q = N[0][0], [V[0][0], V[1][0], V[2][0], V[3][0]]
        for c in range(1, 4):
            if N[c][c] > best:
                best, q = N[c][c], [V[0][c], V[1][c], V[2][c], V[3][c]]
    qw, qx, qy, qz = q
    s = qw * qw + qx * qx + qy * qy + qz * qz
    qn = math.sqrt(s) if s >= 0.0 else math.nan

    def div(a):
        if qn == 0.0 or qn != qn:
            return math.nan
        return a / qn

    qw, qx, qy, qz = div(qw), div(qx), div(qy), div(qz)
    return [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
            [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
            [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]]


def update(T, S, fr, force_jacobi=False):
    """T <- U T from the integer sums; returns the new 16 floats, or None when a value is not finite."""
    n = float(S[0])
    o = fr["o"]
    sp = [float(S[1 + c]) * fr["inv1"] for c in range(3)]
    sq = [float(S[4 + c]) * fr["inv1"] for c in range(3)]
    mp = [sp[c] / n for c in range(3)]
    mq = [sq[c] / n for c in range(3)]
    Sm = [[fma(-sp[a], mq[b], float(S[7 + 3 * a + b]) * fr["inv2"]) for b in range(3)] for a in range(3)]
    R = rotation_of(Sm, force_jacobi)
    pm = [mp[c] + o[c] for c in range(3)]
    qm = [mq[c] + o[c] for c in range(3)]
    Tn = list(T)
    for a in range(3):
        t = qm[a] - fma(R[a][2], pm[2], fma(R[a][1], pm[1], R[a][0] * pm[0]))
        for b in range(3):
            Tn[4 * a + b] = fma(R[a][0], T[b], fma(R[a][1], T[4 + b], R[a][2] * T[8 + b]))
        Tn[4 * a + 3] = fma(R[a][0], T[3], fma(R[a][1], T[7], fma(R[a][2], T[11], t)))
    if not all(math.isfinite(v) for v in Tn[:12]):
        return None
    return Tn


def icp(src, tgt, T0, max_dist, max_iter=30, relative_fitness=1e-6, relative_rmse=1e-6, force_jacobi=False):
    """One problem.  Returns dict(T f64 [16], T32 f32 [16], fitness, rmse, iters, ncorr, corr int32 [n_src], sums)."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    T = [float(v) for v in np.asarray(T0, np.float32).reshape(16)]
    fr = frame(tgt, len(src), max_dist)
    thr2 = float(max_dist) * float(max_dist)
    iters, fit, rm, rnd = 0, 0.0, 0.0, 0
    while True:
        corr, P, D = associate(T, src, tgt, thr2)
        S = sums_of(corr, P, D, tgt, fr)
        n = S[0]
        pfit, prm = fit, rm
        fit = n / float(len(src)) if len(src) else 0.0
        rm = math.sqrt((float(S[16]) * fr["inv2"]) / float(n)) if n > 0 else 0.0
        stop = rnd == max_iter
        if rnd > 0 and abs(fit - pfit) < relative_fitness and abs(rm - prm) < relative_rmse:
            stop = True
        if n < 3 or not math.isfinite(fit) or not math.isfinite(rm):
            stop = True
        if not stop:
            Tn = update(T, S, fr, force_jacobi)
            if Tn is None:
                stop = True
            else:
                T = Tn
                iters += 1
        if stop:
            break
        rnd += 1
    T64 = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        T32 = T64.astype(np.float32)
    return {"T": T64, "T32": T32, "fitness": fit, "rmse": rm, "iters": iters, "ncorr": int(n), "corr": corr, "sums": S}


def icp_batch(src, soff, tgt, toff, src_seg, tgt_seg, T0, max_dist, max_iter=30, relative_fitness=1e-6,
              relative_rmse=1e-6):
    """The whole call: a list of per-problem results; problems with the same inputs are computed once."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    T0 = np.asarray(T0, np.float32).reshape(-1, 16)
    out, memo = [], {}
    for p, (ss, ts) in enumerate(zip(src_seg, tgt_seg)):
        key = (ss, ts, T0[p].tobytes())
        if key not in memo:
            memo[key] = icp(src[soff[ss]:soff[ss + 1]], tgt[toff[ts]:toff[ts + 1]], T0[p], max_dist, max_iter,
                            relative_fitness, relative_rmse)
        out.append(memo[key])
    return out
