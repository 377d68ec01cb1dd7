"""NumPy / Python restatement of cs_icp_plane_batch (include/corsair_hip.h), bit for bit.  Pose chain, association, frame
and loop are those of tests/icp_ref.py (imported, as the library shares the code); this file restates the 29 fixed-point
sums, the unpivoted Cholesky solve as its fixed operation sequence, the Cayley rotation and the stop rules.  Every plain
Python float operation is one IEEE f64 operation; fma is the exact form of tests/icp_ref.py."""
import math

import numpy as np

from tests.icp_ref import associate, fix, fma, frame, pose  # noqa: F401  (pose: re-exported for the tests)

NSUM = 29
PIVOT_MIN = 2.0 ** -30
MIN_CORR = 6
# (i, j) of the 21 products in sum order, and the class of every sum
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]


def plane_frame(fr):
    """The five scales of the plane sums from icp_ref.frame's eM / eN (k_icp_frame)."""
    b, eM = 61 - fr["eN"], fr["eM"]
    e = {"rr": b - 2 * eM - 3, "rt": b - eM - 2, "tt": b - 1, "rd": b - 2 * eM - 2, "td": b - eM - 1}
    out = dict(fr)
    for k, v in e.items():
        out["sc_" + k] = math.ldexp(1.0, v)
        out["inv_" + k] = math.ldexp(1.0, -v)
        out["s_" + k] = v
    return out


def _cls(i, j):
    return "rr" if j < 3 else ("rt" if i < 3 else "tt")


def terms_of(p_posed, q, nrm, fr):
    """(J [6], r) of one kept pair: p_posed f64 [3] (unprimed), q the f32 target row, nrm its f32 normal row."""
    o = fr["o"]
    p = [p_posed[c] - o[c] for c in range(3)]
    n = [float(nrm[c]) for c in range(3)]
    e = [p_posed[c] - float(q[c]) for c in range(3)]
    r = fma(e[2], n[2], fma(e[1], n[1], e[0] * n[0]))
    J = [fma(p[1], n[2], -(p[2] * n[1])), fma(p[2], n[0], -(p[0] * n[2])), fma(p[0], n[1], -(p[1] * n[0]))] + n
    return J, r


def sums_of(corr, P, D, tgt, nrm, fr, watch=None):
    """The 29 integer sums over the kept pairs.  watch (a dict): records the largest |scaled term| / clamp seen."""
    S = [0] * NSUM
    for i, j in enumerate(corr):
        if j < 0:
            continue
        J, r = terms_of(P[i], tgt[j], nrm[j], fr)
        S[0] += 1
        scaled = []
        for at, (a, b) in enumerate(PAIRS):
            sc = fr["sc_" + _cls(a, b)]
            S[1 + at] += fix(J[a] * J[b], sc, fr["clamp"])
            scaled.append((J[a] * J[b]) * sc)
        for a in range(6):
            sc = fr["sc_rd"] if a < 3 else fr["sc_td"]
            S[22 + a] += fix(J[a] * r, sc, fr["clamp"])
            scaled.append((J[a] * r) * sc)
        S[28] += fix(D[i], fr["sc2"], fr["clamp"])
        scaled.append(D[i] * fr["sc2"])
        if watch is not None:
            with np.errstate(all="ignore"):
                m = max(abs(v) if v == v else math.inf for v in scaled) / fr["clamp"]
            watch["term"] = max(watch.get("term", 0.0), m)
    if watch is not None:
        watch["sum"] = max(watch.get("sum", 0), max(abs(v) for v in S))
    assert all(abs(v) < 2 ** 62 for v in S)
    return S


def normal_equations(S, fr):
    A = [[0.0] * 6 for _ in range(6)]
    for at, (i, j) in enumerate(PAIRS):
        A[i][j] = float(S[1 + at]) * fr["inv_" + _cls(i, j)]
        A[j][i] = A[i][j]
    b = [float(S[22 + i]) * (fr["inv_rd"] if i < 3 else fr["inv_td"]) for i in range(6)]
    return A, b


def cholesky_solve(A, b):
    """x of A x = -b by the library's operation sequence; None when a pivot is not finite or not above PIVOT_MIN * A_jj."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = fma(-L[j][k], L[j][k], d)
        if not (math.isfinite(d) and d > PIVOT_MIN * A[j][j]):
            return None
        ljj = math.sqrt(d)
        L[j][j] = ljj
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = fma(-L[i][k], L[j][k], v)
            L[i][j] = v / ljj
    y = [0.0] * 6
    for i in range(6):
        v = -b[i]
        for k in range(i):
            v = fma(-L[i][k], y[k], v)
        y[i] = v / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = fma(-L[k][i], x[k], v)
        x[i] = v / L[i][i]
    return x


def cayley(x0, x1, x2):
    """R of the quaternion (1, x0 / 2, x1 / 2, x2 / 2), normalised by division (cs_ransac_batch's matrix)."""
    qw, qx, qy, qz = 1.0, 0.5 * x0, 0.5 * x1, 0.5 * x2
    qn = math.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    qw, qx, qy, qz = qw / qn, qx / qn, qy / qn, qz / qn
    return [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
            [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
            [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]]


def compose(R, t, T):
    Tn = list(T)
    for a in range(3):
        for b in range(3):
            Tn[4 * a + b] = fma(R[a][0], T[b], fma(R[a][1], T[4 + b], R[a][2] * T[8 + b]))
        Tn[4 * a + 3] = fma(R[a][0], T[3], fma(R[a][1], T[7], fma(R[a][2], T[11], t[a])))
    return Tn


def update(T, S, fr):
    """T <- U T from the integer sums; None when the problem stops (pivot rule, non-finite result)."""
    A, b = normal_equations(S, fr)
    x = cholesky_solve(A, b)
    if x is None or not all(math.isfinite(v) for v in x):
        return None
    o = fr["o"]
    R = cayley(x[0], x[1], x[2])
    t = [(x[3 + a] + o[a]) - fma(R[a][2], o[2], fma(R[a][1], o[1], R[a][0] * o[0])) for a in range(3)]
    Tn = compose(R, t, T)
    if not all(math.isfinite(v) for v in Tn[:12]):
        return None
    return Tn


def icp(src, tgt, nrm, T0, max_dist, max_iter=30, relative_fitness=1e-6, relative_rmse=1e-6, watch=None):
    """One problem.  Returns dict(T f64 [16], T32 f32 [16], fitness, rmse, iters, ncorr, corr int32 [n_src], sums)."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
    assert nrm.shape == tgt.shape
    T = [float(v) for v in np.asarray(T0, np.float32).reshape(16)]
    fr = plane_frame(frame(tgt, len(src), max_dist))
    thr2 = float(max_dist) * float(max_dist)
    iters, fit, rm, rnd = 0, 0.0, 0.0, 0
    while True:
        corr, P, D = associate(T, src, tgt, thr2)
        S = sums_of(corr, P, D, tgt, nrm, fr, watch)
        n = S[0]
        pfit, prm = fit, rm
        fit = n / float(len(src)) if len(src) else 0.0
        rm = math.sqrt((float(S[28]) * fr["inv2"]) / float(n)) if n > 0 else 0.0
        stop = rnd == max_iter
        if rnd > 0 and abs(fit - pfit) < relative_fitness and abs(rm - prm) < relative_rmse:
            stop = True
        if n < MIN_CORR or not math.isfinite(fit) or not math.isfinite(rm):
            stop = True
        if not stop:
            Tn = update(T, S, fr)
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


def icp_batch(src, soff, tgt, nrm, toff, src_seg, tgt_seg, T0, max_dist, max_iter=30, relative_fitness=1e-6,
              relative_rmse=1e-6):
    """The whole call: a list of per-problem results; problems with the same inputs are computed once."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
    T0 = np.asarray(T0, np.float32).reshape(-1, 16)
    out, memo = [], {}
    for p, (ss, ts) in enumerate(zip(src_seg, tgt_seg)):
        key = (ss, ts, T0[p].tobytes())
        if key not in memo:
            memo[key] = icp(src[soff[ss]:soff[ss + 1]], tgt[toff[ts]:toff[ts + 1]], nrm[toff[ts]:toff[ts + 1]], T0[p],
                            max_dist, max_iter, relative_fitness, relative_rmse)
        out.append(memo[key])
    return out
