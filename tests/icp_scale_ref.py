"""NumPy / Python restatement of cs_icp_scale_batch (include/corsair_hip.h), bit for bit.  Pose chain, association, frame,
Horn's solver, the Cayley rotation, the composition and the plane terms are those of tests/icp_ref.py and
tests/icp_plane_ref.py (imported, as the library shares the code); this file restates the 18 and 37 fixed-point sums, the
scale step of both estimations, the 7x7 Cholesky sequence, the scale bookkeeping and its stop rules.  Every plain Python
float operation is one IEEE f64 operation; fma is the exact form of tests/icp_ref.py.

icp(..., with_scaling=False) runs the two rigid estimations through THIS file's loop and sums (the plane system with six
columns, the point sums without the 18th), which is how tests/test_icp_scale_cpu.py shows that the shared parts are the
shared parts: it must return the bits of icp_ref.icp / icp_plane_ref.icp."""
import math

import numpy as np

from tests import icp_ref
from tests.icp_plane_ref import PIVOT_MIN, cayley, compose, plane_frame, terms_of
from tests.icp_ref import associate, fix, fma, frame, rotation_of

NSUM_POINT, NSUM_PLANE = 18, 37


def is_rot(i):
    """A rotational column of the plane Jacobian (bounded by 2 M): a_x, a_y, a_z and p'.n."""
    return i < 3 or i == 6


def cls(i, j):
    ri, rj = is_rot(i), is_rot(j)
    return "rr" if ri and rj else ("rt" if ri or rj else "tt")


def scale_frame(fr):
    """icp_plane_ref.plane_frame plus the scale of the 18th point sum, 2^(s2 - 2)."""
    out = plane_frame(fr)
    out["s_pp"] = fr["s2"] - 2
    out["sc_pp"] = math.ldexp(1.0, out["s_pp"])
    out["inv_pp"] = math.ldexp(1.0, -out["s_pp"])
    return out


def _watch(watch, scaled, S, fr):
    if watch is None:
        return
    with np.errstate(all="ignore"):
        m = max(abs(v) if v == v else math.inf for v in scaled) / fr["clamp"] if scaled else 0.0
    watch["term"] = max(watch.get("term", 0.0), m)
    watch["sum"] = max(watch.get("sum", 0), max(abs(v) for v in S))


def point_sums(corr, P, D, tgt, fr, scaling=True, watch=None):
    """The 17 sums of cs_icp_batch and, with scaling, I(p'.p' * 2^(s2 - 2))."""
    S = icp_ref.sums_of(corr, P, D, tgt, fr)
    scaled = []
    if scaling:
        o, spp = fr["o"], 0
        for i, j in enumerate(corr):
            if j < 0:
                continue
            p = [P[i][c] - o[c] for c in range(3)]
            pp = fma(p[2], p[2], fma(p[1], p[1], p[0] * p[0]))
            spp += fix(pp, fr["sc_pp"], fr["clamp"])
            scaled.append(pp * fr["sc_pp"])
        S = S + [spp]
    _watch(watch, scaled, S, fr)
    assert all(abs(v) < 2 ** 62 for v in S)
    return S


def plane_sums(corr, P, D, tgt, nrm, fr, nj=7, watch=None):
    """count, the nj (nj + 1) / 2 products J_i J_j (i <= j, row-major), the nj products J_i r, d2."""
    pairs = [(i, j) for i in range(nj) for j in range(i, nj)]
    njj = len(pairs)
    S = [0] * (1 + njj + nj + 1)
    scaled = []
    o = fr["o"]
    for i, j in enumerate(corr):
        if j < 0:
            continue
        J, r = terms_of(P[i], tgt[j], nrm[j], fr)
        if nj == 7:
            p = [P[i][c] - o[c] for c in range(3)]
            n = J[3:6]
            J = J + [fma(p[2], n[2], fma(p[1], n[1], p[0] * n[0]))]
        S[0] += 1
        for at, (a, b) in enumerate(pairs):
            sc = fr["sc_" + cls(a, b)]
            S[1 + at] += fix(J[a] * J[b], sc, fr["clamp"])
            scaled.append((J[a] * J[b]) * sc)
        for a in range(nj):
            sc = fr["sc_rd"] if is_rot(a) else fr["sc_td"]
            S[1 + njj + a] += fix(J[a] * r, sc, fr["clamp"])
            scaled.append((J[a] * r) * sc)
        S[1 + njj + nj] += fix(D[i], fr["sc2"], fr["clamp"])
        scaled.append(D[i] * fr["sc2"])
    _watch(watch, scaled, S, fr)
    assert all(abs(v) < 2 ** 62 for v in S)
    return S


def normal_equations(S, fr, nj):
    pairs = [(i, j) for i in range(nj) for j in range(i, nj)]
    A = [[0.0] * nj for _ in range(nj)]
    for at, (i, j) in enumerate(pairs):
        A[i][j] = float(S[1 + at]) * fr["inv_" + cls(i, j)]
        A[j][i] = A[i][j]
    b = [float(S[1 + len(pairs) + i]) * (fr["inv_rd"] if is_rot(i) else fr["inv_td"]) for i in range(nj)]
    return A, b


def cholesky_solve(A, b):
    """icp_plane_ref.cholesky_solve for any size: the same operation sequence, the pivot rule on every pivot."""
    n = len(b)
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        d = A[j][j]
        for k in range(j):
            d = fma(-L[j][k], L[j][k], d)
        if not (math.isfinite(d) and d > PIVOT_MIN * A[j][j]):
            return None
        ljj = math.sqrt(d)
        L[j][j] = ljj
        for i in range(j + 1, n):
            v = A[i][j]
            for k in range(j):
                v = fma(-L[i][k], L[j][k], v)
            L[i][j] = v / ljj
    y = [0.0] * n
    for i in range(n):
        v = -b[i]
        for k in range(i):
            v = fma(-L[i][k], y[k], v)
        y[i] = v / L[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v = fma(-L[k][i], x[k], v)
        x[i] = v / L[i][i]
    return x


def scale_ok(su, scale, bounds):
    """(accepted, new accumulated scale): s_u finite and > 0, s_u * scale inside the interval."""
    new = su * scale
    return (math.isfinite(su) and su > 0.0 and bounds[0] <= new <= bounds[1]), new


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def update_point(T, S, fr, scale, bounds, scaling=True):
    """(T', scale') of the point estimation, or None when the problem stops."""
    n = float(S[0])
    o = fr["o"]
    sp = [float(S[1 + c]) * fr["inv1"] for c in range(3)]
    sq = [float(S[4 + c]) * fr["inv1"] for c in range(3)]
    mp = [sp[c] / n for c in range(3)]
    mq = [sq[c] / n for c in range(3)]
    Sm = [[fma(-sp[a], mq[b], float(S[7 + 3 * a + b]) * fr["inv2"]) for b in range(3)] for a in range(3)]
    if scaling:
        den = float(S[17]) * fr["inv_pp"]
        for a in range(3):
            den = fma(-sp[a], mp[a], den)
        if not (math.isfinite(den) and den > 0.0):
            return None
    R = rotation_of(Sm)
    pm = [mp[c] + o[c] for c in range(3)]
    qm = [mq[c] + o[c] for c in range(3)]
    Rp = [fma(R[a][2], pm[2], fma(R[a][1], pm[1], R[a][0] * pm[0])) for a in range(3)]
    if scaling:
        num = R[0][0] * Sm[0][0]
        for k in range(1, 9):
            num = fma(R[k // 3][k % 3], Sm[k // 3][k % 3], num)
        su = _div(num, den)
        ok, scale = scale_ok(su, scale, bounds)
        if not ok:
            return None
        t = [fma(-su, Rp[a], qm[a]) for a in range(3)]
        R = [[su * R[a][b] for b in range(3)] for a in range(3)]
    else:
        t = [qm[a] - Rp[a] for a in range(3)]
    Tn = compose(R, t, T)
    if not all(math.isfinite(v) for v in Tn[:12]):
        return None
    return Tn, scale


def update_plane(T, S, fr, scale, bounds, nj=7):
    """(T', scale') of the plane estimation with nj unknowns, or None when the problem stops."""
    A, b = normal_equations(S, fr, nj)
    x = cholesky_solve(A, b)
    if x is None or not all(math.isfinite(v) for v in x):   # (a non-finite x makes T non-finite: the same stop)
        return None
    o = fr["o"]
    with np.errstate(all="ignore"):
        R = cayley(x[0], x[1], x[2])
    Ro = [fma(R[a][2], o[2], fma(R[a][1], o[1], R[a][0] * o[0])) for a in range(3)]
    if nj == 7:
        su = 1.0 + x[6]
        ok, scale = scale_ok(su, scale, bounds)
        if not ok:
            return None
        t = [fma(-su, Ro[a], x[3 + a] + o[a]) for a in range(3)]
        R = [[su * R[a][b] for b in range(3)] for a in range(3)]
    else:
        t = [(x[3 + a] + o[a]) - Ro[a] for a in range(3)]
    Tn = compose(R, t, T)
    if not all(math.isfinite(v) for v in Tn[:12]):
        return None
    return Tn, scale


def icp(src, tgt, nrm, T0, max_dist, max_iter=30, relative_fitness=1e-6, relative_rmse=1e-6, scale_bounds=(0.5, 2.0),
        with_scaling=True, watch=None):
    """One problem; nrm = None selects the point estimation.  Returns dict(T f64 [16], T32 f32 [16], scale, fitness, rmse,
    iters, ncorr, corr int32 [n_src], sums)."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    plane = nrm is not None
    if plane:
        nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
        assert nrm.shape == tgt.shape
    nj = 7 if with_scaling else 6
    min_corr = nj if plane else 3
    bounds = (float(scale_bounds[0]), float(scale_bounds[1]))
    T = [float(v) for v in np.asarray(T0, np.float32).reshape(16)]
    fr = scale_frame(frame(tgt, len(src), max_dist))
    thr2 = float(max_dist) * float(max_dist)
    iters, fit, rm, rnd, scale = 0, 0.0, 0.0, 0, 1.0
    while True:
        corr, P, D = associate(T, src, tgt, thr2)
        if plane:
            S = plane_sums(corr, P, D, tgt, nrm, fr, nj, watch)
            d2 = S[-1]
        else:
            S = point_sums(corr, P, D, tgt, fr, with_scaling, watch)
            d2 = S[16]
        n = S[0]
        pfit, prm = fit, rm
        fit = n / float(len(src)) if len(src) else 0.0
        rm = math.sqrt((float(d2) * fr["inv2"]) / float(n)) if n > 0 else 0.0
        stop = rnd == max_iter
        if rnd > 0 and abs(fit - pfit) < relative_fitness and abs(rm - prm) < relative_rmse:
            stop = True
        if n < min_corr or not math.isfinite(fit) or not math.isfinite(rm):
            stop = True
        if not stop:
            with np.errstate(all="ignore"):
                new = update_plane(T, S, fr, scale, bounds, nj) if plane else \
                    update_point(T, S, fr, scale, bounds, with_scaling)
            if new is None:
                stop = True
            else:
                T, scale = new
                iters += 1
        if stop:
            break
        rnd += 1
    T64 = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        T32 = T64.astype(np.float32)
    return {"T": T64, "T32": T32, "scale": scale, "fitness": fit, "rmse": rm, "iters": iters, "ncorr": int(n), "corr": corr,
            "sums": S}


def icp_batch(src, soff, tgt, nrm, toff, src_seg, tgt_seg, T0, max_dist, max_iter=30, relative_fitness=1e-6,
              relative_rmse=1e-6, scale_bounds=(0.5, 2.0), with_scaling=True):
    """The whole call: a list of per-problem results; problems with the same inputs are computed once."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    if nrm is not None:
        nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
    T0 = np.asarray(T0, np.float32).reshape(-1, 16)
    out, memo = [], {}
    for p, (ss, ts) in enumerate(zip(src_seg, tgt_seg)):
        key = (ss, ts, T0[p].tobytes())
        if key not in memo:
            memo[key] = icp(src[soff[ss]:soff[ss + 1]], tgt[toff[ts]:toff[ts + 1]],
                            None if nrm is None else nrm[toff[ts]:toff[ts + 1]], T0[p], max_dist, max_iter,
                            relative_fitness, relative_rmse, scale_bounds, with_scaling)
        out.append(memo[key])
    return out
