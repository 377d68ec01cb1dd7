"""NumPy / Python restatement of cs_icp_gicp_batch (include/corsair_hip.h), bit for bit.  Pose chain, association, frame
and loop are those of tests/icp_ref.py; the plane frame, the Cholesky sequence, the Cayley rotation and the update are those
of tests/icp_plane_ref.py (imported, as the library shares the code).  This file restates the covariances, the 3 x 3 inverse
by the adjugate, the 30 fixed-point sums and the Mahalanobis rmse.  Every plain Python float operation is one IEEE f64
operation; fma is exact (below)."""
import math

import numpy as np

from tests.icp_plane_ref import MIN_CORR, PAIRS, _cls, plane_frame, update  # noqa: F401
from tests.icp_ref import associate, fix, frame

NSUM = 30
EPS_MIN, EPS_MAX = 2.0 ** -10, 1.0


def fma(a, b, c):
    """tests/icp_ref.py's exact fma without its gcd reductions (four times as fast; the per-pair math here is some sixty
    of them): the exact rational a * b + c over a power-of-two denominator, rounded once by the int / int division, which
    CPython rounds correctly.  tests/test_gicp_cpu.py compares the two."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def weight_exponent(eps):
    """eW: the smallest integer with 1 / (2 eps) <= 2^eW, i.e. 1 <= eps * 2^(eW + 1)."""
    eW = -1
    while math.ldexp(eps, eW + 1) < 1.0:
        eW += 1
    return eW


def gicp_frame(fr, eps):
    """plane_frame with b = 61 - eN - eW (k_icp_frame's eW argument); the clamp stays 2^(61 - eN)."""
    eW = weight_exponent(eps)
    shifted = dict(fr)
    shifted["eN"] = fr["eN"] + eW
    out = plane_frame(shifted)
    out["eN"] = fr["eN"]
    out["eW"] = eW
    return out


def gain(n, ome):
    """(n or 0, g) of C = I - g n n^T."""
    nn = fma(n[2], n[2], fma(n[1], n[1], n[0] * n[0]))
    if not (all(math.isfinite(v) for v in n) and math.isfinite(nn) and nn > 0.0):
        return [0.0, 0.0, 0.0], 0.0
    return list(n), ome / nn


def covariance(n, eps):
    """C(n) as a 3 x 3 list (for the tests of the documented covariances; the sums use it through weight_of)."""
    n, g = gain([float(v) for v in n], 1.0 - eps)
    a = [g * v for v in n]
    return [[fma(-a[i], n[j], 1.0 if i == j else 0.0) if i == j else -(a[i] * n[j]) for j in range(3)] for i in range(3)]


def cross(p, v):
    return [fma(p[1], v[2], -(p[2] * v[1])), fma(p[2], v[0], -(p[0] * v[2])), fma(p[0], v[1], -(p[1] * v[0]))]


def weight_of(nt, m, ome):
    """W = (C(nt) + C(m))^-1, symmetric 3 x 3 list, by the header's adjugate sequence."""
    nt, gt = gain(nt, ome)
    m, gs = gain(m, ome)
    a = [gt * v for v in nt]
    b = [gs * v for v in m]
    M00 = fma(-b[0], m[0], fma(-a[0], nt[0], 2.0))
    M01 = fma(-b[0], m[1], -(a[0] * nt[1]))
    M02 = fma(-b[0], m[2], -(a[0] * nt[2]))
    M11 = fma(-b[1], m[1], fma(-a[1], nt[1], 2.0))
    M12 = fma(-b[1], m[2], -(a[1] * nt[2]))
    M22 = fma(-b[2], m[2], fma(-a[2], nt[2], 2.0))
    c00 = fma(M11, M22, -(M12 * M12))
    c01 = fma(M02, M12, -(M01 * M22))
    c02 = fma(M01, M12, -(M02 * M11))
    c11 = fma(M00, M22, -(M02 * M02))
    c12 = fma(M01, M02, -(M00 * M12))
    c22 = fma(M00, M11, -(M01 * M01))
    det = fma(M02, c02, fma(M01, c01, M00 * c00))
    with np.errstate(all="ignore"):
        idet = float(np.float64(1.0) / np.float64(det))
    w = [c00 * idet, c01 * idet, c02 * idet, c11 * idet, c12 * idet, c22 * idet]
    return [[w[0], w[1], w[2]], [w[1], w[3], w[4]], [w[2], w[4], w[5]]]


def rotate_normal(T, s):
    x, y, z = float(s[0]), float(s[1]), float(s[2])
    return [fma(T[4 * c], x, fma(T[4 * c + 1], y, T[4 * c + 2] * z)) for c in range(3)]


def terms_of(p_posed, q, nt, m, fr, ome):
    """(the 21 matrix entries, the 6 right-hand sides, mc, W) of one kept pair."""
    o = fr["o"]
    p = [p_posed[c] - o[c] for c in range(3)]
    e = [p_posed[c] - float(q[c]) for c in range(3)]
    W = weight_of([float(v) for v in nt], m, ome)
    u = [fma(W[i][2], e[2], fma(W[i][1], e[1], W[i][0] * e[0])) for i in range(3)]
    K = [[0.0] * 3 for _ in range(3)]
    for j in range(3):
        col = cross(p, [W[0][j], W[1][j], W[2][j]])
        for i in range(3):
            K[i][j] = col[i]
    RR = [cross(p, K[i]) for i in range(3)]
    A = []
    for i, j in PAIRS:
        A.append(RR[i][j] if j < 3 else (K[i][j - 3] if i < 3 else W[i - 3][j - 3]))
    b = cross(p, u) + u
    mc = fma(e[2], u[2], fma(e[1], u[1], e[0] * u[0]))
    return A, b, mc, W


def sums_of(corr, P, D, tgt, tnrm, snrm, T, fr, ome, watch=None):
    """The 30 integer sums over the kept pairs.  watch (a dict): records the largest |scaled term| / clamp seen, the largest
    |sum| and the W of every pair."""
    S = [0] * NSUM
    for i, j in enumerate(corr):
        if j < 0:
            continue
        A, b, mc, W = terms_of(P[i], tgt[j], tnrm[j], rotate_normal(T, snrm[i]), fr, ome)
        S[0] += 1
        scaled = []
        for at, (r, c) in enumerate(PAIRS):
            sc = fr["sc_" + _cls(r, c)]
            S[1 + at] += fix(A[at], sc, fr["clamp"])
            scaled.append(A[at] * sc)
        for a in range(6):
            sc = fr["sc_rd"] if a < 3 else fr["sc_td"]
            S[22 + a] += fix(b[a], sc, fr["clamp"])
            scaled.append(b[a] * sc)
        S[28] += fix(D[i], fr["sc2"], fr["clamp"])
        S[29] += fix(mc, fr["sc_rd"], fr["clamp"])
        scaled += [D[i] * fr["sc2"], mc * fr["sc_rd"]]
        if watch is not None:
            with np.errstate(all="ignore"):
                mx = max(abs(v) if v == v else math.inf for v in scaled) / fr["clamp"]
            watch["term"] = max(watch.get("term", 0.0), mx)
            watch.setdefault("W", []).append(W)
    if watch is not None:
        watch["sum"] = max(watch.get("sum", 0), max(abs(v) for v in S))
    assert all(abs(v) < 2 ** 62 for v in S)
    return S


def icp(src, snrm, tgt, tnrm, T0, max_dist, max_iter=30, relative_fitness=1e-6, relative_rmse=1e-6, epsilon=1e-3,
        watch=None):
    """One problem.  Returns dict(T, T32, fitness, rmse, mrmse, iters, ncorr, corr, sums)."""
    assert math.isfinite(epsilon) and EPS_MIN <= epsilon <= EPS_MAX
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    snrm = np.asarray(snrm, np.float32).reshape(-1, 3)
    tnrm = np.asarray(tnrm, np.float32).reshape(-1, 3)
    assert tnrm.shape == tgt.shape and snrm.shape == src.shape
    T = [float(v) for v in np.asarray(T0, np.float32).reshape(16)]
    fr = gicp_frame(frame(tgt, len(src), max_dist), epsilon)
    ome = 1.0 - epsilon
    thr2 = float(max_dist) * float(max_dist)
    iters, fit, rm, rnd = 0, 0.0, 0.0, 0
    while True:
        corr, P, D = associate(T, src, tgt, thr2)
        S = sums_of(corr, P, D, tgt, tnrm, snrm, T, fr, ome, watch)
        n = S[0]
        pfit, prm = fit, rm
        fit = n / float(len(src)) if len(src) else 0.0
        rm = math.sqrt((float(S[28]) * fr["inv2"]) / float(n)) if n > 0 else 0.0
        sm = float(S[29]) * fr["inv_rd"]
        mrm = math.sqrt(sm / float(n)) if n > 0 and sm > 0.0 else 0.0
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
    return {"T": T64, "T32": T32, "fitness": fit, "rmse": rm, "mrmse": mrm, "iters": iters, "ncorr": int(n), "corr": corr,
            "sums": S}


def icp_batch(src, snrm, soff, tgt, tnrm, toff, src_seg, tgt_seg, T0, max_dist, max_iter=30, relative_fitness=1e-6,
              relative_rmse=1e-6, epsilon=1e-3):
    """The whole call: a list of per-problem results; problems with the same inputs are computed once."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    snrm = np.asarray(snrm, np.float32).reshape(-1, 3)
    tnrm = np.asarray(tnrm, np.float32).reshape(-1, 3)
    T0 = np.asarray(T0, np.float32).reshape(-1, 16)
    out, memo = [], {}
    for p, (ss, ts) in enumerate(zip(src_seg, tgt_seg)):
        key = (ss, ts, T0[p].tobytes())
        if key not in memo:
            memo[key] = icp(src[soff[ss]:soff[ss + 1]], snrm[soff[ss]:soff[ss + 1]], tgt[toff[ts]:toff[ts + 1]],
                            tnrm[toff[ts]:toff[ts + 1]], T0[p], max_dist, max_iter, relative_fitness, relative_rmse, epsilon)
        out.append(memo[key])
    return out


# ---- the lattice fixture of DESIGN 19 (input data of tests/test_gicp_cpu.py and tests/test_gpu_gicp_surfaces.py) -----------
def _patch(u0, u1, v0, v1, h, off, axes, const):
    u, v = np.arange(u0 + off, u1, h), np.arange(v0 + off, v1, h)
    U, V = np.meshgrid(u, v, indexing="ij")
    P = np.zeros((U.size, 3))
    P[:, axes[0]], P[:, axes[1]], P[:, axes[2]] = U.ravel(), V.ravel(), const
    return P


def _patches(h, off, frac):
    return np.concatenate([_patch(-.25, .25 * frac, -.25, .25, h, off, (0, 1, 2), 0.0),      # seat z = 0
                           _patch(-.25, .25, 0, .5 * frac, h, off, (0, 2, 1), .25),           # back y = .25
                           _patch(-.25, .25 * frac, -.3, 0, h, off, (1, 2, 0), -.25)])        # side x = -.25


_LATTICE = {}


def lattice_fixture(deg=3.0, trans=0.01):
    """Three mutually orthogonal plane patches on a 0.02 lattice (the target, 1 625 rows) and the same patches on a lattice
    shifted by half a voxel along both in-plane axes, cut to 70 % along the first axis of each (the source, 1 265 rows: a
    partial scan), moved by the inverse of a rotation of `deg` degrees about (.6, -.5, .62) plus a translation
    trans * (.5, .7, -.5) and narrowed to f32.  Normals: normals_ref.estimate_normals(k = 8) of each cloud in its own frame.
    Returns dict(src, snrm, tgt, tnrm, G): G is the true pose of the source, the start is the identity."""
    key = (deg, trans)
    if key not in _LATTICE:
        from tests import normals_ref

        h = 0.02
        tgt = _patches(h, 0.0, 1.0).astype(np.float32)
        src0 = _patches(h, 0.5 * h, 0.7).astype(np.float32).astype(np.float64)
        ax = np.array([.6, -.5, .62])
        ax /= np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        th = np.radians(deg)
        G = np.eye(4)
        G[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        G[:3, 3] = trans * np.array([.5, .7, -.5])
        Gi = np.linalg.inv(G)
        src = (src0 @ Gi[:3, :3].T + Gi[:3, 3]).astype(np.float32)
        _LATTICE[key] = {"src": src, "snrm": normals_ref.estimate_normals(src, [0, len(src)], 8), "tgt": tgt,
                         "tnrm": normals_ref.estimate_normals(tgt, [0, len(tgt)], 8), "G": G}
    return _LATTICE[key]


def pose_errors(T, G):
    """(RRE in degrees, RTE) of the 4 x 4 estimate T against the true pose G: the rotation angle and the translation norm of
    T G^-1."""
    E = np.asarray(T, np.float64).reshape(4, 4) @ np.linalg.inv(G)
    return (float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))), float(np.linalg.norm(E[:3, 3])))


_LATTICE_RUNS = {}


def lattice_runs():
    """The three restatements on the lattice fixture (max_dist 0.06, T0 = I, criteria 1e-6 / 1e-6, at most 30 updates),
    computed once: dict(point, plane, gicp)."""
    if not _LATTICE_RUNS:
        from tests import icp_plane_ref, icp_ref

        f = lattice_fixture()
        eye = np.eye(4, dtype=np.float32)
        _LATTICE_RUNS["point"] = icp_ref.icp(f["src"], f["tgt"], eye, 0.06, 30)
        _LATTICE_RUNS["plane"] = icp_plane_ref.icp(f["src"], f["tgt"], f["tnrm"], eye, 0.06, 30)
        _LATTICE_RUNS["gicp"] = icp(f["src"], f["snrm"], f["tgt"], f["tnrm"], eye, 0.06, 30, epsilon=1e-3)
    return _LATTICE_RUNS
