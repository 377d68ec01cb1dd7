"""NumPy / Python restatement of cs_fgr_batch (include/corsair_hip.h), bit for bit: the frame, the tuple test with the
RANSAC's counter generator, the line process with its 16 fixed-point sums as Python ints, the Cholesky solve and Cayley
update of the plane ICP (tests/icp_plane_ref.py), the de-normalised result and the RANSAC's evaluation of it.

The per-pair arithmetic of the specification is single unfused f64 operations, which NumPy executes element-wise as
written (it never contracts), so frame, trials and sums are vectorised; the per-problem solve and the evaluation's fma
chains use the exact rational fma of tests/icp_ref.py.
"""
import math

import numpy as np

from tests.icp_plane_ref import cayley, cholesky_solve, compose
from tests.icp_ref import fma

SUM_BITS = 61
MIN_PAIRS = 10
MAX_TUPLE_CAP = 65536
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
_M64 = (1 << 64) - 1


def rng_u64(seed, itr, j):
    """common.h's rng_u64 for an array of iterations (np.uint64 arithmetic wraps mod 2^64)."""
    itr = np.asarray(itr, np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * (itr * np.uint64(64) + np.uint64(j + 1))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def rng_index(seed, itr, j, m):
    """common.h's rng_index: the upper half of the draw times m, shifted down (m < 2^32, so the product fits 64 bits)."""
    return (((rng_u64(seed, itr, j) >> np.uint64(32)) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def frame(src, tgt):
    """(cs, ct, g) of one problem, or None when the frame is degenerate."""
    if len(src) == 0:
        return None
    with np.errstate(all="ignore"):
        lo = [np.fmin.reduce(a[:, c]) for a in (src, tgt) for c in range(3)]      # fminf / fmaxf: NaN loses
        hi = [np.fmax.reduce(a[:, c]) for a in (src, tgt) for c in range(3)]
        if not all(math.isfinite(float(v)) for v in lo + hi):
            return None
        cen = [0.5 * (float(lo[k]) + float(hi[k])) for k in range(6)]
        d2max = 0.0
        for a, c in ((src, cen[:3]), (tgt, cen[3:])):
            d = a.astype(np.float64) - np.asarray(c)
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            if np.isnan(d2).any():
                return None
            d2max = max(d2max, float(d2.max()))
    g = math.sqrt(d2max)
    if not (g > 0.0 and math.isfinite(g)):
        return None
    return np.asarray(cen[:3]), np.asarray(cen[3:]), g


def _len(a, b):
    d = a - b
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def tuple_test(qh, ph, seed, tuple_scale, max_tuple, chunk=4096, trials=None):
    """Pair indices [3 n_tuple] of the first max_tuple passing trials in trial order.  `chunk` only sizes the
    vectorisation: the result does not depend on it.  trials: a list that receives the numbers of the kept trials."""
    m = len(qh)
    n_trial, ts = 100 * m, float(tuple_scale)
    kept = []
    n_kept = 0
    for base in range(0, n_trial, chunk):
        t = np.arange(base, min(base + chunk, n_trial), dtype=np.uint64)
        idx = [rng_index(seed, t, j, m) for j in range(3)]
        ok = np.ones(len(t), bool)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ls, lt = _len(qh[idx[a]], qh[idx[b]]), _len(ph[idx[a]], ph[idx[b]])
            ok &= (ls * ts < lt) & (lt * ts < ls)
        sel = np.nonzero(ok)[0][:max_tuple - n_kept]
        if len(sel):
            kept.append(np.stack([idx[0][sel], idx[1][sel], idx[2][sel]], 1).reshape(-1))
            n_kept += len(sel)
            if trials is not None:
                trials.extend((base + sel).tolist())
        if n_kept >= max_tuple:
            break
    return np.concatenate(kept) if kept else np.zeros(0, np.int64)


def _fix_sum(v, scale, clamp):
    """sum of I(v * scale) as a Python int (np.fmax / fmin: NaN becomes the lower clamp, like the device's fmax)."""
    with np.errstate(all="ignore"):
        x = np.fmin(np.fmax(v * scale, -clamp), clamp)
    return sum(np.trunc(x).astype(np.int64).tolist())


def sums_of(T, mu, qh, ph, eN):
    """The 16 integer sums of one round and their exponents."""
    b = SUM_BITS - eN
    clamp = math.ldexp(1.0, b)
    with np.errstate(all="ignore"):
        q = [((T[4 * c] * qh[:, 0] + T[4 * c + 1] * qh[:, 1]) + T[4 * c + 2] * qh[:, 2]) + T[4 * c + 3] for c in range(3)]
        e = [q[c] - ph[:, c] for c in range(3)]
        r2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        w0 = mu / (r2 + mu)
        w = w0 * w0
        wq = [w * q[c] for c in range(3)]
        x = [q[1] * e[2] - q[2] * e[1], q[2] * e[0] - q[0] * e[2], q[0] * e[1] - q[1] * e[0]]
        terms = [(w, b)] + [(wq[c], b - 2) for c in range(3)]
        terms += [(wq[a] * q[c], b - 4) for a in range(3) for c in range(a, 3)]
        terms += [(w * e[c], b - 3) for c in range(3)] + [(w * x[c], b - 5) for c in range(3)]
    S = [_fix_sum(v, math.ldexp(1.0, s), clamp) for v, s in terms]
    assert all(abs(v) < 2 ** 62 for v in S)
    return S, [s for _, s in terms]


def update(T, S, exps):
    """T^ <- U T^ from the sums; None when the problem stops (pivot rule, non-finite result)."""
    s = [float(S[k]) * math.ldexp(1.0, -exps[k]) for k in range(16)]
    sw, qx, qy, qz = s[0], s[1], s[2], s[3]
    xx, xy, xz, yy, yz, zz = s[4:10]
    A = [[yy + zz, -xy, -xz, 0.0, -qz, qy],
         [0.0, xx + zz, -yz, qz, 0.0, -qx],
         [0.0, 0.0, xx + yy, -qy, qx, 0.0],
         [0.0, 0.0, 0.0, sw, 0.0, 0.0],
         [0.0, 0.0, 0.0, 0.0, sw, 0.0],
         [0.0, 0.0, 0.0, 0.0, 0.0, sw]]
    for i in range(6):
        for j in range(i):
            A[i][j] = A[j][i]
    b = [s[13], s[14], s[15], s[10], s[11], s[12]]
    x = cholesky_solve(A, b)
    if x is None:
        return None
    with np.errstate(all="ignore"):
        try:
            R = cayley(x[0], x[1], x[2])
            Tn = compose(R, [x[3], x[4], x[5]], T)
        except (OverflowError, ValueError, ZeroDivisionError):
            return None
    if not all(math.isfinite(v) for v in Tn[:12]):
        return None
    return Tn


def evaluate(T, src, tgt, max_corr):
    """(inliers, rmse) of the f64 transform over all pairs, as cs_ransac_batch evaluates a hypothesis."""
    m = len(src)
    thr2 = float(max_corr) * float(max_corr)
    ex = math.frexp(thr2)[1] if math.isfinite(thr2) else 1024
    ex = max(ex, -900)
    eM = 0 if m <= 1 else (m - 1).bit_length()
    scale = math.ldexp(1.0, SUM_BITS - eM - ex)
    cnt, err = 0, 0
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    for i in range(m):
        sx, sy, sz = float(s64[i, 0]), float(s64[i, 1]), float(s64[i, 2])
        dx = fma(T[2], sz, fma(T[1], sy, fma(T[0], sx, T[3]))) - float(t64[i, 0])
        dy = fma(T[6], sz, fma(T[5], sy, fma(T[4], sx, T[7]))) - float(t64[i, 1])
        dz = fma(T[10], sz, fma(T[9], sy, fma(T[8], sx, T[11]))) - float(t64[i, 2])
        d2 = fma(dz, dz, fma(dy, dy, dx * dx))
        if d2 < thr2:
            cnt += 1
            err += int(d2 * scale)
    assert err < 2 ** 62
    rmse = math.sqrt((float(err) / scale) / float(cnt)) if cnt > 0 else 0.0
    return cnt, rmse


def fgr(src, tgt, max_corr, mu_floor=0.025, division_factor=1.4, iteration_number=64, tuple_test_on=True,
        tuple_scale=0.95, max_tuple=1000, seed=0, chunk=4096):
    """One problem.  Returns dict(T f64 [16], T32 f32 [16], inliers, rmse, iters, n_tuple, mu, That)."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    assert src.shape == tgt.shape
    fr = frame(src, tgt)
    n_tuple = 0 if tuple_test_on else -1
    qh = ph = np.zeros((0, 3))
    if fr is not None:
        cs, ct, g = fr
        qh = (src.astype(np.float64) - cs) / g
        ph = (tgt.astype(np.float64) - ct) / g
        if tuple_test_on:
            idx = tuple_test(qh, ph, seed, tuple_scale, max_tuple, chunk)
            n_tuple = len(idx) // 3
            qh, ph = qh[idx], ph[idx]
    n = len(qh)
    solve = fr is not None and n >= MIN_PAIRS
    T, mu, iters = list(IDENTITY), 1.0, 0
    if solve:
        eN = 0 if n <= 1 else (n - 1).bit_length()
        for itr in range(int(iteration_number)):
            S, exps = sums_of(T, mu, qh, ph, eN)
            Tn = update(T, S, exps)
            if Tn is None:
                break
            T = Tn
            iters += 1
            if itr % 4 == 0 and mu > mu_floor:
                mu = mu / division_factor
    That = list(T)
    if solve:
        for a in range(3):
            rc = (T[4 * a] * cs[0] + T[4 * a + 1] * cs[1]) + T[4 * a + 2] * cs[2]
            T[4 * a + 3] = float((g * That[4 * a + 3] + ct[a]) - rc)
    T = [float(v) for v in T]
    inl, rmse = evaluate(T, src, tgt, max_corr)
    T64 = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        T32 = T64.astype(np.float32)
    return {"T": T64, "T32": T32, "inliers": inl, "rmse": rmse, "iters": iters, "n_tuple": n_tuple, "mu": mu,
            "That": np.asarray(That, np.float64)}


def fgr_batch(src, tgt, offsets, max_corr, **kw):
    """The whole call: a list of per-problem results."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    return [fgr(src[offsets[p]:offsets[p + 1]], tgt[offsets[p]:offsets[p + 1]], max_corr, **kw)
            for p in range(len(offsets) - 1)]


# ---- helpers of the tests and of tests/golden/make_fgr_fixture.py -------------------------------------------------------
def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def outlier_case(n, outlier_share, seed, noise=0.005):
    """n pairs in a 1.0 x 1.6 x 0.8 box under a random pose with `noise`; a share of the targets is replaced by uniform
    draws in the posed box.  Returns (src f32, tgt f32, R, t)."""
    rng = np.random.default_rng(seed)
    half = np.array([0.5, 0.8, 0.4])
    src = rng.uniform(-half, half, size=(n, 3))
    R, t = random_rotation(rng), rng.uniform(-0.5, 0.5, size=3)
    tgt = src @ R.T + t + rng.normal(scale=noise, size=(n, 3))
    bad = rng.permutation(n)[:int(round(outlier_share * n))]
    tgt[bad] = rng.uniform(-half, half, size=(len(bad), 3)) @ R.T + t
    return src.astype(np.float32), tgt.astype(np.float32), R, t


def pose_error(T, R, t):
    """(rotation error in degrees, translation error) of the row-major 4x4 T against (R, t)."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    c = (np.trace(T[:3, :3] @ R.T) - 1.0) / 2.0
    return math.degrees(math.acos(min(1.0, max(-1.0, c)))), float(np.linalg.norm(T[:3, 3] - t))


def horn_fit(src, tgt):
    """Least-squares rigid fit on all pairs (Kabsch); the baseline the outlier test compares with."""
    s, q = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    ms, mq = s.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((q - mq).T @ (s - ms))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ ms
    return T
