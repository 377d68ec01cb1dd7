"""NumPy / Python restatement of cs_ppf_batch (include/corsair_hip.h), bit for bit: the rows' frames, the pair
features and their keys, the model table, the votes, the peaks, the candidates' ranks, the poses, the verification count, the
winner, the inverse and the fixed-point rmse.

Steps a, b, d and g of the header use + - * / sqrt and casts only, each of which NumPy performs as ONE IEEE operation per
element, so they are vectorised as they stand (sums are written out: np.sum's pairwise order is never used).  Step h is an
fma chain: an unfused vectorised chain classifies every (scene row, model row) first, with an absolute bound on what the
two chains can differ by, and whatever lies within the bound of the threshold or of the row's minimum takes the exact chain
(tests/gicp_ref.fma), tests/featmatch_ref.py's habit.  The constants are read from corsair_amd/csrc/ppf_bounds.h: those
numbers are the specification.
"""
import functools
import math
import os
import re

import numpy as np

from tests.gicp_ref import fma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_BINS, ANGLE_BINS, ALPHA_BINS = 64, 15, 30
KEYS = DIST_BINS * ANGLE_BINS ** 3
MAX_CAND = 64
K_MIN = 2.0 ** -20
IDENTITY = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
E48 = 2.0 ** -48


def _table(name):
    text = open(os.path.join(ROOT, "corsair_amd", "csrc", "ppf_bounds.h")).read()
    body = text[text.index("#define " + name):].split("#define")[1]
    return [float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+", body)]


COS = np.asarray(_table("CS_PPF_COS"))                                   # 14
BOUNDS = np.asarray(_table("CS_PPF_ALPHA_BOUNDS")).reshape(29, 2)        # (cos, sin) of theta_m, m = 1..29
CENTRES = np.asarray(_table("CS_PPF_ALPHA_CENTRES")).reshape(30, 2)      # (cos, sin) of the centre of bin b
assert COS.shape == (14,) and BOUNDS.shape == (29, 2) and CENTRES.shape == (30, 2)


class Frames:
    """Step 'Row' and step b for every row of a segment: x, ok, u, the three rows of the rotation."""

    def __init__(self, xyz, normals):
        self.x32 = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self.n32 = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        assert self.x32.shape == self.n32.shape
        x, N = self.x32.astype(np.float64), self.n32.astype(np.float64)
        self.n = len(x)
        with np.errstate(all="ignore"):
            nn = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
            ok = np.isfinite(x).all(1) & np.isfinite(N).all(1) & (nn > 0.0)
            u = np.where(ok[:, None], N / nn[:, None], 0.0)
            k = 1.0 + u[:, 0]
            w = (u[:, 1] * u[:, 2]) / k
            one = np.ones(self.n)
            zero = np.zeros(self.n)
            r1 = np.stack([-u[:, 1], 1.0 - (u[:, 1] * u[:, 1]) / k, -w], 1)
            r2 = np.stack([-u[:, 2], -w, 1.0 - (u[:, 2] * u[:, 2]) / k], 1)
        plain = ok & (k >= K_MIN)
        self.x, self.ok, self.u = x, ok, u
        self.r0 = np.where(plain[:, None], u, np.stack([-one, zero, zero], 1))
        self.r1 = np.where(plain[:, None], r1, np.stack([zero, one, zero], 1))
        self.r2 = np.where(plain[:, None], r2, np.stack([zero, zero, -one], 1))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def angle_bin(c):
    """The number of k in 1..14 with c <= C_k."""
    return (np.asarray(c)[..., None] <= COS).sum(-1)


def pair_features(fr, I, J, step):
    """Step a for the ordered pairs (I[k], J[k]) of one segment: (keep bool, key int64, y f32, z f32)."""
    I, J = np.asarray(I), np.asarray(J)
    with np.errstate(all="ignore"):
        d = fr.x[J] - fr.x[I]
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        q = length / step
        keep = fr.ok[I] & fr.ok[J] & (I != J) & (length > 0.0) & (q < float(DIST_BINS))
        c1 = _dot(fr.u[I], d) / length
        c2 = _dot(fr.u[J], d) / length
        c3 = _dot(fr.u[I], fr.u[J])
        y = _dot(fr.r1[I], d).astype(np.float32)
        z = _dot(fr.r2[I], d).astype(np.float32)
        keep &= np.isfinite(y) & np.isfinite(z) & ~((y == 0.0) & (z == 0.0))
        dbin = np.where(keep, q, 0.0).astype(np.int64)
    key = ((dbin * ANGLE_BINS + angle_bin(c1)) * ANGLE_BINS + angle_bin(c2)) * ANGLE_BINS + angle_bin(c3)
    return keep, key, y, z


def alpha_bin(ym, zm, ys, zs):
    """Step d: the bin of the angle of (ym + i zm) * conj(ys + i zs); f32 inputs, widened here."""
    ym, zm, ys, zs = (np.asarray(v, np.float32).astype(np.float64) for v in (ym, zm, ys, zs))
    ym, zm, ys, zs = np.broadcast_arrays(ym, zm, ys, zs)
    px = ym * ys + zm * zs
    py = zm * ys - ym * zs
    lower = py < 0.0
    b = np.where(lower, 0, 15)
    for k in range(14):
        c = np.where(lower, BOUNDS[k, 0], BOUNDS[15 + k, 0])
        s = np.where(lower, BOUNDS[k, 1], BOUNDS[15 + k, 1])
        b = b + ((c * py - s * px) >= 0.0)
    return b


class Model:
    """Step c: the frames of a model segment and its table at one dist_step, the entries sorted by key (inside a key by
    (i, j): the order reaches nothing)."""

    BLOCK = 128

    def __init__(self, xyz, normals, step):
        self.fr = Frames(xyz, normals)
        self.step = float(step)
        m = self.m = self.fr.n
        keys, rows, ys, zs = [], [], [], []
        for i0 in range(0, m, self.BLOCK):
            I, J = np.meshgrid(np.arange(i0, min(m, i0 + self.BLOCK)), np.arange(m), indexing="ij")
            I, J = I.reshape(-1), J.reshape(-1)
            keep, key, y, z = pair_features(self.fr, I, J, self.step)
            keys.append(key[keep]), rows.append(I[keep]), ys.append(y[keep]), zs.append(z[keep])
        cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
        key, row, y, z = cat(keys, np.int64), cat(rows, np.int64), cat(ys, np.float32), cat(zs, np.float32)
        order = np.argsort(key, kind="stable")
        self.key, self.row, self.y, self.z = key[order], row[order], y[order], z[order]
        self.start = np.concatenate([[0], np.cumsum(np.bincount(self.key, minlength=KEYS))]).astype(np.int64)


@functools.lru_cache(maxsize=64)
def _model(xb, nb, step):
    return Model(np.frombuffer(xb, np.float32).reshape(-1, 3), np.frombuffer(nb, np.float32).reshape(-1, 3), step)


def model_of(xyz, normals, step):
    xyz, normals = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(normals, np.float32)
    return _model(xyz.tobytes(), normals.tobytes(), float(step))


def votes(sf, r, model):
    """Step d for the reference r of the scene frames sf: int64 [m * 30], the accumulator."""
    acc = np.zeros(model.m * ALPHA_BINS, np.int64)
    if not sf.ok[r] or sf.n < 2 or model.m == 0:
        return acc
    I = np.arange(sf.n)
    keep, key, ys, zs = pair_features(sf, np.full(sf.n, r), I, model.step)
    key, ys, zs = key[keep], ys[keep], zs[keep]
    n = model.start[key + 1] - model.start[key]
    total = int(n.sum())
    if total == 0:
        return acc
    owner = np.repeat(np.arange(len(key)), n)
    e = model.start[key][owner] + (np.arange(total) - np.repeat(np.cumsum(n) - n, n))
    b = alpha_bin(model.y[e], model.z[e], ys[owner], zs[owner])
    return np.bincount(model.row[e] * ALPHA_BINS + b, minlength=len(acc)).astype(np.int64)


def peak(acc):
    """Step e: (votes, cell) -- the most votes, ties to the smallest cell; (0, -1) without a vote."""
    if len(acc) == 0:
        return 0, -1
    c = int(np.argmax(acc))
    return (int(acc[c]), c) if acc[c] > 0 else (0, -1)


def pose(sf, r, mf, mr, b):
    """Step g: R | t (12 floats) of Tm^-1 Rx(alpha_b) Ts."""
    ca, sa = float(CENTRES[b, 0]), float(CENTRES[b, 1])
    Rs = [[float(v) for v in row[r]] for row in (sf.r0, sf.r1, sf.r2)]
    Rm = [[float(v) for v in row[mr]] for row in (mf.r0, mf.r1, mf.r2)]
    xs, xm = [float(v) for v in sf.x[r]], [float(v) for v in mf.x[mr]]
    A = [[Rs[0][k] for k in range(3)], [ca * Rs[1][k] - sa * Rs[2][k] for k in range(3)],
         [sa * Rs[1][k] + ca * Rs[2][k] for k in range(3)]]
    out = []
    for a in range(3):
        R = [(Rm[0][a] * A[0][k] + Rm[1][a] * A[1][k]) + Rm[2][a] * A[2][k] for k in range(3)]
        out += R + [xm[a] - ((R[0] * xs[0] + R[1] * xs[1]) + R[2] * xs[2])]
    return out


def inverse(T):
    """Step i: the rigid inverse of R | t by the stated chain (12 floats)."""
    out = []
    for a in range(3):
        out += [T[a], T[4 + a], T[8 + a], -((T[a] * T[3] + T[4 + a] * T[7]) + T[8 + a] * T[11])]
    return out


def dist2_exact(T, p, q):
    P = [fma(T[4 * a + 2], p[2], fma(T[4 * a + 1], p[1], fma(T[4 * a], p[0], T[4 * a + 3]))) for a in range(3)]
    e = [P[a] - q[a] for a in range(3)]
    return fma(e[2], e[2], fma(e[1], e[1], e[0] * e[0]))


def verify(sf, mf, T, thr2, want_min=False):
    """Step h: (count, dmin per scene row or None).  dmin is exact, +inf for a row that does not count."""
    T = [float(v) for v in T]
    live = np.isfinite(sf.x).all(1)
    if sf.n == 0 or mf.n == 0:
        return 0, np.full(sf.n, math.inf)
    x = np.where(live[:, None], sf.x, 0.0)
    with np.errstate(all="ignore"):
        P = np.stack([((T[4 * a] * x[:, 0] + T[4 * a + 3]) + T[4 * a + 1] * x[:, 1]) + T[4 * a + 2] * x[:, 2] for a in range(3)], 1)
        S = np.stack([np.abs(T[4 * a] * x[:, 0]) + np.abs(T[4 * a + 3]) + np.abs(T[4 * a + 1] * x[:, 1])
                      + np.abs(T[4 * a + 2] * x[:, 2]) for a in range(3)], 1)
        delta = 2.0 * E48 * S.sum(1)                                  # what the fused and the unfused P can differ by, and more
        e = P[:, None, :] - mf.x[None, :, :]
        d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        d2 = np.where(np.isfinite(d2), d2, math.inf)
        B = 2.0 * np.sqrt(d2) * delta[:, None] + (delta * delta)[:, None] + 4.0 * E48 * d2
        B = np.where(np.isfinite(B), B, 0.0)
    rows = lambda a, i: [float(v) for v in a[i]]
    lo, hi = d2 - B, d2 + B
    dmin = np.full(sf.n, math.inf)
    if not want_min:
        sure = live & (hi < thr2).any(1)
        count = int(sure.sum())
        for i in np.nonzero(live & ~sure & (lo < thr2).any(1))[0]:
            count += any(dist2_exact(T, rows(sf.x, i), rows(mf.x, j)) < thr2 for j in np.nonzero(lo[i] < thr2)[0])
        return count, None
    count = 0
    for i in np.nonzero(live & (lo < thr2).any(1))[0]:
        cand = np.nonzero(lo[i] <= hi[i].min())[0]
        best = min([dist2_exact(T, rows(sf.x, i), rows(mf.x, j)) for j in cand], default=math.inf)
        if best < thr2:
            count += 1
            dmin[i] = best
    return count, dmin


class Problem:
    """One (scene, model, dist_step): the peaks of the references are cached per scene row, so that calls that differ in
    ref_step, n_cand or max_dist share them."""

    def __init__(self, scene, scene_normals, model, model_normals, dist_step):
        self.sf = Frames(scene, scene_normals)
        self.model = model_of(model, model_normals, dist_step)
        self._peak = {}

    def peak(self, r):
        if r not in self._peak:
            self._peak[r] = peak(votes(self.sf, r, self.model))
        return self._peak[r]

    def result(self, max_dist, ref_step=5, n_cand=16):
        """(T 16, Tinv 16, stat 8, rmse, cand_T [n_cand][16], cand_stat [n_cand][4])."""
        sf, mf = self.sf, self.model.fr
        refs = list(range(0, sf.n, ref_step))
        n_ref = len(refs)
        pk = [self.peak(r) for r in refs]
        order = sorted(range(n_ref), key=lambda k: (-pk[k][0], k))[:n_cand]
        thr2 = float(max_dist) * float(max_dist)
        cand_T = [list(IDENTITY) for _ in range(n_cand)]
        cand_stat = [[0, 0, -1, -1] for _ in range(n_cand)]
        best = None
        for c, k in enumerate(order):
            v, cell = pk[k]
            if v == 0:
                continue
            T = pose(sf, refs[k], mf, cell // ALPHA_BINS, cell % ALPHA_BINS)
            count, _ = verify(sf, mf, T, thr2)
            cand_T[c] = T + [0.0, 0.0, 0.0, 1.0]
            cand_stat[c] = [v, count, refs[k], cell]
            if best is None or count > best[0]:
                best = (count, c, T)
        if best is None:
            return list(IDENTITY), list(IDENTITY), [0, 0, -1, -1, -1, 0, -1, n_ref], 0.0, cand_T, cand_stat
        count, c, T = best
        v, _, r, cell = cand_stat[c]
        rmse = 0.0
        if count > 0:
            again, dmin = verify(sf, mf, T, thr2, want_min=True)
            assert again == count
            eM = 0 if sf.n <= 1 else (sf.n - 1).bit_length()
            ex = max(math.frexp(thr2)[1], -900) if thr2 < math.inf else 1024
            k2 = 61 - eM - ex
            E = sum(int(d * math.ldexp(1.0, k2)) for d in dmin if d < thr2)
            assert E < 1 << 63
            rmse = math.sqrt((float(E) * math.ldexp(1.0, -k2)) / float(count))
        stat = [1, v, r, cell // ALPHA_BINS, cell % ALPHA_BINS, count, c, n_ref]
        return T + [0.0, 0.0, 0.0, 1.0], inverse(T) + [0.0, 0.0, 0.0, 1.0], stat, rmse, cand_T, cand_stat


def ppf_one(scene, scene_normals, model, model_normals, dist_step, max_dist, ref_step=5, n_cand=16):
    return Problem(scene, scene_normals, model, model_normals, dist_step).result(max_dist, ref_step, n_cand)


def pack(results, n_cand):
    """The arrays of cs_ppf_batch from a list of Problem.result tuples."""
    P = len(results)
    return (np.asarray([r[0] for r in results], np.float64).reshape(P, 4, 4),
            np.asarray([r[1] for r in results], np.float64).reshape(P, 4, 4),
            np.asarray([r[2] for r in results], np.int32).reshape(P, 8),
            np.asarray([r[3] for r in results], np.float64).reshape(P),
            np.asarray([r[4] for r in results], np.float64).reshape(P, n_cand, 4, 4),
            np.asarray([r[5] for r in results], np.int32).reshape(P, n_cand, 4))


def ppf_batch(scene, scene_normals, soff, model, model_normals, moff, scene_seg, model_seg, dist_step, max_dist, ref_step=5,
              n_cand=16):
    """(T, Tinv f64 [P,4,4], stat int32 [P,8], rmse f64 [P], cand_T f64 [P,n_cand,4,4], cand_stat int32 [P,n_cand,4])."""
    scene, scene_normals = (np.asarray(a, np.float32).reshape(-1, 3) for a in (scene, scene_normals))
    model, model_normals = (np.asarray(a, np.float32).reshape(-1, 3) for a in (model, model_normals))
    out = []
    for p in range(len(scene_seg)):
        s, m = slice(soff[scene_seg[p]], soff[scene_seg[p] + 1]), slice(moff[model_seg[p]], moff[model_seg[p] + 1])
        out.append(ppf_one(scene[s], scene_normals[s], model[m], model_normals[m], dist_step[p], max_dist, ref_step, n_cand))
    return pack(out, n_cand)
