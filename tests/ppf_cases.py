"""Inputs of the point-pair-feature tests, shared by tests/test_ppf_cpu.py and tests/test_gpu_ppf.py: an
asymmetric solid with analytic normals, planted problems whose scene is an exact rigid copy, an independent float
implementation (dictionaries, arccos, arctan2 and SciPy rotations), normals and voxels in NumPy for the real clouds, the
batch of the bit-equality test, the defined cases of the header and the batch of the stream schedules."""
import math
import os

import numpy as np
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_FRACTION = 0.05


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---- the solid --------------------------------------------------------------------------------------------------------
BIG = (1.0, 0.6, 0.35)                 # a box with unequal edges ...
SMALL = (0.3, 0.25, 0.2)               # ... carrying a smaller box on the corner at the origin of its top face
TILT = Rotation.from_euler("zyx", [0.7, -0.4, 1.1])     # a fixed generic attitude: no normal is parallel to an axis


def solid(n, seed, tilt=True, grid=12):
    """n rows on the surface of the solid with their outward normals (f32, f32).  The coordinates are rounded to multiples
    of 2^-grid so that a quarter turn and a dyadic shift of them are exact in f32."""
    if n == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    rng = np.random.default_rng(seed)
    bx, by, bz = BIG
    sx, sy, sz = SMALL
    # (origin, edge a, edge b, normal), the top of the big box first
    faces = [((0, 0, bz), (bx, 0, 0), (0, by, 0), (0, 0, 1)), ((0, 0, 0), (bx, 0, 0), (0, by, 0), (0, 0, -1)),
             ((0, 0, 0), (bx, 0, 0), (0, 0, bz), (0, -1, 0)), ((0, by, 0), (bx, 0, 0), (0, 0, bz), (0, 1, 0)),
             ((0, 0, 0), (0, by, 0), (0, 0, bz), (-1, 0, 0)), ((bx, 0, 0), (0, by, 0), (0, 0, bz), (1, 0, 0)),
             ((0, 0, bz + sz), (sx, 0, 0), (0, sy, 0), (0, 0, 1)),
             ((0, 0, bz), (sx, 0, 0), (0, 0, sz), (0, -1, 0)), ((0, sy, bz), (sx, 0, 0), (0, 0, sz), (0, 1, 0)),
             ((0, 0, bz), (0, sy, 0), (0, 0, sz), (-1, 0, 0)), ((sx, 0, bz), (0, sy, 0), (0, 0, sz), (1, 0, 0))]
    area = np.asarray([np.linalg.norm(np.cross(a, b)) for _, a, b, _ in faces])
    pts, nrm = [], []
    while len(pts) < n:
        o, a, b, nv = faces[rng.choice(len(faces), p=area / area.sum())]
        p = np.asarray(o, float) + rng.uniform() * np.asarray(a, float) + rng.uniform() * np.asarray(b, float)
        if nv == (0, 0, 1) and p[2] == bz and p[0] < sx and p[1] < sy:
            continue                                   # under the small box
        pts.append(p)
        nrm.append(nv)
    pts, nrm = np.asarray(pts), np.asarray(nrm, float)
    if tilt:
        pts, nrm = TILT.apply(pts), TILT.apply(nrm)
    return _f32(np.round(pts * 2.0 ** grid) / 2.0 ** grid), _f32(nrm)


QUARTER = (np.asarray([[0, -1, 0], [1, 0, 0], [0, 0, 1]], float), np.asarray([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], float),
           np.asarray([[0, 0, 1], [1, 0, 0], [0, 1, 0]], float), np.asarray([[-1, 0, 0], [0, 0, 1], [0, 1, 0]], float))


def planted(seed, m=300, n_scene=120):
    """(model, model normals, scene, scene normals, R, t, rows): the scene is an EXACT copy of `rows` of the model under
    scene = R model + t, R a product of quarter turns and t dyadic."""
    rng = np.random.default_rng(1000 + seed)
    mx, mn = solid(m, seed)
    R = QUARTER[seed % len(QUARTER)]
    t = rng.integers(-16, 17, 3) / 8.0
    rows = np.sort(rng.permutation(m)[:n_scene])
    sx = mx[rows].astype(np.float64) @ R.T + t
    sn = mn[rows].astype(np.float64) @ R.T
    assert (_f32(sx).astype(np.float64) == sx).all() and (_f32(sn).astype(np.float64) == sn).all()
    return mx, mn, _f32(sx), _f32(sn), R, t, rows


def diagonal_step(model):
    model = np.asarray(model, np.float64)
    return STEP_FRACTION * float(np.linalg.norm(model.max(0) - model.min(0)))


# ---- the independent float implementation ------------------------------------------------------------------------------
def _frames(x, n):
    """Per row the SciPy rotation that takes its unit normal to +x."""
    out = []
    for v in n / np.linalg.norm(n, axis=1, keepdims=True):
        if 1.0 + v[0] < 2.0 ** -20:
            out.append(Rotation.from_euler("y", 180.0, degrees=True).as_matrix())
            continue
        axis = np.cross(v, [1.0, 0.0, 0.0])
        s = np.linalg.norm(axis)
        out.append(np.eye(3) if s == 0.0 else Rotation.from_rotvec(axis / s * math.atan2(s, v[0])).as_matrix())
    return np.asarray(out).reshape(-1, 3, 3)


def _gap(v):
    """The smallest distance of a value from an integer (a bin boundary), in bins."""
    return float(np.abs(v - np.rint(v)).min()) if len(v) else 1.0


class FloatPpf:
    """Drost's voting in plain float arithmetic: a dictionary from the discretised feature to the model pairs, alpha by
    arctan2.  `gap` is the smallest distance (in bins) of any discretised value from a bin boundary."""

    def __init__(self, model, model_normals, step):
        self.mx, self.mn = np.asarray(model, np.float64), np.asarray(model_normals, np.float64)
        self.step = step
        self.mR = _frames(self.mx, self.mn)
        self.gap = 1.0
        self.table = {}
        m = len(self.mx)
        for i in range(m):
            keep, key, ang = self._features(self.mx, self.mn, self.mR, i)
            for j in np.nonzero(keep)[0]:
                self.table.setdefault(tuple(key[j]), []).append((i, ang[j]))
        self.table = {k: (np.asarray([e[0] for e in v]), np.asarray([e[1] for e in v])) for k, v in self.table.items()}

    def _features(self, x, n, R, i):
        u = n / np.linalg.norm(n, axis=1, keepdims=True)
        d = x - x[i]
        length = np.linalg.norm(d, axis=1)
        keep = length > 0.0
        keep[i] = False
        safe = np.where(keep, length, 1.0)
        a1 = np.degrees(np.arccos(np.clip(d @ u[i] / safe, -1, 1))) / 12.0
        a2 = np.degrees(np.arccos(np.clip((d * u).sum(1) / safe, -1, 1))) / 12.0
        a3 = np.degrees(np.arccos(np.clip(u @ u[i], -1, 1))) / 12.0
        q = length / self.step
        local = (d @ R[i].T).astype(np.float32).astype(np.float64)          # the in-plane direction is stored as f32
        keep &= (q < 64.0) & ~((local[:, 1] == 0.0) & (local[:, 2] == 0.0))
        if keep.any():
            inner = lambda a: a[keep & (a > 0.5) & (a < 14.5)]          # 0 and 180 degrees end the range, they part no bins
            self.gap = min(self.gap, _gap(q[keep]), _gap(inner(a1)), _gap(inner(a2)), _gap(inner(a3)))
        key = np.stack([np.floor(q), np.minimum(np.floor(a1), 14), np.minimum(np.floor(a2), 14), np.minimum(np.floor(a3), 14)],
                       1).astype(int)
        return keep, key, np.arctan2(local[:, 2], local[:, 1])

    def vote(self, scene, scene_normals, ref_step=1):
        """{reference: int64 [m, 30]} and the frames of the scene."""
        sx, sn = np.asarray(scene, np.float64), np.asarray(scene_normals, np.float64)
        sR = _frames(sx, sn)
        out = {}
        for r in range(0, len(sx), ref_step):
            acc = np.zeros((len(self.mx), 30), np.int64)
            keep, key, ang = self._features(sx, sn, sR, r)
            for i in np.nonzero(keep)[0]:
                if tuple(key[i]) not in self.table:
                    continue
                mr, am = self.table[tuple(key[i])]
                a = am - ang[i]
                a = a - 2.0 * math.pi * np.floor((a + math.pi) / (2.0 * math.pi))      # into [-pi, pi)
                v = a * 30.0 / (2.0 * math.pi) + 15.0
                self.gap = min(self.gap, _gap(v))
                np.add.at(acc, (mr, np.minimum(np.floor(v).astype(int), 29)), 1)
            out[r] = acc
        return out, sR

    def best(self, scene, scene_normals, ref_step=1):
        """(scene row, model row, bin, votes, R 3x3, t) of the reference with the most votes: the raw peak pose."""
        accs, sR = self.vote(scene, scene_normals, ref_step)
        sx = np.asarray(scene, np.float64)
        r = max(accs, key=lambda k: (accs[k].max(), -k))
        mr, b = np.unravel_index(np.argmax(accs[r]), accs[r].shape)
        alpha = 2.0 * math.pi * (b - 14.5) / 30.0
        Rx = Rotation.from_euler("x", alpha).as_matrix()
        R = self.mR[mr].T @ Rx @ sR[r]
        return r, int(mr), int(b), int(accs[r].max()), R, self.mx[mr] - R @ sx[r], accs


def angle_deg(Ra, Rb):
    return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(Ra.T @ Rb) - 1.0) / 2.0))))


# ---- real clouds without a device --------------------------------------------------------------------------------------
def voxelize(x, voxel):
    """The centroid of every occupied voxel, in the order of the voxels' first rows."""
    x = np.asarray(x, np.float64)
    keys = np.floor(x / voxel).astype(np.int64)
    _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(first), 3))
    np.add.at(sums, inv, x)
    cent = sums / np.bincount(inv)[:, None]
    return _f32(cent[np.argsort(first)])


def pca_normals(x, k=16, view=None):
    """Normals from the k nearest rows, oriented away from the centroid (towards `view` when given)."""
    x = np.asarray(x, np.float64)
    d2 = ((x[:, None] - x[None]) ** 2).sum(2)
    nn = np.argsort(d2, axis=1)[:, :k]
    out = np.zeros_like(x)
    for i in range(len(x)):
        P = x[nn[i]] - x[nn[i]].mean(0)
        out[i] = np.linalg.eigh(P.T @ P)[1][:, 0]
    toward = (view - x) if view is not None else (x - x.mean(0))
    out[(out * toward).sum(1) < 0] *= -1.0
    return _f32(out)


def real_pair(cloud, voxel, seed):
    """(model, model normals, scene, scene normals, R, t): the scene is the whole posed copy voxelised on its own lattice."""
    rng = np.random.default_rng(seed)
    R = Rotation.from_rotvec(Rotation.random(random_state=seed).as_rotvec()).as_matrix()
    t = rng.uniform(-0.2, 0.2, 3)
    model = voxelize(cloud, voxel)
    scene = voxelize(np.asarray(cloud, np.float64) @ R.T + t, voxel)
    return model, pca_normals(model), scene, pca_normals(scene), R, t


def real_clouds(which=(0, 3, 5)):
    d = np.load(os.path.join(ROOT, "tests", "golden", "real_clouds10.npz"))
    return [np.asarray(d["clouds"][i], np.float64).reshape(-1, 3) for i in which]


# ---- the batch of the bit-equality test --------------------------------------------------------------------------------
MAX_DIST = 0.02
# (scene rows, model segment): the scenes; MODELS: the rows of the model segments.  Model 5 (300 rows) serves three scenes;
# model 7 (1 500 rows) exceeds the LDS accumulator's 1 360 rows and takes the global slabs on every path; models 11 and 12
# (1 360 and 1 361 rows) stand on either side of the switch: the largest LDS launch there is, and the first slab one.
MODELS = (300, 64, 65, 63, 3, 300, 700, 1500, 2, 1, 0, 1360, 1361)
SCENES = ((0, 0), (1, 1), (2, 2), (3, 3), (63, 4), (64, 5), (65, 5), (300, 5), (65, 6), (700, 3), (65, 7), (64, 8), (65, 9),
          (300, 10), (64, 11), (63, 12))
SMALL_PROBLEMS = (1, 2, 3, 4, 5, 6, 11, 12, 13)        # what the calls with ref_step 1 and 2 run (the quick ones)


def _scene_of(mx, mn, n, seed):
    """n rows: a rigid copy of rows of the model (repeated with a little noise when n exceeds it)."""
    rng = np.random.default_rng(seed)
    if len(mx) == 0 or n == 0:
        x, nv = solid(n, seed + 77)
        return x, nv
    rows = rng.integers(0, len(mx), n) if n > len(mx) else rng.permutation(len(mx))[:n]
    R = Rotation.random(random_state=seed).as_matrix()
    x = (mx[rows].astype(np.float64) + rng.normal(0, 0.002, (n, 3))) @ R.T + rng.uniform(-1, 1, 3)
    nv = (mn[rows].astype(np.float64) + rng.normal(0, 0.02, (n, 3))) @ R.T
    return _f32(x), _f32(nv)


def batch(seed=1):
    """{"scene", "scene_n", "model", "model_n" f32 [.,3]}, soff, moff, scene_seg, model_seg, dist_step per problem."""
    models = [solid(m, 10 * seed + k) for k, m in enumerate(MODELS)]
    scenes = [_scene_of(*models[k], n, 100 * seed + p) for p, (n, k) in enumerate(SCENES)]
    d = {"scene": np.concatenate([s[0] for s in scenes]), "scene_n": np.concatenate([s[1] for s in scenes]),
         "model": np.concatenate([m[0] for m in models]), "model_n": np.concatenate([m[1] for m in models])}
    soff = np.concatenate([[0], np.cumsum([n for n, _ in SCENES])]).tolist()
    moff = np.concatenate([[0], np.cumsum(MODELS)]).tolist()
    steps = [diagonal_step(models[k][0]) if MODELS[k] > 1 else 0.05 for _, k in SCENES]
    return d, soff, moff, list(range(len(SCENES))), [k for _, k in SCENES], steps


# ---- the defined cases of the header -----------------------------------------------------------------------------------
def defined_cases():
    """name -> (scene, scene normals, model, model normals, kwargs of ppf_one); shared with the GPU test."""
    mx, mn = solid(60, 5)
    sx, sn = _scene_of(mx, mn, 40, 6)
    step = diagonal_step(mx)
    kw = dict(dist_step=step, max_dist=MAX_DIST, ref_step=1, n_cand=8)
    out = {"plain": (sx, sn, mx, mn, kw)}
    dx, dn = sx.copy(), sn.copy()
    dx[5:9], dn[5:9] = dx[4], dn[4]                                    # duplicate rows: |d| = 0 among them
    dm, dmn = mx.copy(), mn.copy()
    dm[10:13], dmn[10:13] = dm[9], dmn[9]
    out["duplicates"] = (dx, dn, dm, dmn, kw)
    g = _f32(np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 0.25)
    gn = _f32(np.where(np.abs(g - 0.25).max(1, keepdims=True) == np.abs(g - 0.25), np.sign(g - 0.25), 0.0))
    gn[13] = [0, 0, 1]                                                 # the centre of the lattice
    out["lattice"] = (g, gn, g, gn, dict(kw, dist_step=0.125, max_dist=0.05))          # exact ties, angles and quotients on boundaries
    bx, bn = sx.copy(), sn.copy()
    bx[3] = [np.nan, 0, 0]
    bx[7] = [0, np.inf, 0]
    bx[0] = [-np.inf] * 3                                              # the first reference is not a row
    bn[11] = [np.nan] * 3
    bn[12] = [0, 0, 0]
    bn[13] = [np.inf, 0, 0]
    bm, bmn = mx.copy(), mn.copy()
    bm[2] = [np.nan] * 3
    bm[20] = [np.inf, 1, 1]
    bmn[21] = [0, 0, 0]
    bmn[22] = [0, np.nan, 0]
    out["nonfinite"] = (bx, bn, bm, bmn, kw)
    out["zero_normals"] = (sx, np.zeros_like(sn), mx, mn, kw)           # every scene row is invalid: nothing is found
    out["nan_model_normals"] = (sx, sn, mx, np.full_like(mn, np.nan), kw)
    out["offset_70"] = (_f32(sx + 70.0), sn, _f32(mx + 70.0), mn, kw)
    out["offset_1e6"] = (_f32(sx.astype(np.float64) * 64 + 1e6), sn, _f32(mx.astype(np.float64) * 64 + 1e6), mn,
                         dict(kw, dist_step=64 * step, max_dist=64 * MAX_DIST))
    out["step_tiny"] = (sx, sn, mx, mn, dict(kw, dist_step=1e-9))      # every quotient is >= 64: every pair is skipped
    tx, tn = solid(24, 8)
    ux, un = _scene_of(tx, tn, 16, 9)
    out["step_huge"] = (ux, un, tx, tn, dict(kw, dist_step=1e9))       # every pair has distance bin 0
    out["normal_minus_x"] = (_f32(sx), _f32(np.tile([-1.0, 0, 0], (len(sx), 1))), mx, _f32(np.tile([-2.0, 0, 0], (len(mx), 1))), kw)
    out["d_parallel_n"] = (_f32([[0, 0, 0], [1, 0, 0], [2, 0, 0]]), _f32([[1, 0, 0]] * 3), _f32([[0, 0, 0], [0, 0, 1], [0, 0, 3]]),
                           _f32([[0, 0, 1]] * 3), dict(kw, dist_step=1.0))
    out["one_candidate"] = (sx, sn, mx, mn, dict(kw, n_cand=1, ref_step=7))
    out["ref_step_above_scene"] = (sx, sn, mx, mn, dict(kw, ref_step=1000, n_cand=64))
    return out


# ---- the stream and stale-memory schedules ------------------------------------------------------------------------------
S_MODELS = (200, 90)
S_SCENES = ((150, 0), (80, 0), (60, 1), (0, 1))
S_SOFF = np.concatenate([[0], np.cumsum([n for n, _ in S_SCENES])]).tolist()
S_MOFF = np.concatenate([[0], np.cumsum(S_MODELS)]).tolist()
S_STEP = [0.065, 0.065, 0.06, 0.06]


def stream_batch(seed):
    models = [solid(m, 50 * seed + k) for k, m in enumerate(S_MODELS)]
    scenes = [_scene_of(*models[k], n, 500 * seed + p) for p, (n, k) in enumerate(S_SCENES)]
    return {"scene": np.concatenate([s[0] for s in scenes]), "scene_n": np.concatenate([s[1] for s in scenes]),
            "model": np.concatenate([m[0] for m in models]), "model_n": np.concatenate([m[1] for m in models])}
