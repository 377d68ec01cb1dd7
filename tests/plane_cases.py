"""The inputs the plane tests share (tests/test_plane_cpu.py, tests/test_gpu_plane.py): the three clutter clouds of
tests/outlier_cases.py and the three patch clouds of tests/dbscan_cases.py, each standing on a noisy, 3-degree-tilted FLOOR
patch -- what a real scan segment most often carries and neither the outlier filters nor the largest cluster remove."""
import math

import numpy as np

from tests import dbscan_cases as DC
from tests import outlier_cases as OC

VOXEL = OC.VOXEL
CLOUDS = OC.CLOUDS
REAL, CLUTTER, PATCH, FLOOR = DC.REAL, DC.CLUTTER, DC.PATCH, 3
ROWS = {0: (3493, 1085), 3: (1678, 575), 5: (2855, 1290)}            # (rows, floor rows) of floor_cloud
_cache = {}


def _with_floor(xyz, kind, on, i):
    """xyz and kind with a floor under the rows `on` (bool): a VOXEL lattice over their x-y box widened by 30 % of its extent
    per side, at z = (their lowest z) - VOXEL / 2, with uniform noise of +-0.3 VOXEL and a slope of tan(3 degrees) along x
    about the box's middle; cast to f32, appended, the whole permuted by default_rng(200 + i)."""
    base = xyz[on].astype(np.float64)
    lo, hi = base.min(0), base.max(0)
    ext = hi - lo
    ga = np.arange(lo[0] - 0.3 * ext[0], hi[0] + 0.3 * ext[0], VOXEL)
    gb = np.arange(lo[1] - 0.3 * ext[1], hi[1] + 0.3 * ext[1], VOXEL)
    A, Bg = np.meshgrid(ga, gb, indexing="ij")
    rng = np.random.default_rng(200 + i)
    z = lo[2] - 0.5 * VOXEL + rng.uniform(-0.3 * VOXEL, 0.3 * VOXEL, A.size) \
        + math.tan(math.radians(3.0)) * (A.ravel() - (lo[0] + hi[0]) / 2)
    floor = np.stack([A.ravel(), Bg.ravel(), z], 1).astype(np.float32)
    pts = np.concatenate([xyz, floor])
    kinds = np.concatenate([kind, np.full(len(floor), FLOOR)]).astype(np.uint8)
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), kinds[perm]


def floor_cloud(i):
    """(f32 [n,3], kind uint8 [n]: REAL, CLUTTER or FLOOR): clutter_cloud(i) on a floor under its real rows."""
    if ("f", i) not in _cache:
        xyz, clutter = OC.clutter_cloud(i)
        kind = np.where(clutter, CLUTTER, REAL).astype(np.uint8)
        out = _with_floor(xyz, kind, ~clutter, i)
        assert (len(out[0]), int((out[1] == FLOOR).sum())) == ROWS[i]
        _cache[("f", i)] = out
    return _cache[("f", i)]


def floor_patch_cloud(i):
    """The same on patch_cloud(i) (kinds REAL, CLUTTER, PATCH, FLOOR), the floor under the real and the patch rows."""
    if ("p", i) not in _cache:
        xyz, kind = DC.patch_cloud(i)
        _cache[("p", i)] = _with_floor(xyz, kind, (kind == REAL) | (kind == PATCH), i)
    return _cache[("p", i)]


def packed(maker=floor_cloud):
    """(xyz f32 [n,3], offsets, kind) of the three clouds in one call's layout."""
    parts = [maker(i) for i in CLOUDS]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).tolist()
    return np.concatenate([p[0] for p in parts]), off, np.concatenate([p[1] for p in parts])


def float_plane(xyz, dist, iters, seed, triples):
    """The independent float implementation: the given triples, NumPy cross products and point-plane distances, the best count
    (first of the largest), an eigh refit about the inliers' centroid, the mask of the refitted plane.
    Returns (best t, final mask, unit normal, centroid, min relative gap of any s^2 to its bound over all hypotheses)."""
    p = xyz.astype(np.float64)
    T = np.asarray(triples[:iters])
    o = p[T[:, 0]]
    n = np.cross(p[T[:, 1]] - o, p[T[:, 2]] - o)
    nn = (n * n).sum(1)
    s = np.einsum("tqa,ta->tq", p[None] - o[:, None], n)
    bound = dist * dist * nn
    ok = nn > 0
    cnt = np.where(ok, (s * s < bound[:, None]).sum(1), 0)
    gap = float(np.abs(s[ok] ** 2 / bound[ok, None] - 1.0).min())
    t = int(np.argmax(cnt))
    A = p[s[t] ** 2 < bound[t]]
    c = A.mean(0)
    w, v = np.linalg.eigh(np.cov((A - c).T))
    e = v[:, 0]
    sf = (p - c) @ e
    gap = min(gap, float(np.abs(sf * sf / (dist * dist) - 1.0).min()))
    return t, sf * sf < dist * dist, e, c, gap
