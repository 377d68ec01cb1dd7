"""The inputs the clustering tests share (tests/test_dbscan_cpu.py, tests/test_gpu_dbscan.py): the three clutter clouds of
tests/outlier_cases.py, each with a dense PATCH of a second real cloud beside it -- "a few points of a neighbouring object"
(DESIGN 22), which neither outlier filter can remove and the largest DBSCAN cluster leaves out."""
import numpy as np

from tests import outlier_cases as OC

VOXEL = OC.VOXEL
CLOUDS = OC.CLOUDS
OTHER = {0: 3, 3: 5, 5: 0}                              # the cloud the patch is cut from
ROWS = {0: 2691, 3: 1232, 5: 1749}
REAL, CLUTTER, PATCH = 0, 1, 2
# at 2.5 voxels / 5 points: (cluster sizes, noise rows, border rows); at 2.5 / 10: border rows
TABLE = {0: ((2361, 283), 47, 0, 3), 3: ((1082, 129), 21, 0, 4), 5: ((1535, 184), 30, 0, 14)}
_cache = {}


def patch_cloud(i):
    """(f32 [n,3], kind uint8 [n]: REAL, CLUTTER or PATCH).  The rows of clutter_cloud(i); then the int(0.12 * real rows)
    real rows of clutter_cloud(OTHER[i]) nearest to its first real row (f64 sums of squares, a stable argsort), shifted in
    f64 so that their minimum x lies 6 voxels beyond the real rows' maximum x and their minimum y and z at the real rows'
    minima, cast to f32 and appended; the whole permuted by default_rng(100 + i)."""
    if i in _cache:
        return _cache[i]
    xyz, clutter = OC.clutter_cloud(i)
    real = xyz[~clutter]
    oxyz, oclutter = OC.clutter_cloud(OTHER[i])
    other = oxyz[~oclutter].astype(np.float64)
    d = ((other - other[0]) ** 2).sum(1)
    patch = other[np.argsort(d, kind="stable")[:int(0.12 * len(real))]]
    lo, hi = real.min(0).astype(np.float64), real.max(0).astype(np.float64)
    target = np.array([hi[0] + 6 * VOXEL, lo[1], lo[2]])
    patch = (patch + (target - patch.min(0))).astype(np.float32)
    pts = np.concatenate([xyz, patch])
    kind = np.concatenate([np.where(clutter, CLUTTER, REAL), np.full(len(patch), PATCH)]).astype(np.uint8)
    perm = np.random.default_rng(100 + i).permutation(len(pts))
    _cache[i] = (np.ascontiguousarray(pts[perm]), kind[perm])
    assert len(pts) == ROWS[i]
    return _cache[i]


def packed():
    """(xyz f32 [n,3], offsets, kind) of the three clouds in one call's layout."""
    parts = [patch_cloud(i) for i in CLOUDS]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).tolist()
    return np.concatenate([p[0] for p in parts]), off, np.concatenate([p[1] for p in parts])
