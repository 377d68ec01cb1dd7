"""The inputs the outlier tests share (tests/test_outlier_cpu.py, tests/test_gpu_outlier.py): three bundled real clouds
with synthetic clutter, and the float implementation the restatement is compared with."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOXEL = 0.03
CLOUDS = (0, 3, 5)
ROWS = {0: (2361, 47), 3: (1082, 21), 5: (1535, 30)}     # (real rows, clutter rows) of the recipe below
_cache = {}


def clutter_cloud(i):
    """(f32 [n,3], is_clutter bool [n]).  Cloud i of tests/golden/real_clouds10.npz as f32 (as stored, not normalised), at
    voxel 0.03 with the first point per voxel; then 2 % clutter: int(0.02 n) rows, the first draws of default_rng(i),
    uniform in the bounding box widened by 20 % of its extent per side, that lie more than 3 voxels from every real row.
    The clutter rows are spread among the real ones (a fixed permutation), so that no filter can go by position."""
    if i in _cache:
        return _cache[i]
    from scipy.spatial import cKDTree

    pc = np.load(os.path.join(GOLD, "real_clouds10.npz"))["clouds"][i].astype(np.float32)
    g = np.floor(pc.astype(np.float64) / VOXEL).astype(np.int64)
    _, idx = np.unique(g, axis=0, return_index=True)
    real = pc[np.sort(idx)]
    want = int(0.02 * len(real))
    rng = np.random.default_rng(i)
    lo, hi = real.min(0).astype(np.float64), real.max(0).astype(np.float64)
    ext = hi - lo
    draws = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (8 * want, 3)).astype(np.float32)
    far = cKDTree(real.astype(np.float64)).query(draws.astype(np.float64))[0] > 3 * VOXEL
    clutter = draws[far][:want]
    assert len(clutter) == want
    xyz = np.concatenate([real, clutter])
    flag = np.concatenate([np.zeros(len(real), bool), np.ones(len(clutter), bool)])
    perm = rng.permutation(len(xyz))
    _cache[i] = (np.ascontiguousarray(xyz[perm]), flag[perm])
    return _cache[i]


def packed():
    """(xyz f32 [n,3], offsets, is_clutter) of the three clouds in one call's layout."""
    parts = [clutter_cloud(i) for i in CLOUDS]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).tolist()
    return np.concatenate([p[0] for p in parts]), off, np.concatenate([p[1] for p in parts])


def float_statistical(xyz, k, std_ratio):
    """Open3D's rule in plain f64: (keep, means, mu, sigma, tau)."""
    from scipy.spatial import cKDTree

    c = xyz.astype(np.float64)
    d = cKDTree(c).query(c, k=min(k, len(c)))[0].reshape(len(c), -1)
    mean = d.mean(1)
    mu, sigma = float(mean.mean()), float(mean.std(ddof=1))
    tau = mu + std_ratio * sigma
    return (mean > 0) & (mean < tau), mean, mu, sigma, tau


def float_radius(xyz, radius):
    """count of rows inside the radius (self included), and for the gap assertion every pair distance within 1 % of it"""
    from scipy.spatial import cKDTree

    c = xyz.astype(np.float64)
    tree = cKDTree(c)
    count = np.array([len(b) for b in tree.query_ball_point(c, radius)], np.int32)
    pairs = tree.query_pairs(radius * 1.01, output_type="ndarray")
    dist = np.linalg.norm(c[pairs[:, 0]] - c[pairs[:, 1]], axis=1)
    return count, dist
