"""NumPy restatements of the training-batch kernels (include/corsair_hip.h: cs_radius_pairs, cs_sample_pairs,
cs_transform_f64), written from the header's formulas."""
import numpy as np
from scipy.spatial import cKDTree

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def rng_u64_int(seed, j):
    """The header's generator on Python integers (itr = 0)."""
    x = (seed + GOLDEN * (j + 1)) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rng_u64(seed, slot, round_, stream, ctr):
    """Vectorised over ctr (uint64 arithmetic wraps mod 2^64)."""
    ctr = np.asarray(ctr, np.uint64)
    j = np.uint64((slot << 40) | (round_ << 36) | (stream << 32)) | ctr
    with np.errstate(over="ignore"):
        x = np.uint64(seed & M64) + np.uint64(GOLDEN) * (j + np.uint64(1))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def rng_index(x, n):
    u = (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.floor(u * float(n)).astype(np.int64)


def d2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def radius_pairs(src, tgt, r, k=None):
    """List of int arrays: row i's targets with d2 < r*r, ascending (d2, index), at most k."""
    src = np.asarray(src, np.float64)
    tgt = np.asarray(tgt, np.float64)
    if len(src) == 0:
        return []
    if len(tgt) == 0:
        return [np.zeros(0, np.int64) for _ in range(len(src))]
    cand = cKDTree(tgt).query_ball_point(src, r * 1.01 + 1e-12)
    out = []
    for i, c in enumerate(cand):
        c = np.asarray(sorted(c), np.int64)
        dd = d2(src[i][None], tgt[c]) if len(c) else np.zeros(0)
        keep = dd < r * r
        c, dd = c[keep], dd[keep]
        order = np.lexsort((c, dd))
        c = c[order]
        out.append(c[:k] if k is not None else c)
    return out


def sample_slot(base, pos, neg, rows, seed, slot, round_, r, sample):
    """PiP, PiN, NiN of one slot (base / pos / neg: f32 kept canonical points; rows: the uncapped PiP rows)."""
    n_pos = sum(len(x) for x in rows)
    pi = np.repeat(np.arange(len(rows)), [len(x) for x in rows]).astype(np.int64)
    pj = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    t = np.arange(n_pos, dtype=np.uint64)
    key = (rng_u64(seed, slot, round_, 0, t) >> np.uint64(32)) << np.uint64(32) | t
    sel = np.argsort(key, kind="stable")[:min(sample, n_pos)]
    pip = np.stack([pi[sel], pj[sel]], 1) if n_pos else np.zeros((0, 2), np.int64)

    def negatives(other, stream, exclude):
        t = np.arange(n_pos, dtype=np.uint64)
        i = rng_index(rng_u64(seed, slot, round_, stream, 2 * t), len(base))
        j = rng_index(rng_u64(seed, slot, round_, stream, 2 * t + np.uint64(1)), len(other))
        if n_pos == 0:
            return np.zeros((0, 2), np.int64)
        keep = exclude(i, j)
        diff = base[i] - other[j]
        norm = np.linalg.norm(diff, 2, 1)
        keep &= norm > np.float32(0.1)
        return np.stack([i[keep], j[keep]], 1)[:sample]

    pin = negatives(pos, 1, lambda i, j: ~(d2(base[i], pos[j]) < r * r))
    nin = negatives(neg, 2, lambda i, j: ~((i == 0) & (j == 0)))
    return pip, pin, nin


def transform(xyz, T):
    x = np.asarray(xyz, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    out = np.empty_like(x)
    for c in range(3):
        out[:, c] = ((T[c, 0] * x[:, 0] + T[c, 1] * x[:, 1]) + T[c, 2] * x[:, 2]) + T[c, 3]
    return out


def quantize_first(x64, voxel):
    """floor(x / voxel) in f64, first occurrence of every voxel, kept rows ascending."""
    g = np.floor(x64 / voxel).astype(np.int64)
    _, first = np.unique(g, axis=0, return_index=True)
    keep = np.sort(first)
    return keep, g[keep]
