"""NumPy restatement of cs_chamfer_2dir (include/corsair_hip.h) and of the candidate ordering of harness.verify_order,
brute force in plain f64.

The pose of a source row is evaluated in the order of the library's chain, fma(M_c0, x, fma(M_c1, y, fma(M_c2, z, M_c3))):
every product of two f32 values is exact in f64, so each fma of that chain rounds once, exactly like the product followed by
the sum that NumPy evaluates -- the posed points are the library's bit for bit.  The squared distance is the plain
dx*dx + dy*dy + dz*dz (one rounding more than the library's fma chain, all terms non-negative: 2^-52 relative), the nearest
partner is the smallest finite squared distance, a direction's value the NumPy mean of the square roots."""
import numpy as np


def pose_rows(T, s):
    """Rows of s (f32 [n,3]) under the f32 4x4 T, f64 [n,3], in the order of the library's chain."""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    s = np.asarray(s, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([T[c, 0] * s[:, 0] + (T[c, 1] * s[:, 1] + (T[c, 2] * s[:, 2] + T[c, 3])) for c in range(3)], axis=1)


def _mean_nearest(d2, axis):
    """Mean over the rows that remain of sqrt(min over `axis` of the finite entries); NaN for no row, +inf once a row has no
    finite partner."""
    n_rows = d2.shape[1 - axis]
    if n_rows == 0:
        return float("nan")
    if d2.shape[axis] == 0:
        return float("inf")
    best = np.min(np.where(np.isfinite(d2), d2, np.inf), axis=axis)
    return float(np.mean(np.sqrt(best)))


def chamfer_2dir(src, tgt, T):
    """(forward, backward) of one problem: src f32 [ns,3], tgt f32 [nt,3], T f32 [4,4]."""
    p = pose_rows(T, src)
    t = np.asarray(tgt, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        d = p[:, None, :] - t[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    return _mean_nearest(d2, 1), _mean_nearest(d2, 0)


def chamfer_2dir_batch(src, soff, tgt, toff, src_seg, tgt_seg, T):
    """f64 [n_prob,2]: problem p poses segment src_seg[p] of src with T[p] against segment tgt_seg[p] of tgt."""
    out = np.zeros((len(src_seg), 2), np.float64)
    for p, (a, b) in enumerate(zip(src_seg, tgt_seg)):
        out[p] = chamfer_2dir(src[soff[a]:soff[a + 1]], tgt[toff[b]:toff[b + 1]], T[p])
    return out


def order(scores):
    """The candidate order of one query, restated as a loop: the finite scores by (score, retrieval position), then every
    other candidate by retrieval position."""
    s = [float(v) for v in scores]
    finite = sorted((j for j in range(len(s)) if np.isfinite(s[j])), key=lambda j: (s[j], j))
    rest = [j for j in range(len(s)) if not np.isfinite(s[j])]
    return np.asarray(finite + rest, np.int32)
