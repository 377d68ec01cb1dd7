"""References of the non-finite contract of the nearest-neighbour family (include/corsair_hip.h: "a candidate whose
canonical f64 squared distance is NaN or +inf is never a neighbour, and a non-finite row changes nothing outside itself").

Every reference here is the CPU oracle or NumPy f64 run on the CLEANED problem: non-finite target / catalog rows are taken
out and the indices mapped back, non-finite query rows get (-1, +inf) by definition.  Nothing here relies on what the oracle
does with a NaN -- it never sees one.  A finite row of any magnitude (1e30) is an ordinary row and stays in."""
import math

import numpy as np

DIRTY_KINDS = ("nan_elem", "nan_row", "pos_inf", "neg_inf", "huge")


def dirty(row, kind, col):
    """A copy of `row` made dirty: one NaN element, a whole NaN row, one +inf, one -inf, or one finite 1e30 (whose f32
    norm overflows: the range fallbacks, not the non-finite rule -- such a row remains a legitimate, distant neighbour)."""
    r = np.array(row, copy=True)
    if kind == "nan_elem":
        r[col] = np.nan
    elif kind == "nan_row":
        r[:] = np.nan
    elif kind == "pos_inf":
        r[col] = np.inf
    elif kind == "neg_inf":
        r[col] = -np.inf
    elif kind == "huge":
        r[col] = 1e30
    else:
        raise ValueError(kind)
    return r


def finite_rows(x):
    return np.isfinite(np.asarray(x)).all(axis=1)


def knn_clean(oracle, qf, tf, k, qlabel=None, tlabel=None, perm=None):
    """cs_knn_feat of one problem by the contract: (idx int32 [nq,k] local to tf, dist f64 [nq,k])."""
    qf, tf = np.asarray(qf, np.float32), np.asarray(tf, np.float32)
    idx = np.full((len(qf), k), -1, np.int32)
    dist = np.full((len(qf), k), np.inf, np.float64)
    qok, tok = finite_rows(qf), finite_rows(tf)
    rows = np.flatnonzero(tok).astype(np.int32)
    if qok.any() and rows.size:
        args = () if qlabel is None else (np.asarray(qlabel)[qok], np.asarray(tlabel)[tok], perm)
        wi, wd = oracle.knn(qf[qok], tf[tok], k, *args, return_distance=True)
        have = wi >= 0
        idx[qok] = np.where(have, rows[np.where(have, wi, 0)], -1)
        dist[qok] = np.where(have, wd, np.inf)
    return idx, dist


def topk_clean(oracle, q, x, k):
    """cs_l2_topk by the contract: (idx int64 [nq,k], squared distances f64 [nq,k]); the caller takes the root."""
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    idx = np.full((len(q), k), -1, np.int64)
    d2 = np.full((len(q), k), np.inf, np.float64)
    qok, xok = finite_rows(q), finite_rows(x)
    rows = np.flatnonzero(xok)
    if qok.any() and rows.size:
        full = oracle.dist2_matrix(q[qok], x[xok])
        assert np.isfinite(full).all()
        order = np.argsort(full, axis=1, kind="stable")[:, :k]
        m = order.shape[1]
        sub_i, sub_d = idx[qok], d2[qok]
        sub_i[:, :m] = rows[order]
        sub_d[:, :m] = np.take_along_axis(full, order, 1)
        idx[qok], d2[qok] = sub_i, sub_d
    return idx, d2


def nearest_clean(src, tgt, T):
    """f64 distances of every source row (posed by the f32 4x4 T, f64 arithmetic) to its nearest FINITE target row;
    +inf where there is none (a non-finite source row or T, no finite target).  NumPy brute force."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    T = np.asarray(T, np.float64).reshape(4, 4)
    out = np.full(len(src), np.inf)
    tgt = tgt[finite_rows(tgt)]
    if not np.isfinite(T[:3]).all() or not len(tgt):
        return out
    ok = finite_rows(src)
    p = src[ok] @ T[:3, :3].T + T[:3, 3]
    d2 = ((p[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)
    out[ok] = np.sqrt(d2.min(axis=1))
    return out


def chamfer_clean(oracle, src, tgt, T):
    """cs_chamfer_1dir of one problem by the contract: the oracle on the finite target rows, +inf when a source row has no
    target at finite distance."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    tgt = tgt[finite_rows(tgt)]
    if not (finite_rows(src).all() and np.isfinite(np.asarray(T)[:3]).all() and len(tgt)):
        return np.inf
    return oracle.chamfer_1dir(src, tgt, T)


# ---- RANSAC ------------------------------------------------------------------------------------------------------
def ransac_count(R, t, src, tgt, max_corr):
    """(inliers, fixed-point error sum, scale) of the f64 transform over the FINITE pairs: d2 < max_corr^2, the error
    summed as the header's rmse defines it (floor(d2 * 2^(38 - ex)) per inlier, exact integer sum)."""
    thr2 = max_corr * max_corr
    scale = math.ldexp(1.0, 38 - math.frexp(thr2)[1])
    ok = finite_rows(src) & finite_rows(tgt)
    s, q = np.asarray(src, np.float64)[ok], np.asarray(tgt, np.float64)[ok]
    d = s @ np.asarray(R).T + np.asarray(t) - q
    d2 = (d * d).sum(axis=1)
    inl = d2 < thr2
    err = int(np.floor(d2[inl] * scale).astype(np.uint64).sum()) if inl.any() else 0
    return int(inl.sum()), err, scale


def ransac_clean(oracle, src, tgt, max_corr, ransac_n, max_iter, confidence, seed):
    """cs_ransac_batch of one problem by the contract, the loop of the header in Python: the oracle's counter-based
    sampling and rigid fit (given FINITE samples only), the recount above.  A sample with a non-finite coordinate has no
    finite fit: no inliers, never the best.  Returns (T f32 [4,4], T64 [3,4] or None, inliers, rmse, iterations)."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    m = len(src)
    T32 = np.eye(4, dtype=np.float32)
    if m < ransac_n:
        return T32, None, 0, 0.0, 0
    fin = finite_rows(src) & finite_rows(tgt)
    log_1mc = math.log(1.0 - confidence)
    est_k, best_cnt, best_err, best, scale = max_iter, 0, 0, None, 1.0
    itr = 0
    while itr < max_iter and itr < est_k:
        idx = oracle.rng_indices(seed, itr, ransac_n, m)
        itr += 1
        if not fin[idx].all():
            continue
        R, t = oracle.rigid_fit(src[idx].astype(np.float64), tgt[idx].astype(np.float64))
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            continue
        cnt, err, scale = ransac_count(R, t, src, tgt, max_corr)
        if cnt > best_cnt or (cnt == best_cnt and cnt > 0 and err < best_err):
            best_cnt, best_err, best = cnt, err, np.concatenate([R, t[:, None]], axis=1)
            pw = 1.0
            for _ in range(ransac_n):
                pw = pw * min(1.0, cnt / m)
            den = math.log(1.0 - pw) if pw < 1.0 else -math.inf
            if den < 0.0:
                est = log_1mc / den
                if est < est_k:
                    est_k = int(math.ceil(est))
    if best_cnt > 0:
        T32[:3] = best.astype(np.float32)
        return T32, best, best_cnt, math.sqrt((best_err / scale) / best_cnt), itr
    return T32, None, 0, 0.0, itr


# ---- voxelize ------------------------------------------------------------------------------------------------------
def voxelize_clean(clouds, voxel):
    """(keep indices into the concatenated cloud, grid int32 [m,4], out offsets): np.floor(x / voxel) in the cloud's own
    type and the first occurrence of every cell, per segment."""
    keep, grid, out_off, base = [], [], [0], 0
    for b, c in enumerate(clouds):
        g = np.floor(c / voxel)
        assert g.dtype == c.dtype
        _, first = np.unique(g.astype(np.int64), axis=0, return_index=True)
        first = np.sort(first)
        keep.append(first + base)
        grid.append(np.concatenate([np.full((len(first), 1), b, np.int32), g[first].astype(np.int32)], axis=1))
        out_off.append(out_off[-1] + len(first))
        base += len(c)
    return np.concatenate(keep), np.concatenate(grid), out_off
