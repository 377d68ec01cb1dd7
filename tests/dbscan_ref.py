"""NumPy / Python restatement of cs_dbscan and cs_cluster_largest (include/corsair_hip.h): the exhaustive d2 of every pair
of a segment by the header's fma chain, the core flags, the components of the core rows by a sequential union-find, the
canonical numbering, the border rule and the largest cluster.

As in tests/outlier_ref.py the exact chain only runs where it can matter: an unfused vectorised chain d~ decides every
pair outside |d~ - r2| <= 1e-12 r2 (both chains are within 4 * 2^-53 relative of the true sum of the same three squares),
and the border rule compares exact d2 values only.
"""
import math

import numpy as np

from tests.outlier_ref import _approx, d2_exact


def neighbours(seg, eps):
    """[n] index arrays: the rows j of `seg` (f32 [n,3]) with d2 < eps * eps, row i itself included, ascending."""
    s64 = np.asarray(seg, np.float32).reshape(-1, 3).astype(np.float64)
    r2 = float(eps) * float(eps)
    out = []
    for i in range(len(s64)):
        raw = _approx(s64, i)
        if not math.isfinite(r2):
            out.append(np.nonzero(np.isfinite(raw))[0])        # every finite d2 passes; +inf (a non-finite row) never
            continue
        sure = raw < r2 * (1 - 1e-12)
        near = np.nonzero(~sure & (raw <= r2 * (1 + 1e-12)))[0]
        extra = [j for j in near if d2_exact(s64, i, j) < r2]
        out.append(np.sort(np.concatenate([np.nonzero(sure)[0], np.asarray(extra, np.int64)])).astype(np.int64))
    return out


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def dbscan_segment(seg, eps, min_points):
    """(label int32 [n], count int32 [n], core bool [n]) of one segment."""
    seg = np.asarray(seg, np.float32).reshape(-1, 3)
    n = len(seg)
    s64 = seg.astype(np.float64)
    nbr = neighbours(seg, eps)
    count = np.array([len(v) for v in nbr], np.int32).reshape(n)
    core = count >= int(min_points)
    parent = list(range(n))
    for i in np.nonzero(core)[0]:
        for j in nbr[i]:
            if j < i and core[j]:
                a, b = _find(parent, int(i)), _find(parent, int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)             # the root is the smallest row of its tree
    label = np.full(n, -1, np.int32)
    ids = {}
    for i in np.nonzero(core)[0]:                             # ascending: a root is met before the rest of its tree
        r = _find(parent, int(i))
        if r not in ids:
            assert r == i
            ids[r] = len(ids)
        label[i] = ids[r]
    for i in np.nonzero(~core & (count > 1))[0]:
        best = None
        for j in nbr[i]:
            if core[j]:
                key = (d2_exact(s64, i, j), int(j))
                if best is None or key < best:
                    best = key
        if best is not None:
            label[i] = label[best[1]]
    return label, count, core


def dbscan(xyz, offsets, eps, min_points):
    """(label int32 [n], count int32 [n], core bool [n]): cs_dbscan per segment."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    label, count, core = np.full(len(xyz), -1, np.int32), np.zeros(len(xyz), np.int32), np.zeros(len(xyz), bool)
    for a, b in zip(offsets[:-1], offsets[1:]):
        label[a:b], count[a:b], core[a:b] = dbscan_segment(xyz[a:b], eps, min_points)
    return label, count, core


def cluster_largest(label, offsets):
    """(keep bool [n], stat int32 [n_seg,3] = (clusters, id of the largest, its size)): cs_cluster_largest."""
    label = np.asarray(label, np.int64)
    keep = np.zeros(len(label), bool)
    stat = np.zeros((len(offsets) - 1, 3), np.int32)
    for p, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        l = label[a:b]
        l = np.where((l >= 0) & (l < b - a), l, -1)
        size = np.bincount(l[l >= 0], minlength=1)
        if size.max(initial=0) == 0:
            stat[p] = (0, -1, 0)
            continue
        big = int(np.argmax(size))                            # the first maximum: the smallest id
        stat[p] = (int((size > 0).sum()), big, int(size[big]))
        keep[a:b] = l == big
    return keep, stat


def same_partition(a, b):
    """True when two label arrays name the same partition (and the same -1 rows)."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = {(int(x), int(y)) for x, y in zip(a[a >= 0], b[a >= 0])}
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})
