"""NumPy / Python restatement of cs_estimate_normals_hybrid (include/corsair_hip.h), bit for bit: the neighbours are the
rows of the segment with d2 < radius * radius (strict), of those the max_nn smallest by (canonical distance, row);
everything after the list -- the scatter about the query row, jacobi3, the selection, normalisation and sign rules -- is
tests/normals_ref.py's, imported, as the kernels share it.

As in normals_ref.neighbours the exact fma chain only runs on the rows that can be in the list: an unfused vectorised chain
d~ ranks all rows first, both chains are within 4 * 2^-53 relative of the true sum of the same three squares, so a row
outside d~ <= min(r2, max_nn-th smallest d~) * (1 + 1e-12) can neither pass the radius test nor enter or tie the list.
"""
import math

import numpy as np

from tests.icp_ref import fma
from tests.normals_ref import K_MAX, K_MIN, normal_of, scatter


def neighbours(seg, i, radius, max_nn):
    """Rows of `seg` (f32 [n,3]) around row i: [(d2, row)] ascending, d2 < radius^2, at most max_nn of them."""
    r2 = float(radius) * float(radius)          # one f64 product; +inf when it overflows, 0 when it underflows
    s64 = seg.astype(np.float64)
    x = s64[i]
    with np.errstate(all="ignore"):
        dx, dy, dz = s64[:, 0] - x[0], s64[:, 1] - x[1], s64[:, 2] - x[2]
        approx = dx * dx + dy * dy + dz * dz
    approx = np.where(np.isfinite(approx), approx, np.inf)
    lim = r2
    if len(seg) > max_nn:
        lim = min(lim, float(np.partition(approx, max_nn - 1)[max_nn - 1]))
    cand = np.nonzero(approx <= lim * (1 + 1e-12))[0]
    out = []
    for j in cand:
        ux, uy, uz = float(s64[j, 0]) - float(x[0]), float(s64[j, 1]) - float(x[1]), float(s64[j, 2]) - float(x[2])
        d = fma(uz, uz, fma(uy, uy, ux * ux))
        if math.isfinite(d) and d < r2:
            out.append((d, int(j)))
    out.sort()
    return out[:max_nn]


def estimate_normals(xyz, offsets, radius, max_nn):
    """The whole call: f32 [n,3]."""
    assert K_MIN <= max_nn <= K_MAX and math.isfinite(radius) and radius > 0
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros((len(xyz), 3), np.float32)
    for s in range(len(offsets) - 1):
        seg = xyz[offsets[s]:offsets[s + 1]]
        for i in range(len(seg)):
            nbr = neighbours(seg, i, radius, max_nn)
            if len(nbr) < 3:
                out[offsets[s] + i] = (0.0, 0.0, 1.0)
                continue
            out[offsets[s] + i] = np.asarray(normal_of(scatter(seg, i, [j for _, j in nbr])), np.float64).astype(np.float32)
    return out
