"""cs_render_views restated bit for bit (the header comment of include/corsair_hip.h is the specification): every operation
one IEEE f64 operation in the header's order, the fused ones through an exact rational fma.  Plain Python floats per row; the
depth buffer is a numpy f64 image whose minimum is, like the device's u64 atomicMin, free of the order of the rows."""
import math

import numpy as np

INF = float("inf")


def fma(a, b, c):
    """fma(a, b, c) rounded once: tests/icp_ref.py's exact rational fma without its gcd reductions (the integer division is
    rounded correctly by CPython).  tests/test_view_cpu.py compares the two."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    num, den = na * nb * dc + nc * da * db, da * db * dc
    if num == 0:                     # the sign of an exact zero: that of the sum of the (rounded) terms
        return a * b + c
    try:
        return num / den
    except OverflowError:
        return INF if num > 0 else -INF


def _div(a, b):
    """a / b in IEEE arithmetic for b > 0 finite (Python raises where the result overflows)."""
    try:
        return a / b
    except OverflowError:
        return INF if a > 0 else -INF


def _edge(a, hi):
    f = math.floor(a) if math.isfinite(a) else a
    f = -1.0 if f < -1.0 else float(f)
    f = float(hi) if f > hi else f
    return int(f)


def row(p, cam, width, height, focal, point_size):
    """One row: None when it is not in front, else (Z, in frame, cu, cv, xa, xb, ya, yb) with the footprint clipped to the
    image (xa > xb or ya > yb: it covers nothing)."""
    x, y, z = float(p[0]), float(p[1]), float(p[2])
    P = [fma(cam[4 * c + 2], z, fma(cam[4 * c + 1], y, fma(cam[4 * c], x, cam[4 * c + 3]))) for c in range(3)]
    Z = P[2]
    if not (math.isfinite(P[0]) and math.isfinite(P[1]) and math.isfinite(P[2]) and Z > 0.0):
        return None
    w, hgt = float(width), float(height)
    u = fma(focal, _div(P[0], Z), 0.5 * w)
    v = fma(focal, _div(P[1], Z), 0.5 * hgt)
    hh = _div((0.5 * focal) * point_size, Z)
    h = hh if hh < 16.0 else 16.0
    fu = math.floor(u) if math.isfinite(u) else u
    fv = math.floor(v) if math.isfinite(v) else v
    frame = 0.0 <= fu < w and 0.0 <= fv < hgt
    xa, xb = max(_edge(u - h, w), 0), min(_edge(u + h, w), width - 1)
    ya, yb = max(_edge(v - h, hgt), 0), min(_edge(v + h, hgt), height - 1)
    return Z, frame, int(fu) if frame else 0, int(fv) if frame else 0, xa, xb, ya, yb


def render_one(xyz, cam, width, height, focal, point_size, depth_tol):
    """One segment: (visible u8 [m], depth f64 [height,width], stat [4])."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    cam = [float(c) for c in np.asarray(cam, np.float64).reshape(12)]
    focal, point_size, depth_tol = float(focal), float(point_size), float(depth_tol)
    zbuf = np.full((height, width), np.inf, np.float64)
    rows = [row(p, cam, width, height, focal, point_size) for p in xyz]
    for r in rows:
        if r is not None:
            Z, _, _, _, xa, xb, ya, yb = r
            if xa <= xb and ya <= yb:
                np.minimum(zbuf[ya:yb + 1, xa:xb + 1], Z, out=zbuf[ya:yb + 1, xa:xb + 1])
    visible = np.zeros(len(xyz), np.uint8)
    front = frame = 0
    for i, r in enumerate(rows):
        if r is None:
            continue
        front += 1
        if r[1]:
            frame += 1
            visible[i] = 1 if r[0] - float(zbuf[r[3], r[2]]) < depth_tol else 0
    return visible, zbuf, [front, frame, int(visible.sum()), int(np.isfinite(zbuf).sum())]


def render(xyz, off, cams, width, height, focal, point_size, depth_tol):
    """The call: (visible u8 [n], depth f32 [n_seg,height,width], stat int32 [n_seg,4]).  Rows outside the offset table keep 0."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64).reshape(-1, 12)
    n_seg = len(off) - 1
    visible = np.zeros(len(xyz), np.uint8)
    depth = np.empty((n_seg, height, width), np.float32)
    stat = np.zeros((n_seg, 4), np.int32)
    for s in range(n_seg):
        a, b = int(off[s]), int(off[s + 1])
        vis, z, st = render_one(xyz[a:b], cams[s], width, height, focal, point_size, depth_tol)
        visible[a:b] = vis
        with np.errstate(over="ignore"):
            depth[s] = z.astype(np.float32)
        stat[s] = st
    return visible, depth, stat
