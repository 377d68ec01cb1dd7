"""Partial views: the torch-tensor front end of cs_render_views (include/corsair_hip.h holds the specification,
tests/view_ref.py restates it bit for bit) and the host helpers that place its cameras.

The module is separate from backend.py, whose public names are pinned by the stream and stale-memory tables of the tests;
it keeps its own `torch` attribute and allocates every output uninitialised through it, so those tables' output-poisoning
proxy can be pointed at this module.  No CPU fallback: inputs must be device tensors.  The camera helpers are f64 numpy on
the host: no device trigonometry is needed.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, i64_array, ptr, stream_ptr

FAMILY = "view"


class ViewResult(NamedTuple):
    visible: torch.Tensor            # u8 [n] 0 / 1
    stat: torch.Tensor               # int32 [n_seg,4] (rows in front, rows in frame, rows visible, pixels with a finite depth)
    depth: Optional[torch.Tensor]    # f32 [n_seg,height,width], +inf where nothing was drawn; None unless asked for


def render_views(xyz, offsets, cams, width, height, focal, point_size, depth_tol, return_depth=False):
    """cs_render_views: segment s of xyz (f32 [n,3] device, host offset table) as camera s sees it -- cams f64 [n_seg,12]
    device, the rows R | t of the world -> camera map (look_at / view_cameras build them on the host), looking along +z
    through a pinhole of `focal` pixels into a width x height image.  Every row is a square of point_size world units; a
    row is visible when it is in front, in frame and less than depth_tol behind the nearest square over its centre pixel.
    The semantics are the header comment of cs_render_views.  Returns a ViewResult; no host wait."""
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise _lib.CorsairHipError("render_views: xyz must be a device tensor (the HIP path has no CPU fallback)")
    if xyz.dtype != torch.float32:
        raise TypeError(f"render_views: xyz must be torch.float32, got {xyz.dtype}")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("render_views: xyz must be [n, 3]")
    if len(offsets) < 1 or int(offsets[-1]) > xyz.shape[0]:
        raise ValueError("render_views: the offset table exceeds the array")
    n_seg = len(offsets) - 1
    if not isinstance(cams, torch.Tensor) or not cams.is_cuda:
        raise _lib.CorsairHipError("render_views: cams must be a device tensor")
    if cams.dtype != torch.float64:
        raise TypeError(f"render_views: cams must be torch.float64, got {cams.dtype}")
    if cams.numel() != 12 * n_seg:
        raise ValueError("render_views: one camera of 12 values per segment")
    xyz, cams = xyz.contiguous(), cams.contiguous()
    width, height = int(width), int(height)
    dev = xyz.device
    visible = torch.empty(xyz.shape[0], dtype=torch.uint8, device=dev)
    stat = torch.empty((n_seg, 4), dtype=torch.int32, device=dev)
    depth = torch.empty((n_seg, max(height, 0), max(width, 0)), dtype=torch.float32, device=dev) if return_depth else None
    check(_lib.load().cs_render_views(ptr(xyz), i64_array(offsets), n_seg, ptr(cams), width, height, float(focal),
                                      float(point_size), float(depth_tol), ptr(visible), ptr(depth), ptr(stat), stream_ptr()))
    return ViewResult(visible, stat, depth)


# ---- cameras (host, f64) -------------------------------------------------------------------------------------------------
def look_at(eye, center, up=None):
    """The 12 values R | t (rows) of the world -> camera map of a camera at `eye` that looks at `center` along its +z, with
    +x to the right and +y down the image.  up = None: the world axis with the smallest |component| of the viewing
    direction (the first such on ties), so no direction is degenerate."""
    eye, center = np.asarray(eye, np.float64).reshape(3), np.asarray(center, np.float64).reshape(3)
    f = center - eye
    n = np.linalg.norm(f)
    if not (n > 0 and np.isfinite(n)):
        raise ValueError("look_at: eye and center must be finite and distinct")
    f = f / n
    if up is None:
        up = np.zeros(3)
        up[int(np.argmin(np.abs(f)))] = 1.0
    up = np.asarray(up, np.float64).reshape(3)
    r = np.cross(f, up)
    rn = np.linalg.norm(r)
    if not (rn > 1e-12 and np.isfinite(rn)):
        raise ValueError("look_at: up is parallel to the viewing direction")
    r = r / rn
    d = np.cross(f, r)                      # exactly orthogonal to both; renormalised against the rounding of r and f
    d = d / np.linalg.norm(d)
    R = np.stack([r, d, f])
    t = -R @ eye
    return np.concatenate([R, t[:, None]], 1).reshape(12)


def focal_from_fov(width, fov_deg):
    """The focal length in pixels of a pinhole whose image of `width` pixels spans fov_deg degrees, in (0, 180)."""
    fov = float(fov_deg)
    if not 0.0 < fov < 180.0:
        raise ValueError("focal_from_fov: fov_deg must be in (0, 180), got %r" % (fov_deg,))
    return 0.5 * float(width) / math.tan(math.radians(0.5 * fov))


def view_cameras(lo, hi, directions, distance):
    """One camera per cloud, f64 [P,12]: lo, hi [P,3] are the clouds' bounding boxes, directions [P,3] (any length > 0) point
    from each box's midpoint to its camera; the eye stands at midpoint + distance x half diagonal x unit direction and looks
    at the midpoint."""
    lo, hi = np.asarray(lo, np.float64).reshape(-1, 3), np.asarray(hi, np.float64).reshape(-1, 3)
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    if not (len(lo) == len(hi) == len(d)):
        raise ValueError("view_cameras: one box and one direction per cloud")
    cams = np.empty((len(lo), 12), np.float64)
    for p in range(len(lo)):
        mid = 0.5 * (lo[p] + hi[p])
        half = 0.5 * np.linalg.norm(hi[p] - lo[p])
        n = np.linalg.norm(d[p])
        if not (n > 0 and np.isfinite(n) and half > 0 and np.isfinite(half)):
            raise ValueError("view_cameras: cloud %d has an empty box or no direction" % p)
        cams[p] = look_at(mid + float(distance) * half * (d[p] / n), mid)
    return cams
