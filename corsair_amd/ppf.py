"""Point-pair-feature voting: the torch-tensor front end of cs_ppf_batch (include/corsair_hip.h holds the
specification, tests/ppf_ref.py restates it bit for bit).  A pose of a scene against a model from oriented points alone: no
descriptors, no correspondence list.

The module is separate from backend.py, whose public names are pinned by the stream and stale-memory tables of the tests;
it keeps its own `torch` attribute and allocates every output uninitialised through it, so those tables' output-poisoning
proxy can be pointed at this module.  No CPU fallback: inputs must be device tensors.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check, i32_array, i64_array, ptr, stream_ptr

FAMILY = "ppf"
MAX_MODEL_ROWS = 4096      # rows of a model segment (its table of all ordered pairs is 192 MiB)
MAX_SCENE_ROWS = 16384     # rows of a scene segment
MAX_CAND = 64
DIST_STEP_FRACTION = 0.05  # of the model's bounding-box diagonal (Drost et al.'s sampling); untuned, no real scan measured


def _dev(t, dtype, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.CorsairHipError(f"{what} must be a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, got {t.dtype}")
    return t.contiguous()


class PpfResult(NamedTuple):
    T: torch.Tensor              # f64 [P,4,4] scene -> model, the identity where nothing was found
    T_inv: torch.Tensor          # f64 [P,4,4] model -> scene, the rigid inverse formed on the device
    found: torch.Tensor          # int32 [P] 0 / 1
    votes: torch.Tensor          # int32 [P] the votes of the winner's peak
    scene_row: torch.Tensor      # int32 [P] its reference, local to the scene segment, -1 where nothing was found
    model_row: torch.Tensor      # int32 [P] its model row, local to the model segment
    alpha_bin: torch.Tensor      # int32 [P] its bin of the in-plane angle
    count: torch.Tensor          # int32 [P] scene rows whose nearest model row lies strictly inside max_dist
    rank: torch.Tensor           # int32 [P] the winner's rank among the candidates
    n_ref: torch.Tensor          # int32 [P] the references of the problem
    rmse: torch.Tensor           # f64 [P] over the rows that count
    cand_T: torch.Tensor         # f64 [P,n_cand,4,4] every candidate's pose, the identity for an invalid one
    cand_stat: torch.Tensor      # int32 [P,n_cand,4] (votes, count, scene row, cell = model row * 30 + alpha bin)


def default_dist_step(model, moff, fraction=DIST_STEP_FRACTION):
    """`fraction` (0.05) of the bounding-box diagonal of every model segment: a list of floats, one per segment.  The rows
    that are not finite are left out; a segment without a finite row, or whose box is a point, gets 1.0.  The boxes are
    formed on the device and come to the host in ONE copy, which the call waits for."""
    n_seg = len(moff) - 1
    if n_seg <= 0:
        return []
    x = model[int(moff[0]):int(moff[-1])].double()
    lens = torch.as_tensor([int(moff[s + 1]) - int(moff[s]) for s in range(n_seg)], device=x.device)
    seg = torch.repeat_interleave(torch.arange(n_seg, device=x.device), lens, output_size=x.shape[0])
    finite = torch.isfinite(x).all(1, keepdim=True)
    idx = seg[:, None].expand(-1, 3)
    inf = torch.full((n_seg, 3), float("inf"), dtype=torch.float64, device=x.device)
    lo = inf.scatter_reduce(0, idx, torch.where(finite, x, inf[:1]), "amin")
    hi = (-inf).scatter_reduce(0, idx, torch.where(finite, x, -inf[:1]), "amax")
    diag = torch.linalg.norm(hi - lo, dim=1).cpu().tolist()
    return [fraction * d if 0.0 < d < float("inf") else 1.0 for d in diag]


def ppf_batch(scene, scene_normals, soff, model, model_normals, moff, scene_seg, model_seg, dist_step, max_dist, ref_step=5,
              n_cand=16):
    """cs_ppf_batch: problem p votes scene segment scene_seg[p] of `scene` (f32 [n,3], host offsets soff) against model
    segment model_seg[p] of `model` (host offsets moff); both sides carry ORIENTED normals (estimate_normals +
    orient_normals).  dist_step: one distance step per problem (a number = the same for all; default_dist_step gives one per
    model SEGMENT); max_dist: the radius of the verification count; every ref_step-th scene row is a reference; the n_cand
    references with the most votes are verified.  The semantics are the header comment of cs_ppf_batch.  The defaults are
    UNTUNED: no real scan was measured.  Returns a PpfResult; no host wait."""
    scene = _dev(scene, torch.float32, "scene points")
    scene_normals = _dev(scene_normals, torch.float32, "scene normals")
    model = _dev(model, torch.float32, "model points")
    model_normals = _dev(model_normals, torch.float32, "model normals")
    for a, b, what in ((scene, scene_normals, "scene"), (model, model_normals, "model")):
        if a.dim() != 2 or a.shape[1] != 3 or a.shape != b.shape:
            raise ValueError("ppf_batch: the %s points and normals must be two [n, 3] arrays of one shape" % what)
    n_prob = len(scene_seg)
    if len(model_seg) != n_prob:
        raise ValueError("ppf_batch: one scene segment and one model segment per problem")
    for seg, off, arr, what in ((scene_seg, soff, scene, "scene"), (model_seg, moff, model, "model")):
        if len(off) < 1 or int(off[-1]) > arr.shape[0]:
            raise ValueError("ppf_batch: the %s offset table exceeds the array" % what)
        if any(int(s) >= len(off) - 1 for s in seg):
            raise ValueError("ppf_batch: a %s segment id exceeds the offset table" % what)
    steps = [float(dist_step)] * n_prob if np.ndim(dist_step) == 0 else [float(v) for v in dist_step]
    if len(steps) != n_prob:
        raise ValueError("ppf_batch: one dist_step per problem")
    n_cand = int(n_cand)
    dev = scene.device
    rows = max(n_cand, 0)
    T = torch.empty((n_prob, 4, 4), dtype=torch.float64, device=dev)
    T_inv = torch.empty((n_prob, 4, 4), dtype=torch.float64, device=dev)
    stat = torch.empty((n_prob, 8), dtype=torch.int32, device=dev)
    rmse = torch.empty(n_prob, dtype=torch.float64, device=dev)
    cand_T = torch.empty((n_prob, rows, 4, 4), dtype=torch.float64, device=dev)
    cand_stat = torch.empty((n_prob, rows, 4), dtype=torch.int32, device=dev)
    check(_lib.load().cs_ppf_batch(ptr(scene), ptr(scene_normals), i64_array(soff), ptr(model), ptr(model_normals),
                                   i64_array(moff), i32_array(scene_seg), i32_array(model_seg), n_prob,
                                   (ctypes.c_double * max(n_prob, 1))(*steps), float(max_dist), int(ref_step), n_cand, ptr(T),
                                   ptr(T_inv), ptr(stat), ptr(rmse), ptr(cand_T), ptr(cand_stat), stream_ptr()))
    return PpfResult(T, T_inv, stat[:, 0], stat[:, 1], stat[:, 2], stat[:, 3], stat[:, 4], stat[:, 5], stat[:, 6], stat[:, 7], rmse,
                     cand_T, cand_stat)
