"""Feature-matching RANSAC: torch-tensor front ends of cs_corr_mutual and cs_ransac_fm_batch
(include/corsair_hip.h holds the specification, tests/featmatch_ref.py restates it bit for bit).

The module is separate from backend.py, whose public names are pinned by the stream and stale-memory tables of the tests;
it keeps its own `torch` attribute and allocates every output uninitialised through it, so those tables' output-poisoning
proxy can be pointed at this module.  No CPU fallback: inputs must be device tensors.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib
from ._lib import check, i64_array, ptr, stream_ptr

FAMILY = "featmatch"


def _dev(t, dtype, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.CorsairHipError(f"{what} must be a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _xyz(t, offsets, what):
    t = _dev(t, torch.float32, what)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what} must be [n, 3]")
    if len(offsets) < 1 or int(offsets[-1]) > t.shape[0]:
        raise ValueError(f"{what}: the offset table exceeds the array")
    return t


class MutualResult(NamedTuple):
    src: torch.Tensor      # f32 [N0,3] query points of the kept rows, pair p from slot off0[p]
    tgt: torch.Tensor      # f32 [N0,3] their CAD points
    m: torch.Tensor        # int32 [P] rows kept per pair (device)
    stat: torch.Tensor     # int32 [P,2] (mutual matches -- valid rows with mutual=False --, 1 = the fallback was taken)


def mutual_correspondences(nn_fwd, nn_bwd, xyz0, off0, xyz1, off1, ransac_n=3, mutual=True):
    """cs_corr_mutual: the 1-NN correspondences of P (query, CAD) pairs that survive the mutual filter, compacted in the
    order of the query rows into the slots off0[p]... of two f32 [N0,3] arrays, with the counts on the device.  nn_fwd int32
    [N0] or [N0,1]: local CAD row per query row (backend.knn_feat at k = 1); nn_bwd likewise per CAD row (the same call with
    the sides swapped; may be None with mutual=False).  A pair with fewer than 3 * ransac_n mutual matches keeps all of its
    valid 1-NN rows (Open3D's fallback, decided on the device).  Returns a MutualResult; no host wait."""
    xyz0 = _xyz(xyz0, off0, "query points")
    xyz1 = _xyz(xyz1, off1, "CAD points")
    if len(off0) != len(off1):
        raise ValueError("mutual_correspondences: the two offset tables must describe the same pairs")
    nn_fwd = _dev(nn_fwd, torch.int32, "forward 1-NN list").reshape(-1)
    if nn_fwd.shape[0] < int(off0[-1]):
        raise ValueError("mutual_correspondences: the forward list is shorter than the query rows")
    if nn_bwd is not None:
        nn_bwd = _dev(nn_bwd, torch.int32, "backward 1-NN list").reshape(-1)
        if nn_bwd.shape[0] < int(off1[-1]):
            raise ValueError("mutual_correspondences: the backward list is shorter than the CAD rows")
    elif mutual:
        raise ValueError("mutual_correspondences: the mutual filter needs the backward list")
    n_pair = len(off0) - 1
    dev = xyz0.device
    src = torch.empty((xyz0.shape[0], 3), dtype=torch.float32, device=dev)
    tgt = torch.empty((xyz0.shape[0], 3), dtype=torch.float32, device=dev)
    m = torch.empty(n_pair, dtype=torch.int32, device=dev)
    stat = torch.empty((n_pair, 2), dtype=torch.int32, device=dev)
    check(_lib.load().cs_corr_mutual(ptr(nn_fwd), ptr(nn_bwd), ptr(xyz0), i64_array(off0), ptr(xyz1), i64_array(off1),
                                     n_pair, int(ransac_n), 1 if mutual else 0, ptr(src), ptr(tgt), ptr(m), ptr(stat),
                                     stream_ptr()))
    return MutualResult(src, tgt, m, stat)


class FmResult(NamedTuple):
    T: torch.Tensor          # f64 [P,4,4] the best hypothesis, the identity where none was found
    inliers: torch.Tensor    # int32 [P] its count
    rmse: torch.Tensor       # f64 [P] of those inliers
    found: torch.Tensor      # int32 [P] 0 / 1
    t_best: torch.Tensor     # int32 [P] its hypothesis index, -1 where none was found
    n_valid: torch.Tensor    # int32 [P] hypotheses that passed the checkers and the fit


def ransac_fm_batch(src, tgt, offsets, max_corr, m=None, ransac_n=3, edge_similarity=0.9, check_distance=True,
                    iterations=100000, seed=0):
    """cs_ransac_fm_batch: RANSAC over feature matches with Open3D's edge-length and distance checkers, `iterations`
    hypotheses of ransac_n (3 or 4) pairs per problem.  src, tgt f32 [M,3] device pairs; offsets: the host table of the
    problems' slots (mutual_correspondences' layout); m int32 [P] device counts of the pairs in those slots, None = full.
    The semantics are the header comment of cs_ransac_fm_batch.  The defaults are Open3D's and untuned.  Returns an FmResult;
    no host wait."""
    src = _dev(src, torch.float32, "source correspondences")
    tgt = _dev(tgt, torch.float32, "target correspondences")
    if src.shape != tgt.shape or src.dim() != 2 or src.shape[1] != 3:
        raise ValueError("ransac_fm_batch: correspondences must be two [M, 3] arrays of one shape")
    if len(offsets) < 1 or int(offsets[-1]) > src.shape[0]:
        raise ValueError("ransac_fm_batch: the offset table exceeds the correspondence arrays")
    n_prob = len(offsets) - 1
    if m is not None:
        m = _dev(m, torch.int32, "pair counts").reshape(-1)
        if m.shape[0] != n_prob:
            raise ValueError("ransac_fm_batch: one count per problem")
    dev = src.device
    T = torch.empty((n_prob, 4, 4), dtype=torch.float64, device=dev)
    stat = torch.empty((n_prob, 4), dtype=torch.int32, device=dev)
    rmse = torch.empty(n_prob, dtype=torch.float64, device=dev)
    check(_lib.load().cs_ransac_fm_batch(ptr(src), ptr(tgt), i64_array(offsets), ptr(m), n_prob, float(max_corr),
                                         int(ransac_n), float(edge_similarity), 1 if check_distance else 0, int(iterations),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(T), ptr(stat), ptr(rmse), stream_ptr()))
    return FmResult(T, stat[:, 2], rmse, stat[:, 0], stat[:, 1], stat[:, 3])
