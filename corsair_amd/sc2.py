"""The compatibility-graph correspondence estimator: the torch-tensor front end of cs_sc2_batch
(include/corsair_hip.h holds the specification, tests/sc2_ref.py restates it bit for bit).

The module is separate from backend.py, whose public names are pinned by the stream and stale-memory tables of the tests;
it keeps its own `torch` attribute and allocates every output uninitialised through it, so those tables' output-poisoning
proxy can be pointed at this module.  No CPU fallback: inputs must be device tensors.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import check, i64_array, ptr, stream_ptr

FAMILY = "sc2"
MAX_SLOTS = 32768      # slots of one problem (its bit matrix is 128 MiB)


def _dev(t, dtype, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.CorsairHipError(f"{what} must be a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{what} must be {dtype}, got {t.dtype}")
    return t.contiguous()


class Sc2Result(NamedTuple):
    T: torch.Tensor              # f64 [P,4,4] the best seed's pose, the identity where none was found
    inliers: torch.Tensor        # int32 [P] its count
    rmse: torch.Tensor           # f64 [P] of those inliers
    found: torch.Tensor          # int32 [P] 0 / 1
    seed_row: torch.Tensor       # int32 [P] the row of the winning seed, -1 where none was found
    n_valid: torch.Tensor        # int32 [P] seeds with a consensus set of three rows or more and an accepted fit
    seed_rank: torch.Tensor      # int32 [P] the rank of the winning seed (0 = the largest degree), -1 where none was found
    seed_degree: torch.Tensor    # int32 [P] its degree in the compatibility graph
    mask: Optional[torch.Tensor]   # u8 [offsets[-1]] the best pose's inliers, None without return_inliers


def sc2_batch(src, tgt, offsets, max_corr, compat_dist, m=None, n_seeds=1024, k_consensus=20, return_inliers=False):
    """cs_sc2_batch: a pose per problem from the graph of pairwise length-compatible correspondences.  src, tgt f32 [M,3]
    device pairs; offsets: the host table of the problems' slots (mutual_correspondences' layout); m int32 [P] device counts
    of the pairs in those slots, None = full.  compat_dist: two pairs are compatible when their source and target distances
    differ by less than it; n_seeds: the rows of the largest degree that are tried (0 = every row); k_consensus: the rows a
    seed's fit takes beside the seed.  The semantics are the header comment of cs_sc2_batch.  The defaults are UNTUNED: no
    real scan was measured.  Returns an Sc2Result; no host wait."""
    src = _dev(src, torch.float32, "source correspondences")
    tgt = _dev(tgt, torch.float32, "target correspondences")
    if src.shape != tgt.shape or src.dim() != 2 or src.shape[1] != 3:
        raise ValueError("sc2_batch: correspondences must be two [M, 3] arrays of one shape")
    if len(offsets) < 1 or int(offsets[-1]) > src.shape[0]:
        raise ValueError("sc2_batch: the offset table exceeds the correspondence arrays")
    n_prob = len(offsets) - 1
    if m is not None:
        m = _dev(m, torch.int32, "pair counts").reshape(-1)
        if m.shape[0] != n_prob:
            raise ValueError("sc2_batch: one count per problem")
    dev = src.device
    T = torch.empty((n_prob, 4, 4), dtype=torch.float64, device=dev)
    stat = torch.empty((n_prob, 6), dtype=torch.int32, device=dev)
    rmse = torch.empty(n_prob, dtype=torch.float64, device=dev)
    mask = torch.empty(max(int(offsets[-1]), 0), dtype=torch.uint8, device=dev) if return_inliers else None
    check(_lib.load().cs_sc2_batch(ptr(src), ptr(tgt), i64_array(offsets), ptr(m), n_prob, float(compat_dist),
                                   float(max_corr), int(n_seeds), int(k_consensus), ptr(T), ptr(stat), ptr(rmse), ptr(mask),
                                   stream_ptr()))
    return Sc2Result(T, stat[:, 2], rmse, stat[:, 0], stat[:, 1], stat[:, 3], stat[:, 4], stat[:, 5], mask)
