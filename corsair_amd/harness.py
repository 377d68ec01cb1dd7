"""The build's counterpart of the hot part of the reference's evaluation.py:207-383:
catalog / query feature extraction, descriptor retrieval, symmetry-aided registration and the metric
aggregation, on the MI355X-native library.  Inputs are synthetic or arbitrary f32 / f64 clouds;
dataset parsing, checkpoints-on-disk and the GUI of the reference are out of scope.

Differences in structure (not in results) from the reference loops:
  * voxelisation + collate run on the GPU (cs_voxelize) instead of in DataLoader workers;
  * per-sample feature splits are CSR offsets, not 32 boolean-mask gathers per batch
    (evaluation.py:226-229);
  * registrations are batched (registration.sym_pose_batch) instead of one Python iteration each.
"""
from __future__ import annotations

import math
import os

from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

from . import backend as B
from . import engine as E
from . import estimators
from . import registration as R
from .utils.eval_pose import eval_pose

ICP_KERNEL_NAMES = tuple(B.ICP_KERNELS)       # "l2", "huber", "cauchy", "tukey"
VERIFY_SCORES = ("symmetric", "forward")
VERIFY_MAX_K = 32
SCAN_FILTERS = ("none", "statistical", "radius", "cluster")
SCAN_PLANES = ("none", "remove")
SCAN_FILTER_MIN_ROWS = 10      # ransac_n: a cloud the filter would leave with fewer rows keeps all of them


@dataclass
class Config:
    """Hyper-parameters of evaluation.py:41-65 (dataclass defaults there, not CLI flags)."""
    voxel_size: float = 0.03
    k_nn: int = 5
    max_corr: float = 0.2
    random_seed: int = 31
    n_points: int = 10000
    batch_size: int = 32
    # clouds per forward of the network when the caller gives no batch size of its own.  The reference's DataLoader hands the
    # network 32 (= batch_size); the rows of an eval-mode forward do not depend on what else is in the batch, and a 32-cloud
    # batch leaves the stride-4 / 8 layers with fewer workgroups than the chip has CUs: 128 here
    embed_batch_size: int = 128
    ransac_max_iter: int = 100000
    ransac_confidence: float = 0.999
    # point-to-point ICP refinement of the kept pose (registration.sym_pose_batch, cs_icp_batch): updates at most; 0 = off,
    # the reference's behaviour.  icp_max_dist = 0.0 means 2 * voxel_size -- a plausible radius for voxel centres one cell
    # apart that NOBODY HAS TUNED; set it explicitly for real data
    icp_max_iter: int = 0
    icp_max_dist: float = 0.0
    # "point" (cs_icp_batch) or "plane" (cs_icp_plane_batch on the normals of the CAD voxels, cs_estimate_normals over
    # icp_normal_k neighbours).  16 is UNTUNED: 8 and 16 behaved alike in the experiment that motivated it
    # "gicp" (cs_icp_gicp_batch): plane-to-plane Generalized ICP on the normals of BOTH clouds, the CAD voxels' as
    # for "plane" (a catalog's are computed once), the query voxels' estimated per batch with the same icp_normal_k /
    # icp_normal_radius.  gicp_epsilon in [2^-10, 1] is the covariance floor along the normal: 1e-3 is Open3D's default and
    # NOBODY HAS TUNED it here, nor icp_normal_k for this estimation.  No robust kernel, no scale
    icp_estimation: str = "point"
    gicp_epsilon: float = 1e-3
    icp_normal_k: int = 16
    # 0.0 = those k nearest rows (the default); > 0: the at most icp_normal_k nearest rows strictly inside this radius
    # (cs_estimate_normals_hybrid), in the units of the clouds.  NO RADIUS HAS BEEN TUNED
    icp_normal_radius: float = 0.0
    # robust kernel of the plane estimation: "l2" (none), "huber", "cauchy" or "tukey" (cs_icp_plane_robust_batch).
    # icp_kernel_scale = 0.0 means 1 * voxel_size -- the size of the residual a voxel grid leaves on a matching surface,
    # which NOBODY HAS TUNED; set it explicitly for real data
    icp_kernel: str = "l2"
    icp_kernel_scale: float = 0.0
    # the refinement also fits an isotropic scale of the query (cs_icp_scale_batch), either estimation, no robust
    # kernel.  A query whose accumulated scale would leave icp_scale_bounds stops before that update; (0.5, 2.0) is UNTUNED
    icp_with_scaling: bool = False
    icp_scale_bounds: tuple = (0.5, 2.0)
    # the correspondence estimator of stage 4: "ransac" (cs_ransac_batch, the reference's) or "fgr" (cs_fgr_batch, Fast Global
    # Registration).  fgr_mu_floor is Open3D's maximum_correspondence_distance in units of the normalised frame
    # (the clouds' radius = 1); 0.025 is Open3D's default and NOBODY HAS TUNED it here
    registration: str = "ransac"
    fgr_mu_floor: float = 0.025
    # candidate verification (run_eval): the first verify_top_k retrieved CADs of every query are registered and
    # re-ranked by the Chamfer distance of their registered pose (cs_chamfer_2dir).  0 and 1 = off (the descriptor top-1 alone,
    # the reference's behaviour), 2 .. 32 are valid.  verify_score "symmetric" = forward + backward (the sum the reference's
    # evaluate_retrieval forms), "forward" = posed query -> CAD alone, meant for scans that see a fraction of the object.
    # NEITHER DEFAULT HAS BEEN TUNED on real scans: no K is recommended, and which score suits partial scans is not measured
    verify_top_k: int = 0
    verify_score: str = "symmetric"
    # cleaning of RAW QUERY scans before the network sees them (embed_clouds(scan_filter=True)), on the f32 origins
    # after voxelisation: "none" (the default, the reference's behaviour), "statistical" (cs_knn_mean_dist +
    # cs_outlier_statistical, Open3D's remove_statistical_outlier) or "radius" (cs_outlier_radius, remove_radius_outlier).
    # scan_filter_k = 20 and scan_filter_std = 2.0 are the values of Open3D's tutorial, UNTUNED here
    scan_filter: str = "none"
    scan_filter_k: int = 20
    scan_filter_std: float = 2.0
    # in VOXELS (the radius is scan_filter_radius * voxel_size): 2.5 is the radius inside which DESIGN 15 counted 12 - 24 rows
    # of a voxelised surface.  UNTUNED, and so is scan_filter_min_nb = 4 (a row is kept with MORE than that many rows inside
    # the radius, itself included)
    scan_filter_radius: float = 2.5
    scan_filter_min_nb: int = 4
    # "cluster" (cs_dbscan + cs_cluster_largest, Open3D's cluster_dbscan): only the rows of the scan's LARGEST
    # cluster stay, which also drops a dense patch of a neighbouring object that neither outlier filter can remove.
    # scan_filter_eps is in VOXELS (eps = scan_filter_eps * voxel_size) and a row is a core row with scan_filter_min_points
    # rows inside eps, itself included: 2.5 and 5 are the radius filter's defaults (its keep rule, count > 4).  Both are
    # UNTUNED, NO REAL SCAN MEASURED
    scan_filter_eps: float = 2.5
    scan_filter_min_points: int = 5
    # removal of the SUPPORT PLANE (the floor a scanned object stands on, or the wall behind it) from raw query scans, a step
    # of its own BEFORE scan_filter (cs_segment_plane, Open3D's segment_plane): "none" (the default) or "remove".
    # scan_plane_dist is in VOXELS, scan_plane_iters the number of hypotheses.  The dominant plane is removed only when it
    # is a support plane (is_support_plane): it holds scan_plane_min_share of the finite rows, at most scan_plane_max_below
    # of the other rows lie beyond it, and -- when scan_plane_up is given -- its normal lies within scan_plane_max_tilt
    # degrees of that direction.  Without scan_plane_up a bare table top seen from above passes the first two rules and is
    # removed: that is why the step is off by default.  ALL OF THEM UNTUNED, NO REAL SCAN MEASURED
    scan_plane: str = "none"
    scan_plane_dist: float = 1.0
    scan_plane_iters: int = 1024
    scan_plane_min_share: float = 0.2
    scan_plane_max_below: float = 0.02
    scan_plane_up: Optional[Tuple[float, float, float]] = None
    scan_plane_max_tilt: float = 30.0

    def check_scan_plane(self):
        if self.scan_plane not in SCAN_PLANES:
            raise ValueError("Config.scan_plane must be one of %s, got %r" % (SCAN_PLANES, self.scan_plane))
        if not 0.0 < float(self.scan_plane_dist) < float("inf"):
            raise ValueError("Config.scan_plane_dist must be positive and finite, got %r" % (self.scan_plane_dist,))
        it = self.scan_plane_iters
        if isinstance(it, bool) or not isinstance(it, (int, np.integer)) or not 1 <= int(it) <= 65536:
            raise ValueError("Config.scan_plane_iters must be an integer in [1, 65536], got %r" % (it,))
        if not 0.0 <= float(self.scan_plane_min_share) <= 1.0:
            raise ValueError("Config.scan_plane_min_share must lie in [0, 1], got %r" % (self.scan_plane_min_share,))
        if not 0.0 <= float(self.scan_plane_max_below) <= 1.0:
            raise ValueError("Config.scan_plane_max_below must lie in [0, 1], got %r" % (self.scan_plane_max_below,))
        up = self.scan_plane_up
        if up is not None:
            try:
                v = [float(x) for x in up]
            except (TypeError, ValueError):
                v = []
            if len(v) != 3 or not all(math.isfinite(x) for x in v) or not any(x != 0.0 for x in v):
                raise ValueError("Config.scan_plane_up must be None or three finite numbers, not all zero, got %r" % (up,))
        if not 0.0 < float(self.scan_plane_max_tilt) <= 90.0:
            raise ValueError("Config.scan_plane_max_tilt must lie in (0, 90] degrees, got %r" % (self.scan_plane_max_tilt,))

    def check_scan_filter(self):
        if self.scan_filter not in SCAN_FILTERS:
            raise ValueError("Config.scan_filter must be one of %s, got %r" % (SCAN_FILTERS, self.scan_filter))
        k = self.scan_filter_k
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 2 <= int(k) <= 32:
            raise ValueError("Config.scan_filter_k must be an integer in [2, 32], got %r" % (k,))
        if not 0.0 <= float(self.scan_filter_std) < float("inf"):
            raise ValueError("Config.scan_filter_std must be finite and >= 0, got %r" % (self.scan_filter_std,))
        if not 0.0 < float(self.scan_filter_radius) < float("inf"):
            raise ValueError("Config.scan_filter_radius must be positive and finite, got %r" % (self.scan_filter_radius,))
        nb = self.scan_filter_min_nb
        if isinstance(nb, bool) or not isinstance(nb, (int, np.integer)) or int(nb) < 0:
            raise ValueError("Config.scan_filter_min_nb must be an integer >= 0, got %r" % (nb,))
        if not 0.0 < float(self.scan_filter_eps) < float("inf"):
            raise ValueError("Config.scan_filter_eps must be positive and finite, got %r" % (self.scan_filter_eps,))
        mp = self.scan_filter_min_points
        if isinstance(mp, bool) or not isinstance(mp, (int, np.integer)) or int(mp) < 1:
            raise ValueError("Config.scan_filter_min_points must be an integer >= 1, got %r" % (mp,))

    def verify_k(self):
        """Candidates per query that are registered and re-ranked; 0 when the verification is off."""
        self.check_verify()
        return int(self.verify_top_k) if int(self.verify_top_k) > 1 else 0

    def check_verify(self):
        k = self.verify_top_k
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= VERIFY_MAX_K:
            raise ValueError("Config.verify_top_k must be an integer in [0, %d] (0 and 1 = off), got %r" % (VERIFY_MAX_K, k))
        if self.verify_score not in VERIFY_SCORES:
            raise ValueError("Config.verify_score must be one of %s, got %r" % (VERIFY_SCORES, self.verify_score))

    def icp_distance(self):
        return self.icp_max_dist if self.icp_max_dist > 0 else 2.0 * self.voxel_size

    def icp_scale(self):
        return self.icp_kernel_scale if self.icp_kernel_scale > 0 else 1.0 * self.voxel_size

    def check_icp(self):
        for e in estimators.TABLE:
            if not e.wired and self.registration == e.name:
                raise ValueError("Config.registration %r (%s, DESIGN %d) is not wired into the harness, the sharded evaluation "
                                 "or the cache format: use registration.sym_pose_batch or shapenet_eval"
                                 % (e.name, e.what, e.design))
        estimators.lookup(self.registration, "Config.registration", estimators.WIRED)
        if not (0.0 < float(self.fgr_mu_floor) < float("inf")):
            raise ValueError("Config.fgr_mu_floor must be positive and finite, got %r" % (self.fgr_mu_floor,))
        if self.icp_estimation not in ("point", "plane", "gicp"):
            raise ValueError("Config.icp_estimation must be 'point', 'plane' or 'gicp', got %r" % (self.icp_estimation,))
        if self.icp_estimation == "gicp":
            if self.icp_kernel != "l2" or self.icp_with_scaling:
                raise ValueError("Config.icp_estimation 'gicp' with a robust icp_kernel or icp_with_scaling is out of scope")
            if not (np.isfinite(float(self.gicp_epsilon)) and 2.0 ** -10 <= float(self.gicp_epsilon) <= 1.0):
                raise ValueError("Config.gicp_epsilon must lie in [2^-10, 1], got %r" % (self.gicp_epsilon,))
        if self.icp_kernel not in ICP_KERNEL_NAMES:
            raise ValueError("Config.icp_kernel must be one of %s, got %r" % (ICP_KERNEL_NAMES, self.icp_kernel))
        if self.icp_kernel != "l2" and self.icp_estimation != "plane":
            raise ValueError("Config.icp_kernel %r needs icp_estimation = 'plane'" % (self.icp_kernel,))
        if self.icp_with_scaling:
            if self.icp_kernel != "l2":
                raise ValueError("Config.icp_with_scaling with a robust icp_kernel (%r) is out of scope" % (self.icp_kernel,))
            if self.icp_max_iter <= 0:
                raise ValueError("Config.icp_with_scaling needs icp_max_iter > 0 (the refinement is off)")
            lo, hi = (float(v) for v in self.icp_scale_bounds)
            if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= 1.0 <= hi):
                raise ValueError("Config.icp_scale_bounds must be finite with 0 < min <= 1 <= max, got %r"
                                 % (self.icp_scale_bounds,))
        if not 3 <= int(self.icp_normal_k) <= 32:
            raise ValueError("Config.icp_normal_k must lie in [3, 32], got %r" % (self.icp_normal_k,))
        if not 0 <= float(self.icp_normal_radius) < float("inf"):
            raise ValueError("Config.icp_normal_radius must be finite and >= 0 (0 = k-NN), got %r"
                             % (self.icp_normal_radius,))

    def normal_radius(self):
        return float(self.icp_normal_radius) if self.icp_normal_radius > 0 else None

    def icp_plane(self):
        """True when the run refines with the point-to-plane or the plane-to-plane (GICP) estimation (and so needs the CAD
        voxels' normals)."""
        self.check_icp()
        return self.icp_max_iter > 0 and self.icp_estimation in ("plane", "gicp")


@dataclass
class EmbeddedSet:
    """Features of a set of clouds, packed: voxel features F [sumN,16], origins [sumN,3], offsets
    (host list, len n+1), global descriptors [n,256] (row-normalised); optionally the normals [sumN,3] of the origins
    (backend.estimate_normals; the point-to-plane refinement's targets carry them)."""
    F: torch.Tensor
    origin: torch.Tensor
    offsets: list
    desc: torch.Tensor
    normal: torch.Tensor = None

    def __len__(self):
        return len(self.offsets) - 1

    def gather(self, ids):
        """Sub-set (with repetition) as a new packed set; device-side row gather."""
        dev = self.F.device
        off = np.asarray(self.offsets, dtype=np.int64)
        ids = np.asarray(ids, dtype=np.int64)
        lens = off[ids + 1] - off[ids]
        new_off = np.concatenate([[0], np.cumsum(lens)])
        starts = torch.from_numpy(off[ids] - new_off[:-1]).to(dev)
        rows = torch.arange(int(new_off[-1]), device=dev) + torch.repeat_interleave(
            starts, torch.from_numpy(lens).to(dev), output_size=int(new_off[-1]))
        return EmbeddedSet(self.F[rows], self.origin[rows], new_off.tolist(),
                           self.desc[torch.from_numpy(ids).to(dev)],
                           None if self.normal is None else self.normal[rows])


def is_support_plane(stat_row, plane_row, cfg):
    """Whether the plane cs_segment_plane found (one row of its stat and of its plane) is a SUPPORT plane under cfg, pure
    Python: (a) its final inliers are at least scan_plane_min_share of the finite rows, (b) at most scan_plane_max_below of
    the other finite rows lie beyond it (n_neg; the normal points to the side most rows are on), (c) when scan_plane_up is
    given, the normal lies within scan_plane_max_tilt degrees of it.  Rules (a) and (b) alone cannot tell a floor from a
    bare table top seen from above: both are one-sided."""
    found, _, _, _, final, n_pos, n_neg, finite = (int(v) for v in stat_row)
    if not found:
        return False
    if final < float(cfg.scan_plane_min_share) * finite:
        return False
    if n_neg > float(cfg.scan_plane_max_below) * (n_pos + n_neg):
        return False
    if cfg.scan_plane_up is not None:
        up = [float(v) for v in cfg.scan_plane_up]
        dot = sum(float(plane_row[a]) * up[a] for a in range(3)) / math.sqrt(sum(v * v for v in up))
        if dot < math.cos(math.radians(float(cfg.scan_plane_max_tilt))):
            return False
    return True


class Pipeline:
    def __init__(self, state_dict, embedding_state_dict, device="cuda", config=None):
        self.cfg = config or Config()
        self.device = torch.device(device)
        self.engine = E.ResUNetEngine(state_dict, embedding_state_dict, device=self.device)
        self.scan_filter_stat = {"rows_in": 0, "rows_kept": 0, "clouds_skipped": 0}     # filter_scan adds to it
        self.scan_plane_stat = {"clouds": 0, "planes_removed": 0, "rows_removed": 0}    # remove_plane adds to it

    # ---- feature extraction (evaluation.py:213-269) ----------------------------------------------
    def embed_batch(self, xyz, offsets, scan_filter=False):
        """xyz f32 [n,3] device (concatenated raw clouds, already normalised), offsets host list.
        Returns an EmbeddedSet for the batch."""
        return self.embed_batch_raw(xyz, offsets, self.cfg.voxel_size, scan_filter)

    def filter_scan(self, origin, offsets, voxel_size):
        """The configured scan filter (Config.scan_filter) on packed f32 origins: (idx int64 [m] device or None
        when every row stays, new host offsets).  A cloud that would be left with fewer than SCAN_FILTER_MIN_ROWS rows keeps
        all of its rows.  Adds to self.scan_filter_stat.  One host wait (backend.select_rows)."""
        c = self.cfg
        c.check_scan_filter()
        if c.scan_filter == "statistical":
            mask, _ = B.outlier_statistical(origin, offsets, int(c.scan_filter_k), float(c.scan_filter_std))
        elif c.scan_filter == "cluster":
            label, _ = B.dbscan(origin, offsets, float(c.scan_filter_eps) * float(voxel_size), int(c.scan_filter_min_points))
            mask, _ = B.cluster_largest(label, offsets)
        else:
            mask, _ = B.outlier_radius(origin, offsets, float(c.scan_filter_radius) * float(voxel_size),
                                       int(c.scan_filter_min_nb))
        idx, new_off = B.select_rows(mask, offsets)
        short = [p for p in range(len(offsets) - 1)
                 if new_off[p + 1] - new_off[p] < SCAN_FILTER_MIN_ROWS and new_off[p + 1] - new_off[p] < offsets[p + 1] - offsets[p]]
        if short:
            for p in short:
                mask[offsets[p]:offsets[p + 1]] = True
            idx, new_off = B.select_rows(mask, offsets)
        st = self.scan_filter_stat
        st["rows_in"] += int(offsets[-1] - offsets[0])
        st["rows_kept"] += int(new_off[-1])
        st["clouds_skipped"] += len(short)
        return (None if new_off[-1] == offsets[-1] - offsets[0] else idx), new_off

    def remove_plane(self, origin, offsets, voxel_size):
        """The support-plane step (Config.scan_plane) on packed f32 origins: (idx int64 [m] device or None when every
        row stays, new host offsets).  The final inliers of cs_segment_plane leave every cloud whose plane is_support_plane
        accepts, unless the cloud would be left with fewer than SCAN_FILTER_MIN_ROWS rows.  Adds to self.scan_plane_stat.
        Two host waits: stat and plane come to the host for the rule, then backend.select_rows."""
        c = self.cfg
        c.check_scan_plane()
        inlier, plane, stat = B.segment_plane(origin, offsets, float(c.scan_plane_dist) * float(voxel_size),
                                              int(c.scan_plane_iters))
        stat_h, plane_h = stat.cpu().tolist(), plane.cpu().tolist()
        n_seg = len(offsets) - 1
        drop = [p for p in range(n_seg)
                if is_support_plane(stat_h[p], plane_h[p], c) and (offsets[p + 1] - offsets[p]) - stat_h[p][4] >= SCAN_FILTER_MIN_ROWS]
        st = self.scan_plane_stat
        st["clouds"] += n_seg
        st["planes_removed"] += len(drop)
        st["rows_removed"] += sum(stat_h[p][4] for p in drop)
        if not drop:
            return None, [int(o) - int(offsets[0]) for o in offsets]
        keep = torch.ones(inlier.shape[0], dtype=torch.bool, device=inlier.device)
        for p in drop:
            keep[offsets[p]:offsets[p + 1]] = ~inlier[offsets[p]:offsets[p + 1]]
        return B.select_rows(keep, offsets)

    def embed_batch_raw(self, xyz, offsets, voxel_size, scan_filter=False):
        """xyz f32 or f64: quantised in its own type (backend.voxelize); the kept points of an f64 cloud
        become f32 origins AFTER the selection (evaluation-shapenet.py:103-105; the collate of
        datasets/ChairDataset.py:204-237 does the same to the f64 `rot_coords`).  scan_filter: when the configuration
        names a filter (Config.scan_filter), it runs on those origins and the voxels it drops never reach the network;
        the support-plane step (Config.scan_plane) runs before it under the same gate."""
        keep, grid, out_off = B.voxelize(xyz, offsets, voxel_size)
        origin = xyz[keep].to(torch.float32)
        if scan_filter and self.cfg.scan_plane != "none":
            sel, out_off = self.remove_plane(origin, out_off, voxel_size)
            if sel is not None:
                origin, grid = origin[sel], grid[sel]
        if scan_filter and self.cfg.scan_filter != "none":
            sel, out_off = self.filter_scan(origin, out_off, voxel_size)
            if sel is not None:
                origin, grid = origin[sel], grid[sel]
        feats = torch.ones((grid.shape[0], 1), dtype=torch.float32, device=xyz.device)
        out, feat8, maps = self.engine.forward(grid, feats, n_batch=len(offsets) - 1)
        return EmbeddedSet(out, origin, out_off, self._descriptors(feat8, maps, len(offsets) - 1))

    def _descriptors(self, feat8, maps, n):
        """Global descriptors [n,256]; a checkpoint without `embedding_state_dict` (evaluation-shapenet.py:283-289 loads
        the network only) gives an empty [n,0] block: registration needs none, retrieval would fail loudly."""
        if self.engine.emb is None:
            return torch.zeros((n, 0), dtype=torch.float32, device=feat8.device)
        return self.engine.embed(feat8, maps, n)

    def embed_groups(self, groups, voxel_size=None):
        """One forward over several groups of clouds that differ in type: groups = [(xyz, offsets), ...], each
        quantised by its own cs_voxelize / cs_voxelize_f64 call, then collated into one batch (sample index =
        position in the concatenation of the groups).  evaluation-shapenet.py:299-310 does this for a model
        (f32, load_pc) and its posed copy (f64, generate_test_pc_pair) in every forward."""
        vs = self.cfg.voxel_size if voxel_size is None else voxel_size
        grids, origins, out_off, base = [], [], [0], 0
        for xyz, offsets in groups:
            keep, grid, off = B.voxelize(xyz, offsets, vs)
            if base:
                grid = grid.clone()
                grid[:, 0] += base
            grids.append(grid)
            origins.append(xyz[keep].to(torch.float32))
            out_off += [out_off[-1] + int(o) for o in off[1:]]
            base += len(offsets) - 1
        grid = torch.cat(grids)
        feats = torch.ones((grid.shape[0], 1), dtype=torch.float32, device=grid.device)
        out, feat8, maps = self.engine.forward(grid, feats, n_batch=base)
        return EmbeddedSet(out, torch.cat(origins), out_off, self._descriptors(feat8, maps, base))

    def embed_clouds(self, clouds, batch_size=None, scan_filter=False):
        """clouds: list of f32 or f64 [n,3] NumPy arrays (host), one type per call: a cloud is quantised in
        the type it arrives in, so promoting or narrowing here would move points across voxel boundaries.
        Forwards of batch_size clouds (default cfg.embed_batch_size; the reference's DataLoader: 32 -- same rows either way).
        scan_filter: the clouds are raw scans, cleaned by the configured filter (Config.scan_filter; "none" = nothing runs)."""
        bs = batch_size or self.cfg.embed_batch_size
        kinds = {np.asarray(c).dtype for c in clouds}
        if len(kinds) > 1 or not kinds <= {np.dtype(np.float32), np.dtype(np.float64)}:
            raise TypeError("embed_clouds: clouds must all be float32 or all be float64, got %s" % sorted(map(str, kinds)))
        sets = []
        for i in range(0, len(clouds), bs):
            chunk = clouds[i:i + bs]
            xyz = torch.from_numpy(np.concatenate(chunk, 0)).to(self.device)
            off = np.concatenate([[0], np.cumsum([len(c) for c in chunk])]).tolist()
            sets.append(self.embed_batch(xyz, off, True) if scan_filter else self.embed_batch(xyz, off))
        return concat_sets(sets)

    def voxel_counts(self, clouds, chunk=64):
        """Voxels each cloud quantises to (cs_voxelize / cs_voxelize_f64 only): the weight multi-GPU runs balance their
        shards by (N1 varies 1.6 k - 8 k per model)."""
        counts = []
        for i in range(0, len(clouds), chunk):
            part = [np.asarray(c) for c in clouds[i:i + chunk]]
            off = np.concatenate([[0], np.cumsum([len(c) for c in part])]).tolist()
            _, _, out_off = B.voxelize(torch.from_numpy(np.concatenate(part, 0)).to(self.device), off, self.cfg.voxel_size)
            counts += [int(v) for v in np.diff(out_off)]
        return counts

    # ---- retrieval (evaluation.py:272-283) ----------------------------------------------------------
    def retrieve(self, q_desc, lib_desc, k):
        return B.l2_topk(q_desc, lib_desc, k)

    # ---- registration (evaluation.py:297-331) -----------------------------------------------------
    def register(self, queries, cads, syms, anchor_ids=None, use_symmetry=True, force_gate=False,
                 query_anchors=None):
        """queries / cads: EmbeddedSets of equal length (pair p = query p vs cad p)."""
        c = self.cfg
        return R.sym_pose_batch(queries.F, queries.origin, queries.offsets, cads.F, cads.origin,
                                cads.offsets, syms, c.k_nn, c.max_corr, 0, anchor_ids, 100,
                                c.ransac_max_iter, c.ransac_confidence, use_symmetry, force_gate,
                                query_anchors, c.icp_max_iter, c.icp_distance() if c.icp_max_iter > 0 else None,
                                c.icp_estimation, c.icp_normal_k, cads.normal, c.normal_radius(),
                                icp_with_scaling=c.icp_with_scaling,
                                icp_scale_bounds=tuple(c.icp_scale_bounds) if c.icp_with_scaling else None,
                                icp_kernel=c.icp_kernel, icp_kernel_scale=c.icp_scale() if c.icp_kernel != "l2" else None,
                                registration=c.registration, fgr_mu_floor=c.fgr_mu_floor, gicp_epsilon=c.gicp_epsilon)

    def with_normals(self, s):
        """`s` with the normals of its origins (one cs_estimate_normals call over the whole set, or one
        cs_estimate_normals_hybrid call when the configuration has an icp_normal_radius) when the configuration refines
        point-to-plane or plane-to-plane (GICP) and the set has none yet; `s` itself otherwise."""
        if not self.cfg.icp_plane() or s.normal is not None:
            return s
        return EmbeddedSet(s.F, s.origin, s.offsets, s.desc, B.estimate_normals(s.origin, s.offsets, self.cfg.icp_normal_k, self.cfg.normal_radius()))


def concat_sets(sets):
    off = [0]
    for s in sets:
        off += [o + off[-1] for o in s.offsets[1:]]
    normal = torch.cat([s.normal for s in sets]) if sets and all(s.normal is not None for s in sets) else None
    return EmbeddedSet(torch.cat([s.F for s in sets]), torch.cat([s.origin for s in sets]), off,
                       torch.cat([s.desc for s in sets]), normal)


# ---- metric aggregation (evaluation.py:334-383) -----------------------------------------------------
def aggregate(r_losses, t_losses, chamfer=None):
    """Mean RRE (deg) and RRE <= 5/15/45 deg, mean RTE and RTE <= .02/.05/.10/.15 (fractions),
    mean Chamfer -- the numbers of the README tables (README.md:175-178,215-218)."""
    r = np.asarray(r_losses, np.float64)
    t = np.asarray(t_losses, np.float64)
    out = {
        "rre_mean_deg": float(np.mean(r) / np.pi * 180),
        "rre_5": float(np.sum(r <= 5 / 180 * np.pi) / len(r)),
        "rre_15": float(np.sum(r <= 15 / 180 * np.pi) / len(r)),
        "rre_45": float(np.sum(r <= 45 / 180 * np.pi) / len(r)),
        "rte_mean": float(np.mean(t)),
        "rte_002": float(np.sum(t <= 0.02) / len(t)),
        "rte_005": float(np.sum(t <= 0.05) / len(t)),
        "rte_010": float(np.sum(t <= 0.10) / len(t)),
        "rte_015": float(np.sum(t <= 0.15) / len(t)),
    }
    if chamfer is not None:
        out["chamfer_mean"] = float(np.mean(np.asarray(chamfer, np.float64)))
    return out


def pose_losses(T_est, T0s, T1s, syms):
    """eval_pose over a batch (evaluation.py:319-322).  T_est f32 [P,4,4] (device or host)."""
    if isinstance(T_est, torch.Tensor):
        T_est = T_est.cpu().numpy()
    t_l, r_l = [], []
    for p in range(len(T_est)):
        t, r = eval_pose(T_est[p], T0s[p], T1s[p], int(syms[p]))
        t_l.append(t)
        r_l.append(r)
    return np.asarray(t_l), np.asarray(r_l)


# ---- the evaluation entry (evaluation.py:207-441) ---------------------------------------------------------
@dataclass
class EvalResult:
    """Everything App.__init__ of evaluation.py computes after the model is loaded."""
    stat: dict                      # precision, top1_error, top1_predict, gt (evaluation.py:272-283)
    per_query: dict                 # the nine arrays of evaluation.py:421-441 (cache.NAMES)
    ransac: dict                    # aggregate() of the vanilla RANSAC poses (evaluation.py:334-358)
    sym: dict                       # aggregate() of the symmetry-aided poses
    sym_success_rate: float
    from_cache: bool
    report: str                     # the log block of evaluation.py:359-383
    icp: dict = None                # aggregate() of the ICP-refined poses (+ iters_mean) when the refinement ran


def _report(ransac, sym, rate):
    def block(title, a, tail):
        return (f"\n==================================================================\n"
                f"{title}:\n"
                f"translation error: {a['rte_mean']},\n"
                f"rte 0.02: {a['rte_002']}, rte 0.05: {a['rte_005']}, rte 0.10: {a['rte_010']}, rte 0.15: {a['rte_015']}\n"
                f"------------------------------------------------------------------\n"
                f"rotation error: {a['rre_mean_rad']},\n"
                f"rre 5: {a['rre_5']}, rre 15: {a['rre_15']}, rre 45: {a['rre_45']},\n"
                f"chamfer distance: {a['chamfer_mean']}" + tail)

    return (block("vanilla ransac", ransac, "") +
            block("sym ransac", sym, "\n==================================================================\n") +
            f"\nsym success rate: {rate}")


def _icp_report(a):
    return (f"\nicp refinement:\ntranslation error: {a['rte_mean']},\n"
            f"rte 0.02: {a['rte_002']}, rte 0.05: {a['rte_005']}, rte 0.10: {a['rte_010']}, rte 0.15: {a['rte_015']}\n"
            f"rotation error: {a['rre_mean_rad']},\nrre 5: {a['rre_5']}, rre 15: {a['rre_15']}, rre 45: {a['rre_45']},\n"
            f"chamfer distance: {a['chamfer_mean']}\nmean icp updates: {a['iters_mean']}" +
            (f"\nicp scale: mean |s - 1| {a['scale_dev_mean']}, largest |s - 1| {a['scale_dev_max']}"
             if "scale_dev_mean" in a else ""))


def _verify_report(v):
    return (f"\ncandidate verification (top-{v['k']} re-ranked by the {v['score']} Chamfer of the registered pose):\n"
            f"top-1 hit: {v['top1_hit_before']} -> {v['top1_hit']}, queries whose top-1 changed: {v['moved']}\n"
            f"precision: {v['precision']}\ntop1_error: {v['top1_error']}")


# ---- candidate verification --------------------------------------------------------------------------------
def verify_order(scores):
    """The order of the candidates of one query (scores [K]) or of every query (scores [Q,K]) by verification score:
    stable ascending over the FINITE scores (equal scores keep the retrieval order), then every candidate whose score is NaN
    or infinite, in retrieval order (-inf too, which a sum of distances never is); when nothing is finite nothing moves.
    Returns int32 column numbers of the shape of `scores`: position 0 is the winner's column."""
    s = np.asarray(scores, np.float64)
    key = np.where(np.isfinite(s), s, np.inf)       # every non-finite score ties at the end; the stable sort does the rest
    return np.argsort(key, axis=-1, kind="stable").astype(np.int32)


def verify_scores(fb, score):
    """Score column of the [.., 2] (forward, backward) pairs of backend.chamfer_2dir: "symmetric" = forward + backward, added
    in f64 on the host (the sum of evaluate_retrieval, evaluation-scan2cad.py:356-357); "forward" = forward alone."""
    fb = np.asarray(fb, np.float64)
    if score == "symmetric":
        return fb[..., 0] + fb[..., 1]
    if score == "forward":
        return fb[..., 0].copy()
    raise ValueError("verify score must be one of %s, got %r" % (VERIFY_SCORES, score))


def verify_rerank(rank, order):
    """`rank` [Q,R] with its first K = order.shape[1] columns re-ordered by `order` and the remainder untouched."""
    rank = np.asarray(rank)
    order = np.asarray(order, np.int64)
    K = order.shape[1]
    return np.concatenate([np.take_along_axis(rank[:, :K], order, axis=1), rank[:, K:]], axis=1)


def verify_stat(rank, order, table, best_match, pos_n, score="symmetric"):
    """stat["verify"]: scan2cad_retrieval_eval_rank on the re-ranked list (verify_rerank), plus `moved` (number of queries
    whose top-1 changed), `top1_hit` / `top1_hit_before` (share of queries whose first CAD after / before is the nearest
    one of the annotation, stat["gt"]), and the `k` and `score` of the run."""
    from .utils import retrieval

    rank = np.asarray(rank)
    new = verify_rerank(rank, order)
    out = retrieval.scan2cad_retrieval_eval_rank(new, table, best_match, pos_n)
    gt = np.asarray(out["gt"], np.int64)
    out["moved"] = int(np.sum(new[:, 0] != rank[:, 0]))
    out["top1_hit"] = float(np.mean(new[:, 0] == gt))
    out["top1_hit_before"] = float(np.mean(rank[:, 0] == gt))
    out["k"] = int(np.asarray(order).shape[1])
    out["score"] = score
    return out


def verify_queries(pipe, qs, query_ids, cat, cand, syms, base_T, lib_T, force_gate=False, batch_size=None, in_flight=1,
                   score="symmetric"):
    """Candidate verification of the embedded queries `qs` (global numbers `query_ids`): every query is registered against
    each of its K candidates cand[q] (int [Q,K], CAD ids in retrieval order) through the registration path of
    register_queries -- all Q K pairs, query-major, in batches of batch_size pairs, every candidate of query i on the anchor
    counters (2 i, 2 i + 1) --, each batch scores its last poses with one backend.chamfer_2dir call, and the candidates are
    ordered by verify_order.  Returns the arrays of register_queries for the WINNING candidate of every query plus those of
    cache.VERIFY_NAMES."""
    from . import cache as C_

    query_ids = np.asarray(query_ids, dtype=np.int64)
    cand = np.asarray(cand, dtype=np.int64)
    Q, K = cand.shape
    pairs = _register_pairs(pipe, qs, np.repeat(np.arange(Q), K), np.repeat(query_ids, K), cat, cand.reshape(-1), syms, base_T,
                            lib_T, force_gate, batch_size, in_flight, verify=True)
    sc = verify_scores(pairs.pop("verify_fb"), score).reshape(Q, K)
    vT = pairs.pop("verify_T").reshape(Q, K, 4, 4)
    order = verify_order(sc)
    win = np.arange(Q) * K + order[:, 0] if K else np.zeros(0, np.int64)
    out = {k: v[win] for k, v in pairs.items()}
    out.update(verify_cand=cand, verify_score=sc, verify_order=order, verify_T=vT)
    return {k: (np.asarray(v, C_.VERIFY_DTYPES[k]) if k in C_.VERIFY_DTYPES else v) for k, v in out.items()}


def run_eval(pipe, catalog, queries, best_match, table, base_T, lib_T, syms, category="chair",
             register_top1=True, cache_dir=None, ignore_cache=False, force_gate=False, batch_size=None, in_flight=1):
    """The reference's evaluation, end to end (evaluation.py:207-441), on the MI355X path.

    catalog / queries: lists of [n,3] clouds (already normalised; f32 catalog clouds as CADLib loads them,
    f64 posed queries as apply_transform leaves them -- each is quantised in its own type) or EmbeddedSets; best_match int
    [Q] (annotated CAD of every query), table f64 [C,C] pairwise Chamfer of the catalog (diag 0),
    base_T [Q,4,4] / lib_T [C,4,4] ground-truth poses (`base_T`, `pos_T` of the datasets), syms int [C].
      1. feature extraction of both sets in batches (evaluation.py:213-269),
      2. scan2cad_retrieval_eval with Precision@M = 0.1 C (evaluation.py:272-283),
      3. registration of every query against its top-1 prediction (or the GT CAD) with sym_pose, and
         eval_pose of both estimates (evaluation.py:297-331) -- batched, not one Python iteration each;
         skipped when the nine cache files exist (evaluation.py:287, _load_data),
      4. aggregation + the log block (evaluation.py:334-383), 5. the result cache (evaluation.py:421-441).
    Config.verify_top_k = K > 1: step 3 registers every query against its first K retrieved CADs and re-ranks them
    by the Chamfer score of the registered pose (verify_queries); the per-query arrays are then those of the winning candidate,
    cache.VERIFY_NAMES arrays are added and stat["verify"] holds the retrieval statistics of the re-ranked list (verify_stat);
    every other entry of `stat` is what it is without the verification.  Needs register_top1 and K <= C.
    in_flight: registration batches in flight (host threads x HIP streams; identical results).  Returns an EvalResult."""
    from . import cache as C_

    cfg = pipe.cfg
    K = cfg.verify_k() if hasattr(cfg, "verify_k") else 0
    if K:
        if not register_top1:
            raise ValueError("run_eval: Config.verify_top_k = %d re-ranks the RETRIEVED candidates; it cannot be combined with "
                             "register_top1=False (the annotated CAD)" % K)
        if K > len(catalog):
            raise ValueError("run_eval: Config.verify_top_k = %d exceeds the catalog (%d CADs)" % (K, len(catalog)))
    bs = batch_size or cfg.batch_size
    ebs = cfg.embed_batch_size   # (batch_size is the REGISTRATION batch; the network's forward has its own size)
    cat = catalog if isinstance(catalog, EmbeddedSet) else pipe.embed_clouds(catalog, ebs)
    # raw queries alone are cleaned by the configured scan filter: never the catalog, never an EmbeddedSet
    filt = getattr(cfg, "scan_filter", "none") != "none" and not isinstance(queries, EmbeddedSet)
    plane = getattr(cfg, "scan_plane", "none") != "none" and not isinstance(queries, EmbeddedSet)   # the step before it
    if filt or plane:
        cfg.check_scan_filter()
        cfg.check_scan_plane()
        pipe.scan_filter_stat = {"rows_in": 0, "rows_kept": 0, "clouds_skipped": 0}
        pipe.scan_plane_stat = {"clouds": 0, "planes_removed": 0, "rows_removed": 0}
        qs = pipe.embed_clouds(queries, ebs, scan_filter=True)
    else:
        qs = queries if isinstance(queries, EmbeddedSet) else pipe.embed_clouds(queries, ebs)
    Q = len(qs)
    best_match = np.asarray(best_match).astype(np.int64)
    syms = np.asarray(syms)
    if K:
        # ONE ranking of max(pos_n, K) columns: `stat` consumes its first pos_n columns as without the verification, the
        # candidates are its first K, so candidate 0 is stat["top1_predict"] by construction
        stat, rank = retrieval_stat(pipe, qs.desc, cat.desc, best_match, table, min_columns=K, return_rank=True)
        pos_n = int(0.1 * np.asarray(table).shape[1])
        cand = rank[:, :K].astype(np.int64)
    else:
        stat = retrieval_stat(pipe, qs.desc, cat.desc, best_match, table)

    if filt:
        stat["scan_filter"] = dict(pipe.scan_filter_stat)
    if plane:
        stat["scan_plane"] = dict(pipe.scan_plane_stat)
    per_query = None if (ignore_cache or cache_dir is None) else \
        C_.load_results(cache_dir, category, register_top1, icp=cfg.icp_max_iter > 0,
                        icp_scale=bool(getattr(cfg, "icp_with_scaling", False)), **({"verify": K} if K else {}))
    if K and per_query is not None and not np.array_equal(per_query["verify_cand"], cand):
        per_query = None            # written for other candidates (another catalog or other descriptors): a miss
    from_cache = per_query is not None
    if per_query is None:
        if K:
            per_query = verify_queries(pipe, qs, np.arange(Q), cat, cand, syms, base_T, lib_T, force_gate, bs, in_flight,
                                       cfg.verify_score)
        else:
            pos_idx = np.asarray(stat["top1_predict" if register_top1 else "gt"], dtype=np.int64)
            per_query = register_queries(pipe, qs, np.arange(Q), cat, pos_idx, syms, base_T, lib_T, force_gate, bs, in_flight)
        if cache_dir is not None:
            C_.save_results(cache_dir, category, register_top1, per_query)
    if K:
        stat["verify"] = verify_stat(rank, per_query["verify_order"], table, best_match, pos_n, cfg.verify_score)
    return finish_eval(stat, per_query, from_cache)


def retrieval_stat(pipe, q_desc, lib_desc, best_match, table, min_columns=0, return_rank=False):
    """scan2cad_retrieval_eval with Precision@M, M = int(0.1 C) (evaluation.py:272-283): the ranking comes from
    pipe.retrieve (cs_l2_topk), the statistics from utils.retrieval.  min_columns: the ranking has at least that many columns
    (the statistics consume the first M only); return_rank: (statistics, ranking int [Q, max(M, 1, min_columns)])."""
    from .utils import retrieval

    pos_n = int(0.1 * np.asarray(table).shape[1])
    rank = pipe.retrieve(q_desc, lib_desc, max(pos_n, 1, int(min_columns)))
    rank = rank.cpu().numpy() if torch.is_tensor(rank) else np.asarray(rank)
    stat = retrieval.scan2cad_retrieval_eval_rank(rank, table, best_match, pos_n)
    return (stat, rank) if return_rank else stat


# Worker threads (and one torch stream each per device) of the batches-in-flight mode, kept for the life of the process: the
# library gives every host thread its own side streams and scratch cache and HIP maps all streams of a process onto a handful
# of hardware queues, so a fresh set of threads per evaluation (a ThreadPoolExecutor per call, rounds 3-4) kept adding live
# streams -- repeated evaluations in one process (bench.py --scaling strong) then share queues between workers.
_WORKERS = {}
_WORKER_STREAMS = {}


def _worker(w):
    from concurrent.futures import ThreadPoolExecutor

    if w not in _WORKERS:
        _WORKERS[w] = ThreadPoolExecutor(max_workers=1, thread_name_prefix="corsair-register%d" % w)
    return _WORKERS[w]


def _worker_stream(dev, w):
    key = (dev.type, dev.index, w)
    if key not in _WORKER_STREAMS:
        _WORKER_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _WORKER_STREAMS[key]


def register_queries(pipe, qs, query_ids, cat, pos_idx, syms, base_T, lib_T, force_gate=False, batch_size=None,
                     in_flight=1):
    """The registration loop of evaluation.py:297-331 over the embedded queries `qs`, whose GLOBAL query numbers are
    `query_ids` (they seed the anchor draws, so a query gives the same result whichever rank or batch it lands in):
    sym_pose against CAD pos_idx[q] and eval_pose of both estimates, batched.  Returns the nine arrays of
    evaluation.py:421-441 (cache.NAMES) for these queries, in the order of `query_ids`; with ICP refinement on
    (pipe.cfg.icp_max_iter > 0) also the arrays of cache.ICP_NAMES, and with pipe.cfg.icp_with_scaling those of
    cache.ICP_SCALE_NAMES; the ICP losses are then eval_pose's on T_icp with its 3x3 block divided by the scale (the trace
    formula assumes a rotation).
    in_flight > 1: that many batches at a time, each on its own host thread and HIP stream (batches are independent;
    the library's scratch cache is per thread and stream-ordered) -- same results, the host work of one batch hides
    behind the kernels of the others (bench.py's `batches_in_flight`)."""
    query_ids = np.asarray(query_ids, dtype=np.int64)
    return _register_pairs(pipe, qs, np.arange(len(query_ids)), query_ids, cat, np.asarray(pos_idx)[query_ids], syms, base_T,
                           lib_T, force_gate, batch_size, in_flight)


def _register_pairs(pipe, qs, q_loc, query_ids, cat, cad_ids, syms, base_T, lib_T, force_gate=False, batch_size=None,
                    in_flight=1, verify=False):
    """register_queries' loop over explicit (query, CAD) PAIRS: pair j registers row q_loc[j] of `qs`, whose global query
    number query_ids[j] seeds its anchor draws, against CAD cad_ids[j]; a query may occur in several pairs (the candidates of
    one query then share its anchor counters, so each is registered exactly as if it were that query's only CAD).  Batches of
    batch_size PAIRS.  verify: every batch also scores the last pose it produced (T_icp when the refinement runs, else
    T_best) with one backend.chamfer_2dir call; the result then carries "verify_T" f32 [P,4,4] and "verify_fb" f64 [P,2]
    (forward, backward)."""
    from . import cache as C_

    bs = batch_size or pipe.cfg.batch_size
    q_loc = np.asarray(q_loc, dtype=np.int64)
    query_ids = np.asarray(query_ids, dtype=np.int64)
    cad_ids = np.asarray(cad_ids, dtype=np.int64)
    icp_on = getattr(pipe.cfg, "icp_max_iter", 0) > 0
    if icp_on and len(query_ids) and hasattr(pipe, "with_normals"):
        cat = pipe.with_normals(cat)     # point-to-plane: the catalog's normals once per evaluation, gathered per batch
    scale_on = icp_on and bool(getattr(pipe.cfg, "icp_with_scaling", False))
    names = C_.NAMES + (C_.ICP_NAMES if icp_on else ()) + (C_.ICP_SCALE_NAMES if scale_on else ()) + \
        (("verify_T", "verify_fb") if verify else ())
    dtypes = dict(C_.DTYPES, **C_.ICP_DTYPES, **C_.ICP_SCALE_DTYPES, verify_T=np.float32, verify_fb=np.float64)
    if not len(query_ids):
        return {k: np.zeros((0, 4, 4) if k.startswith("Ts_est") or k == "verify_T" else ((0, 2) if k == "verify_fb" else 0),
                            dtypes[k]) for k in names}
    batches = [np.arange(s, min(len(query_ids), s + bs)) for s in range(0, len(query_ids), bs)]

    def one(loc):
        ids = query_ids[loc]
        q = qs.gather(q_loc[loc])
        cads = cat.gather(cad_ids[loc])
        cad_sym = syms[cad_ids[loc]]
        res = pipe.register(q, cads, cad_sym, anchor_ids=[(2 * int(i), 2 * int(i) + 1) for i in ids],
                            force_gate=force_gate)
        if verify:      # enqueued before the downloads below wait for the registration
            T_last = res.T_icp if icp_on else res.T_best
            n = list(range(len(loc)))
            fb = B.chamfer_2dir(q.origin, q.offsets, cads.origin, cads.offsets, n, n, T_last)
        Tr, Tb, cdr, cdb = (t.cpu().numpy() for t in (res.T_ransac, res.T_best, res.cd_ransac, res.cd_best))
        T0 = [base_T[i] for i in ids]
        T1 = [lib_T[j] for j in cad_ids[loc]]
        t_r, r_r = pose_losses(Tr, T0, T1, cad_sym)
        t_s, r_s = pose_losses(Tb, T0, T1, cad_sym)
        out = {"Ts_est_ransac": Tr, "Ts_est_best": Tb, "t_losses_ransac": t_r, "t_losses_sym": t_s,
               "r_losses_ransac": r_r, "r_losses_sym": r_s, "sym_ransac_success": np.asarray(res.ok),
               "chamfer_dist_ransac": cdr, "chamfer_dist_sym": cdb}
        if icp_on:
            Ti, cdi, iti = (t.cpu().numpy() for t in (res.T_icp, res.cd_icp, res.icp_iters))
            Tl = Ti
            if scale_on:
                sc = res.icp_scale.cpu().numpy()
                Tl = Ti.copy()
                Tl[:, :3, :3] = (Ti[:, :3, :3].astype(np.float64) / sc[:, None, None]).astype(Ti.dtype)
            t_i, r_i = pose_losses(Tl, T0, T1, cad_sym)
            extra = {"Ts_est_icp": Ti, "t_losses_icp": t_i, "r_losses_icp": r_i, "chamfer_dist_icp": cdi, "icp_iters": iti}
            if scale_on:
                extra["icp_scale"] = sc
            out.update({k: np.asarray(v, dtypes[k]) for k, v in extra.items()})
        if verify:
            out["verify_T"] = Ti if icp_on else Tb
            out["verify_fb"] = fb.cpu().numpy()
        return out

    depth = min(int(in_flight), len(batches))
    on_gpu = torch.device(getattr(pipe, "device", "cpu")).type == "cuda"
    if depth <= 1 or not on_gpu:
        done = [one(loc) for loc in batches]
    else:
        dev = torch.device(pipe.device)
        torch.cuda.synchronize(dev)          # the embedded sets were made on the caller's stream
        done = [None] * len(batches)

        def work(w):
            if dev.index is not None:
                torch.cuda.set_device(dev.index)
            st = _worker_stream(dev, w)
            with torch.cuda.stream(st):
                for i in range(w, len(batches), depth):
                    done[i] = one(batches[i])
                st.synchronize()

        if os.environ.get("CORSAIR_REGISTER_FRESH_THREADS") == "1":     # (A/B: a fresh set of threads per call, as in rounds 3-4)
            from concurrent.futures import ThreadPoolExecutor

            with ThreadPoolExecutor(max_workers=depth, thread_name_prefix="corsair-register") as ex:
                for f in [ex.submit(work, w) for w in range(depth)]:
                    f.result()
        else:
            for f in [_worker(w).submit(work, w) for w in range(depth)]:
                f.result()               # surfaces worker failures
    return {k: np.concatenate([np.asarray(d[k]) for d in done]) for k in names}


def finish_eval(stat, per_query, from_cache):
    """Aggregation + the log block (evaluation.py:334-383) over the per-query arrays of ALL queries; one more block when the
    candidate verification ran (stat["verify"])."""
    ransac = aggregate(per_query["r_losses_ransac"], per_query["t_losses_ransac"], per_query["chamfer_dist_ransac"])
    sym = aggregate(per_query["r_losses_sym"], per_query["t_losses_sym"], per_query["chamfer_dist_sym"])
    for a, r in ((ransac, per_query["r_losses_ransac"]), (sym, per_query["r_losses_sym"])):
        a["rre_mean_rad"] = float(np.mean(np.asarray(r, np.float64)))
    rate = float(np.mean(per_query["sym_ransac_success"]))
    res = EvalResult(stat, per_query, ransac, sym, rate, from_cache, _report(ransac, sym, rate))
    if "r_losses_icp" in per_query:
        icp = aggregate(per_query["r_losses_icp"], per_query["t_losses_icp"], per_query["chamfer_dist_icp"])
        icp["rre_mean_rad"] = float(np.mean(np.asarray(per_query["r_losses_icp"], np.float64)))
        icp["iters_mean"] = float(np.mean(per_query["icp_iters"]))
        if "icp_scale" in per_query:
            dev = np.abs(np.asarray(per_query["icp_scale"], np.float64) - 1.0)
            icp["scale_dev_mean"] = float(np.mean(dev)) if len(dev) else 0.0
            icp["scale_dev_max"] = float(np.max(dev)) if len(dev) else 0.0
        res.icp = icp
        res.report += _icp_report(icp)
    if isinstance(stat, dict) and "verify" in stat:
        res.report += _verify_report(stat["verify"])
    return res


# ---- synthetic Scan2CAD-shaped workload ---------------------------------------------------------------
@dataclass
class SyntheticScan2CAD:
    """Chair-sized synthetic evaluation set, the input of run_eval when the Scan2CAD annotations are
    not available: C catalog clouds, Q queries = posed copies of catalog clouds (known GT pose),
    symmetry labels with the chair label statistics; `table()` computes the pairwise
    Chamfer table the retrieval metric needs (utils/pc_dist.py, 2000 points per cloud)."""
    n_catalog: int = 652
    n_query: int = 993
    n_points: int = 10000
    catalog: list = field(default_factory=list)
    queries: list = field(default_factory=list)
    query_T: list = field(default_factory=list)
    query_cad: list = field(default_factory=list)
    sym: np.ndarray = None

    def build(self, catalog_ids=None, query_ids=None):
        from . import synth

        cids = list(range(self.n_catalog)) if catalog_ids is None else list(catalog_ids)
        self.catalog = [synth.make_cloud(c, 15000)[: self.n_points] for c in cids]
        self.sym = np.ones(len(cids), np.int32)
        self.sym[::326] = 4  # chair labels: 650 x 1, 2 x 4 (configs/03001627_scan2cad_rot_sym_label.txt)
        qids = list(range(self.n_query)) if query_ids is None else list(query_ids)
        self.queries, self.query_T, self.query_cad = [], [], []
        for q in qids:
            cad = q % len(cids)
            T = synth.random_pose(q, max_trans=0.0)
            # the reference's query is the scan in the fixed test rotation fix_trans[idx,0]
            # (datasets/ScannetDataset.py:274); here: the CAD cloud itself under a seeded rotation,
            # re-sampled (other 10k of the 15k points) so voxel occupancy differs
            pc = synth.make_cloud(cids[cad], 15000)[15000 - self.n_points:]
            self.queries.append(synth.apply_pose(pc, T, np.float64))   # apply_transform yields f64
            self.query_T.append(T)
            self.query_cad.append(cad)
        return self

    def table(self, n_points=2000):
        from .utils import pc_dist

        t = pc_dist.compute_dist([c[:n_points] for c in self.catalog])
        np.fill_diagonal(t, 0.0)                     # datasets/ScannetDataset.py:65-66
        return t

    def eval_inputs(self):
        """(catalog, queries, best_match, base_T, lib_T, syms) for run_eval; the CADs sit in their
        canonical frame (lib_T = identity, like the bench's T1)."""
        return (self.catalog, self.queries, np.asarray(self.query_cad), np.stack(self.query_T),
                np.stack([np.eye(4)] * len(self.catalog)), self.sym)


# ---- file-level entry: `python -m corsair_amd.harness` (evaluation.py:68-129,195-201) -----------------------------------
def load_cloud_dir(path, n_points, what):
    """Sorted *.npy files of a directory, first n_points rows each (load_raw_pc, utils/preprocess.py:27-29 through
    datasets/Reader.py:75-86), in the type they are stored in.  Returns (names, clouds)."""
    import os

    names = sorted(f for f in os.listdir(path) if f.endswith(".npy"))
    if not names:
        raise FileNotFoundError(f"{what}: no .npy cloud in {path}")
    clouds = []
    for f in names:
        a = np.load(os.path.join(path, f))
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError(f"{what}: {f} is not an [n,3] cloud (shape {a.shape})")
        a = np.ascontiguousarray(a[:n_points, :3])
        clouds.append(a if a.dtype in (np.float32, np.float64) else a.astype(np.float32))
    return names, clouds


def read_sym_labels(path, names):
    """`<cad path> <label>` per line (configs/*_scan2cad_rot_sym_label.txt, read at evaluation.py:175-179): matched to
    the catalog files by basename when every name occurs, by line order otherwise."""
    import os

    rows = [ln.split() for ln in open(path) if ln.strip()]
    by_name = {os.path.basename(r[0]): int(r[-1]) for r in rows}
    if all(n in by_name for n in names):
        return np.asarray([by_name[n] for n in names], np.int32)
    if len(rows) != len(names):
        raise ValueError(f"{path}: {len(rows)} labels for {len(names)} catalog clouds")
    return np.asarray([int(r[-1]) for r in rows], np.int32)


def build_parser():
    import argparse

    ap = argparse.ArgumentParser(
        prog="python -m corsair_amd.harness",
        description="CORSAIR evaluation on the MI355X path from FILES: a reference checkpoint (utils/ckpts.py format) and "
                    "directories of .npy clouds; the counterpart of `python evaluation.py` (evaluation.py:68-129) with the "
                    "Scan2CAD annotation parsing (out of scope, SURVEY 2) replaced by plain arrays.")
    ap.add_argument("--checkpoint", "--ckpt", required=True, help="torch.save dict with state_dict / embedding_state_dict "
                                                                  "(evaluation.py:195-201)")
    ap.add_argument("--catalog-dir", required=True, help="CAD clouds, one [n,3] .npy each (sorted by name = catalog index)")
    ap.add_argument("--query-dir", required=True, help="scan clouds, one [n,3] .npy each (sorted by name = query index)")
    ap.add_argument("--category", default="table", choices=["table", "chair"])
    ap.add_argument("--query-poses", help=".npy [Q,4,4] or [Q,k,4,4] (configs/fix_trans.npy: element [:,0]) applied to the "
                                          "queries with apply_transform (f64) before quantisation; default: none")
    ap.add_argument("--lib-poses", help=".npy [C,4,4] ground-truth poses of the CADs (`pos_T`); default identity")
    ap.add_argument("--best-match", help=".npy int [Q]: annotated CAD index of every query; default: query i -> i mod C")
    ap.add_argument("--table", help=".npy f64 [C,C] pairwise Chamfer of the catalog (configs/<catid>_scan2cad.npy); "
                                    "default: computed from the first 2000 points of every CAD (utils/pc_dist.py)")
    ap.add_argument("--sym-labels", help="`<path> <label>` per line (configs/<catid>_scan2cad_rot_sym_label.txt); default 1")
    ap.add_argument("--cache-dir", default=None, help="load / save the nine result files (evaluation.py:390-441)")
    ap.add_argument("--register-gt", action="store_false", dest="register_top1", help="register the annotated CAD")
    ap.add_argument("--ignore-cache", action="store_true")
    ap.add_argument("--n-points", type=int, default=10000)
    ap.add_argument("--batch-size", type=int, default=32, help="queries per registration batch")
    ap.add_argument("--embed-batch-size", type=int, default=128,
                    help="clouds per forward of the network (the reference's DataLoader: 32; the rows do not depend on it)")
    ap.add_argument("--ransac-max-iter", type=int, default=100000)
    ap.add_argument("--icp-iters", type=int, default=0,
                    help="refine every kept pose with at most N point-to-point ICP updates (0 = off, the reference's behaviour)")
    ap.add_argument("--icp-max-dist", type=float, default=0.0,
                    help="ICP correspondence distance; 0 = 2 * voxel size (an untuned default)")
    ap.add_argument("--icp-estimation", default="point", choices=["point", "plane", "gicp"],
                    help="ICP estimation: point-to-point, point-to-plane on the CAD voxels' normals, or plane-to-plane "
                         "(Generalized ICP) on the normals of both clouds")
    ap.add_argument("--gicp-epsilon", type=float, default=1e-3,
                    help="covariance floor along the normal for --icp-estimation gicp, in [2^-10, 1] (Open3D's default, untuned)")
    ap.add_argument("--icp-normal-k", type=int, default=16,
                    help="neighbours of a CAD voxel's normal for --icp-estimation plane, 3..32 (an untuned default)")
    ap.add_argument("--icp-normal-radius", type=float, default=0.0,
                    help="radius of the normals' hybrid search (at most --icp-normal-k rows inside it); 0 = k-NN.  Untuned")
    ap.add_argument("--icp-kernel", default="l2", choices=list(ICP_KERNEL_NAMES),
                    help="robust kernel on the point-to-plane residual (needs --icp-estimation plane); l2 = none")
    ap.add_argument("--icp-kernel-scale", type=float, default=0.0,
                    help="scale k of --icp-kernel; 0 = 1 * voxel size (an untuned default)")
    ap.add_argument("--icp-with-scaling", action="store_true",
                    help="the ICP refinement also fits an isotropic scale of the query (needs --icp-iters > 0, no robust kernel)")
    ap.add_argument("--icp-scale-min", type=float, default=0.5,
                    help="lower bound of the scale the ICP may add, in (0, 1] (an untuned default)")
    ap.add_argument("--icp-scale-max", type=float, default=2.0,
                    help="upper bound of the scale the ICP may add, >= 1 (an untuned default)")
    ap.add_argument("--registration", default="ransac", choices=list(estimators.WIRED),
                    help="correspondence estimator: the reference's RANSAC, or Fast Global Registration (cs_fgr_batch)")
    ap.add_argument("--fgr-mu-floor", type=float, default=0.025,
                    help="floor of FGR's mu, in units of the clouds' radius (Open3D's default, untuned)")
    ap.add_argument("--verify-top-k", type=int, default=0,
                    help="register every query against its first K retrieved CADs and re-rank them by the Chamfer score of the "
                         "registered pose (cs_chamfer_2dir); 0 and 1 = off, 2..32 (untuned; not with --register-gt)")
    ap.add_argument("--verify-score", default="symmetric", choices=list(VERIFY_SCORES),
                    help="score of --verify-top-k: forward + backward Chamfer, or forward alone (for partial scans; untuned)")
    ap.add_argument("--scan-filter", default="none", choices=list(SCAN_FILTERS),
                    help="clean every raw query scan after voxelisation: Open3D's statistical or radius outlier removal "
                         "(cs_outlier_statistical / cs_outlier_radius), or the largest DBSCAN cluster alone (cs_dbscan / "
                         "cs_cluster_largest); never the catalog.  Untuned; not recorded in the cache")
    ap.add_argument("--scan-filter-k", type=int, default=20, help="neighbours of --scan-filter statistical, 2..32 (untuned)")
    ap.add_argument("--scan-filter-std", type=float, default=2.0,
                    help="a row is dropped when its mean neighbour distance reaches mean + STD * deviation (untuned)")
    ap.add_argument("--scan-filter-radius", type=float, default=2.5, help="radius of --scan-filter radius, in voxels (untuned)")
    ap.add_argument("--scan-filter-min-nb", type=int, default=4,
                    help="--scan-filter radius keeps a row with MORE than this many rows inside the radius, itself included")
    ap.add_argument("--scan-filter-eps", type=float, default=2.5,
                    help="eps of --scan-filter cluster, in voxels (untuned, no real scan measured)")
    ap.add_argument("--scan-filter-min-points", type=int, default=5,
                    help="--scan-filter cluster: a row is a core row with this many rows inside eps, itself included "
                         "(untuned, no real scan measured)")
    ap.add_argument("--scan-plane", default="none", choices=list(SCAN_PLANES),
                    help="remove the support plane (floor or wall; cs_segment_plane, Open3D's segment_plane) from every raw "
                         "query scan before --scan-filter; never the catalog.  Without --scan-plane-up a bare table top seen "
                         "from above is removed too (untuned, no real scan measured); not recorded in the cache")
    ap.add_argument("--scan-plane-dist", type=float, default=1.0,
                    help="distance threshold of --scan-plane, in voxels (untuned, no real scan measured)")
    ap.add_argument("--scan-plane-iters", type=int, default=1024,
                    help="plane hypotheses of --scan-plane, 1..65536 (untuned, no real scan measured)")
    ap.add_argument("--scan-plane-min-share", type=float, default=0.2,
                    help="--scan-plane removes a plane that holds at least this share of the scan's rows "
                         "(untuned, no real scan measured)")
    ap.add_argument("--scan-plane-max-below", type=float, default=0.02,
                    help="--scan-plane removes a plane with at most this share of the other rows beyond it "
                         "(untuned, no real scan measured)")
    ap.add_argument("--scan-plane-up", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="the up direction of the scans: --scan-plane then removes only a plane whose normal lies within "
                         "--scan-plane-max-tilt of it (untuned, no real scan measured)")
    ap.add_argument("--scan-plane-max-tilt", type=float, default=30.0,
                    help="largest angle between the plane's normal and --scan-plane-up, in degrees, (0, 90] "
                         "(untuned, no real scan measured)")
    ap.add_argument("--in-flight", type=int, default=3, help="registration batches in flight (host threads x HIP streams)")
    ap.add_argument("--device", default="cuda", choices=["cuda"], help="there is no CPU path")
    return ap


def main(argv=None):
    """Returns the EvalResult (and prints the log block of evaluation.py:359-383)."""
    from . import synth
    from .utils import ckpts, pc_dist

    a = build_parser().parse_args(argv)
    if Config(verify_top_k=a.verify_top_k, verify_score=a.verify_score).verify_k() and not a.register_top1:
        raise ValueError("--verify-top-k %d re-ranks the retrieved candidates; it cannot be combined with --register-gt"
                         % a.verify_top_k)             # (before anything is loaded or set)
    # (eight hardware queues for the streams of the registration batches in flight: bench.py's note; only effective when
    # nothing has touched the GPU yet -- the command-line entry --, an explicit setting wins)
    import os

    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    sd, esd = ckpts.load_state_dicts(a.checkpoint)
    if esd is None:
        raise SystemExit("checkpoint has no embedding_state_dict: retrieval needs the descriptor head (evaluation.py:199)")
    cfg = Config(n_points=a.n_points, batch_size=a.batch_size, embed_batch_size=a.embed_batch_size,
                 verify_top_k=a.verify_top_k, verify_score=a.verify_score,
                 ransac_max_iter=a.ransac_max_iter, icp_max_iter=a.icp_iters, icp_max_dist=a.icp_max_dist,
                 icp_estimation=a.icp_estimation, icp_normal_k=a.icp_normal_k, icp_kernel=a.icp_kernel,
                 icp_kernel_scale=a.icp_kernel_scale, icp_normal_radius=a.icp_normal_radius,
                 icp_with_scaling=a.icp_with_scaling, icp_scale_bounds=(a.icp_scale_min, a.icp_scale_max),
                 registration=a.registration, fgr_mu_floor=a.fgr_mu_floor, gicp_epsilon=a.gicp_epsilon,
                 scan_filter=a.scan_filter, scan_filter_k=a.scan_filter_k, scan_filter_std=a.scan_filter_std,
                 scan_filter_radius=a.scan_filter_radius, scan_filter_min_nb=a.scan_filter_min_nb,
                 scan_filter_eps=a.scan_filter_eps, scan_filter_min_points=a.scan_filter_min_points,
                 scan_plane=a.scan_plane, scan_plane_dist=a.scan_plane_dist, scan_plane_iters=a.scan_plane_iters,
                 scan_plane_min_share=a.scan_plane_min_share, scan_plane_max_below=a.scan_plane_max_below,
                 scan_plane_up=None if a.scan_plane_up is None else tuple(a.scan_plane_up),
                 scan_plane_max_tilt=a.scan_plane_max_tilt)
    cfg.check_icp()
    cfg.check_scan_filter()
    cfg.check_scan_plane()
    pipe = Pipeline(sd, esd, device=a.device, config=cfg)
    cad_names, catalog = load_cloud_dir(a.catalog_dir, a.n_points, "catalog")
    _, queries = load_cloud_dir(a.query_dir, a.n_points, "queries")
    C, Q = len(catalog), len(queries)
    base_T = np.stack([np.eye(4)] * Q)
    if a.query_poses:
        P = np.load(a.query_poses)
        base_T = np.asarray(P[:Q, 0] if P.ndim == 4 else P[:Q], np.float64)
        if base_T.shape != (Q, 4, 4):
            raise SystemExit(f"--query-poses: need {Q} 4x4 poses, got {P.shape}")
        queries = [synth.apply_pose(q, T, np.float64) for q, T in zip(queries, base_T)]     # apply_transform: f64
    lib_T = np.asarray(np.load(a.lib_poses), np.float64) if a.lib_poses else np.stack([np.eye(4)] * C)
    best_match = np.load(a.best_match).astype(np.int64) if a.best_match else np.arange(Q) % C
    syms = read_sym_labels(a.sym_labels, cad_names) if a.sym_labels else np.ones(C, np.int32)
    if a.table:
        table = np.array(np.load(a.table), np.float64)
    else:
        table = pc_dist.compute_dist([c[:2000] for c in catalog])
    np.fill_diagonal(table, 0.0)                                     # datasets/ScannetDataset.py:65-66
    if table.shape != (C, C) or len(best_match) != Q or len(lib_T) != C:
        raise SystemExit(f"shape mismatch: table {table.shape}, best_match {len(best_match)}, lib poses {len(lib_T)} "
                         f"for C = {C}, Q = {Q}")
    # the clouds and tables loaded above live as long as the process: out of the cycle collector's way (a full collection
    # otherwise walks them between registration batches: 10 - 50 ms pauses)
    import gc
    gc.collect()
    gc.freeze()
    res = run_eval(pipe, catalog, queries, best_match, table, base_T, lib_T, syms, a.category, a.register_top1,
                   a.cache_dir, a.ignore_cache, False, a.batch_size, a.in_flight)
    print(f"category: {a.category}")
    print(f"precision: {res.stat['precision']}\ntop1_error: {res.stat['top1_error']}")
    print(res.report)
    return res


if __name__ == "__main__":
    main()
