"""Registration-only evaluation on clouds with synthetic poses: counterpart of the reference's
evaluation-shapenet.py:70-343.  Same stages as the Scan2CAD path without
retrieval: geometric symmetry label -> batch-of-2 ResUNet forward (model + randomly posed copy) ->
sym_pose(max_corr 0.4) -> eval_pose(T, I, pose_gt, label).  The reference fans the registrations out
to joblib worker processes (:341-343); here pairs are batched on the GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import backend as B
from . import estimators as E
from . import ppf as PPF
from . import registration as R
from .synth import euler2mat
from .utils.eval_pose import eval_pose


@dataclass
class Config:
    """Defaults of evaluation-shapenet.py:38-67."""
    voxel_size: float = 0.03
    k_nn: int = 5
    max_corr: float = 0.4
    random_seed: int = 31
    n_poses_per_model: int = 1
    max_roll_deg: float = 180.0
    max_pitch_deg: float = 180.0
    max_yaw_deg: float = 180.0
    max_translation: float = 1.0
    symmetry_cd_threshold: float = 0.1
    ransac_max_iter: int = 100000
    ransac_confidence: float = 0.999
    # ICP refinement of the kept pose (registration.sym_pose_batch): updates at most, 0 = off (the reference's behaviour);
    # icp_max_dist = 0.0 means 2 * voxel_size (untuned, as in harness.Config); "point" or "plane" (normals over
    # icp_normal_k neighbours of the posed copy's voxels, untuned)
    icp_max_iter: int = 0
    icp_max_dist: float = 0.0
    # "gicp": plane-to-plane Generalized ICP (cs_icp_gicp_batch) on the normals of both clouds, each over icp_normal_k
    # neighbours; gicp_epsilon in [2^-10, 1] is Open3D's default covariance floor, UNTUNED as in harness.Config
    icp_estimation: str = "point"
    gicp_epsilon: float = 1e-3
    icp_normal_k: int = 16
    # 0.0 = k-NN (the default); > 0: the at most icp_normal_k nearest rows strictly inside this radius (UNTUNED)
    icp_normal_radius: float = 0.0
    # robust kernel of the plane estimation ("l2" = none, "huber", "cauchy", "tukey"); icp_kernel_scale = 0.0 means
    # 1 * voxel_size (UNTUNED, as in harness.Config)
    icp_kernel: str = "l2"
    icp_kernel_scale: float = 0.0
    # > 0: the posed copy is also scaled by exp(u), u uniform in +-max_log_scale (drawn only then: the random stream and
    # every output of the default are what they were); icp_with_scaling: the refinement fits that isotropic scale
    # (cs_icp_scale_batch, no robust kernel) inside icp_scale_bounds -- (0.5, 2.0) is UNTUNED, as in harness.Config
    max_log_scale: float = 0.0
    icp_with_scaling: bool = False
    icp_scale_bounds: tuple = (0.5, 2.0)
    # the correspondence estimator: "ransac" or "fgr" (cs_fgr_batch); fgr_mu_floor is UNTUNED, as in harness.Config
    registration: str = "ransac"
    fgr_mu_floor: float = 0.025
    # "ransac_fm" (DESIGN 25): 1-NN matches both ways with the mutual filter, then cs_ransac_fm_batch -- fm_iterations
    # hypotheses of fm_ransac_n pairs with the edge-length checker (fm_edge_similarity, 0 = off) and the distance checker at
    # max_corr.  Open3D's defaults, UNTUNED, no real scan measured.  The symmetry hypotheses are off under it.
    fm_ransac_n: int = 3
    fm_edge_similarity: float = 0.9
    fm_mutual: bool = True
    fm_iterations: int = 100000
    # "sc2" (DESIGN 27): the compatibility-graph estimator (cs_sc2_batch) over the k_nn lists -- sc2_seeds rows of the largest
    # degree among the correspondences whose lengths agree within sc2_compat_dist (in VOXELS), each fitted over its sc2_k best
    # neighbours.  Every default is UNTUNED, no real scan measured.  The symmetry hypotheses stay as they are.
    sc2_compat_dist: float = 1.0
    sc2_seeds: int = 1024
    sc2_k: int = 20
    # "ppf" (DESIGN 28): point-pair-feature voting (cs_ppf_batch) on the voxels and their oriented normals -- no descriptors
    # are computed and no checkpoint is needed.  The scene is the posed copy (oriented towards its camera under partial_view,
    # else away from its centroid), the model the whole cloud.  ppf_dist_step is a FRACTION of the model's bounding-box
    # diagonal.  Every default is UNTUNED, no real scan measured.  The symmetry hypotheses are off under it.
    ppf_ref_step: int = 5
    ppf_n_cand: int = 16
    ppf_dist_step: float = 0.05
    # the descriptors: "network" (the ResUNet forward, needs a checkpoint) or "fpfh" (registration.fpfh_features: no weights;
    # sym_pose_batch then runs with use_symmetry=False, the part cut takes the network's widths only).  fpfh_radius is in
    # VOXELS, 5 is Open3D's example value, UNTUNED; fpfh_max_nn is cs_fpfh's max_nn
    features: str = "network"
    fpfh_radius: float = 5.0
    fpfh_max_nn: int = 100
    # partial_view: the posed copy of every job is reduced to what one virtual depth camera sees of it
    # (views.render_views) before the descriptors; the model stays whole.  The camera stands view_distance half diagonals of
    # the copy's bounding box from the box's midpoint, in a direction drawn per job from a generator of its own, with a square
    # image of view_size pixels over view_fov_deg degrees; view_point_size and view_depth_tol are in VOXELS.  Every default is
    # UNTUNED, no real scan measured.
    partial_view: bool = False
    view_fov_deg: float = 40.0
    view_size: int = 256
    view_distance: float = 3.0
    view_point_size: float = 1.5
    view_depth_tol: float = 1.5

    def check_partial_view(self):
        if not isinstance(self.partial_view, (bool, np.bool_)):
            raise ValueError("Config.partial_view must be a bool, got %r" % (self.partial_view,))
        real = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v)
        if not (real(self.view_fov_deg) and 0.0 < self.view_fov_deg < 180.0):
            raise ValueError("Config.view_fov_deg must be in (0, 180) degrees, got %r" % (self.view_fov_deg,))
        if not (isinstance(self.view_size, (int, np.integer)) and not isinstance(self.view_size, bool)
                and 1 <= self.view_size <= 4096):
            raise ValueError("Config.view_size must be an integer in [1, 4096] pixels, got %r" % (self.view_size,))
        if not (real(self.view_distance) and self.view_distance > 1.0):
            raise ValueError("Config.view_distance must be finite and > 1 half diagonal, got %r" % (self.view_distance,))
        if not (real(self.view_point_size) and self.view_point_size > 0.0):
            raise ValueError("Config.view_point_size must be finite and > 0 voxels, got %r" % (self.view_point_size,))
        if not (real(self.view_depth_tol) and self.view_depth_tol > 0.0):
            raise ValueError("Config.view_depth_tol must be finite and > 0 voxels, got %r" % (self.view_depth_tol,))

    def registration_options(self, entry=None, models=None, view_points=None):
        """The estimator options of registration.sym_pose_batch from this Config's own units -- sc2_compat_dist in voxels, the
        scene of "ppf" the posed copy (side 1) --, every estimator's, or `entry`'s alone; then ppf_dist_step, a fraction of the
        diagonal here, is the length for each of `models` (the batch's whole clouds) and the scene looks at `view_points`."""
        if isinstance(self.sc2_compat_dist, bool) or not isinstance(self.sc2_compat_dist, (int, float, np.floating)):
            raise ValueError("Config.sc2_compat_dist must be positive and finite (voxels), got %r" % (self.sc2_compat_dist,))
        step = self.ppf_dist_step
        if entry is not None and entry.name == "ppf":
            step = PPF.default_dist_step(models.origin, models.offsets, step)
        kw = dict(fgr_mu_floor=self.fgr_mu_floor, fm_ransac_n=self.fm_ransac_n, fm_edge_similarity=self.fm_edge_similarity,
                  fm_mutual=self.fm_mutual, fm_iterations=self.fm_iterations,
                  sc2_compat_dist=self.sc2_compat_dist * self.voxel_size, sc2_seeds=self.sc2_seeds, sc2_k=self.sc2_k,
                  ppf_scene_side=1, ppf_dist_step=step, ppf_ref_step=self.ppf_ref_step, ppf_n_cand=self.ppf_n_cand,
                  ppf_view_points=view_points)
        return kw if entry is None else {key: kw[key] for key in entry.options if key in kw}

    def check_registration(self):
        entry = E.lookup(self.registration, "Config.registration")
        E.checked_options(entry, self.registration_options(), self.max_corr, "Config")
        return entry

    def icp_distance(self):
        return self.icp_max_dist if self.icp_max_dist > 0 else 2.0 * self.voxel_size

    def icp_scale(self):
        return self.icp_kernel_scale if self.icp_kernel_scale > 0 else 1.0 * self.voxel_size

    def normal_radius(self):
        if not 0 <= float(self.icp_normal_radius) < float("inf"):
            raise ValueError("Config.icp_normal_radius must be finite and >= 0 (0 = k-NN), got %r"
                             % (self.icp_normal_radius,))
        return float(self.icp_normal_radius) if self.icp_normal_radius > 0 else None


class FpfhPipe:
    """Stands where harness.Pipeline stands in `evaluate` when Config.features = "fpfh": the same `device` / `embed_groups`
    surface, voxelisation and cs_fpfh descriptors (normals over 16 neighbours, oriented away from each cloud's centroid) in
    the place of the forward.  No weights, no global descriptors."""

    def __init__(self, device="cuda", radius_voxels=5.0, max_nn=100):
        self.device = torch.device(device)
        self.radius_voxels = float(radius_voxels)
        self.max_nn = int(max_nn)

    def embed_groups(self, groups, voxel_size):
        from .harness import EmbeddedSet

        origins, out_off = [], [0]
        for xyz, offsets in groups:
            keep, _, off = B.voxelize(xyz, offsets, voxel_size)
            origins.append(xyz[keep].to(torch.float32))
            out_off += [out_off[-1] + int(o) for o in off[1:]]
        origin = torch.cat(origins).contiguous()
        F, normal = R.fpfh_features(origin, out_off, self.radius_voxels * voxel_size, self.max_nn)
        return EmbeddedSet(F, origin, out_off, torch.zeros((len(out_off) - 1, 0), dtype=torch.float32, device=origin.device),
                           normal)


class PpfPipe:
    """Stands where FpfhPipe stands when Config.registration = "ppf": voxelisation only.  The descriptors are an [n, 0]
    array that nothing reads; sym_pose_batch estimates and orients the normals itself (it knows the cameras)."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)

    def embed_groups(self, groups, voxel_size):
        from .harness import EmbeddedSet

        origins, out_off = [], [0]
        for xyz, offsets in groups:
            keep, _, off = B.voxelize(xyz, offsets, voxel_size)
            origins.append(xyz[keep].to(torch.float32))
            out_off += [out_off[-1] + int(o) for o in off[1:]]
        origin = torch.cat(origins).contiguous()
        none = torch.zeros((origin.shape[0], 0), dtype=torch.float32, device=origin.device)
        return EmbeddedSet(none, origin, out_off, torch.zeros((len(out_off) - 1, 0), dtype=torch.float32, device=origin.device))


def load_pc(pc):
    """Centre and scale to unit radius, IN PLACE in the array's own type like evaluation-shapenet.py:70-76
    (`pc -= t; pc /= r` on what np.load returned: the ShapeNetPC15k files are f32, so everything up to the
    pose product is f32 there); takes an array, works on a copy."""
    pc = np.array(pc)
    if pc.dtype not in (np.float32, np.float64):
        pc = pc.astype(np.float64)
    t = pc.mean(axis=0, keepdims=True)
    pc -= t
    r = np.linalg.norm(pc, axis=1).max()
    pc /= r
    return pc


def generate_random_pose(cfg, rng):
    """evaluation-shapenet.py:79-94 with an explicit generator instead of NumPy's global RNG."""
    r, p, y = (np.deg2rad(rng.uniform(-m, m)) for m in (cfg.max_roll_deg, cfg.max_pitch_deg, cfg.max_yaw_deg))
    pose = np.eye(4)
    pose[:3, :3] = euler2mat(r, p, y)
    pose[:3, 3] = rng.uniform(-cfg.max_translation, cfg.max_translation, 3)
    return pose


VIEW_MIN_ROWS = 10      # a view with fewer visible rows keeps the whole cloud (and is counted)


def view_direction(seed, job):
    """The direction from the posed copy to its camera: a normalised standard_normal(3) from a generator seeded by
    (seed, job index) alone, so the evaluation's own generator -- the pose draws -- never sees the option."""
    d = np.random.default_rng([int(seed), int(job)]).standard_normal(3)
    return d / np.linalg.norm(d)


def build_jobs(clouds, cfg, rng, symmetry_label=None):
    """The (model, pose index, model points, posed copy, pose, symmetry label, scale) tuples of `evaluate`, in its order."""
    symmetry_label = symmetry_label or get_symmetry_label
    jobs = []
    for mi, raw in enumerate(clouds):
        pc = load_pc(raw)
        label = symmetry_label(pc, cfg.symmetry_cd_threshold)
        for pi in range(cfg.n_poses_per_model):
            pose = generate_random_pose(cfg, rng)
            # generate_test_pc_pair (:115-119): the model stays in its own type, the posed copy is the f64
            # product with the f64 pose; quantize_pc (:97-107) floors each in its type and narrows afterwards
            if cfg.max_log_scale > 0:
                s_gt = float(np.exp(rng.uniform(-cfg.max_log_scale, cfg.max_log_scale)))
                jobs.append((mi, pi, pc, s_gt * (pc @ pose[:3, :3].T) + pose[:3, [3]].T, pose, label, s_gt))
            else:
                jobs.append((mi, pi, pc, pc @ pose[:3, :3].T + pose[:3, [3]].T, pose, label, 1.0))
    return jobs


def partial_views(xyz, offsets, host, cfg, seed, first_job):
    """The posed copies of one batch (xyz device [n,3] in its own type, host offsets; host: the same clouds as numpy arrays,
    for the bounding boxes) reduced to what each one's camera sees: (kept rows of xyz, new offsets, visible share per cloud,
    views skipped).  The mask is computed on the f32 cast; the selection (backend.select_rows, the one host wait) is applied
    to the array in its own type."""
    from . import views as V

    x32 = xyz.to(torch.float32).contiguous()
    P = len(offsets) - 1
    h32 = [np.asarray(h, np.float32) for h in host]
    lo, hi = np.stack([h.min(0) for h in h32]), np.stack([h.max(0) for h in h32])
    dirs = np.stack([view_direction(seed, first_job + i) for i in range(P)])
    cams = torch.from_numpy(V.view_cameras(lo, hi, dirs, cfg.view_distance)).to(xyz.device)
    res = V.render_views(x32, offsets, cams, cfg.view_size, cfg.view_size, V.focal_from_fov(cfg.view_size, cfg.view_fov_deg),
                         cfg.view_point_size * cfg.voxel_size, cfg.view_depth_tol * cfg.voxel_size)
    idx, off = B.select_rows(res.visible, offsets)
    kept = np.diff(off)
    rows = np.diff(np.asarray(offsets))
    skipped = [i for i in range(P) if kept[i] < VIEW_MIN_ROWS]
    if skipped:
        keep = res.visible.clone()
        for i in skipped:
            keep[offsets[i]:offsets[i + 1]] = 1
        idx, off = B.select_rows(keep, offsets)
    share = [1.0 if i in skipped else float(kept[i]) / float(rows[i]) for i in range(P)]
    return xyz[idx], off, share, len(skipped)


def partial_views_with_cameras(xyz, offsets, host, cfg, seed, first_job):
    """partial_views, and as a fifth value the eye of each cloud's camera in world coordinates, f64 [P,3] (the view points
    registration = "ppf" orients the scene's normals towards): the same boxes, directions and views.view_cameras call."""
    from . import views as V

    out = partial_views(xyz, offsets, host, cfg, seed, first_job)
    P = len(offsets) - 1
    h32 = [np.asarray(h, np.float32) for h in host]
    lo, hi = np.stack([h.min(0) for h in h32]), np.stack([h.max(0) for h in h32])
    dirs = np.stack([view_direction(seed, first_job + i) for i in range(P)])
    Rt = V.view_cameras(lo, hi, dirs, cfg.view_distance).reshape(P, 3, 4)
    eyes = -np.einsum("pba,pb->pa", Rt[:, :, :3], Rt[:, :, 3])          # the world -> camera map is R | t: the eye is -R^T t
    return out + (eyes,)


def chamfer_max(pc0, pc1):
    """Two-sided Hausdorff distance (evaluation-shapenet.py:122-135), two cs_hausdorff_1dir problems."""
    dev = torch.device("cuda")
    a = torch.from_numpy(np.ascontiguousarray(pc0, np.float32)).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(pc1, np.float32)).to(dev)
    X = torch.cat([a, b])
    off = [0, len(a), len(a) + len(b)]
    I = torch.eye(4, dtype=torch.float32, device=dev).repeat(2, 1, 1)
    return float(B.hausdorff_1dir(X, off, X, off, [0, 1], [1, 0], I).max().cpu())


def _hausdorff_many(pc, Rs):
    """max(H(pc -> R pc), H(R pc -> pc)) for every rotation in Rs (4x4), one batched launch.
    H(R pc -> pc) = H over source points transformed by R against the unrotated cloud;
    H(pc -> R pc) = H over source points transformed by R^-1 against the unrotated cloud (distances
    are rotation invariant), so both directions use the same resident cloud."""
    dev = torch.device("cuda")
    x = torch.from_numpy(np.ascontiguousarray(pc, np.float32)).to(dev)
    Ts = []
    for Rm in Rs:
        Ts.append(np.asarray(Rm, np.float64))
        Ts.append(np.linalg.inv(np.asarray(Rm, np.float64)))
    T = torch.from_numpy(np.stack(Ts).astype(np.float32)).to(dev)
    n = len(Ts)
    d = B.hausdorff_1dir(x, [0, len(x)], x, [0, len(x)], [0] * n, [0] * n, T).cpu().numpy()
    return d.reshape(-1, 2).max(axis=1)


def test_symmetry_label(sym_label, pc, cd_threshold):
    """True iff pc maps onto itself (Hausdorff <= threshold) under every rotation i*2pi/sym about y,
    i = 1..sym//2 (evaluation-shapenet.py:138-148)."""
    Rs = []
    for i in range(1, int(sym_label / 2) + 1):
        T = np.eye(4)
        T[:3, :3] = euler2mat(0, i * (2 * np.pi) / sym_label, 0)
        Rs.append(T)
    if not Rs:
        return True
    return bool((_hausdorff_many(pc, Rs) <= cd_threshold).all())


def get_symmetry_label(pc, cd_threshold):
    """Largest of (12, 8, 6, 4, 3, 2, 1) under which the cloud is symmetric; 1 = none
    (evaluation-shapenet.py:151-155)."""
    for sym_label in [12, 8, 6, 4, 3, 2, 1]:
        if test_symmetry_label(sym_label, pc, cd_threshold):
            return sym_label
    return 0


def evaluate(pipe, clouds, cfg=None, pairs_per_batch=16, seed=None, force_gate=False, stat=None):
    """clouds: list of raw [n,3] arrays.  Returns a list of result dicts (one per model x pose) with
    the keys of registration_worker (evaluation-shapenet.py:242-275); with cfg.icp_max_iter > 0 also T_est_icp, rte_icp,
    rre_icp, chamfer_dist_icp and icp_iters of the refined pose.  cfg.max_log_scale > 0: the posed copy is s R x + t with
    s = exp(u); the result keys do not change for that alone.  cfg.icp_with_scaling: T_est_icp is a similarity, rte_icp / rre_icp are
    eval_pose's on it with its 3x3 block divided by the fitted scale, and the results gain scale_gt, scale_icp and
    scale_err_icp = |scale_icp / scale_gt - 1|.  cfg.features = "fpfh": the descriptors are cs_fpfh's (FpfhPipe; `pipe` may
    be None, no checkpoint is needed) and the registration runs without the symmetry hypotheses, so the *_sym entries equal
    the *_ransac ones; the result keys do not change.  cfg.partial_view: the posed copy of every job is reduced to
    what one camera sees of it (partial_views) before the descriptors; every result gains visible_share, and a dict passed as
    `stat` gains stat["partial_view"] = {clouds, rows_in, rows_visible, views_skipped}."""
    cfg = cfg or Config()
    cfg.check_partial_view()
    if cfg.features not in ("network", "fpfh"):
        raise ValueError("Config.features must be 'network' or 'fpfh', got %r" % (cfg.features,))
    entry = cfg.check_registration()
    fpfh_on = cfg.features == "fpfh" and entry.descriptors
    use_symmetry = not fpfh_on and entry.no_symmetry is None
    if fpfh_on:
        pipe = FpfhPipe("cuda" if pipe is None else pipe.device, cfg.fpfh_radius, cfg.fpfh_max_nn)
    if not entry.descriptors:
        pipe = PpfPipe("cuda" if pipe is None else pipe.device)
    icp_on = cfg.icp_max_iter > 0
    scale_on = bool(cfg.icp_with_scaling)
    if scale_on and not icp_on:
        raise ValueError("Config.icp_with_scaling needs icp_max_iter > 0 (the refinement is off)")
    if scale_on and cfg.icp_kernel != "l2":
        raise ValueError("Config.icp_with_scaling with a robust icp_kernel (%r) is out of scope" % (cfg.icp_kernel,))
    if not 0 <= float(cfg.max_log_scale) < float("inf"):
        raise ValueError("Config.max_log_scale must be finite and >= 0, got %r" % (cfg.max_log_scale,))
    rng = np.random.default_rng(cfg.random_seed if seed is None else seed)
    dev = pipe.device
    jobs = build_jobs(clouds, cfg, rng)
    view_seed = cfg.random_seed if seed is None else seed
    view_stat = dict(clouds=0, rows_in=0, rows_visible=0, views_skipped=0)
    results = []
    for s in range(0, len(jobs), pairs_per_batch):
        chunk = jobs[s:s + pairs_per_batch]
        # one forward over [all models | all posed copies] of the chunk, every cloud quantised in its own type
        groups = []
        for col in (2, 3):
            xyz = torch.from_numpy(np.concatenate([j[col] for j in chunk])).to(dev)
            offsets = np.concatenate([[0], np.cumsum([len(j[col]) for j in chunk])]).tolist()
            if col == 3 and cfg.partial_view:
                rows_in = offsets[-1]
                xyz, offsets, shares, skipped, eyes = partial_views_with_cameras(xyz, offsets, [j[col] for j in chunk], cfg,
                                                                                 view_seed, s)
                view_stat["clouds"] += len(chunk)
                view_stat["rows_in"] += int(rows_in)
                view_stat["rows_visible"] += int(offsets[-1])
                view_stat["views_skipped"] += int(skipped)
            groups.append((xyz, offsets))
        es = pipe.embed_groups(groups, cfg.voxel_size)
        P = len(chunk)
        base = es.gather(list(range(P)))
        posed = es.gather(list(range(P, 2 * P)))
        labels = [j[5] for j in chunk]
        est_kw = cfg.registration_options(entry, base, eyes if cfg.partial_view else None)
        res = R.sym_pose_batch(base.F, base.origin, base.offsets, posed.F, posed.origin, posed.offsets,
                               labels, cfg.k_nn, cfg.max_corr, 0,
                               [(2 * (s + i), 2 * (s + i) + 1) for i in range(P)], 100,
                               cfg.ransac_max_iter, cfg.ransac_confidence, use_symmetry, force_gate, None,
                               cfg.icp_max_iter, cfg.icp_distance() if icp_on else None, cfg.icp_estimation,
                               cfg.icp_normal_k, None, cfg.normal_radius(), icp_with_scaling=scale_on,
                               icp_scale_bounds=tuple(cfg.icp_scale_bounds) if scale_on else None,
                               icp_kernel=cfg.icp_kernel,
                               icp_kernel_scale=cfg.icp_scale() if cfg.icp_kernel != "l2" else None,
                               registration=entry.name, gicp_epsilon=cfg.gicp_epsilon, **est_kw)
        Tb, Tr = res.T_best.cpu().numpy(), res.T_ransac.cpu().numpy()
        cdb, cdr = res.cd_best.cpu().numpy(), res.cd_ransac.cpu().numpy()
        for i, (mi, pi, _, _, pose, label, s_gt) in enumerate(chunk):
            rte_s, rre_s = eval_pose(Tb[i], np.eye(4), pose, axis_symmetry=label)
            rte_r, rre_r = eval_pose(Tr[i], np.eye(4), pose, axis_symmetry=label)
            results.append(dict(model=mi, pose_idx=pi, symmetry_label=label, sym_success=bool(res.ok[i]),
                                T_est_sym=Tb[i], chamfer_dist_sym=float(cdb[i]), T_est_ransac=Tr[i],
                                chamfer_dist_ransac=float(cdr[i]), rte_sym=float(rte_s), rre_sym=float(rre_s),
                                rte_ransac=float(rte_r), rre_ransac=float(rre_r), pose_gt=pose))
            if scale_on:
                results[-1]["scale_gt"] = s_gt
            if cfg.partial_view:
                results[-1]["visible_share"] = float(shares[i])
        if icp_on:
            Ti, cdi, iti = res.T_icp.cpu().numpy(), res.cd_icp.cpu().numpy(), res.icp_iters.cpu().numpy()
            sci = res.icp_scale.cpu().numpy() if scale_on else None
            for i, (_, _, _, _, pose, label, s_gt) in enumerate(chunk):
                Tl = Ti[i]
                if scale_on:             # eval_pose's trace formula assumes a rotation
                    Tl = Ti[i].copy()
                    Tl[:3, :3] = (Ti[i][:3, :3].astype(np.float64) / sci[i]).astype(Ti.dtype)
                rte_i, rre_i = eval_pose(Tl, np.eye(4), pose, axis_symmetry=label)
                results[s + i].update(T_est_icp=Ti[i], chamfer_dist_icp=float(cdi[i]), rte_icp=float(rte_i),
                                      rre_icp=float(rre_i), icp_iters=int(iti[i]))
                if scale_on:
                    results[s + i].update(scale_icp=float(sci[i]), scale_err_icp=float(abs(sci[i] / s_gt - 1.0)))
    if cfg.partial_view and stat is not None:
        stat["partial_view"] = view_stat
    return results


def _has_view(results):
    return bool(results) and "visible_share" in results[0]


def _has_icp(results):
    return bool(results) and "rre_icp" in results[0]


def _has_scale(results):
    return bool(results) and "scale_err_icp" in results[0]


def threshold_table(results, rre_deg=(5, 15, 45), rte=(0.02, 0.05, 0.10, 0.15)):
    """compute_metrics_shapenet.py-style summary: fraction of cases under each threshold."""
    out = {}
    for tag in ("ransac", "sym") + (("icp",) if _has_icp(results) else ()):
        r = np.array([x[f"rre_{tag}"] for x in results])
        t = np.array([x[f"rte_{tag}"] for x in results])
        out[tag] = {**{f"rre<={d}": float(np.mean(r <= np.deg2rad(d))) for d in rre_deg},
                    **{f"rte<={v}": float(np.mean(t <= v)) for v in rte}}
    if _has_scale(results):          # (Scan2CAD accepts an alignment whose scale is within 20 %)
        e = np.array([x["scale_err_icp"] for x in results])
        out["icp"].update({f"scale<={v}": float(np.mean(e <= v)) for v in SCALE_THRESHOLDS})
    return out


# ---- file-level entry: `python -m corsair_amd.shapenet_eval` (evaluation-shapenet.py:158-240,277-380) ---------------------
CSV_COLUMNS = ("model", "pose_idx", "symmetry_label", "sym_success", "rte_sym", "rre_sym", "cd_sym", "rte_ransac",
               "rre_ransac", "cd_ransac")            # evaluation-shapenet.py:323-334
ICP_CSV_COLUMNS = ("rte_icp", "rre_icp", "cd_icp", "icp_iters")      # trailing, only when the refinement ran
SCALE_CSV_COLUMNS = ("scale_gt", "scale_icp", "scale_err_icp")       # trailing, only when the refinement fitted a scale
VIEW_CSV_COLUMNS = ("visible_share",)                                # trailing, only when the posed copies were partial views
SCALE_THRESHOLDS = (0.05, 0.10, 0.20)


def write_results(results, names, csv_file, npz_file):
    """results-*.csv with the reference's columns and poses-*.npz with poses_gt / poses_pred_sym / poses_pred_ransac
    (evaluation-shapenet.py:345-380); results of a run with ICP refinement add the trailing ICP_CSV_COLUMNS and
    poses_pred_icp, those of one with a fitted scale also the SCALE_CSV_COLUMNS and the arrays of the same names, those of one
    on partial views the VIEW_CSV_COLUMNS and the array visible_share."""
    import csv

    icp = _has_icp(results)
    sc = _has_scale(results)
    pv = _has_view(results)
    with open(csv_file, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS + (ICP_CSV_COLUMNS if icp else ()) + (SCALE_CSV_COLUMNS if sc else ()) +
                   (VIEW_CSV_COLUMNS if pv else ()))
        for r in results:
            w.writerow([names[r["model"]], r["pose_idx"], r["symmetry_label"], r["sym_success"], r["rte_sym"], r["rre_sym"],
                        r["chamfer_dist_sym"], r["rte_ransac"], r["rre_ransac"], r["chamfer_dist_ransac"]] +
                       ([r["rte_icp"], r["rre_icp"], r["chamfer_dist_icp"], r["icp_iters"]] if icp else []) +
                       ([r[k] for k in SCALE_CSV_COLUMNS] if sc else []) + ([r[k] for k in VIEW_CSV_COLUMNS] if pv else []))
    extra = {"poses_pred_icp": np.stack([r["T_est_icp"] for r in results])} if icp else {}
    if sc:
        extra.update({k: np.asarray([r[k] for r in results], np.float64) for k in SCALE_CSV_COLUMNS})
    if pv:
        extra.update({k: np.asarray([r[k] for r in results], np.float64) for k in VIEW_CSV_COLUMNS})
    with open(npz_file, "wb") as f:
        np.savez(f, poses_gt=np.stack([r["pose_gt"] for r in results]),
                 poses_pred_sym=np.stack([r["T_est_sym"] for r in results]),
                 poses_pred_ransac=np.stack([r["T_est_ransac"] for r in results]), **extra)


def summary(results):
    """The three lines evaluation-shapenet.py:226-234 prints; each gains an `icp` entry when the refinement ran."""
    icp = _has_icp(results)
    r = {k: np.asarray([x[k] for x in results])
         for k in ("rte_sym", "rte_ransac", "rre_sym", "rre_ransac") + (("rte_icp", "rre_icp") if icp else ())}
    n, five = len(results), np.deg2rad(5)
    lines = []
    for title, fs, fr in (("RTE <= 0.02", r["rte_sym"] <= 0.02, r["rte_ransac"] <= 0.02),
                          ("RRE <= 5 deg", r["rre_sym"] <= five, r["rre_ransac"] <= five),
                          ("RTE <= 0.02 & RRE <= 5 deg", (r["rte_sym"] <= 0.02) & (r["rre_sym"] <= five),
                           (r["rte_ransac"] <= 0.02) & (r["rre_ransac"] <= five))):
        lines.append(f"{title}: sym: {fs.sum() / n:.4f}, ransac: {fr.sum() / n:.4f}")
    if icp:
        ti, ri = r["rte_icp"] <= 0.02, r["rre_icp"] <= five
        for i, f in enumerate((ti, ri, ti & ri)):
            lines[i] += f", icp: {f.sum() / n:.4f}"
    if _has_scale(results):
        e = np.asarray([x["scale_err_icp"] for x in results])
        lines.append("scale error " + ", ".join(f"<= {v:.2f}: {np.mean(e <= v):.4f}" for v in SCALE_THRESHOLDS))
    return "\n".join(lines)


def build_parser():
    import argparse

    ap = argparse.ArgumentParser(prog="python -m corsair_amd.shapenet_eval",
                                 description="Registration evaluation with synthetic poses on a directory of .npy clouds "
                                             "(evaluation-shapenet.py:158-240): writes results-*.csv / poses-*.npz")
    ap.add_argument("--data-dir", help="directory of [n,3] .npy clouds; or --shapenet-root + --category as in the reference")
    ap.add_argument("--shapenet-root")
    ap.add_argument("--category", default="chair", choices=["chair", "table"])
    ap.add_argument("--n-models", type=int, default=1)
    ap.add_argument("--n-poses-per-model", type=int, default=10)
    ap.add_argument("--max-roll-deg", type=float, default=360)
    ap.add_argument("--max-pitch-deg", type=float, default=360)
    ap.add_argument("--max-yaw-deg", type=float, default=360)
    ap.add_argument("--max-translation", type=float, default=1.0)
    ap.add_argument("--model-ckpt", "--ckpt", dest="ckpt", help="required unless --features fpfh")
    ap.add_argument("--features", default="network", choices=["network", "fpfh"],
                    help="descriptors: the network's, or FPFH (cs_fpfh: no checkpoint, no symmetry hypotheses)")
    ap.add_argument("--fpfh-radius", type=float, default=5.0, help="FPFH radius in voxels (Open3D's example value, untuned)")
    ap.add_argument("--fpfh-max-nn", type=int, default=100, help="FPFH max_nn, in [4, 128]")
    ap.add_argument("--random-seed", type=int, default=0)
    ap.add_argument("--ransac-max-iter", type=int, default=100000)
    ap.add_argument("--icp-iters", type=int, default=0,
                    help="refine every kept pose with at most N ICP updates (0 = off, the reference's behaviour)")
    ap.add_argument("--icp-max-dist", type=float, default=0.0, help="ICP correspondence distance; 0 = 2 * voxel size")
    ap.add_argument("--icp-estimation", default="point", choices=["point", "plane", "gicp"])
    ap.add_argument("--gicp-epsilon", type=float, default=1e-3,
                    help="covariance floor along the normal for --icp-estimation gicp, in [2^-10, 1] (Open3D's default, untuned)")
    ap.add_argument("--icp-normal-k", type=int, default=16)
    ap.add_argument("--icp-normal-radius", type=float, default=0.0,
                    help="radius of the normals' hybrid search (at most --icp-normal-k rows inside it); 0 = k-NN (untuned)")
    ap.add_argument("--icp-kernel", default="l2", choices=["l2", "huber", "cauchy", "tukey"],
                    help="robust kernel on the point-to-plane residual (needs --icp-estimation plane); l2 = none")
    ap.add_argument("--icp-kernel-scale", type=float, default=0.0, help="scale of --icp-kernel; 0 = 1 * voxel size (untuned)")
    ap.add_argument("--max-log-scale", type=float, default=0.0,
                    help="the posed copy is also scaled by exp(u), u uniform in +-this (0 = the reference's rigid poses)")
    ap.add_argument("--icp-with-scaling", action="store_true",
                    help="the ICP refinement also fits an isotropic scale (needs --icp-iters > 0, no robust kernel)")
    ap.add_argument("--icp-scale-min", type=float, default=0.5, help="lower bound of the fitted scale, in (0, 1] (untuned)")
    ap.add_argument("--icp-scale-max", type=float, default=2.0, help="upper bound of the fitted scale, >= 1 (untuned)")
    ap.add_argument("--registration", default="ransac", choices=list(E.NAMES),
                    help="correspondence estimator: the reference's RANSAC, Fast Global Registration (cs_fgr_batch), "
                         "feature-matching RANSAC with a mutual filter and pose checkers (cs_ransac_fm_batch; no symmetry "
                         "hypotheses), the compatibility-graph estimator for low inlier shares (cs_sc2_batch), or "
                         "point-pair-feature voting on the voxels and their normals (cs_ppf_batch; no descriptors, no "
                         "--ckpt, no symmetry hypotheses)")
    ap.add_argument("--fgr-mu-floor", type=float, default=0.025,
                    help="floor of FGR's mu, in units of the clouds' radius (Open3D's default, untuned)")
    ap.add_argument("--fm-ransac-n", type=int, default=3, choices=[3, 4],
                    help="pairs per hypothesis of --registration ransac_fm (Open3D's default; untuned, no real scan measured)")
    ap.add_argument("--fm-edge-similarity", type=float, default=0.9,
                    help="edge-length checker of ransac_fm, in [0, 1]; 0 = off (Open3D's default; untuned, no real scan "
                         "measured)")
    ap.add_argument("--fm-no-mutual", action="store_true",
                    help="ransac_fm keeps every 1-NN match instead of the mutual ones (untuned, no real scan measured)")
    ap.add_argument("--fm-iterations", type=int, default=100000,
                    help="hypotheses per pair of ransac_fm, a fixed number (Open3D's default; untuned, no real scan measured)")
    ap.add_argument("--sc2-compat-dist", type=float, default=1.0,
                    help="two correspondences of --registration sc2 are compatible when their source and target distances "
                         "differ by less than this, in voxels (untuned, no real scan measured)")
    ap.add_argument("--sc2-seeds", type=int, default=1024,
                    help="correspondences of the largest degree that sc2 tries, 0 = all (untuned, no real scan measured)")
    ap.add_argument("--sc2-k", type=int, default=20,
                    help="correspondences a seed of sc2 is fitted over beside itself, in [2, 64] (untuned, no real scan "
                         "measured)")
    ap.add_argument("--ppf-ref-step", type=int, default=5,
                    help="every n-th row of the posed copy is a reference of --registration ppf (untuned, no real scan "
                         "measured)")
    ap.add_argument("--ppf-n-cand", type=int, default=16,
                    help="references with the most votes that ppf verifies, in [1, 64] (untuned, no real scan measured)")
    ap.add_argument("--ppf-dist-step", type=float, default=0.05,
                    help="distance step of ppf as a fraction of the model's bounding-box diagonal (Drost et al.'s sampling; "
                         "untuned, no real scan measured)")
    ap.add_argument("--partial-view", action="store_true",
                    help="reduce the posed copy of every pair to what one virtual depth camera sees of it (cs_render_views; "
                         "the model stays whole)")
    ap.add_argument("--view-fov", type=float, default=40.0,
                    help="field of view of that camera in degrees, in (0, 180) (untuned, no real scan measured)")
    ap.add_argument("--view-size", type=int, default=256,
                    help="side of its square image in pixels, in [1, 4096] (untuned, no real scan measured)")
    ap.add_argument("--view-distance", type=float, default=3.0,
                    help="its distance from the cloud in half diagonals of the bounding box, > 1 (untuned, no real scan measured)")
    ap.add_argument("--view-point-size", type=float, default=1.5,
                    help="side of a row's square in voxels (untuned, no real scan measured)")
    ap.add_argument("--view-depth-tol", type=float, default=1.5,
                    help="depth tolerance of the visibility test in voxels (untuned, no real scan measured)")
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--device", default="cuda", choices=["cuda"])
    return ap


def main(argv=None):
    import os

    from . import harness
    from .utils import ckpts

    a = build_parser().parse_args(argv)
    if a.icp_kernel != "l2" and a.icp_estimation != "plane":
        raise SystemExit("--icp-kernel %s needs --icp-estimation plane" % a.icp_kernel)
    if not a.data_dir:
        if not a.shapenet_root:
            raise SystemExit("give --data-dir, or --shapenet-root with --category")
        a.data_dir = os.path.join(a.shapenet_root, {"chair": "03001627", "table": "04379243"}[a.category], "test")
    files = sorted(f for f in os.listdir(a.data_dir) if f.endswith(".npy"))
    rng = np.random.default_rng(a.random_seed)
    if 0 < a.n_models < len(files):                                   # evaluation-shapenet.py:200-203
        files = sorted(rng.choice(files, a.n_models, replace=False).tolist())
    clouds = [np.load(os.path.join(a.data_dir, f)) for f in files]
    if a.features == "fpfh" or not E.lookup(a.registration, "--registration").descriptors:
        pipe = None
    else:
        if not a.ckpt:
            raise SystemExit("--ckpt is required with --features network")
        sd, esd = ckpts.load_state_dicts(a.ckpt)
        pipe = harness.Pipeline(sd, esd, device=a.device)
    cfg = Config(random_seed=a.random_seed, n_poses_per_model=a.n_poses_per_model, max_roll_deg=a.max_roll_deg,
                 max_pitch_deg=a.max_pitch_deg, max_yaw_deg=a.max_yaw_deg, max_translation=a.max_translation,
                 ransac_max_iter=a.ransac_max_iter, icp_max_iter=a.icp_iters, icp_max_dist=a.icp_max_dist,
                 icp_estimation=a.icp_estimation, icp_normal_k=a.icp_normal_k, icp_kernel=a.icp_kernel,
                 icp_kernel_scale=a.icp_kernel_scale, icp_normal_radius=a.icp_normal_radius, max_log_scale=a.max_log_scale,
                 icp_with_scaling=a.icp_with_scaling, icp_scale_bounds=(a.icp_scale_min, a.icp_scale_max),
                 registration=a.registration, fgr_mu_floor=a.fgr_mu_floor, gicp_epsilon=a.gicp_epsilon, features=a.features,
                 fpfh_radius=a.fpfh_radius, fpfh_max_nn=a.fpfh_max_nn, fm_ransac_n=a.fm_ransac_n,
                 fm_edge_similarity=a.fm_edge_similarity, fm_mutual=not a.fm_no_mutual, fm_iterations=a.fm_iterations,
                 sc2_compat_dist=a.sc2_compat_dist, sc2_seeds=a.sc2_seeds, sc2_k=a.sc2_k,
                 ppf_ref_step=a.ppf_ref_step, ppf_n_cand=a.ppf_n_cand, ppf_dist_step=a.ppf_dist_step,
                 partial_view=a.partial_view, view_fov_deg=a.view_fov, view_size=a.view_size, view_distance=a.view_distance,
                 view_point_size=a.view_point_size, view_depth_tol=a.view_depth_tol)
    cfg.check_partial_view()
    stat = {}
    results = evaluate(pipe, clouds, cfg, stat=stat)
    postfix = f"shapenet-seed{a.random_seed}-{a.category}-{len(files)}-{a.n_poses_per_model}"
    os.makedirs(a.out_dir, exist_ok=True)
    csv_file = os.path.join(a.out_dir, f"results-{postfix}.csv")
    npz_file = os.path.join(a.out_dir, f"poses-{postfix}.npz")
    write_results(results, files, csv_file, npz_file)
    print(summary(results))
    if "partial_view" in stat:
        pv = stat["partial_view"]
        print("partial views: %d clouds, %d of %d rows visible, %d views skipped"
              % (pv["clouds"], pv["rows_visible"], pv["rows_in"], pv["views_skipped"]))
    return results, csv_file, npz_file


if __name__ == "__main__":
    main()
