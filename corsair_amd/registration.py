"""Batched symmetry-aided registration on the GPU.

Counterpart of ``sym_pose`` (utils/symmetry.py:262-358 of the reference) for a whole batch of
(query, CAD) pairs at once: the reference runs the pairs one after another in Python
(evaluation.py:297-331) and each stage on the CPU (SciPy KD-trees, Open3D RANSAC, sklearn k-means);
here every stage is one batched HIP launch over all pairs / hypotheses:

  1. feature 5-NN correspondences query -> CAD                  cs_knn_feat
  2. symmetry part cut of both clouds (100 anchors each)        cs_symcut_fit + host gate + cs_symcut_labels
  3. per-part correspondences for every cyclic / mirrored
     part assignment (K or K+4 hypotheses per pair)             cs_knn_feat (labelled)
  4. one RANSAC per hypothesis, all in one call                 cs_ransac_batch
     (registration="fgr": Fast Global Registration instead)     cs_fgr_batch
     (registration="ransac_fm": 1-NN both ways + mutual filter in
      stage 1, RANSAC with the edge and distance checkers here)  cs_corr_mutual, cs_ransac_fm_batch
  5. one-directional Chamfer of every estimate                  cs_chamfer_1dir
  6. keep the estimate with the smallest Chamfer (first wins)   argmin

torch is used for index plumbing on the device (stable sort of part labels, gathers).
"""
from __future__ import annotations

import inspect
import os
from collections import namedtuple
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from . import _helper
from . import backend as B
from . import estimators as E
from . import featmatch as FM
from ._lib import to_host
from .estimators import check_fm_options, check_ppf_options, check_sc2_options  # noqa: F401  (their callers find them here)

ANCHOR_KEY = 0x5A11C0DE

# The vanilla RANSACs of a batch need nothing from the symmetry stages: they run on the helper thread
# (_helper.py) with its own stream while the calling thread goes through part cut, host gate and labelled
# 5-NN (a launch sequence with two host decisions in it, during which the GPU would otherwise idle), then
# the symmetric hypotheses get their own cs_ransac_batch call.  The draws of a problem depend on (seed,
# iteration) only, so splitting the call changes no result.  CORSAIR_SPLIT_RANSAC=0 keeps one call.


@dataclass
class SymPoseResult:
    T_best: torch.Tensor        # f32 [P,4,4]
    cd_best: torch.Tensor       # f64 [P]
    T_ransac: torch.Tensor      # f32 [P,4,4]
    cd_ransac: torch.Tensor     # f64 [P]
    ok: np.ndarray              # bool [P]  (sym_ransac_success)
    iters: torch.Tensor         # int32 [n_problems] RANSAC iterations consumed
    n_problems: int
    # every hypothesis evaluated (problem j): the first P are the vanilla find_kcorr RANSACs of the pairs,
    # then the part configurations of the pairs whose cut passed, pair-major, in the reference's order
    # (utils/symmetry.py:303-356)
    T_all: torch.Tensor = None      # f32 [n_problems,4,4]
    cd_all: torch.Tensor = None     # f64 [n_problems]
    inliers: torch.Tensor = None    # int32 [n_problems]
    prob_pair: list = None          # pair of problem j
    prob_cfg: list = None           # part assignment of problem j (None = vanilla)
    best: np.ndarray = None         # int64 [P] problem kept per pair (first strict Chamfer minimum)
    # ICP refinement of T_best (sym_pose_batch(icp_max_iter > 0)); None when it is off
    T_icp: torch.Tensor = None      # f32 [P,4,4]
    cd_icp: torch.Tensor = None     # f64 [P] one-directional Chamfer under T_icp (cs_chamfer_1dir)
    icp_fitness: torch.Tensor = None    # f64 [P]
    icp_rmse: torch.Tensor = None       # f64 [P]
    icp_iters: torch.Tensor = None      # int32 [P] updates applied
    icp_wfitness: torch.Tensor = None   # f64 [P] weighted inlier share; only with a robust icp_kernel
    icp_scale: torch.Tensor = None      # f64 [P] the isotropic scale the ICP added to T_best; only with icp_with_scaling
    icp_mrmse: torch.Tensor = None      # f64 [P] Mahalanobis rmse; only with icp_estimation = "gicp"

    def hypotheses(self, p):
        """Problems of pair p in evaluation order."""
        return [j for j, q in enumerate(self.prob_pair) if q == p]


def draw_anchors(n, n_anchor, counter):
    """np.random.choice(n, n_anchor, replace=False) (utils/symmetry.py:193) from an explicit Philox
    stream keyed by `counter` instead of NumPy's global RNG."""
    if n < n_anchor:
        return None
    gen = np.random.Generator(np.random.Philox(key=ANCHOR_KEY, counter=counter))
    return gen.choice(n, n_anchor, replace=False).astype(np.int32)


# The acceptance test of symmetric_cut4 is `dist.min() > 0.15 > max(error)` (utils/symmetry.py:232-257): the two
# thresholds are hyper-parameters tuned to TRAINED features (the reference's caches report sym_ransac_success for every
# query).  They are an argument here, default = the reference's constants.  GATE_ANY = "any finite model passes" is what
# bench.py uses with its random-init weights, under which the reference's thresholds never pass and 2/3 of the
# registration work would silently leave the timed region (`force_gate=True` of the entry points is shorthand for it).
GATE_REFERENCE = (0.15, 0.15)
GATE_ANY = (0.0, float("inf"))


def gate_and_order(centers, counts, min_cdist, max_err, n, K, gate=GATE_REFERENCE):
    """Acceptance gate + centre ordering of symmetric_cut4 (utils/symmetry.py:232-257) for one cloud.
    centers [A,4,3], counts [A,4], min_cdist/max_err [A] (NumPy).  Returns [4,3] centres ordered
    [0, nearest, farthest, middle] (K=4) or None when no anchor passes the gate."""
    ratios = counts[:, :K].astype(np.float64) / float(n)
    std = np.sqrt(np.var(ratios, axis=1))
    valid = (min_cdist > gate[0]) & (gate[1] > max_err) & (std < 100)
    if not valid.any():
        return None
    a = int(np.argmin(np.where(valid, std, np.inf)))
    c = centers[a]
    out = np.zeros((4, 3), np.float64)
    if K == 2:
        out[:2] = c[:2]
        return out
    d = np.linalg.norm(c[0][None, :] - c[1:4], axis=1)
    rank = np.argsort(d, kind="stable")
    out[:] = c[[0, rank[0] + 1, rank[2] + 1, rank[1] + 1]]
    return out


def gate_and_order_batch(centers, counts, min_cdist, max_err, n, Ks, cand, gate=GATE_REFERENCE):
    """gate_and_order for the pairs in `cand` at once (same arithmetic, NumPy over the pair axis).
    centers [P,A,4,3], counts [P,A,4], min_cdist / max_err [P,A], n [P], Ks [P].
    Returns (sel [P,4,3], ok [P])."""
    P = centers.shape[0]
    sel = np.zeros((P, 4, 3), np.float64)
    ok = np.zeros(P, dtype=bool)
    n = np.asarray(n, dtype=np.float64)
    Ks = np.asarray(Ks)
    cand = np.asarray(cand, dtype=np.int64)
    for K in (2, 4):
        idx = cand[Ks[cand] == K]
        if idx.size == 0:
            continue
        ratios = counts[idx][:, :, :K].astype(np.float64) / n[idx][:, None, None]
        std = np.sqrt(np.var(ratios, axis=2))
        valid = (min_cdist[idx] > gate[0]) & (gate[1] > max_err[idx]) & (std < 100)
        has = valid.any(axis=1)
        a = np.argmin(np.where(valid, std, np.inf), axis=1)
        c = centers[idx, a]                                   # [G,4,3]
        out = np.zeros((idx.size, 4, 3), np.float64)
        if K == 2:
            out[:, :2] = c[:, :2]
        else:
            d = np.linalg.norm(c[:, 0:1] - c[:, 1:4], axis=2)  # [G,3]
            rank = np.argsort(d, axis=1, kind="stable")
            order = np.stack([np.zeros(idx.size, np.int64), rank[:, 0] + 1, rank[:, 2] + 1, rank[:, 1] + 1], 1)
            out = np.take_along_axis(c, order[:, :, None], axis=1)
        sel[idx[has]] = out[has]
        ok[idx[has]] = True
    return sel, ok


def part_configs(K, pos_sym):
    """Part assignments tried by sym_pose: K cyclic shifts, plus 4 shifts of the mirrored order
    [0,3,2,1] when pos_sym >= 2 (utils/symmetry.py:303-356)."""
    cfgs = [[(i + s) % K for i in range(K)] for s in range(K)]
    if pos_sym >= 2:
        mirror = [0, 3, 2, 1]
        cfgs += [[mirror[(i + s) % 4] for i in range(4)] for s in range(4)]
    return cfgs


def _refuse_nonfinite(bad_query, bad_cad):
    """ValueError for the first pair whose descriptors hold a NaN or an infinite value (flags per pair, see step 1)."""
    for side, bad, said in (("CAD", bad_cad, "data must be finite"), ("query", bad_query, "'x' must be finite")):
        hit = np.flatnonzero(np.asarray(bad))
        if hit.size:
            raise ValueError("sym_pose_batch: the %s descriptors of pair %d hold a NaN or an infinite value (the "
                             "reference's KD-tree refuses them: %s)" % (side, int(hit[0]), said))


# What sym_pose_batch takes by keyword only, as it hands it to its body: the entry of estimators.TABLE, every estimator's options
# by keyword (as given or the table's default, unchecked), and the two ICP options that ride along
_KeywordOnly = namedtuple("_KeywordOnly", "entry options normals0 gicp_epsilon")


def _sym_pose_batch(estimator, baseF, xyz0, off0, posF, xyz1, off1, pos_syms, k_nn=5, max_corr=0.20, seed=0,
                    anchor_ids=None, n_anchor=100, max_iter=100000, confidence=0.999,
                    use_symmetry=True, force_gate=False, query_anchors=None, icp_max_iter=0, icp_max_dist=None,
                    icp_estimation="point", icp_normal_k=16, normals1=None, icp_normal_radius=None, icp_with_scaling=False,
                    icp_scale_bounds=None, icp_kernel="l2", icp_kernel_scale=None):
    """The body of sym_pose_batch (below, with the documentation).  estimator: the call's _KeywordOnly."""
    entry, normals0, gicp_epsilon = estimator.entry, estimator.normals0, estimator.gicp_epsilon
    # the options of every estimator are checked, the chosen one's kept by keyword; here, where max_corr is a parameter
    # (sc2_compat_dist = None is half of it)
    o = E.checked_options(entry, estimator.options, max_corr)
    if entry.no_symmetry and use_symmetry:
        raise ValueError("sym_pose_batch: registration %r needs use_symmetry=False (%s)" % (entry.name, entry.no_symmetry))
    if icp_estimation == "gicp" and (icp_with_scaling or icp_kernel != "l2"):
        raise ValueError("sym_pose_batch: icp_estimation 'gicp' with icp_with_scaling or a robust icp_kernel is out of scope")
    if icp_estimation != "gicp" and normals0 is not None and entry.descriptors:
        raise ValueError("sym_pose_batch: normals0 is used by icp_estimation = 'gicp' only")
    if icp_with_scaling and icp_kernel != "l2":
        raise ValueError("sym_pose_batch: icp_with_scaling with a robust icp_kernel (%r) is out of scope" % (icp_kernel,))
    if icp_kernel not in B.ICP_KERNELS:
        raise ValueError("sym_pose_batch: icp_kernel must be one of %s, got %r" % (sorted(B.ICP_KERNELS), icp_kernel))
    if icp_kernel != "l2" and icp_estimation != "plane":
        raise ValueError("sym_pose_batch: icp_kernel %r needs icp_estimation = 'plane'" % (icp_kernel,))
    if icp_max_iter > 0 and icp_kernel != "l2" and not (icp_kernel_scale is not None and icp_kernel_scale > 0):
        raise ValueError("sym_pose_batch: icp_kernel %r needs a positive icp_kernel_scale" % (icp_kernel,))
    if icp_estimation not in ("point", "plane", "gicp"):
        raise ValueError("sym_pose_batch: icp_estimation must be 'point', 'plane' or 'gicp', got %r" % (icp_estimation,))
    if icp_normal_radius is not None and not (0 < icp_normal_radius < float("inf")):
        raise ValueError("sym_pose_batch: icp_normal_radius must be positive and finite (None = k-NN), got %r"
                         % (icp_normal_radius,))
    if icp_max_iter > 0 and not (icp_max_dist is not None and icp_max_dist > 0):
        raise ValueError("sym_pose_batch: icp_max_iter > 0 needs a positive icp_max_dist")
    if use_symmetry and baseF.shape[1] not in (16, 32):
        raise ValueError("sym_pose_batch: use_symmetry needs 16- or 32-wide descriptors (cs_symcut_fit), got %d columns; "
                         "FPFH descriptors (33) register with use_symmetry=False" % (baseF.shape[1],))
    dev = baseF.device if entry.descriptors else xyz0.device      # descriptors that are not read may be None
    P = len(off0) - 1
    off0 = [int(v) for v in off0]
    off1 = [int(v) for v in off1]
    n0 = [off0[p + 1] - off0[p] for p in range(P)]
    n1 = [off1[p + 1] - off1[p] for p in range(P)]
    k = entry.k or k_nn      # the feature-matching recipe takes 1-NN matches; k_nn is not used

    def finish(T, inl, iters, prob_pair, prob_cfg, ok, nonfinite):
        """Stages 5 - 7, the same behind every estimator."""
        # ---- 5. Chamfer of every estimate (utils/preprocess.py:39-48,67-70) -----------------------------
        cd = B.chamfer_1dir(xyz0, off0, xyz1, off1, prob_pair, prob_pair, T)

        # ---- 6. best hypothesis per pair: first minimum, vanilla first (utils/symmetry.py:322-324) ----
        if nonfinite is not None:
            cd_h, bad_q, bad_c = to_host(cd, *nonfinite)   # (every launch above has finished, the helper's RANSAC included)
            _refuse_nonfinite(bad_q, bad_c)
        else:
            cd_h = to_host(cd)[0]
        pair_h = np.asarray(prob_pair)
        best = np.arange(P)
        for j in range(P, len(pair_h)):
            p = pair_h[j]
            if cd_h[best[p]] > cd_h[j]:
                best[p] = j
        best_t = torch.from_numpy(best).to(dev)
        res = SymPoseResult(T_best=T[best_t], cd_best=cd[best_t], T_ransac=T[:P], cd_ransac=cd[:P],
                            ok=ok, iters=iters, n_problems=len(prob_pair), T_all=T, cd_all=cd, inliers=inl,
                            prob_pair=prob_pair, prob_cfg=prob_cfg, best=best)

        # ---- 7. optional refinement of the kept estimate on the geometry itself (Open3D: registration_icp) ----
        if icp_max_iter > 0:
            pairs = list(range(P))
            nrm = None
            if icp_estimation in ("plane", "gicp"):
                nrm = normals1 if normals1 is not None else B.estimate_normals(xyz1, off1, icp_normal_k, icp_normal_radius)
            scaling = {}
            if icp_with_scaling:
                scaling = {"with_scaling": True}
                if icp_scale_bounds is not None:
                    scaling["scale_bounds"] = icp_scale_bounds
            if icp_estimation == "gicp":     # the query voxels' normals, in the query's own (posed) frame
                snrm = normals0 if normals0 is not None else B.estimate_normals(xyz0, off0, icp_normal_k, icp_normal_radius)
                scaling = {"estimation": "gicp", "src_normals": snrm, "gicp_epsilon": gicp_epsilon}
            r = B.icp_batch(xyz0, off0, xyz1, off1, pairs, pairs, res.T_best, icp_max_dist, icp_max_iter, tgt_normals=nrm,
                            kernel=icp_kernel, kernel_scale=icp_kernel_scale, **scaling)
            res.T_icp, res.icp_fitness, res.icp_rmse, res.icp_iters = r.T32, r.fitness, r.rmse, r.iters
            res.icp_wfitness = r.wfitness
            res.icp_scale = r.scale
            res.icp_mrmse = r.mrmse
            res.cd_icp = B.chamfer_1dir(xyz0, off0, xyz1, off1, pairs, pairs, r.T32)
        return res

    if not entry.descriptors:
        # ---- 4'. point-pair-feature voting on the geometry itself: no descriptors, no correspondence lists ----
        side = o["ppf_scene_side"]
        clouds, offs, given = (xyz0, xyz1), (off0, off1), (normals0, normals1)
        nrm = []
        for c in (side, 1 - side):                       # the scene, then the model
            v = given[c]
            if v is None:
                v = B.estimate_normals(clouds[c], offs[c], icp_normal_k, icp_normal_radius)
                towards = o["ppf_view_points"] if c == side else None
                B.orient_normals(clouds[c], offs[c], v, towards, towards is None)
            nrm.append(v)
        T, inl, _, iters = E.run_stage4(entry, o, SimpleNamespace(
            clouds=(clouds[side], clouds[1 - side]), normals=nrm, offs=(offs[side], offs[1 - side]), max_corr=max_corr))
        return finish(T, inl, iters, list(range(P)), [None] * P, np.zeros(P, dtype=bool), None)

    # ---- 1. vanilla correspondences (find_kcorr, utils/eval_pose.py:48-79) -----------------
    # A CAD cloud with fewer than k voxels has no k-th neighbour: SciPy's KD-tree returns the out-of-range index n
    # there and the reference's fancy indexing raises IndexError (utils/eval_pose.py:66-72).  Same here, before any
    # launch.  (This excludes the -1 entries of SHORT CAD clouds only; those of non-finite descriptors are found on the
    # device, below, and k_corr_assemble reads the cloud's row 0 through any that is left.)
    short = [p for p in range(P) if n0[p] > 0 and n1[p] < k]
    if short:
        raise IndexError("sym_pose_batch: CAD cloud of pair %d has %d voxels, fewer than k_nn = %d (the reference's "
                         "find_kcorr fails on such a pair too)" % (short[0], n1[short[0]], k))
    nn = B.knn_feat(baseF, off0, posF, off1, k)                     # [N0, k] local CAD rows
    # Descriptors that are not finite (row_l2_normalize at eps = 0 turns a zero row into NaN): SciPy's KD-tree refuses
    # them -- "data must be finite" when the CAD tree is built, "'x' must be finite" on the query -- and so does this
    # function, with ValueError.  Two flags per pair, made on the device behind the search: a query row with a
    # non-finite element has -1 in its whole list (n1 >= k is known), which is cs_cfg_bad over the vanilla list with
    # one range per pair; a CAD row leaves no -1, so cs_rows_nonfinite looks at posF itself.  They come to the host
    # with a download the function waits for anyway (the part-cut statistics, else the Chamfer distances of stage
    # 6): no wait of their own.  Until then the lists go on as they are -- a -1 reads as the CAD cloud's row 0 --
    # and nothing made from them is returned.
    nonfinite = None
    if P:
        pair_rows = torch.from_numpy(np.asarray(off0 + off1, dtype=np.int64)).to(dev, non_blocking=True)
        nonfinite = (B.cfg_bad(nn, pair_rows[:P + 1], P), B.rows_nonfinite(posF, pair_rows[P + 1:], P))
    # correspondence lists straight from the neighbour lists (one launch; rounds 1-2 built index tensors with
    # repeat_interleave / arange / gathers): pair p = query rows off0[p]:off0[p+1] against the CAD cloud at off1[p]
    fm_m = None
    if entry.name == "ransac_fm":
        # the backward 1-NN (the segments swap their roles), then the mutual filter with Open3D's fallback on the device:
        # pair p's correspondences fill the slots off0[p]... and their number stays on the device (fm_m)
        nn_bwd = B.knn_feat(posF, off1, baseF, off0, 1) if o["fm_mutual"] else None
        v_src, v_tgt, fm_m, _ = FM.mutual_correspondences(nn, nn_bwd, xyz0, off0, xyz1, off1, o["fm_ransac_n"], o["fm_mutual"])
    else:
        desc_v = np.asarray([[off0[p], off0[p], off1[p], n0[p], off0[p]] for p in range(P)], dtype=np.int64).reshape(P, 5)
        v_src, v_tgt = B.corr_assemble(xyz0, xyz1, None, nn, desc_v, off0[-1], max(n0) if P else 0)
    corr_src = [v_src]
    corr_tgt = [v_tgt]
    prob_len = [n0[p] * k for p in range(P)]
    prob_pair = list(range(P))
    prob_cfg = [None] * P
    ok = np.zeros(P, dtype=bool)
    vanilla = None
    if entry.name == "ransac" and use_symmetry and dev.type == "cuda" and \
            os.environ.get("CORSAIR_SPLIT_RANSAC", "1") != "0":
        v_offs = np.concatenate([[0], np.cumsum(prob_len)]).tolist()
        for t in (v_src, v_tgt):
            t.record_stream(_helper.stream(dev))
        vanilla = _helper.submit(dev, lambda: B.ransac_batch(v_src, v_tgt, v_offs, max_corr, 10, max_iter,
                                                            confidence, seed))

    try:
        # ---- 2./3. symmetry hypotheses ---------------------------------------------------------------
        if use_symmetry:
            Ks = [4 if int(pos_syms[p]) >= 2 else 2 for p in range(P)]
            if anchor_ids is None:
                anchor_ids = [(2 * p, 2 * p + 1) for p in range(P)]
            anc0 = query_anchors if query_anchors is not None else \
                [draw_anchors(n0[p], n_anchor, anchor_ids[p][0]) for p in range(P)]
            anc1 = [draw_anchors(n1[p], n_anchor, anchor_ids[p][1]) for p in range(P)]
            cand = [p for p in range(P) if anc0[p] is not None and anc1[p] is not None]
            sel0 = np.zeros((P, 4, 3))
            sel1 = np.zeros((P, 4, 3))
            if cand:
                # one launch set for both sides (query clouds, then CAD clouds): the k-means stage is
                # latency-bound (one thread per restart), twice the clouds cost the same time
                def anchors_of(anc):
                    return np.stack([anc[p] if anc[p] is not None else np.zeros(n_anchor, np.int32) for p in range(P)])

                a_all = torch.from_numpy(np.concatenate([anchors_of(anc0), anchors_of(anc1)])).to(dev)
                off_all = off0 + [off0[-1] + o for o in off1[1:]]
                c, cnt, mcd, mer = B.symcut_fit(torch.cat([baseF, posF]), torch.cat([xyz0, xyz1]), off_all, a_all,
                                                Ks + Ks, 50, 10, 300)
                if nonfinite is not None:
                    c, cnt, mcd, mer, bad_q, bad_c = to_host(c, cnt, mcd, mer, *nonfinite)
                    nonfinite = None
                    _refuse_nonfinite(bad_q, bad_c)
                else:
                    c, cnt, mcd, mer = to_host(c, cnt, mcd, mer)
                c0, cnt0, mcd0, mer0 = c[:P], cnt[:P], mcd[:P], mer[:P]
                c1, cnt1, mcd1, mer1 = c[P:], cnt[P:], mcd[P:], mer[P:]
                gate = GATE_ANY if force_gate else GATE_REFERENCE
                g0, ok0 = gate_and_order_batch(c0, cnt0, mcd0, mer0, n0, Ks, cand, gate)
                g1, ok1 = gate_and_order_batch(c1, cnt1, mcd1, mer1, n1, Ks, cand, gate)
                ok = ok0 & ok1
                sel0[ok], sel1[ok] = g0[ok], g1[ok]
            good = [p for p in range(P) if ok[p]]
            if good:
                lab0 = B.symcut_labels(xyz0, off0, Ks, torch.from_numpy(sel0).to(dev))
                lab1 = B.symcut_labels(xyz1, off1, Ks, torch.from_numpy(sel1).to(dev))
                qseg, tseg, perms, cfg_pair = [], [], [], []
                for p in good:
                    for cfg in part_configs(Ks[p], int(pos_syms[p])):
                        qseg.append(p)
                        tseg.append(p)
                        perms.append(cfg + [-3] * (8 - len(cfg)))
                        cfg_pair.append(p)
                # one small upload for everything the device needs from the host here: segment offsets,
                # configuration row ranges, part permutations
                lens = np.asarray([n0[p] for p in cfg_pair], dtype=np.int64)
                row_start = np.concatenate([[0], np.cumsum(lens)])
                n_cfg = len(cfg_pair)
                host_blk = np.concatenate([np.asarray(off0, np.int64), row_start,
                                           np.asarray(perms, np.int32).reshape(-1).view(np.int64)])
                dev_blk = torch.from_numpy(host_blk).to(dev)
                off0_t = dev_blk[:P + 1]
                first_t = dev_blk[P + 1:P + 2 + n_cfg]
                perm_t = dev_blk[P + 2 + n_cfg:].view(torch.int32).view(n_cfg, 8)
                # stable partition of every query cloud by part label (split_corr concatenates the parts
                # in order, rows in original order inside a part): one launch.  The labelled search runs on
                # the partitioned rows, so a wave of 64 queries shares one label and skips the targets of
                # the other parts wholesale.
                sorted_rows = B.partition_by_label(lab0, off0_t, P)
                nn_cfg = B.knn_feat(baseF[sorted_rows], off0, posF, off1, k, qseg=qseg, tseg=tseg,
                                    qlabel=lab0[sorted_rows].contiguous(), tlabel=lab1, perm=perm_t)
                # configuration j owns the query rows sorted_rows[off0[p] : off0[p+1]] and the result rows
                # nn_cfg[row_start[j] : row_start[j+1]].  A CAD part with fewer than k voxels leaves -1 entries:
                # the reference cannot build that configuration (one launch + one small copy decide all of them)
                bad = to_host(B.cfg_bad(nn_cfg, first_t, n_cfg))[0] > 0
                keep = [j for j in range(n_cfg) if not bad[j]]
                if keep:
                    out_first = np.concatenate([[0], np.cumsum(lens[keep])])
                    desc = np.asarray([[off0[cfg_pair[j]], row_start[j], off1[cfg_pair[j]], lens[j], out_first[i]]
                                       for i, j in enumerate(keep)], dtype=np.int64)
                    s_src, s_tgt = B.corr_assemble(xyz0, xyz1, sorted_rows, nn_cfg, desc, int(out_first[-1]),
                                                   int(lens[keep].max()))
                    corr_src.append(s_src)
                    corr_tgt.append(s_tgt)
                    for j in keep:
                        prob_len.append(n0[cfg_pair[j]] * k)
                        prob_pair.append(cfg_pair[j])
                        prob_cfg.append([c for c in perms[j] if c >= 0])
    except BaseException:
        if vanilla is not None:       # do not leave the helper's call running into freed tensors
            try:
                vanilla.result()
            except Exception:
                pass
        raise

    # ---- 4. RANSAC over all hypotheses (registration_based_on_corr, utils/eval_pose.py:82-100) ----
    if vanilla is None:
        src = corr_src[0] if len(corr_src) == 1 else torch.cat(corr_src)
        tgt = corr_tgt[0] if len(corr_tgt) == 1 else torch.cat(corr_tgt)
        offs = np.concatenate([[0], np.cumsum(prob_len)]).tolist()
        T, inl, rmse, iters = E.run_stage4(entry, o, SimpleNamespace(
            src=src, tgt=tgt, offs=offs, m=fm_m, max_corr=max_corr, max_iter=max_iter, confidence=confidence, seed=seed))
    else:
        parts = []
        if len(corr_src) > 1:
            offs = np.concatenate([[0], np.cumsum(prob_len[P:])]).tolist()
            parts = [B.ransac_batch(corr_src[1], corr_tgt[1], offs, max_corr, 10, max_iter, confidence, seed)]
        first = vanilla.result()              # cs_ransac_batch returns with its stream drained
        cur = torch.cuda.current_stream(dev)
        for t in first:
            t.record_stream(cur)
        T, inl, rmse, iters = (torch.cat([a] + [q[i] for q in parts]) for i, a in enumerate(first))

    return finish(T, inl, iters, prob_pair, prob_cfg, ok, nonfinite)


def sym_pose_batch(*args, registration="ransac", fgr_mu_floor=0.025, fgr_iterations=64, fgr_tuple_test=True, **kwargs):
    """baseF f32 [N0,16], xyz0 f32 [N0,3] (query voxels of all pairs, segment p = off0[p]:off0[p+1]);
    posF/xyz1/off1 likewise for the CAD side; pos_syms: symmetry label per pair.
    Refused like the reference: IndexError for a CAD cloud with fewer than k_nn voxels, ValueError (naming the pair and the
    side, query or CAD) for descriptors with a NaN or infinite value -- raised before the function returns, once every
    launch it made has finished.
    anchor_ids[p] = (counter0, counter1) seeds the anchor draw of pair p (default (2p, 2p+1)).
    query_anchors: the query-side draws (draw_anchors(n0[p], n_anchor, anchor_ids[p][0]) for every p)
    when the caller has already made them -- e.g. while the embedding kernels were still running; the
    ~1 ms of host work would otherwise sit between the 5-NN and the part-cut launches.

    icp_max_iter > 0: T_best of every pair is refined by point-to-point ICP (cs_icp_batch: source = the query's voxels,
    target = the CAD's voxels, the direction of stage 5; correspondence distance icp_max_dist, required then) and the
    result's T_icp / cd_icp / icp_* fields are filled; with the default 0 nothing is launched.
    icp_estimation = "plane": the refinement is point-to-plane (cs_icp_plane_batch) on the normals of the CAD voxels,
    normals1 f32 [N1,3] when the caller has them (a catalog's are computed once), else cs_estimate_normals over
    icp_normal_k neighbours here; the same result fields are filled.  icp_normal_radius (None = k-NN): those normals
    come from the at most icp_normal_k nearest rows strictly inside that radius instead (cs_estimate_normals_hybrid).
    icp_kernel = "huber" / "cauchy" / "tukey" with icp_kernel_scale > 0 (plane estimation only): the residuals are weighted
    by that robust kernel (cs_icp_plane_robust_batch) and icp_wfitness is filled too.
    icp_with_scaling: either estimation also fits an isotropic scale of the query (cs_icp_scale_batch); T_icp is then a
    similarity, icp_scale the factor, and cd_icp is cs_chamfer_1dir under that similarity (its pose chain is affine).
    icp_scale_bounds = (min, max), None = backend.icp_batch's untuned default (0.5, 2.0).  Robust kernels with a scale are
    out of scope and refused.  These two parameters stand BEFORE icp_kernel / icp_kernel_scale, which stay the last two: a
    caller that passed icp_kernel by position must pass it by keyword now (such a call fails on the scale bounds, it does
    not run with other settings).
    icp_estimation = "gicp": the refinement is plane-to-plane Generalized ICP (cs_icp_gicp_batch), which models a local
    plane on BOTH clouds: the CAD side works as for "plane" (normals1, else estimated here), the query side takes normals0
    f32 [N0,3] in the query's own frame, else cs_estimate_normals over the query voxels with the same icp_normal_k /
    icp_normal_radius.  gicp_epsilon in [2^-10, 1] is the covariance floor along the normal (Open3D's default; untuned here,
    as is icp_normal_k for this estimation).  normals0 (default None) and gicp_epsilon (default 1e-3) are accepted by keyword
    only, like the fgr_* options, and are taken out of **kwargs here.  icp_mrmse is filled too.  A robust icp_kernel or
    icp_with_scaling with "gicp" is out of scope and refused.
    Descriptors of another width (fpfh_features: 33 columns) register with use_symmetry=False; with use_symmetry the part
    cut takes 16 or 32 columns and anything else is refused with ValueError before any launch.

    registration = "fgr" (keyword-only, like the fgr_* arguments): stage 4 sends the vanilla and every part-configuration
    list through ONE cs_fgr_batch call (Fast Global Registration: tuple test + graduated non-convexity, backend.fgr_batch)
    in place of both RANSAC calls and the helper-thread split; T_all, inliers and iters (= updates applied) are filled from
    it and stages 5 - 7 are what they are for the RANSAC.  fgr_mu_floor (untuned), fgr_iterations and fgr_tuple_test are
    fgr_batch's mu_floor, iteration_number and tuple_test; max_iter and confidence are the RANSAC's and unused then.  With
    the default "ransac" nothing of it is launched.  These four are accepted by keyword ONLY, behind every parameter
    above; `inspect.signature` keeps reporting the parameters above (`__signature__` below), whose order and end existing
    callers and tests rely on.

    registration = "ransac_fm": Open3D's registration_ransac_based_on_feature_matching recipe, for hand-crafted
    descriptors.  Stage 1 runs cs_knn_feat at k = 1 in BOTH directions (k_nn is not used) and cs_corr_mutual keeps the mutual
    matches (a pair with fewer than 3 fm_ransac_n of them keeps all of its 1-NN matches); stage 4 is ONE cs_ransac_fm_batch
    call -- fm_iterations hypotheses of fm_ransac_n (3 or 4) pairs, the edge-length checker at fm_edge_similarity before the
    fit and the distance checker at max_corr after it; T_all, inliers and iters (= the hypotheses that passed the checkers)
    are filled from it and stages 5 - 7 are what they are for the RANSAC.  fm_ransac_n = 3, fm_edge_similarity = 0.9,
    fm_mutual = True, fm_iterations = 100000 are Open3D's defaults, untuned, no real scan measured; like normals0 they are
    accepted by keyword only and taken out of **kwargs here.  It needs use_symmetry=False (ValueError otherwise); max_iter
    and confidence are unused.  With "ransac" and "fgr" nothing of it is launched.

    registration = "sc2": the compatibility-graph estimator, for lists with an inlier share of a few per cent.
    Stage 1 is unchanged (the k_nn lists); stage 4 sends the SAME lists "fgr" gets -- the vanilla list and every part
    configuration, so use_symmetry=True works -- through ONE cs_sc2_batch call (sc2.sc2_batch): sc2_seeds rows of the largest
    degree in the graph of correspondences whose lengths agree within sc2_compat_dist, each fitted over its sc2_k best
    neighbours, the pose with the most inliers at max_corr.  T_all, inliers and iters (= the valid seeds) are filled from it
    and stages 5 - 7 are what they are for the RANSAC.  sc2_compat_dist = None (half of max_corr), sc2_seeds = 1024 and
    sc2_k = 20 are UNTUNED, no real scan measured; keyword-only, taken out of **kwargs here.  A list of more than 32 768
    correspondences is refused by the library (a smaller k_nn).  max_iter, confidence and seed are unused.  With "ransac",
    "fgr" and "ransac_fm" nothing of it is launched.

    registration = "ppf": point-pair-feature voting, which reads NO descriptors: baseF and posF may be None,
    stages 1 - 3 are skipped and use_symmetry=True is refused.  Stage 4 is ONE cs_ppf_batch call (ppf.ppf_batch) on the
    voxels and their ORIENTED normals: the scene is side ppf_scene_side (0 = the query, 1 = the CAD side) and the model the
    other one; normals0 / normals1 are used as they are when given (normals0 is accepted for this estimator with any
    icp_estimation), else they come from estimate_normals (icp_normal_k, icp_normal_radius) and orient_normals -- the scene
    towards ppf_view_points f64 [P,3] (the camera of a depth view) when given, else away from its centroid; the model away
    from its centroid.  ppf_dist_step = None: 0.05 of every model's bounding-box diagonal (one small download), else one
    positive number for all pairs or a list of one per pair; every ppf_ref_step-th scene row is a reference, the ppf_n_cand
    references with the most votes are verified within max_corr.
    T_ransac is the pose in this function's direction, xyz0 -> xyz1: the scene -> model pose when the scene is side 0, the
    inverse the library forms when it is side 1; inliers = the verification count, iters = the votes of the winner's peak.
    Stages 5 - 7 are what they are for the RANSAC.  ppf_scene_side = 0, ppf_dist_step = None, ppf_ref_step = 5, ppf_n_cand =
    16 are UNTUNED, no real scan measured; keyword-only, taken out of **kwargs here.  A model above 4 096 rows or a scene above
    16 384 is refused by the library (a coarser voxel).  k_nn, max_iter, confidence and seed are unused.  With the four other
    estimators nothing of it is launched."""
    entry = E.lookup(registration, "sym_pose_batch: registration")
    options = dict(fgr_mu_floor=fgr_mu_floor, fgr_iterations=fgr_iterations, fgr_tuple_test=fgr_tuple_test)
    for e in E.TABLE:
        options.update((key, kwargs.pop(key, default)) for key, default in e.options.items() if key not in options)
    return _sym_pose_batch(_KeywordOnly(entry, options, kwargs.pop("normals0", None), kwargs.pop("gicp_epsilon", 1e-3)),
                           *args, **kwargs)


# the positional interface (everything but the keyword-only estimator options), as introspection has always shown it
sym_pose_batch.__signature__ = inspect.Signature(list(inspect.signature(_sym_pose_batch).parameters.values())[1:])


def fpfh_features(xyz, offsets, radius, max_nn=100, normal_radius=None, normal_k=16):
    """Fast Point Feature Histograms of packed clouds, the descriptor that needs no weights: normals
    (backend.estimate_normals over normal_k neighbours, inside normal_radius when one is given), oriented away from each
    cloud's centroid (backend.orient_normals: cs_estimate_normals' sign rule depends on the pose and FPFH is not invariant to a
    flipped normal), then backend.fpfh at `radius` / `max_nn`.  xyz f32 [n,3] device, offsets a host list.  Returns
    (features f32 [n,33], normals f32 [n,3]); the features go to sym_pose_batch with use_symmetry=False.  No host wait."""
    normals = B.estimate_normals(xyz, offsets, normal_k, normal_radius)
    B.orient_normals(xyz, offsets, normals, None, True)
    return B.fpfh(xyz, offsets, normals, radius, max_nn), normals
