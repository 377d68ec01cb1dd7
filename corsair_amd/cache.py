"""Result-cache format of the reference (evaluation.py:390-441): nine .npy files per
(category, top1|gt) in the cache directory.  Files written here load in the reference's `_load_data`
and vice versa (the shipped data/cache_* directories load with `load_results`)."""
import os

import numpy as np

NAMES = ("Ts_est_ransac", "Ts_est_best", "t_losses_ransac", "t_losses_sym", "r_losses_ransac",
         "r_losses_sym", "sym_ransac_success", "chamfer_dist_ransac", "chamfer_dist_sym")
# element types of the nine arrays as the registration loop produces them (eval_pose's t_loss is the norm of an f32
# vector, hence f32; its r_loss goes through np.float64): what an EMPTY result set carries, and what the sharded
# evaluation puts on the wire -- fixed by NAME so that ranks with and without queries agree on every collective
DTYPES = {"Ts_est_ransac": np.float32, "Ts_est_best": np.float32, "t_losses_ransac": np.float32,
          "t_losses_sym": np.float32, "r_losses_ransac": np.float64, "r_losses_sym": np.float64,
          "sym_ransac_success": np.bool_, "chamfer_dist_ransac": np.float64, "chamfer_dist_sym": np.float64}
# the extra arrays of a run with ICP refinement (Config.icp_max_iter > 0): written beside the nine, which keep their format
ICP_NAMES = ("Ts_est_icp", "t_losses_icp", "r_losses_icp", "chamfer_dist_icp", "icp_iters")
ICP_DTYPES = {"Ts_est_icp": np.float32, "t_losses_icp": np.float32, "r_losses_icp": np.float64,
              "chamfer_dist_icp": np.float64, "icp_iters": np.int32}
# one more array of a run whose ICP also fitted an isotropic scale (Config.icp_with_scaling): written, read and returned only
# then, so ICP_NAMES and the key set of every other run stay what they were
ICP_SCALE_NAMES = ("icp_scale",)
ICP_SCALE_DTYPES = {"icp_scale": np.float64}
# the arrays of a run with candidate verification (Config.verify_top_k = K > 1): written, read and returned only then; the
# arrays above then describe the WINNING candidate of every query, and all of them live in a file set of their own
# (_suffix).  verify_cand [Q,K] the CAD ids in retrieval order,
# verify_score [Q,K] their scores in that order, verify_order [Q,K] the columns by rank (position 0 = the winner's column),
# verify_T [Q,K,4,4] the scored poses
VERIFY_NAMES = ("verify_cand", "verify_score", "verify_order", "verify_T")
VERIFY_DTYPES = {"verify_cand": np.int64, "verify_score": np.float64, "verify_order": np.int32, "verify_T": np.float32}


def _suffix(register_top1, verify=False):
    """File-name tail of a result set.  A run with candidate verification has a file set of its OWN (`_top1_verify.npy`):
    its nine arrays (and its ICP arrays) are those of the winning candidates, so they must never be read as, nor overwrite,
    the descriptor top-1's arrays of a plain run -- whose files keep the reference's names."""
    if verify:
        return "_top1_verify.npy"
    return "_top1.npy" if register_top1 else "_gt.npy"


def save_results(cache_dir, category, register_top1, results):
    """results: dict with the NAMES keys (and the ICP_NAMES keys of a run with ICP refinement, the ICP_SCALE_NAMES keys of one
    with a scale); transforms as [Q,4,4] (stored flattened [Q,16] f32).  A dict with the VERIFY_NAMES keys is the result of
    a run with candidate verification: every array of it goes to the verification file set (_suffix), the VERIFY_NAMES arrays
    in their own shapes, and the optional files of that set which this run does not write are removed, so that the set on
    disk is always ONE run's."""
    os.makedirs(cache_dir, exist_ok=True)
    verify = all(n in results for n in VERIFY_NAMES)
    suf = _suffix(register_top1, verify)
    optional = ICP_NAMES + ICP_SCALE_NAMES
    for name in NAMES + tuple(n for n in optional if n in results) + (VERIFY_NAMES if verify else ()):
        data = np.asarray(results[name])
        if name.startswith("Ts_est"):
            data = data.reshape(len(data), 16).astype(np.float32)
        np.save(os.path.join(cache_dir, f"{name}_{category}{suf}"), data)
    if verify:
        for name in optional:
            path = os.path.join(cache_dir, f"{name}_{category}{suf}")
            if name not in results and os.path.exists(path):
                os.remove(path)


def load_results(cache_dir, category, register_top1, icp=False, icp_scale=False, verify=0):
    """Returns the dict, or None when any of the nine files is missing (the reference then
    recomputes, evaluation.py:287).  icp: the ICP_NAMES files are wanted too; a cache without them is a miss.  icp_scale
    (with icp): the ICP_SCALE_NAMES files likewise -- wanted, read and returned only then.  verify = K > 1: the verification
    file set of a run with Config.verify_top_k = K is read instead (the plain files are not looked at, and a plain run never
    looks at that set): a set that lacks a file, was written with another K, or whose winners' poses are not the scored poses
    of its first-ranked candidates (Ts_est_icp with icp, else Ts_est_best, against verify_T[q, verify_order[q, 0]] -- a set
    written with and read without the refinement, or put together from two runs) is a miss."""
    verify = int(verify) if int(verify) > 1 else 0
    if verify and not register_top1:
        return None             # (the verification re-ranks retrieved candidates: there is no such set for the annotated CAD)
    suf = _suffix(register_top1, bool(verify))
    out = {}
    for name in NAMES + (ICP_NAMES if icp else ()) + (ICP_SCALE_NAMES if icp and icp_scale else ()) + \
            (VERIFY_NAMES if verify else ()):
        path = os.path.join(cache_dir, f"{name}_{category}{suf}")
        if not os.path.exists(path):
            return None
        data = np.load(path)
        if name.startswith("Ts_est"):
            data = data.reshape(-1, 4, 4)
        if name in VERIFY_NAMES and (data.ndim < 2 or data.shape[1] != verify):
            return None
        out[name] = data
    if verify:
        won = out["Ts_est_icp" if icp else "Ts_est_best"]
        order, vT = out["verify_order"], out["verify_T"]
        if not (len(won) == len(order) == len(vT) and vT.shape[1:] == (verify, 4, 4) and order.min(initial=0) >= 0
                and order.max(initial=0) < verify):
            return None
        scored = vT[np.arange(len(order)), order[:, 0].astype(np.int64)]
        if np.asarray(won, np.float32).tobytes() != np.ascontiguousarray(scored, np.float32).tobytes():
            return None
    return out
