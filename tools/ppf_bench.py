"""Point-pair-feature voting at the chair registration shape: `python tools/ppf_bench.py [--json PATH]`.

The 32 (query, CAD) pairs of tools/featmatch_bench.py (10 000-point synthetic clouds voxelised at 0.03).  cs_ppf_batch takes the
voxels and their oriented normals (16 neighbours, away from the centroid), the scene = the query, the model = the CAD cloud,
dist_step 0.05 of the model's diagonal, ref_step 5, 16 candidates, max_dist 2 voxels.  When a CAD cloud exceeds the 4 096 rows
a model may have, the library refuses the call; the refusal is recorded and cs_ppf_batch alone runs on the same clouds
voxelised once more at the first of 0.045, 0.06, 0.08 at which every model fits ("ppf_voxel").  The yardsticks run in the same process on the FPFH lists of those pairs, each at
the k its lists allow: cs_sc2_batch (256 seeds), cs_fgr_batch and cs_ransac_fm_batch (4 096 hypotheses).  One process, the calls
taking turns, medians (and the range) of --reps device-event timings after --warmup rounds.  The normals of ppf and the
descriptors and lists of the yardsticks are made once, outside the timings.  Also recorded: the share of the family "ppf" in
the call's time as the profile scope sees it (the unit brackets its kernels with ONE scope, so there is no split per kernel),
and the pose errors (RRE, RTE against the known pose) of every call.  No ratio was fixed in advance.  Writes
profiles/ppf_bench.json and prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, featmatch as FM, ppf as PPF, registration as R, sc2 as S2  # noqa: E402
import icp_bench  # noqa: E402
from featmatch_bench import MAX_CORR, MAX_NN, NORMAL_K, RADIUS_VOXELS, alternating, errors  # noqa: E402

REF_STEP, N_CAND = 5, 16
COARSE_VOXELS = (0.045, 0.06, 0.08)      # the first at which every model fits


def oriented(x, off):
    return B.orient_normals(x, off, B.estimate_normals(x, off, NORMAL_K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--note", default="", help="free text kept in the result (date)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "ppf_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    x0, off0, x1, off1, _, truth, _, _ = icp_bench.problems(dev, 0.0, 0.0)
    truth = np.asarray(truth.cpu() if isinstance(truth, torch.Tensor) else truth, np.float64)
    P = len(off0) - 1
    n0, n1 = np.diff(off0), np.diff(off1)
    res = {"tool": "tools/ppf_bench.py", "note": a.note, "device": torch.cuda.get_device_name(0), "pairs_of_clouds": P,
           "scene_rows": [int(n0.min()), int(np.median(n0)), int(n0.max())], "model_rows": [int(n1.min()), int(np.median(n1)), int(n1.max())],
           "reps": a.reps, "warmup": a.warmup, "max_dist": 2 * icp_bench.VOXEL, "ref_step": REF_STEP, "n_cand": N_CAND,
           "ppf_voxel": icp_bench.VOXEL}
    s, so, m, mo = x0, off0, x1, off1
    if n1.max() > PPF.MAX_MODEL_ROWS or n0.max() > PPF.MAX_SCENE_ROWS:
        try:
            PPF.ppf_batch(s, oriented(s, so), so, m, oriented(m, mo), mo, list(range(P)), list(range(P)), 0.1, 2 * icp_bench.VOXEL)
        except _lib.CorsairHipError as e:
            res["refused_at_voxel_%g" % icp_bench.VOXEL] = str(e)
        for coarse in COARSE_VOXELS:
            ks, _, so = B.voxelize(x0, off0, coarse)
            km, _, mo = B.voxelize(x1, off1, coarse)
            if max(np.diff(mo)) <= PPF.MAX_MODEL_ROWS and max(np.diff(so)) <= PPF.MAX_SCENE_ROWS:
                break
        s, m, so, mo = x0[ks].contiguous(), x1[km].contiguous(), [int(v) for v in so], [int(v) for v in mo]
        res["ppf_voxel"] = coarse
        res["scene_rows_ppf"], res["model_rows_ppf"] = [int(v) for v in np.diff(so)[[0, -1]]], [int(np.diff(mo).min()), int(np.diff(mo).max())]
    sn, mn = oriented(s, so), oriented(m, mo)
    steps = PPF.default_dist_step(m, mo)
    pairs = list(range(P))
    ppf_call = lambda: PPF.ppf_batch(s, sn, so, m, mn, mo, pairs, pairs, steps, 2 * icp_bench.VOXEL, REF_STEP, N_CAND)
    # the yardsticks on the FPFH lists of the same pairs
    radius = RADIUS_VOXELS * icp_bench.VOXEL
    Fq, _ = R.fpfh_features(x0, off0, radius, MAX_NN, None, NORMAL_K)
    Fc, _ = R.fpfh_features(x1, off1, radius, MAX_NN, None, NORMAL_K)
    k_nn = max(k for k in (5, 3, 2, 1) if k * int(n0.max()) <= S2.MAX_SLOTS)
    nn = B.knn_feat(Fq, off0, Fc, off1, k_nn)
    desc = np.asarray([[off0[p], off0[p], off1[p], n0[p], off0[p]] for p in range(P)], dtype=np.int64).reshape(P, 5)
    ls, lt = B.corr_assemble(x0, x1, None, nn, desc, off0[-1], int(n0.max()))
    loff = [k_nn * v for v in off0]
    res["k_nn"] = k_nn
    fns = {"ppf": ppf_call,
           "sc2_256": lambda: S2.sc2_batch(ls, lt, loff, MAX_CORR, 1.0 * icp_bench.VOXEL, n_seeds=256, k_consensus=20),
           "fgr_batch": lambda: B.fgr_batch(ls, lt, loff, MAX_CORR),
           "ransac_fm_4096": lambda: FM.ransac_fm_batch(ls, lt, loff, MAX_CORR, iterations=4096)}
    for k, (med, lo, hi) in alternating(fns, a.reps, a.warmup).items():
        res[k + "_ms"], res[k + "_ms_range"] = med, [lo, hi]
    for yard in ("sc2_256", "fgr_batch", "ransac_fm_4096"):
        res["ppf_over_" + yard] = round(res["ppf_ms"] / res[yard + "_ms"], 3)
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        r = ppf_call()
        torch.cuda.synchronize()
        ms, launches, units = _lib.prof_get("ppf")
    finally:
        _lib.prof_enable(False)
    res["ppf_family_ms"], res["ppf_family_scopes"], res["ppf_family_share_of_call"] = round(ms, 4), int(launches), round(ms / res["ppf_ms"], 3)
    res["pose_ppf"] = dict(errors(r.T, truth), found=int(r.found.sum()), votes_median=int(np.median(r.votes.cpu().numpy())),
                           count_median=int(np.median(r.count.cpu().numpy())), winner_rank_max=int(r.rank.max()))
    res["pose_sc2_256"] = errors(fns["sc2_256"]().T, truth)
    res["pose_fgr_batch"] = errors(fns["fgr_batch"]().T64, truth)
    res["pose_ransac_fm_4096"] = errors(fns["ransac_fm_4096"]().T, truth)
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
