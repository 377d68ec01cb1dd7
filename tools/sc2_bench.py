"""The compatibility-graph estimator at the chair registration shape: `python tools/sc2_bench.py [--json PATH]`.

The lists of tools/featmatch_bench.py: the 32 (query, CAD) pairs of tools/icp_bench.py (10 000-point synthetic clouds
voxelised at 0.03) with cs_fpfh descriptors at radius 5 voxels, max_nn 100, and their k-NN correspondence lists at the largest
k of 5, 3, 2, 1 whose longest list fits cs_sc2_batch's limit of 32 768 pairs (recorded as "k_nn").  One process, the calls
taking turns, medians (and the range) of --reps device-event timings after --warmup rounds, every call on the SAME lists:
  sc2_256, sc2_1024, sc2_all   cs_sc2_batch at n_seeds 256, 1 024 and 0 (every row), K = 20, compat_dist = 1 voxel
  ransac_fm_4096               cs_ransac_fm_batch, 4 096 hypotheses of 3 pairs, edge similarity 0.9, distance checker: a yardstick
  fgr_batch                    cs_fgr_batch, defaults: the second yardstick
Also recorded: the list lengths, the degrees of the winning seeds, the valid seeds, and the pose errors (RRE, RTE against the
known pose) of every call on the 32 pairs.  No ratio was fixed in advance and nothing is compared with an earlier version:
there is none.  Writes profiles/sc2_bench.json and prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, featmatch as FM, registration as R, sc2 as S2  # noqa: E402
import icp_bench  # noqa: E402
from featmatch_bench import MAX_CORR, MAX_NN, NORMAL_K, RADIUS_VOXELS, alternating, errors  # noqa: E402

SEEDS = (("sc2_256", 256), ("sc2_1024", 1024), ("sc2_all", 0))
K = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--note", default="", help="free text kept in the result (date)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sc2_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    x0, off0, x1, off1, _, truth, _, _ = icp_bench.problems(dev, 0.0, 0.0)
    truth = np.asarray(truth.cpu() if isinstance(truth, torch.Tensor) else truth, np.float64)
    radius = RADIUS_VOXELS * icp_bench.VOXEL
    tau = 1.0 * icp_bench.VOXEL
    P = len(off0) - 1
    Fq, _ = R.fpfh_features(x0, off0, radius, MAX_NN, None, NORMAL_K)
    Fc, _ = R.fpfh_features(x1, off1, radius, MAX_NN, None, NORMAL_K)
    n0 = [off0[p + 1] - off0[p] for p in range(P)]
    k_nn = max(k for k in (5, 3, 2, 1) if k * max(n0) <= S2.MAX_SLOTS)
    nn5 = B.knn_feat(Fq, off0, Fc, off1, k_nn)
    desc = np.asarray([[off0[p], off0[p], off1[p], n0[p], off0[p]] for p in range(P)], dtype=np.int64).reshape(P, 5)
    s5, t5 = B.corr_assemble(x0, x1, None, nn5, desc, off0[-1], max(n0))
    off5 = [k_nn * v for v in off0]
    fns = {name: (lambda n=n: S2.sc2_batch(s5, t5, off5, MAX_CORR, tau, n_seeds=n, k_consensus=K)) for name, n in SEEDS}
    fns["ransac_fm_4096"] = lambda: FM.ransac_fm_batch(s5, t5, off5, MAX_CORR, iterations=4096)
    fns["fgr_batch"] = lambda: B.fgr_batch(s5, t5, off5, MAX_CORR)
    lens = np.diff(off5)
    res = {"tool": "tools/sc2_bench.py", "note": a.note, "device": torch.cuda.get_device_name(0), "pairs_of_clouds": P, "k_nn": k_nn,
           "list_rows": int(off5[-1]), "list_rows_per_pair": [int(lens.min()), int(np.median(lens)), int(lens.max())],
           "pair_tests": int((lens.astype(np.int64) ** 2).sum()), "reps": a.reps, "warmup": a.warmup, "max_corr": MAX_CORR,
           "compat_dist": tau, "k_consensus": K}
    for k, (med, lo, hi) in alternating(fns, a.reps, a.warmup).items():
        res[k + "_ms"], res[k + "_ms_range"] = med, [lo, hi]
    for name, _ in SEEDS:
        for yard in ("ransac_fm_4096", "fgr_batch"):
            res["%s_over_%s" % (name, yard)] = round(res[name + "_ms"] / res[yard + "_ms"], 3)
    for name, n in SEEDS:
        r = S2.sc2_batch(s5, t5, off5, MAX_CORR, tau, n_seeds=n, k_consensus=K)
        deg, nv, rank = (t.cpu().numpy() for t in (r.seed_degree, r.n_valid, r.seed_rank))
        res["pose_" + name] = dict(errors(r.T, truth), found=int(r.found.sum()), winner_degree_median=int(np.median(deg)),
                                   winner_rank_max=int(rank.max()), valid_seeds_median=int(np.median(nv)),
                                   inliers_median=int(np.median(r.inliers.cpu().numpy())))
    fm = FM.ransac_fm_batch(s5, t5, off5, MAX_CORR, iterations=4096)
    res["pose_ransac_fm_4096"] = dict(errors(fm.T, truth), found=int(fm.found.sum()),
                                      inliers_median=int(np.median(fm.inliers.cpu().numpy())))
    res["pose_fgr_batch"] = errors(B.fgr_batch(s5, t5, off5, MAX_CORR).T64, truth)
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
