"""FPFH descriptors at the chair registration shape: `python tools/fpfh_bench.py [--json PATH]`.

The 32 (query, CAD) pairs of tools/icp_bench.py (10 000-point synthetic clouds voxelised at 0.03); descriptors of the 32
CAD targets at radius 5 voxels, max_nn 100.  Medians of --reps repetitions after warm-up, device events (wall time next
to them), every figure from this one process:
  normals      backend.estimate_normals over 16 neighbours (the call registration.fpfh_features makes)
  orient       backend.orient_normals, centroid, away
  fpfh         backend.fpfh: both passes;  fpfh_pass1: CS_FPFH_PASS=1, the SPFH pass alone (neighbour lists, pair
               features, counts);  fpfh_pass2 = the difference (the weighted sums)
  exhaustive   backend.fpfh under CS_FPFH_GRID=0 (the definition's scan)
  knn33        backend.knn_feat, 5-NN of the 32 queries' descriptors among their CADs' (k_knn_feat<33>)
and, from a CS_FPFH_STATS=1 call of its own, the neighbours found (pairs), the mean per row and the rows whose on-chip
list was ranked in parts.  pairs_per_s = pairs / time.  For information: the median RRE / RTE of sym_pose_batch
(use_symmetry=False, default RANSAC) on the 32 pairs with these descriptors.  There is no earlier version to compare with.
Writes profiles/fpfh_bench.json and prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, registration as R  # noqa: E402
import icp_bench  # noqa: E402

RADIUS_VOXELS, MAX_NN, NORMAL_K = 5.0, 100, 16


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "fpfh_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    x0, off0, x1, off1, _, truth, _, _ = icp_bench.problems(dev, 0.0, 0.0)
    radius = RADIUS_VOXELS * icp_bench.VOXEL
    rows = off1[-1]
    nrm = B.estimate_normals(x1, off1, NORMAL_K)
    B.orient_normals(x1, off1, nrm)
    res = {"pairs_of_clouds": len(off1) - 1, "rows": rows, "radius": radius, "max_nn": MAX_NN, "reps": a.reps}
    t = {}
    t["normals"] = icp_bench.timed(lambda: B.estimate_normals(x1, off1, NORMAL_K), a.reps)
    t["orient"] = icp_bench.timed(lambda: B.orient_normals(x1, off1, nrm), a.reps)
    # the two fpfh settings alternate in one window each; the grid path first and last to show the drift
    t["fpfh"] = icp_bench.timed(lambda: B.fpfh(x1, off1, nrm, radius, MAX_NN), a.reps)
    with env(CS_FPFH_PASS="1"):
        t["fpfh_pass1"] = icp_bench.timed(lambda: B.fpfh(x1, off1, nrm, radius, MAX_NN), a.reps)
    t["fpfh_again"] = icp_bench.timed(lambda: B.fpfh(x1, off1, nrm, radius, MAX_NN), a.reps)
    with env(CS_FPFH_GRID="0"):
        t["exhaustive"] = icp_bench.timed(lambda: B.fpfh(x1, off1, nrm, radius, MAX_NN), max(3, a.reps // 5), warmup=1)
    with env(CS_FPFH_STATS="1"):
        B.fpfh_stats(reset=True)
        Fc = B.fpfh(x1, off1, nrm, radius, MAX_NN)
        pairs, parted = B.fpfh_stats(reset=True)
    Fq, _ = R.fpfh_features(x0, off0, radius, MAX_NN, None, NORMAL_K)
    t["knn33"] = icp_bench.timed(lambda: B.knn_feat(Fq, off0, Fc, off1, 5), a.reps)
    for k, (d, w) in t.items():
        res[k + "_ms"], res[k + "_wall_ms"] = d, w
    res["fpfh_pass2_ms"] = round(res["fpfh_ms"] - res["fpfh_pass1_ms"], 4)
    res["pairs"], res["mean_neighbours"], res["rows_ranked_in_parts"] = pairs, round(pairs / rows, 2), parted
    res["pairs_per_s_call"] = round(pairs / (res["fpfh_ms"] * 1e-3))
    res["pairs_per_s_pass1"] = round(pairs / (res["fpfh_pass1_ms"] * 1e-3))
    res["pairs_per_s_pass2"] = round(pairs / max(res["fpfh_pass2_ms"], 1e-6) / 1e-3)
    # pass 2 per pair: 33 f64 divisions (one per lane that owns a bin), 33 B of counts + 4 B of the neighbour's m gathered
    # from L2, 12 B of the row's list streamed
    res["pass2_div_per_s"] = round(33 * res["pairs_per_s_pass2"])
    res["pass2_gather_bytes_per_s"] = round(37 * res["pairs_per_s_pass2"])
    # information: registration of the 32 pairs on these descriptors
    out = R.sym_pose_batch(Fq, x0, off0, Fc, x1, off1, [1] * (len(off0) - 1), 5, 0.2, 0, None, 100, 100000, 0.999, False)
    T = out.T_best.cpu().numpy()
    rre = [np.degrees(np.arccos(np.clip((np.trace(T[p, :3, :3] @ truth[p, :3, :3].T) - 1) / 2, -1, 1))) for p in range(len(T))]
    rte = [np.linalg.norm(T[p, :3, 3] - truth[p, :3, 3]) for p in range(len(T))]
    res["info_rre_deg_median"] = round(float(np.median(rre)), 3)
    res["info_rte_median"] = round(float(np.median(rte)), 4)
    res["info_rre_le_15deg"] = round(float(np.mean(np.asarray(rre) <= 15)), 3)
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
