"""Feature-matching RANSAC at the chair registration shape: `python tools/featmatch_bench.py [--json PATH]`.

The input of tools/fpfh_bench.py: the 32 (query, CAD) pairs of tools/icp_bench.py (10 000-point synthetic clouds voxelised
at 0.03) with cs_fpfh descriptors at radius 5 voxels, max_nn 100.  One process, the calls taking turns (a, b, c, a, b, c,
...), medians (and the range) of --reps device-event timings after --warmup rounds:
  corr_mutual     cs_corr_mutual over the two 1-NN lists (mutual filter on)
  ransac_fm_1e4   cs_ransac_fm_batch, 10^4 hypotheses of 3 pairs, edge similarity 0.9, distance checker, on its output
  ransac_fm_1e5   the same at 10^5 hypotheses (Open3D's default)
  ransac_batch    cs_ransac_batch on the 5-NN lists (ransac_n 10, 100 000 iterations at most, confidence 0.999): the yardstick
  fgr_batch       cs_fgr_batch on the same 5-NN lists, defaults: the second yardstick
  knn_k1_fwd, knn_k1_bwd, knn_k5   cs_knn_feat at k = 1 in both directions against the one call at k = 5
Also recorded: the mutual matches per pair, the share of hypotheses that pass the checkers and the fit (n_valid /
iterations), and the pose errors (RRE, RTE against the known pose) of the three estimators on the 32 pairs.  Nothing is
compared with an earlier version: there is none.  Writes profiles/featmatch_bench.json and prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, featmatch as FM, registration as R  # noqa: E402
import icp_bench  # noqa: E402

RADIUS_VOXELS, MAX_NN, NORMAL_K, MAX_CORR = 5.0, 100, 16, 0.2


def alternating(fns, reps, warmup):
    """{name: (median, min, max) device ms}, the calls interleaved in this process."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)) for k, v in ms.items()}


def errors(T, truth):
    T = T.detach().double().cpu().numpy()
    rre = [np.degrees(np.arccos(np.clip((np.trace(T[p, :3, :3] @ truth[p, :3, :3].T) - 1) / 2, -1, 1))) for p in range(len(T))]
    rte = [np.linalg.norm(T[p, :3, 3] - truth[p, :3, 3]) for p in range(len(T))]
    return {"rre_deg_median": round(float(np.median(rre)), 3), "rre_deg_max": round(float(np.max(rre)), 3),
            "rte_median": round(float(np.median(rte)), 4), "rre_le_15deg": round(float(np.mean(np.asarray(rre) <= 15)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--note", default="", help="free text kept in the result (date)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "featmatch_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    x0, off0, x1, off1, _, truth, _, _ = icp_bench.problems(dev, 0.0, 0.0)
    truth = np.asarray(truth.cpu() if isinstance(truth, torch.Tensor) else truth, np.float64)
    radius = RADIUS_VOXELS * icp_bench.VOXEL
    P = len(off0) - 1
    Fq, _ = R.fpfh_features(x0, off0, radius, MAX_NN, None, NORMAL_K)
    Fc, _ = R.fpfh_features(x1, off1, radius, MAX_NN, None, NORMAL_K)
    fwd, bwd = B.knn_feat(Fq, off0, Fc, off1, 1), B.knn_feat(Fc, off1, Fq, off0, 1)
    nn5 = B.knn_feat(Fq, off0, Fc, off1, 5)
    n0 = [off0[p + 1] - off0[p] for p in range(P)]
    desc = np.asarray([[off0[p], off0[p], off1[p], n0[p], off0[p]] for p in range(P)], dtype=np.int64).reshape(P, 5)
    s5, t5 = B.corr_assemble(x0, x1, None, nn5, desc, off0[-1], max(n0))
    off5 = [5 * v for v in off0]
    mu = FM.mutual_correspondences(fwd, bwd, x0, off0, x1, off1, 3, True)
    fns = {
        "corr_mutual": lambda: FM.mutual_correspondences(fwd, bwd, x0, off0, x1, off1, 3, True),
        "ransac_fm_1e4": lambda: FM.ransac_fm_batch(mu.src, mu.tgt, off0, MAX_CORR, m=mu.m, iterations=10000),
        "ransac_fm_1e5": lambda: FM.ransac_fm_batch(mu.src, mu.tgt, off0, MAX_CORR, m=mu.m, iterations=100000),
        "ransac_batch": lambda: B.ransac_batch(s5, t5, off5, MAX_CORR, 10, 100000, 0.999, 0),
        "fgr_batch": lambda: B.fgr_batch(s5, t5, off5, MAX_CORR),
        "knn_k1_fwd": lambda: B.knn_feat(Fq, off0, Fc, off1, 1),
        "knn_k1_bwd": lambda: B.knn_feat(Fc, off1, Fq, off0, 1),
        "knn_k5": lambda: B.knn_feat(Fq, off0, Fc, off1, 5),
    }
    res = {"note": a.note, "pairs_of_clouds": P, "query_rows": off0[-1], "cad_rows": off1[-1], "reps": a.reps,
           "warmup": a.warmup, "max_corr": MAX_CORR}
    for k, (med, lo, hi) in alternating(fns, a.reps, a.warmup).items():
        res[k + "_ms"], res[k + "_ms_range"] = med, [lo, hi]
    res["ransac_fm_1e5_over_ransac_batch"] = round(res["ransac_fm_1e5_ms"] / res["ransac_batch_ms"], 3)
    res["ransac_fm_1e4_over_ransac_batch"] = round(res["ransac_fm_1e4_ms"] / res["ransac_batch_ms"], 3)
    res["knn_k1_both_over_knn_k5"] = round((res["knn_k1_fwd_ms"] + res["knn_k1_bwd_ms"]) / res["knn_k5_ms"], 3)
    m = mu.m.cpu().numpy()
    st = mu.stat.cpu().numpy()
    res["mutual_matches_median"], res["mutual_matches_min"], res["mutual_matches_max"] = int(np.median(m)), int(m.min()), int(m.max())
    res["mutual_share_of_query_rows"] = round(float(st[:, 0].sum()) / off0[-1], 4)
    res["pairs_that_fell_back"] = int(st[:, 1].sum())
    for name, it in (("1e4", 10000), ("1e5", 100000)):
        r = FM.ransac_fm_batch(mu.src, mu.tgt, off0, MAX_CORR, m=mu.m, iterations=it)
        nv = r.n_valid.cpu().numpy().astype(np.float64)
        res["valid_share_" + name] = round(float(nv.mean()) / it, 5)
        res["valid_share_%s_range" % name] = [round(float(nv.min()) / it, 5), round(float(nv.max()) / it, 5)]
        res["found_" + name] = int(r.found.sum())
        res["pose_ransac_fm_" + name] = errors(r.T, truth)
    res["pose_ransac_batch"] = errors(B.ransac_batch(s5, t5, off5, MAX_CORR, 10, 100000, 0.999, 0)[0], truth)
    res["pose_fgr_batch"] = errors(B.fgr_batch(s5, t5, off5, MAX_CORR).T64, truth)
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
