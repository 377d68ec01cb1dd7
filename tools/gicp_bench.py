"""Generalized ICP at the chair registration shape: `python tools/gicp_bench.py [--json PATH]`.

The 32-pair problem of tools/icp_bench.py (10 000-point synthetic clouds voxelised at 0.03; source = the query's voxels,
target = the CAD's; T0 = the true pose perturbed by --deg degrees and --trans; at most 30 updates, max_dist = 2 voxels).
Measured in ONE process on the same clouds, the calls interleaved point, plane, gicp, ... and timed with device events
(median of --reps repetitions after warm-up, and the spread min .. max next to it):
 (point)   backend.icp_batch, cs_icp_batch;
 (plane)   the same with the target normals supplied, cs_icp_plane_batch -- the yardstick;
 (gicp)    the same with both normal arrays supplied, cs_icp_gicp_batch at --epsilon;
 (*_full)  each of the three with both convergence thresholds 0 and max_iter 10: exactly 11 full rounds, the clean figure
           for the time of a round;
 (normals_query / normals_cad) backend.estimate_normals over --normal-k neighbours of the 32 sources / targets: what a
           registration step pays for the query voxels' normals (the catalog's are computed once per evaluation).
Also per estimation: the updates applied, ms per round (ms / (most updates + 1), DESIGN 13's definition), the share of
workgroups the f16 association handed to the exhaustive kernel, mean RRE / RTE against the true poses, mean fitness; for
GICP the mean Mahalanobis rmse.  Without --json the result goes to profiles/gicp_bench.json.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import icp_bench as IB  # noqa: E402
from corsair_amd import backend as B  # noqa: E402


def timed_alternating(fns, reps, warmup=3):
    """{name: (median, min, max) device ms}, the calls interleaved a, b, c, a, b, c, ... in this process."""
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
    return {k: (round(float(np.median(v)), 4), round(float(min(v)), 4), round(float(max(v)), 4)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--deg", type=float, default=3.0)
    ap.add_argument("--trans", type=float, default=0.01)
    ap.add_argument("--normal-k", type=int, default=16)
    ap.add_argument("--epsilon", type=float, default=1e-3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gicp_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    max_dist = 2 * IB.VOXEL
    x0, off0, x1, off1, T0, truth, _, _ = IB.problems(dev, a.deg, a.trans)
    pairs = list(range(IB.N_PAIRS))
    n0, n1 = B.estimate_normals(x0, off0, a.normal_k), B.estimate_normals(x1, off1, a.normal_k)
    kw = {"point": {}, "plane": {"tgt_normals": n1},
          "gicp": {"tgt_normals": n1, "estimation": "gicp", "src_normals": n0, "gicp_epsilon": a.epsilon}}

    def call(k, max_iter=IB.MAX_ITER, **more):
        return B.icp_batch(x0, off0, x1, off1, pairs, pairs, T0, max_dist, max_iter, **kw[k], **more)

    full = dict(relative_fitness=0.0, relative_rmse=0.0)           # no problem converges: max_iter + 1 full rounds
    fns = {k: (lambda k=k: call(k)) for k in kw}
    fns.update({k + "_full": (lambda k=k: call(k, 10, **full)) for k in kw})
    fns["normals_query"] = lambda: B.estimate_normals(x0, off0, a.normal_k)
    fns["normals_cad"] = lambda: B.estimate_normals(x1, off1, a.normal_k)
    ms = timed_alternating(fns, a.reps)
    res = {"device": torch.cuda.get_device_name(dev), "hip": torch.version.hip, "pairs": IB.N_PAIRS, "voxel": IB.VOXEL,
           "source_rows": off0[-1], "target_rows": off1[-1], "max_dist": max_dist, "max_iter": IB.MAX_ITER,
           "perturbation": {"deg": a.deg, "trans": a.trans}, "normal_k": a.normal_k, "epsilon": a.epsilon, "reps": a.reps,
           "timing": "device events, median (min, max) over reps, calls interleaved in one process",
           "normals_query_ms": ms["normals_query"][0], "normals_query_ms_min_max": ms["normals_query"][1:],
           "normals_cad_ms": ms["normals_cad"][0], "normals_cad_ms_min_max": ms["normals_cad"][1:]}

    def errs(T):
        T = T.cpu().numpy().astype(np.float64)
        rre = [np.degrees(np.arccos(np.clip((np.trace(T[p, :3, :3] @ truth[p, :3, :3].T) - 1) / 2, -1, 1))) for p in pairs]
        rte = [np.linalg.norm(T[p, :3, 3] - truth[p, :3, 3]) for p in pairs]
        return round(float(np.mean(rre)), 4), round(float(np.mean(rte)), 5)

    res["rre_deg_rte_before"] = errs(T0)
    os.environ["CS_ICP_STATS"] = "1"
    for k in kw:
        B.icp_stats(reset=True)
        r = call(k)
        st = B.icp_stats(reset=True)
        it = r.iters.cpu().numpy()
        full_it = call(k, 10, **full).iters.cpu().numpy()
        res[k] = {"ms": ms[k][0], "ms_min_max": ms[k][1:],
                  "updates": {"mean": round(float(it.mean()), 2), "min": int(it.min()), "max": int(it.max())},
                  "ms_per_round": round(ms[k][0] / (float(it.max()) + 1), 4),
                  "full_rounds_ms": ms[k + "_full"][0], "full_rounds_ms_min_max": ms[k + "_full"][1:],
                  "full_rounds_updates_min": int(full_it.min()),
                  "full_rounds_ms_per_round": round(ms[k + "_full"][0] / 11.0, 4),
                  "fallback_share": round(st[1] / max(st[0], 1), 5), "rre_deg_rte_after": errs(r.T),
                  "fitness_mean": round(float(r.fitness.mean()), 4)}
        if r.mrmse is not None:
            res[k]["mrmse_mean"] = round(float(r.mrmse.mean()), 6)
    del os.environ["CS_ICP_STATS"]
    res["gicp_over_plane_total"] = round(res["gicp"]["ms"] / res["plane"]["ms"], 4)
    res["gicp_over_plane_per_full_round"] = round(res["gicp"]["full_rounds_ms_per_round"] /
                                                  res["plane"]["full_rounds_ms_per_round"], 4)
    res["gicp_over_point_per_full_round"] = round(res["gicp"]["full_rounds_ms_per_round"] /
                                                  res["point"]["full_rounds_ms_per_round"], 4)
    res["query_normals_over_gicp_call"] = round(res["normals_query_ms"] / res["gicp"]["ms"], 4)
    print(json.dumps(res))
    with open(a.json or os.path.join(ROOT, "profiles", "gicp_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
