"""The scan filters at the chair registration shape: `python tools/outlier_bench.py [--json PATH]`.

The 32 CAD targets of tools/icp_bench.py (10 000-point synthetic clouds voxelised at 0.03) with 2 % clutter added to each:
rows drawn uniformly in the target's bounding box widened by 20 % per side, appended and then spread among the target's
rows by a fixed permutation.  One call over the 32 segments each; medians of --reps device-event timings after warm-up, all
in one process, the calls taking turns round by round:
  mean16 / mean20   backend.knn_mean_dist at k = 16 and 20 (cs_knn_mean_dist);
  statistical       cs_outlier_statistical alone, on the means of k = 20;
  radius            backend.outlier_radius at 2.5 voxels, nb_points = 4 (cs_outlier_radius);
  *_scan            the same calls under CS_OUTLIER_GRID=0 (the exhaustive scan alone);
  normals16         backend.estimate_normals at k = 16: the yardstick -- the same search plus an eigen-solve, with indices.
Also the rows the grid paths answered and the rows the voucher sent back to the scan (CS_OUTLIER_STATS=1, runs of their
own), and what the two filters keep and drop.  Prints one JSON line; default PATH profiles/outlier_bench.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, synth  # noqa: E402

N_SEG, N_POINTS, VOXEL, CLUTTER = 32, 10000, 0.03, 0.02


def targets(dev):
    """(xyz f32 [n,3] device, offsets, is_clutter bool [n] host)."""
    cads = [synth.make_cloud(c, 15000)[:N_POINTS] for c in range(N_SEG)]
    xyz = torch.from_numpy(np.concatenate(cads)).to(dev)
    keep, _, off = B.voxelize(xyz, (np.arange(N_SEG + 1) * N_POINTS).tolist(), VOXEL)
    vox = xyz[keep].cpu().numpy()
    parts, flags = [], []
    for p in range(N_SEG):
        real = vox[off[p]:off[p + 1]]
        rng = np.random.default_rng(p)
        lo, hi = real.min(0).astype(np.float64), real.max(0).astype(np.float64)
        ext = hi - lo
        extra = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (int(CLUTTER * len(real)), 3)).astype(np.float32)
        perm = rng.permutation(len(real) + len(extra))
        parts.append(np.concatenate([real, extra])[perm])
        flags.append(np.concatenate([np.zeros(len(real), bool), np.ones(len(extra), bool)])[perm])
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    return torch.from_numpy(np.concatenate(parts)).to(dev), offsets, np.concatenate(flags)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "outlier_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--note", default="", help="free text kept in the result (date, visit)")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    xyz, off, flag = targets(dev)
    n_seg = len(off) - 1
    lib = _lib.load()
    mean20 = B.knn_mean_dist(xyz, off, 20)
    keep_u8 = torch.zeros(xyz.shape[0], dtype=torch.uint8, device=dev)
    stat = torch.zeros((n_seg, 4), dtype=torch.float64, device=dev)
    h_off = _lib.i64_array(off)

    def statistical():
        _lib.check(lib.cs_outlier_statistical(_lib.ptr(mean20), h_off, n_seg, 2.0, _lib.ptr(keep_u8), _lib.ptr(stat),
                                              _lib.stream_ptr()))

    def scan(fn):
        def run():
            os.environ["CS_OUTLIER_GRID"] = "0"       # read per call
            try:
                fn()
            finally:
                os.environ.pop("CS_OUTLIER_GRID", None)
        return run

    radius = 2.5 * VOXEL
    calls = {
        "mean16": lambda: B.knn_mean_dist(xyz, off, 16),
        "mean20": lambda: B.knn_mean_dist(xyz, off, 20),
        "statistical": statistical,
        "radius": lambda: B.outlier_radius(xyz, off, radius, 4),
        "normals16": lambda: B.estimate_normals(xyz, off, 16),
    }
    for name in ("mean16", "mean20", "radius"):
        calls[name + "_scan"] = scan(calls[name])
    os.environ.pop("CS_OUTLIER_GRID", None)
    os.environ.pop("CS_OUTLIER_STATS", None)
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    ms = {name: [] for name in calls}
    for _ in range(a.reps):                           # the calls take turns: drift of the clocks reaches all alike
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    res = {"tool": "tools/outlier_bench.py", "note": a.note, "device": torch.cuda.get_device_name(0),
           "segments": n_seg, "rows": int(off[-1]), "rows_min": int(np.diff(off).min()), "rows_max": int(np.diff(off).max()),
           "clutter_rows": int(flag.sum()), "reps": a.reps, "warmup": a.warmup,
           "median_ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
           "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
           "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()}}
    os.environ["CS_OUTLIER_STATS"] = "1"
    for k in (16, 20):
        B.outlier_stats(reset=True)
        B.knn_mean_dist(xyz, off, k)
        res["grid_rows_k%d" % k], res["redo_rows_k%d" % k] = B.outlier_stats(reset=True)
    B.outlier_radius(xyz, off, radius, 4)
    res["grid_rows_radius"] = B.outlier_stats(reset=True)[0]
    os.environ.pop("CS_OUTLIER_STATS", None)
    keep_s, _ = B.outlier_statistical(xyz, off, 20, 2.0)
    keep_r, _ = B.outlier_radius(xyz, off, radius, 4)
    for name, keep in (("statistical_20_2.0", keep_s), ("radius_2.5vox_4", keep_r)):
        keep = keep.cpu().numpy()
        # (the clutter is uniform in the widened box: part of it lands on the surface and is no outlier by any rule)
        res[name] = {"clutter_dropped": int((~keep[flag]).sum()), "clutter_rows": int(flag.sum()),
                     "real_dropped": int((~keep[~flag]).sum()), "real_rows": int((~flag).sum())}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
