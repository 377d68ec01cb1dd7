"""Support-plane segmentation at the chair registration shape: `python tools/plane_bench.py [--json PATH]`.

The input of tools/outlier_bench.py -- the 32 CAD targets (10 000-point synthetic clouds voxelised at 0.03) with 2 % clutter --
with a FLOOR under every target: the recipe of tests/plane_cases.py (a voxel lattice over the x-y box widened by 30 % per
side, half a voxel below the lowest row, +-0.3 voxel of noise, a slope of 3 degrees), every segment permuted.
One call over the 32 segments each; medians of --reps device-event timings after warm-up, all in one process, the calls
taking turns round by round:
  plane             backend.segment_plane at 1 voxel, 1 024 hypotheses (cs_segment_plane: count, best, the row passes, the fit);
  plane_256, plane_4096     the same at 256 and at 4 096 hypotheses;
  plane_slice512, plane_slice4096   the 1 024-hypothesis call under CS_PLANE_SLICE=512 and =4096 (read per call);
  dbscan            backend.dbscan at 2.5 voxels / 5 points on the same input: a YARDSTICK, the step that follows in the pipeline;
  radius            backend.outlier_radius at 2.5 voxels / 4 on the same input: the second yardstick.
No target was fixed in advance: there is no earlier version of this call.  The kernels of a call are not timed one by one
(that would take events inside the library), no hardware counter is read, and no real scan is measured.  Also what the
step removes under the default Config.  Prints one JSON line; default PATH profiles/plane_bench.json."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, harness as H  # noqa: E402
from tools.outlier_bench import VOXEL, targets  # noqa: E402

DIST_VOXELS, ITERS = 1.0, 1024


def with_floors(xyz, off, flag):
    """(xyz f32 [n,3] host, offsets, kind uint8 [n]: 0 real, 1 clutter, 2 floor)."""
    parts, kinds = [], []
    for p in range(len(off) - 1):
        seg, clutter = xyz[off[p]:off[p + 1]], flag[off[p]:off[p + 1]]
        real = seg[~clutter].astype(np.float64)
        lo, hi = real.min(0), real.max(0)
        ext = hi - lo
        ga = np.arange(lo[0] - 0.3 * ext[0], hi[0] + 0.3 * ext[0], VOXEL)
        gb = np.arange(lo[1] - 0.3 * ext[1], hi[1] + 0.3 * ext[1], VOXEL)
        A, Bg = np.meshgrid(ga, gb, indexing="ij")
        rng = np.random.default_rng(200 + p)
        z = lo[2] - 0.5 * VOXEL + rng.uniform(-0.3 * VOXEL, 0.3 * VOXEL, A.size) \
            + math.tan(math.radians(3.0)) * (A.ravel() - (lo[0] + hi[0]) / 2)
        floor = np.stack([A.ravel(), Bg.ravel(), z], 1).astype(np.float32)
        perm = rng.permutation(len(seg) + len(floor))
        parts.append(np.concatenate([seg, floor])[perm])
        kinds.append(np.concatenate([clutter.astype(np.uint8), np.full(len(floor), 2, np.uint8)])[perm])
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).tolist()
    return np.concatenate(parts), offsets, np.concatenate(kinds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "plane_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--note", default="", help="free text kept in the result (date, visit)")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    xyz_d, off, flag = targets(dev)
    host, off, kind = with_floors(xyz_d.cpu().numpy(), off, flag)
    xyz = torch.from_numpy(host).to(dev)
    n_seg = len(off) - 1
    dist = DIST_VOXELS * VOXEL

    def sliced(rows):
        def run():
            os.environ["CS_PLANE_SLICE"] = str(rows)   # read per call
            try:
                B.segment_plane(xyz, off, dist, ITERS)
            finally:
                os.environ.pop("CS_PLANE_SLICE", None)
        return run

    calls = {
        "plane": lambda: B.segment_plane(xyz, off, dist, ITERS),
        "plane_256": lambda: B.segment_plane(xyz, off, dist, 256),
        "plane_4096": lambda: B.segment_plane(xyz, off, dist, 4096),
        "plane_slice512": sliced(512),
        "plane_slice4096": sliced(4096),
        "dbscan": lambda: B.dbscan(xyz, off, 2.5 * VOXEL, 5),
        "radius": lambda: B.outlier_radius(xyz, off, 2.5 * VOXEL, 4),
    }
    for name in ("CS_PLANE_SLICE", "CS_DBSCAN_GRID", "CS_DBSCAN_STATS", "CS_OUTLIER_GRID", "CS_OUTLIER_STATS"):
        os.environ.pop(name, None)
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
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rows = int(off[-1])
    res = {"tool": "tools/plane_bench.py", "note": a.note, "device": torch.cuda.get_device_name(0),
           "segments": n_seg, "rows": rows, "rows_min": int(np.diff(off).min()), "rows_max": int(np.diff(off).max()),
           "floor_rows": int((kind == 2).sum()), "clutter_rows": int((kind == 1).sum()), "dist_voxels": DIST_VOXELS,
           "iters": ITERS, "slice_default": 1024, "reps": a.reps, "warmup": a.warmup,
           "median_ms": {k: round(v, 4) for k, v in med.items()},
           "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
           "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
           "plane_over_dbscan": round(med["plane"] / med["dbscan"], 3),
           "plane_over_radius": round(med["plane"] / med["radius"], 3),
           # ten f64 operations per (row, hypothesis): the nominal rate of the whole call, the count kernel not isolated
           "plane_gflops_nominal": round(10.0 * rows * ITERS / (med["plane"] * 1e-3) / 1e9, 1),
           "not_measured": ["single kernels", "hardware counters", "any real scan"]}
    inlier, plane, stat = B.segment_plane(xyz, off, dist, ITERS)
    inlier, plane, stat = inlier.cpu().numpy(), plane.cpu().tolist(), stat.cpu().tolist()
    cfg = H.Config()
    support = [H.is_support_plane(stat[p], plane[p], cfg) for p in range(n_seg)]
    drop = np.zeros(rows, bool)
    for p in range(n_seg):
        if support[p]:
            drop[off[p]:off[p + 1]] = inlier[off[p]:off[p + 1]]
    res["remove_1vox_1024"] = {"support_planes": int(sum(support)), "floor_dropped": int(drop[kind == 2].sum()),
                               "floor_rows": int((kind == 2).sum()), "real_dropped": int(drop[kind == 0].sum()),
                               "real_rows": int((kind == 0).sum()), "refits": int(sum(s[3] for s in stat))}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
