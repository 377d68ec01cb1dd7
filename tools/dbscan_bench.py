"""Scan clustering at the chair registration shape: `python tools/dbscan_bench.py [--json PATH]`.

The input of tools/outlier_bench.py: the 32 CAD targets (10 000-point synthetic clouds voxelised at 0.03) with 2 % clutter.
One call over the 32 segments each; medians of --reps device-event timings after warm-up, all in one process, the calls
taking turns round by round:
  dbscan            backend.dbscan at 2.5 voxels, min_points = 5 (cs_dbscan: count, hook, compress, number, border);
  dbscan_scan       the same call under CS_DBSCAN_GRID=0 (the exhaustive scan alone);
  largest           cs_cluster_largest alone, on the labels of that call;
  radius            backend.outlier_radius at 2.5 voxels, nb_points = 4 (cs_outlier_radius): the YARDSTICK -- the count is
                    cs_dbscan's first pass, so dbscan / radius says what the components cost on top of it;
  radius_scan       the yardstick under CS_OUTLIER_GRID=0.
The kernels of a call are not timed one by one (that would take events inside the library).  Also the rows the grid
answered and the border rows (CS_DBSCAN_STATS=1, a run of its own) and what the largest cluster keeps and drops.  Prints
one JSON line; default PATH profiles/dbscan_bench.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B  # noqa: E402
from tools.outlier_bench import VOXEL, targets  # noqa: E402

EPS_VOXELS, MIN_POINTS = 2.5, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dbscan_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--note", default="", help="free text kept in the result (date, visit)")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    xyz, off, flag = targets(dev)
    n_seg = len(off) - 1
    lib = _lib.load()
    eps = EPS_VOXELS * VOXEL
    label, _ = B.dbscan(xyz, off, eps, MIN_POINTS)
    keep_u8 = torch.zeros(xyz.shape[0], dtype=torch.uint8, device=dev)
    stat = torch.zeros((n_seg, 3), dtype=torch.int32, device=dev)
    h_off = _lib.i64_array(off)

    def largest():
        _lib.check(lib.cs_cluster_largest(_lib.ptr(label), h_off, n_seg, _lib.ptr(keep_u8), _lib.ptr(stat),
                                          _lib.stream_ptr()))

    def scan(fn, switch):
        def run():
            os.environ[switch] = "0"                  # read per call
            try:
                fn()
            finally:
                os.environ.pop(switch, None)
        return run

    calls = {
        "dbscan": lambda: B.dbscan(xyz, off, eps, MIN_POINTS),
        "largest": largest,
        "radius": lambda: B.outlier_radius(xyz, off, eps, MIN_POINTS - 1),
    }
    calls["dbscan_scan"] = scan(calls["dbscan"], "CS_DBSCAN_GRID")
    calls["radius_scan"] = scan(calls["radius"], "CS_OUTLIER_GRID")
    for name in ("CS_DBSCAN_GRID", "CS_DBSCAN_STATS", "CS_OUTLIER_GRID", "CS_OUTLIER_STATS"):
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
    res = {"tool": "tools/dbscan_bench.py", "note": a.note, "device": torch.cuda.get_device_name(0),
           "segments": n_seg, "rows": int(off[-1]), "rows_min": int(np.diff(off).min()), "rows_max": int(np.diff(off).max()),
           "clutter_rows": int(flag.sum()), "eps_voxels": EPS_VOXELS, "min_points": MIN_POINTS, "reps": a.reps,
           "warmup": a.warmup,
           "median_ms": {k: round(v, 4) for k, v in med.items()},
           "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
           "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
           "dbscan_over_radius": round(med["dbscan"] / med["radius"], 3),
           "dbscan_scan_over_radius_scan": round(med["dbscan_scan"] / med["radius_scan"], 3)}
    os.environ["CS_DBSCAN_STATS"] = "1"
    B.dbscan_stats(reset=True)
    label, count = B.dbscan(xyz, off, eps, MIN_POINTS)
    res["grid_rows"], res["border_rows"] = B.dbscan_stats(reset=True)
    os.environ.pop("CS_DBSCAN_STATS", None)
    keep, st = B.cluster_largest(label, off)
    keep, st, lab = keep.cpu().numpy(), st.cpu().numpy(), label.cpu().numpy()
    # (the clutter is uniform in the widened box: part of it lands on the surface and is no outlier by any rule)
    res["largest_2.5vox_5"] = {"clutter_dropped": int((~keep[flag]).sum()), "clutter_rows": int(flag.sum()),
                               "real_dropped": int((~keep[~flag]).sum()), "real_rows": int((~flag).sum()),
                               "noise_rows": int((lab < 0).sum()), "clusters_min": int(st[:, 0].min()),
                               "clusters_max": int(st[:, 0].max())}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
