"""cs_render_views at the chair registration shape: `python tools/view_bench.py [--json PATH]`.

The 32 posed clouds of tools/icp_bench.py (10 000 raw points each, 320 000 rows in one call), each under the camera
shapenet_eval's partial views would give it (3 half diagonals away, 40 degrees, squares and tolerance of 1.5 voxels of 0.03).
Medians of --reps device-event timings after warm-up, all in one process, the calls taking turns round by round:
  view_256, view_512                views.render_views at 256 x 256 and at 512 x 512 pixels, mask and stat only;
  view_256_depth                    the same with the f32 depth image exported;
  view_256_noread, view_512_noread  under CS_VIEW_PRECHECK=0 (read per call): every covered pixel gets its atomic;
  view_256_chunk8                   under CS_VIEW_CHUNK_BYTES of 8 images: four chunks instead of one;
  voxelize                          backend.voxelize at 0.03 on the same rows: the YARDSTICK, another one-pass-per-row call with
                                    integer atomics (it ends in a host wait for its offsets, inside the timed span).
No target was fixed in advance: there is no earlier version of this call.  The kernels of a call are not timed one by one, no
hardware counter is read, and no real scan is measured.  Prints one JSON line; default PATH profiles/view_bench.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, shapenet_eval as SE, views as V  # noqa: E402
import icp_bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "view_bench.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--note", default="", help="free text kept in the result (date, visit)")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    queries = icp_bench.problems(dev, 0.0, 0.0)[6]
    cfg = SE.Config()
    host = np.concatenate(queries).astype(np.float32)
    off = (np.arange(len(queries) + 1) * icp_bench.N_POINTS).tolist()
    xyz = torch.from_numpy(host).to(dev)
    lo, hi = np.stack([q.min(0) for q in queries]), np.stack([q.max(0) for q in queries])
    dirs = np.stack([SE.view_direction(cfg.random_seed, c) for c in range(len(queries))])
    cams = torch.from_numpy(V.view_cameras(lo, hi, dirs, cfg.view_distance)).to(dev)
    size, tol = cfg.view_point_size * icp_bench.VOXEL, cfg.view_depth_tol * icp_bench.VOXEL

    def view(side, depth=False, **env):
        focal = V.focal_from_fov(side, cfg.view_fov_deg)

        def run():
            os.environ.update(env)                    # read per call
            try:
                return V.render_views(xyz, off, cams, side, side, focal, size, tol, return_depth=depth)
            finally:
                for k in env:
                    os.environ.pop(k, None)
        return run

    calls = {
        "view_256": view(256),
        "view_512": view(512),
        "view_256_depth": view(256, True),
        "view_256_noread": view(256, CS_VIEW_PRECHECK="0"),
        "view_512_noread": view(512, CS_VIEW_PRECHECK="0"),
        "view_256_chunk8": view(256, CS_VIEW_CHUNK_BYTES=str(8 * 8 * 256 * 256)),
        "voxelize": lambda: B.voxelize(xyz, off, icp_bench.VOXEL),
    }
    for name in ("CS_VIEW_PRECHECK", "CS_VIEW_CHUNK_BYTES"):
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
    stat = {side: view(side)().stat.cpu().numpy().astype(np.int64) for side in (256, 512)}
    rows = int(off[-1])
    res = {"tool": "tools/view_bench.py", "note": a.note, "device": torch.cuda.get_device_name(0), "segments": len(queries),
           "rows": rows, "fov_deg": cfg.view_fov_deg, "distance_half_diagonals": cfg.view_distance,
           "point_size": size, "depth_tol": tol, "reps": a.reps, "warmup": a.warmup,
           "median_ms": {k: round(v, 4) for k, v in med.items()},
           "min_ms": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
           "max_ms": {k: round(float(np.max(v)), 4) for k, v in ms.items()},
           "view_256_over_voxelize": round(med["view_256"] / med["voxelize"], 3),
           "view_512_over_voxelize": round(med["view_512"] / med["voxelize"], 3),
           "noread_over_read_256": round(med["view_256_noread"] / med["view_256"], 3),
           "noread_over_read_512": round(med["view_512_noread"] / med["view_512"], 3),
           "rows_per_s_256": round(rows / (med["view_256"] * 1e-3)),
           "visible_share": {str(k): round(float(v[:, 2].sum()) / rows, 4) for k, v in stat.items()},
           "rows_in_frame": {str(k): int(v[:, 1].sum()) for k, v in stat.items()},
           "finite_pixels_mean": {str(k): round(float(v[:, 3].mean()), 1) for k, v in stat.items()},
           "not_measured": ["single kernels", "hardware counters", "any real scan"]}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
