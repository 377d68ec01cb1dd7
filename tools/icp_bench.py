"""Batched ICP at the chair registration shape: `python tools/icp_bench.py [--json PATH]`.

32 (query, CAD) pairs of 10 000-point synthetic clouds (corsair_amd.synth, the construction of
harness.SyntheticScan2CAD) voxelised at 0.03; source = the query's voxels, target = the CAD's; T0 = the true pose
perturbed by --deg degrees and --trans; at most 30 updates, max_dist = 2 voxels.  Median of --reps repetitions after
warm-up, device events (wall time next to it):
 (a) backend.icp_batch (one cs_icp_batch call, no host wait inside);
 (b) the stand-in a user would write today from existing calls, per iteration: pose with torch in f64,
     backend.knn_feat on the 3-d points (k = 1), gather, batched Kabsch by torch.linalg.svd, and the host wait of the
     convergence test (it stops when every problem has converged);
 (c) for information: max_iter + 1 calls of backend.chamfer_1dir on the same problems -- the cost of the search alone
     with its target packers re-run every time.
Also the updates (a) and (b) actually applied, the share of workgroups the f16 association handed to the exhaustive kernel
(CS_ICP_STATS=1, a run of its own), the library's own time of the call (profile family "icp"), and -- information only --
one registration step (embed 32 queries, sym_pose_batch against their CADs) with icp_max_iter = 0 and 30 in this process.

`--estimation plane` measures instead, alternating in one process and on the same clouds: (a) the point call
above, (p) the point-to-plane call (cs_icp_plane_batch) with the target normals supplied, (n) backend.estimate_normals of
the 32 targets over --normal-k neighbours; with the updates per problem, the time per round, the fallback share and the
pose errors of both.  `--start large` is the 12 degree / 5 cm start with max_dist 0.12 (default: 3 degrees / 1 cm, 0.06).

`--normal-radius R` (with --estimation plane) times beside (n): (h) the hybrid search of at most --normal-k
rows inside R, and (n0) the exhaustive scan alone (CS_NORMALS_GRID=0); it records the share of the grid's rows that the
voucher sent back to the scan.
`--kernel huber|cauchy|tukey [--kernel-scale K]` (K defaults to one voxel, untuned) measures, alternating in one
process on the same problems: (l2) the point-to-plane call above and (k) cs_icp_plane_robust_batch with that kernel; per
call ms, updates, ms per round (DESIGN 13's definition, ms / (most updates + 1), and -- the cleaner figure -- a run of
exactly 11 full rounds: max_iter 10 with both convergence thresholds 0), mean RRE / RTE and the fallback share.
`--clutter F` makes the share F of every source clutter first: rows of the pair's target displaced by 0.035 / 0.06 of
max_dist along +x or +y (two slabs just off the surface, every row inside max_dist of a target row), moved into the
source's frame.  Without --json the result goes to profiles/icp_robust_<kernel>[_clutter].json.
`--with-scaling [--scale-mismatch S]` measures, alternating in one process on the same problems: point, plane,
point + scale and plane + scale (cs_icp_scale_batch), normals supplied.  Every source is shrunk by S about the origin of its
frame first (default 1.0; the true scale is 1 / S) and the start stays rigid.  Per call: ms, updates, ms per round (both
definitions of --kernel), the fallback share, mean RRE / RTE (on the rotation: the 3x3 block divided by the fitted scale)
and the mean scale error |scale * S - 1|.  Without --json the result goes to profiles/icp_scale.json.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, harness as H, synth  # noqa: E402

N_PAIRS, N_POINTS, VOXEL, MAX_ITER = 32, 10000, 0.03, 30


def timed(fn, reps, warmup=3):
    """(median device ms, median wall ms)."""
    for _ in range(warmup):
        fn()
    dev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    return round(float(np.median(dev)), 4), round(float(np.median(wall)), 4)


def perturbed(T, deg, trans, rng):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    a = np.deg2rad(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    D[:3, 3] = rng.uniform(-trans, trans, 3)
    return D @ T


def problems(dev, deg, trans):
    """Voxelised query / CAD clouds and the perturbed true poses (query -> CAD)."""
    rng = np.random.default_rng(31)
    cads = [synth.make_cloud(c, 15000)[:N_POINTS] for c in range(N_PAIRS)]
    poses = [synth.random_pose(c, max_trans=0.0) for c in range(N_PAIRS)]
    queries = [synth.apply_pose(synth.make_cloud(c, 15000)[15000 - N_POINTS:], poses[c], np.float32) for c in range(N_PAIRS)]
    raw_off = (np.arange(N_PAIRS + 1) * N_POINTS).tolist()
    out = []
    for clouds in (queries, cads):
        xyz = torch.from_numpy(np.concatenate(clouds)).to(dev)
        keep, _, off = B.voxelize(xyz, raw_off, VOXEL)
        out += [xyz[keep].contiguous(), [int(o) for o in off]]
    truth = np.stack([np.linalg.inv(T) for T in poses])
    T0 = np.stack([perturbed(T, deg, trans, rng) for T in truth]).astype(np.float32)
    return out[0], out[1], out[2], out[3], torch.from_numpy(T0).to(dev), truth, queries, cads


def torch_icp(x0, off0, x1, off1, T0, max_dist, max_iter, rf=1e-6, rr=1e-6):
    """The stand-in (b).  Returns (T f64 [P,4,4], updates applied per problem as a list)."""
    dev = x0.device
    P = len(off0) - 1
    lens = torch.tensor(np.diff(off0), device=dev)
    seg = torch.repeat_interleave(torch.arange(P, device=dev), lens, output_size=off0[-1])
    tstart = torch.tensor(off1[:-1], device=dev)[seg]
    x0d, x1d = x0.double(), x1.double()
    nsrc = lens.double()
    T = T0.double().clone()
    thr2 = max_dist * max_dist

    def evaluate(T):
        p = torch.bmm(T[seg, :3, :3], x0d[:, :, None])[:, :, 0] + T[seg, :3, 3]
        idx = B.knn_feat(p.float(), off0, x1, off1, 1)[:, 0].long() + tstart
        q = x1d[idx]
        d2 = ((p - q) ** 2).sum(1)
        w = (d2 < thr2).double()
        n = torch.zeros(P, dtype=torch.float64, device=dev).index_add_(0, seg, w)
        sd = torch.zeros(P, dtype=torch.float64, device=dev).index_add_(0, seg, w * d2)
        return p, q, w, n, n / nsrc, torch.sqrt(sd / n.clamp(min=1))

    p, q, w, n, fit, rm = evaluate(T)
    active = n >= 3
    iters = torch.zeros(P, dtype=torch.int32, device=dev)
    eye = torch.eye(4, dtype=torch.float64, device=dev)
    for _ in range(max_iter):
        mp = torch.zeros(P, 3, dtype=torch.float64, device=dev).index_add_(0, seg, w[:, None] * p) / n.clamp(min=1)[:, None]
        mq = torch.zeros(P, 3, dtype=torch.float64, device=dev).index_add_(0, seg, w[:, None] * q) / n.clamp(min=1)[:, None]
        dp, dq = (p - mp[seg]) * w[:, None], q - mq[seg]
        Hm = torch.zeros(P, 3, 3, dtype=torch.float64, device=dev).index_add_(0, seg, dp[:, :, None] * dq[:, None, :])
        U, _, Vt = torch.linalg.svd(Hm)
        V = Vt.transpose(1, 2)
        sgn = torch.sign(torch.linalg.det(V @ U.transpose(1, 2)))
        D = torch.diag_embed(torch.stack([torch.ones_like(sgn), torch.ones_like(sgn), sgn], 1))
        R = V @ D @ U.transpose(1, 2)
        Up = eye.repeat(P, 1, 1)
        Up[:, :3, :3] = R
        Up[:, :3, 3] = mq - torch.bmm(R, mp[:, :, None])[:, :, 0]
        T = torch.where(active[:, None, None], Up @ T, T)
        iters += active.int()
        pf, pr = fit, rm
        p, q, w, n, fit, rm = evaluate(T)
        active = active & ~(((fit - pf).abs() < rf) & ((rm - pr).abs() < rr)) & (n >= 3)
        if not bool(active.any().item()):          # the host wait of the convergence test
            break
    return T, iters.tolist()


def timed_alternating(fns, reps, warmup=3):
    """Median device ms of every function of `fns`, the calls interleaved a, b, c, a, b, c, ... in this process."""
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
    return {k: round(float(np.median(v)), 4) for k, v in ms.items()}


def plane_report(a, res, x0, off0, x1, off1, T0, truth, max_dist):
    """The measurement of DESIGN 13: (a) point, (p) plane with normals supplied, (n) the normals of the targets."""
    pairs = list(range(N_PAIRS))
    nrm = B.estimate_normals(x1, off1, a.normal_k)
    fns = {"point": lambda: B.icp_batch(x0, off0, x1, off1, pairs, pairs, T0, max_dist, MAX_ITER),
           "plane": lambda: B.icp_batch(x0, off0, x1, off1, pairs, pairs, T0, max_dist, MAX_ITER, tgt_normals=nrm),
           "normals": lambda: B.estimate_normals(x1, off1, a.normal_k)}
    if a.normal_radius > 0:     # (h) the hybrid search beside (n): at most normal_k rows inside the radius
        fns["normals_hybrid"] = lambda: B.estimate_normals(x1, off1, a.normal_k, radius=a.normal_radius)
    os.environ["CS_NORMALS_GRID"] = "0"     # (n0) the exhaustive scan alone, the definition
    ms0 = timed_alternating({"normals": fns["normals"]}, a.reps)
    del os.environ["CS_NORMALS_GRID"]
    ms = timed_alternating(fns, a.reps)
    res.update({"estimation": "plane", "normal_k": a.normal_k, "icp_point_ms": ms["point"], "icp_plane_ms": ms["plane"],
                "normals_ms": ms["normals"], "normals_exhaustive_ms": ms0["normals"],
                "plane_over_point": round(ms["plane"] / ms["point"], 4),
                "bar_plane_le_point": bool(ms["plane"] <= ms["point"])})
    os.environ["CS_NORMALS_STATS"] = "1"
    B.normals_stats(reset=True)
    fns["normals"]()
    st = B.normals_stats(reset=True)
    res["normals_grid_rows"], res["normals_fallback_share"] = st[0], round(st[1] / max(st[0], 1), 6)
    if a.normal_radius > 0:
        found = fns["normals_hybrid"]()
        res.update({"normal_radius": a.normal_radius, "normals_hybrid_ms": ms["normals_hybrid"],
                    "normals_hybrid_grid_rows": B.normals_stats(reset=True)[0],
                    "normals_hybrid_differs_from_knn_rows": int((found != nrm).any(1).sum())})
    del os.environ["CS_NORMALS_STATS"]

    def errs(T):
        T = T.cpu().numpy().astype(np.float64)
        rre = [np.degrees(np.arccos(np.clip((np.trace(T[p, :3, :3] @ truth[p, :3, :3].T) - 1) / 2, -1, 1))) for p in pairs]
        rte = [np.linalg.norm(T[p, :3, 3] - truth[p, :3, 3]) for p in pairs]
        return round(float(np.mean(rre)), 4), round(float(np.mean(rte)), 5)

    res["rre_deg_rte_before"] = errs(T0)
    os.environ["CS_ICP_STATS"] = "1"
    for k in ("point", "plane"):
        B.icp_stats(reset=True)
        r = fns[k]()
        st = B.icp_stats(reset=True)
        it = r.iters.cpu().numpy()
        res["updates_" + k] = {"mean": round(float(it.mean()), 2), "min": int(it.min()), "max": int(it.max())}
        res["icp_%s_ms_per_round" % k] = round(ms[k] / (float(it.max()) + 1), 4)
        res["fallback_share_" + k] = round(st[1] / max(st[0], 1), 5)
        res["rre_deg_rte_after_" + k] = errs(r.T)
        res["fitness_mean_" + k] = round(float(r.fitness.mean()), 4)
    del os.environ["CS_ICP_STATS"]
    return res


def add_clutter(x0, off0, x1, off1, truth, share, max_dist):
    """Sources of which `share` is clutter: per pair, rows of the target shifted by 0.035 / 0.06 * max_dist along +x (half)
    or +y (half) and moved by the inverse of the true pose (query -> CAD) into the query's frame."""
    rng = np.random.default_rng(14)
    s, t = x0.cpu().numpy().astype(np.float64), x1.cpu().numpy().astype(np.float64)
    shift = 0.035 / 0.06 * max_dist
    parts, off = [], [0]
    for p in range(len(off0) - 1):
        src, tgt = s[off0[p]:off0[p + 1]], t[off1[p]:off1[p + 1]]
        n = int(round(share / (1.0 - share) * len(src)))
        rows = tgt[rng.integers(0, len(tgt), n)].copy()
        rows[:n // 2, 0] += shift
        rows[n // 2:, 1] += shift
        Tinv = np.linalg.inv(truth[p])
        parts += [src, rows @ Tinv[:3, :3].T + Tinv[:3, 3]]
        off.append(off[-1] + len(src) + n)
    return torch.from_numpy(np.concatenate(parts).astype(np.float32)).to(x0.device), off


def robust_report(a, res, x0, off0, x1, off1, T0, truth, max_dist):
    """The measurement of DESIGN 14: (l2) the plane call and (k) the call with a robust kernel, alternating."""
    pairs = list(range(N_PAIRS))
    scale = a.kernel_scale if a.kernel_scale > 0 else VOXEL
    if a.clutter > 0:
        x0, off0 = add_clutter(x0, off0, x1, off1, truth, a.clutter, max_dist)
    nrm = B.estimate_normals(x1, off1, a.normal_k)
    kw = {"l2": {}, a.kernel: {"kernel": a.kernel, "kernel_scale": scale}}

    def call(k, max_iter=MAX_ITER, **more):
        return B.icp_batch(x0, off0, x1, off1, pairs, pairs, T0, max_dist, max_iter, tgt_normals=nrm, **kw[k], **more)

    full = dict(relative_fitness=0.0, relative_rmse=0.0)           # no problem converges: max_iter + 1 full rounds
    ms = timed_alternating({"l2": lambda: call("l2"), a.kernel: lambda: call(a.kernel),
                            "l2_full": lambda: call("l2", 10, **full), a.kernel + "_full": lambda: call(a.kernel, 10, **full)},
                           a.reps)
    res.update({"estimation": "plane", "normal_k": a.normal_k, "kernel": a.kernel, "kernel_scale": scale,
                "clutter": a.clutter, "source_rows": off0[-1]})

    def errs(T):
        T = T.cpu().numpy().astype(np.float64)
        rre = [np.degrees(np.arccos(np.clip((np.trace(T[p, :3, :3] @ truth[p, :3, :3].T) - 1) / 2, -1, 1))) for p in pairs]
        rte = [np.linalg.norm(T[p, :3, 3] - truth[p, :3, 3]) for p in pairs]
        return round(float(np.mean(rre)), 4), round(float(np.mean(rte)), 5)

    res["rre_deg_rte_before"] = errs(T0)
    os.environ["CS_ICP_STATS"] = "1"
    for k in ("l2", a.kernel):
        B.icp_stats(reset=True)
        r = call(k)
        st = B.icp_stats(reset=True)
        it = r.iters.cpu().numpy()
        full_it = call(k, 10, **full).iters.cpu().numpy()
        res[k] = {"ms": ms[k], "updates": {"mean": round(float(it.mean()), 2), "min": int(it.min()), "max": int(it.max())},
                  "ms_per_round": round(ms[k] / (float(it.max()) + 1), 4),
                  "full_rounds_ms": ms[k + "_full"], "full_rounds_updates_min": int(full_it.min()),
                  "full_rounds_ms_per_round": round(ms[k + "_full"] / 11.0, 4),
                  "fallback_share": round(st[1] / max(st[0], 1), 5), "rre_deg_rte_after": errs(r.T),
                  "fitness_mean": round(float(r.fitness.mean()), 4),
                  "wfitness_mean": None if r.wfitness is None else round(float(r.wfitness.mean()), 4)}
    del os.environ["CS_ICP_STATS"]
    res["kernel_over_l2_per_round"] = round(res[a.kernel]["ms_per_round"] / res["l2"]["ms_per_round"], 4)
    res["kernel_over_l2_per_full_round"] = round(res[a.kernel]["full_rounds_ms_per_round"] /
                                                 res["l2"]["full_rounds_ms_per_round"], 4)
    res["bar_kernel_le_1p10_l2_per_round"] = bool(res["kernel_over_l2_per_round"] <= 1.10)
    return res


def scale_report(a, res, x0, off0, x1, off1, T0, truth, max_dist):
    """The measurement of DESIGN 16: the two rigid calls and their siblings with a scale, alternating."""
    pairs = list(range(N_PAIRS))
    S = a.scale_mismatch
    x0 = (x0.double() * S).float().contiguous()
    nrm = B.estimate_normals(x1, off1, a.normal_k)
    kw = {"point": {}, "plane": {"tgt_normals": nrm}, "point_scale": {"with_scaling": True},
          "plane_scale": {"tgt_normals": nrm, "with_scaling": True}}

    def call(k, max_iter=MAX_ITER, **more):
        return B.icp_batch(x0, off0, x1, off1, pairs, pairs, T0, max_dist, max_iter, **kw[k], **more)

    full = dict(relative_fitness=0.0, relative_rmse=0.0)           # no problem converges: max_iter + 1 full rounds
    fns = {k: (lambda k=k: call(k)) for k in kw}
    fns.update({k + "_full": (lambda k=k: call(k, 10, **full)) for k in kw})
    ms = timed_alternating(fns, a.reps)
    res.update({"normal_k": a.normal_k, "scale_mismatch": S, "true_scale": 1.0 / S, "scale_bounds": [0.5, 2.0]})

    def errs(T, scale):
        T = T.cpu().numpy().astype(np.float64)
        rre = [np.degrees(np.arccos(np.clip((np.trace((T[p, :3, :3] / scale[p]) @ truth[p, :3, :3].T) - 1) / 2, -1, 1)))
               for p in pairs]
        rte = [np.linalg.norm(T[p, :3, 3] - truth[p, :3, 3]) for p in pairs]
        return round(float(np.mean(rre)), 4), round(float(np.mean(rte)), 5)

    res["rre_deg_rte_before"] = errs(T0, np.ones(N_PAIRS))
    os.environ["CS_ICP_STATS"] = "1"
    for k in kw:
        B.icp_stats(reset=True)
        r = call(k)
        st = B.icp_stats(reset=True)
        it = r.iters.cpu().numpy()
        full_it = call(k, 10, **full).iters.cpu().numpy()
        sc = np.ones(N_PAIRS) if r.scale is None else r.scale.cpu().numpy()
        res[k] = {"ms": ms[k], "updates": {"mean": round(float(it.mean()), 2), "min": int(it.min()), "max": int(it.max())},
                  "ms_per_round": round(ms[k] / (float(it.max()) + 1), 4),
                  "full_rounds_ms": ms[k + "_full"], "full_rounds_updates_min": int(full_it.min()),
                  "full_rounds_ms_per_round": round(ms[k + "_full"] / 11.0, 4),
                  "fallback_share": round(st[1] / max(st[0], 1), 5), "rre_deg_rte_after": errs(r.T, sc),
                  "scale_error_mean": round(float(np.mean(np.abs(sc * S - 1.0))), 6),
                  "scale_error_max": round(float(np.max(np.abs(sc * S - 1.0))), 6),
                  "fitness_mean": round(float(r.fitness.mean()), 4)}
    del os.environ["CS_ICP_STATS"]
    for k in ("point", "plane"):
        res["%s_scale_over_%s_per_round" % (k, k)] = round(res[k + "_scale"]["ms_per_round"] / res[k]["ms_per_round"], 4)
        res["%s_scale_over_%s_per_full_round" % (k, k)] = round(res[k + "_scale"]["full_rounds_ms_per_round"] /
                                                                res[k]["full_rounds_ms_per_round"], 4)
    res["plane_scale_over_point_scale_total"] = round(res["plane_scale"]["ms"] / res["point_scale"]["ms"], 4)
    res["bar_plane_scale_le_point_scale_total"] = bool(res["plane_scale"]["ms"] <= res["point_scale"]["ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--deg", type=float, default=3.0)
    ap.add_argument("--trans", type=float, default=0.01)
    ap.add_argument("--no-step", action="store_true", help="skip the registration-step timing (it builds the network)")
    ap.add_argument("--estimation", default="point", choices=["point", "plane"],
                    help="plane: point against point-to-plane against the normals, alternating (DESIGN 13)")
    ap.add_argument("--normal-k", type=int, default=16)
    ap.add_argument("--normal-radius", type=float, default=0.0,
                    help="with --estimation plane: also time the hybrid search (at most --normal-k rows inside this radius)")
    ap.add_argument("--start", default="small", choices=["small", "large"],
                    help="large: 12 degrees / 5 cm with max_dist 0.12 (overrides --deg / --trans)")
    ap.add_argument("--kernel", default="l2", choices=["l2", "huber", "cauchy", "tukey"],
                    help="a robust kernel: the plane call against cs_icp_plane_robust_batch with it, alternating (DESIGN 14)")
    ap.add_argument("--kernel-scale", type=float, default=0.0, help="scale of --kernel; 0 = one voxel (untuned)")
    ap.add_argument("--clutter", type=float, default=0.0,
                    help="share of every source that is clutter just off the target's surface (with --kernel)")
    ap.add_argument("--with-scaling", action="store_true",
                    help="point / plane against point + scale / plane + scale (cs_icp_scale_batch), alternating (DESIGN 16)")
    ap.add_argument("--scale-mismatch", type=float, default=1.0,
                    help="with --with-scaling: every source is shrunk by this factor first; the start stays rigid")
    a = ap.parse_args()
    if not 0.5 < a.scale_mismatch < 2.0 or (a.scale_mismatch != 1.0 and not a.with_scaling):
        ap.error("--scale-mismatch needs a factor in (0.5, 2) and --with-scaling")
    if a.with_scaling and a.kernel != "l2":
        ap.error("--with-scaling with a robust --kernel is out of scope")
    if not 0.0 <= a.clutter < 1.0 or (a.clutter > 0 and a.kernel == "l2"):
        ap.error("--clutter needs a share in [0, 1) and a --kernel")
    dev = torch.device("cuda:0")
    max_dist = 2 * VOXEL
    if a.start == "large":
        a.deg, a.trans, max_dist = 12.0, 0.05, 4 * VOXEL
    x0, off0, x1, off1, T0, truth, queries, cads = problems(dev, a.deg, a.trans)
    pairs = list(range(N_PAIRS))
    res = {"device": torch.cuda.get_device_name(dev), "hip": torch.version.hip, "pairs": N_PAIRS, "voxel": VOXEL,
           "source_rows": off0[-1], "target_rows": off1[-1], "max_dist": max_dist, "max_iter": MAX_ITER,
           "perturbation": {"deg": a.deg, "trans": a.trans}}
    if a.with_scaling:
        res = scale_report(a, res, x0, off0, x1, off1, T0, truth, max_dist)
        print(json.dumps(res))
        with open(a.json or os.path.join(ROOT, "profiles", "icp_scale.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if a.kernel != "l2":
        res = robust_report(a, res, x0, off0, x1, off1, T0, truth, max_dist)
        print(json.dumps(res))
        path = a.json or os.path.join(ROOT, "profiles", "icp_robust_%s%s.json" % (a.kernel, "_clutter" if a.clutter > 0 else ""))
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        return
    if a.estimation == "plane":
        res = plane_report(a, res, x0, off0, x1, off1, T0, truth, max_dist)
        print(json.dumps(res))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return

    def hip():
        return B.icp_batch(x0, off0, x1, off1, pairs, pairs, T0, max_dist, MAX_ITER)

    res["icp_hip_ms"], res["icp_hip_wall_ms"] = timed(hip, a.reps)
    res["icp_torch_ms"], res["icp_torch_wall_ms"] = timed(lambda: torch_icp(x0, off0, x1, off1, T0, max_dist, MAX_ITER),
                                                          a.reps)
    res["torch_over_hip"] = round(res["icp_torch_ms"] / res["icp_hip_ms"], 2)
    res["chamfer_x%d_ms" % (MAX_ITER + 1)], _ = timed(
        lambda: [B.chamfer_1dir(x0, off0, x1, off1, pairs, pairs, T0) for _ in range(MAX_ITER + 1)], a.reps)
    r = hip()
    Tt, it_t = torch_icp(x0, off0, x1, off1, T0, max_dist, MAX_ITER)
    it_h = r.iters.cpu().numpy()
    res["updates_hip"] = {"mean": round(float(it_h.mean()), 2), "min": int(it_h.min()), "max": int(it_h.max())}
    res["updates_torch"] = {"mean": round(float(np.mean(it_t)), 2), "min": int(min(it_t)), "max": int(max(it_t))}
    res["max_abs_T_diff_vs_torch"] = float((r.T - Tt).abs().max())
    res["icp_hip_ms_per_round"] = round(res["icp_hip_ms"] / (float(it_h.max()) + 1), 4)

    def errs(T):
        T = T.cpu().numpy().astype(np.float64)
        rre = [np.degrees(np.arccos(np.clip((np.trace(T[p, :3, :3] @ truth[p, :3, :3].T) - 1) / 2, -1, 1))) for p in pairs]
        rte = [np.linalg.norm(T[p, :3, 3] - truth[p, :3, 3]) for p in pairs]
        return round(float(np.mean(rre)), 4), round(float(np.mean(rte)), 5)

    res["rre_deg_rte_before"], res["rre_deg_rte_after"] = errs(T0), errs(r.T)
    res["fitness_mean"] = round(float(r.fitness.mean()), 4)
    _lib.prof_enable(True)
    _lib.prof_reset()
    for _ in range(a.reps):
        hip()
    torch.cuda.synchronize()
    ms, n, flop = _lib.prof_get("icp")
    _lib.prof_enable(False)
    res["icp_family_ms_per_call"] = round(ms / a.reps, 4)
    os.environ["CS_ICP_STATS"] = "1"
    B.icp_stats(reset=True)
    hip()
    st = B.icp_stats(reset=True)
    del os.environ["CS_ICP_STATS"]
    res["f16_workgroups"], res["fallback_share"] = st[0], round(st[1] / max(st[0], 1), 5)
    os.environ["CS_ICP_F16"] = "0"
    res["icp_hip_exhaustive_ms"], _ = timed(hip, max(a.reps // 3, 3))
    del os.environ["CS_ICP_F16"]

    # ---- information only: one registration step with and without the refinement ----------------------------------------
    if not a.no_step:
        sd, emb = synth.make_state_dicts(31)
        q64 = [c.astype(np.float64) for c in queries]
        for iters in (0, MAX_ITER):
            pipe = H.Pipeline(sd, emb, device=dev, config=H.Config(icp_max_iter=iters))
            cat = pipe.embed_clouds(cads)
            qx = torch.from_numpy(np.concatenate(q64)).to(dev)
            qoff = (np.arange(N_PAIRS + 1) * N_POINTS).tolist()

            def step():
                pipe.register(pipe.embed_batch(qx, qoff), cat, np.ones(N_PAIRS, np.int32), force_gate=True)

            res["register_step_ms_icp%d" % iters], res["register_step_wall_ms_icp%d" % iters] = timed(step, 5, 2)
        res["register_step_icp_over_plain"] = round(res["register_step_ms_icp%d" % MAX_ITER] / res["register_step_ms_icp0"], 4)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
