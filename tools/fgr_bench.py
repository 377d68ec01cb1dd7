"""Fast Global Registration against the RANSAC on the correspondence lists of one chair-shaped registration step:
`python tools/fgr_bench.py [--json PATH]`.

32 (query, CAD) pairs from the bench's generator (corsair_amd.synth: CAD c = make_cloud(c, 15000)[:10000], the query its
last 10 000 points under random_pose(c), voxelised at 0.03) with the bench's converging-regime features: a voxel's feature
is its CAD-frame coordinate zero-padded to 16-d, so the feature 5-NN is a spatial 5-NN and at best one neighbour in five
is right.  Symmetry labels: the chair histogram's shape (one query with label 4, the rest 1), forced gate, so every query
has its vanilla list and its part-configuration lists, about a hundred problems of 5 x (voxels of the query) pairs.

The lists are the ones registration.sym_pose_batch(registration="fgr") hands to stage 4 (captured from one call).  On
them, alternating in this process, median of --reps repetitions after 3 warm-up rounds, device events:
  (f) backend.fgr_batch with the defaults (tuple test on, 64 iterations, mu_floor 0.025 -- untuned),
  (r) backend.ransac_batch (100 000 x 10-point, confidence 0.999),
and, on request, (f0) fgr_batch without the tuple test (--no-tuple: the slow case, whole lists in the line process).
For each: the library's own time (profile family), and after stages 5 - 6 (Chamfer of every estimate, first minimum per
pair) the share of pairs with RRE <= 5 / 15 degrees, RTE <= 0.10, the mean Chamfer of the kept pose; for FGR the tuples
kept and updates applied, for the RANSAC the iterations consumed.  No speed ratio is a target: the figures are recorded.
Prints one JSON line; without --json it also goes to profiles/fgr_bench.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, harness as H, registration as R, synth  # noqa: E402

N_PAIRS, N_POINTS, VOXEL, MAX_CORR = 32, 10000, 0.03, 0.2


def step_inputs(dev):
    """Voxel origins and converging-regime features of the 32 pairs; the true poses (query -> CAD is their inverse)."""
    cads = [synth.make_cloud(c, 15000)[:N_POINTS] for c in range(N_PAIRS)]
    poses = [synth.random_pose(c, max_trans=0.0) for c in range(N_PAIRS)]
    queries = [synth.apply_pose(synth.make_cloud(c, 15000)[15000 - N_POINTS:], poses[c], np.float32) for c in range(N_PAIRS)]
    raw_off = (np.arange(N_PAIRS + 1) * N_POINTS).tolist()
    out = []
    for clouds in (queries, cads):
        xyz = torch.from_numpy(np.concatenate(clouds)).to(dev)
        keep, _, off = B.voxelize(xyz, raw_off, VOXEL)
        out += [xyz[keep].contiguous(), [int(o) for o in off]]
    x0, off0, x1, off1 = out
    Ts = np.stack(poses)
    Rm = torch.from_numpy(Ts[:, :3, :3].astype(np.float32)).to(dev)
    t = torch.from_numpy(Ts[:, :3, 3].astype(np.float32)).to(dev)
    seg = torch.repeat_interleave(torch.arange(N_PAIRS, device=dev), torch.as_tensor(np.diff(off0), device=dev),
                                  output_size=x0.shape[0])
    x_cad = torch.einsum("nj,njk->nk", x0 - t[seg], Rm[seg])                 # R^T (x - t): the bench's stand-in
    pad = torch.nn.functional.pad
    return pad(x_cad, (0, 13)).contiguous(), x0, off0, pad(x1, (0, 13)).contiguous(), x1, off1, poses


def capture_lists(F0, x0, off0, F1, x1, off1, syms):
    """The (src, tgt, offsets) stage 4 receives, and the pair of every problem."""
    got = {}
    real = B.fgr_batch

    def spy(src, tgt, offsets, *a, **k):
        got["lists"] = (src, tgt, list(offsets))
        return real(src, tgt, offsets, *a, **k)

    B.fgr_batch = spy
    try:
        res = R.sym_pose_batch(F0, x0, off0, F1, x1, off1, syms, 5, MAX_CORR, 0, force_gate=True, registration="fgr")
    finally:
        B.fgr_batch = real
    return got["lists"], res.prob_pair


def timed_alternating(fns, reps, warmup=3):
    """Median device ms of every function of `fns`, the calls interleaved a, b, a, b, ... in this process."""
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
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4),
                "max_ms": round(float(max(v)), 4)} for k, v in ms.items()}


def family_ms(fn, families, reps):
    _lib.prof_enable(True)
    _lib.prof_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    out = {f: round(_lib.prof_get(f)[0] / reps, 4) for f in families}
    _lib.prof_enable(False)
    return out


def accuracy(T, x0, off0, x1, off1, pair, poses, syms):
    """Stages 5 - 6 on the estimates T [n_problems,4,4] and the pose metrics of the kept ones."""
    cd = B.chamfer_1dir(x0, off0, x1, off1, pair, pair, T).cpu().numpy()
    best = np.arange(N_PAIRS)
    for j in range(N_PAIRS, len(pair)):
        if cd[best[pair[j]]] > cd[j]:
            best[pair[j]] = j
    Tb = T.cpu().numpy().astype(np.float64)[best]
    t_l, r_l = [], []
    for p in range(N_PAIRS):
        t, r = H.eval_pose(Tb[p], poses[p], np.eye(4), int(syms[p]))
        t_l.append(t)
        r_l.append(r)
    agg = H.aggregate(r_l, t_l)
    return {"rre_5": agg["rre_5"], "rre_15": agg["rre_15"], "rre_mean_deg": round(agg["rre_mean_deg"], 3),
            "rte_010": agg["rte_010"], "chamfer_mean": float(cd[best].mean()),
            "kept_is_vanilla_share": float(np.mean(best < N_PAIRS))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mu-floor", type=float, default=0.025)
    ap.add_argument("--no-tuple", action="store_true", help="also time and score fgr_batch without the tuple test")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    syms = np.ones(N_PAIRS, np.int32)
    syms[0] = 4
    F0, x0, off0, F1, x1, off1, poses = step_inputs(dev)
    (src, tgt, offs), pair = capture_lists(F0, x0, off0, F1, x1, off1, syms)
    lens = np.diff(offs)
    res = {"device": torch.cuda.get_device_name(0), "pairs": N_PAIRS, "problems": len(pair),
           "pairs_per_problem": {"min": int(lens.min()), "mean": round(float(lens.mean()), 1), "max": int(lens.max())},
           "max_corr": MAX_CORR, "mu_floor": a.mu_floor, "reps": a.reps}
    fns = {"fgr": lambda: B.fgr_batch(src, tgt, offs, MAX_CORR, mu_floor=a.mu_floor),
           "ransac": lambda: B.ransac_batch(src, tgt, offs, MAX_CORR, 10, 100000, 0.999, 0)}
    if a.no_tuple:
        fns["fgr_no_tuple"] = lambda: B.fgr_batch(src, tgt, offs, MAX_CORR, mu_floor=a.mu_floor, tuple_test=False)
    res["device_ms"] = timed_alternating(fns, a.reps)
    res["ransac_over_fgr"] = round(res["device_ms"]["ransac"]["median_ms"] / res["device_ms"]["fgr"]["median_ms"], 2)
    res["family_ms_per_call"] = {"fgr": family_ms(fns["fgr"], ("fgr",), a.reps),
                                 "ransac": family_ms(fns["ransac"], ("ransac_hyp", "ransac_pre", "ransac_eval"), a.reps)}
    r = fns["fgr"]()
    nt, it = r.n_tuple.cpu().numpy(), r.iters.cpu().numpy()
    res["fgr"] = accuracy(r.T, x0, off0, x1, off1, pair, poses, syms)
    res["fgr"].update({"tuples": {"min": int(nt.min()), "mean": round(float(nt.mean()), 1), "max": int(nt.max())},
                       "updates": {"min": int(it.min()), "mean": round(float(it.mean()), 2), "max": int(it.max())},
                       "inliers_mean": round(float(r.inliers.float().mean()), 1)})
    T, inl, _, its = fns["ransac"]()
    res["ransac"] = accuracy(T, x0, off0, x1, off1, pair, poses, syms)
    res["ransac"].update({"iterations_mean": round(float(its.float().mean()), 1), "inliers_mean": round(float(inl.float().mean()), 1)})
    if a.no_tuple:
        r0 = fns["fgr_no_tuple"]()
        res["fgr_no_tuple"] = accuracy(r0.T, x0, off0, x1, off1, pair, poses, syms)
        res["fgr_no_tuple"]["updates_mean"] = round(float(r0.iters.float().mean()), 2)
    print(json.dumps(res))
    path = a.json or os.path.join(ROOT, "profiles", "fgr_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
