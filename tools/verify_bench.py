"""Candidate verification on one chair-shaped registration step: `python tools/verify_bench.py [--json PATH]`.

32 queries of the bench's generator (corsair_amd.synth: CAD c = make_cloud(c, 15000)[:10000], the query its last 10 000
points under random_pose(c), voxelised at 0.03) with the bench's converging-regime features (a voxel's CAD-frame coordinate
zero-padded to 16-d), symmetry labels of the chair histogram's shape (one CAD with label 4, the rest 1), forced gate.  Query q
has K = 5 candidates: CADs q, q + 1, .. q + 4 (mod 32) -- its own CAD first and four others --, registered query-major in
batches of 32 pairs through harness.Pipeline.register, as harness.run_eval does with Config.verify_top_k = 5.

Recorded, medians of --reps repetitions after 2 warm-up rounds, the variants alternating in this process, wall clock around a
device synchronisation (the registration has host stages, so wall clock is the common measure):
  (s)  the scoring: one backend.chamfer_2dir call per batch on the batch's kept poses (5 calls);
  (s1) the stand-in a user writes without it: per batch two backend.chamfer_1dir calls on the default path, the second with
       the roles swapped and the pose inverted in f64 on the host (a download of the poses, so it synchronises);
  (r5) the K = 5 registration step (5 batches of 32 pairs) and (r1) the K = 1 step (the first candidates, one batch).
Also the device time of (s) and (s1) by events, and the largest relative difference of the backward values of the two (the
stand-in rounds the inverted pose to f32; informational).
One bar (DESIGN 10's convention): (s) costs at most 10 % of (r5), both from this run -- `score_over_registration`, `bar_met`.
No other ratio is a target.  Prints one JSON line; without --json it also goes to profiles/verify_bench.json."""
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

N_Q, K, N_POINTS, VOXEL, BATCH = 32, 5, 10000, 0.03, 32


def step_sets(dev):
    """EmbeddedSets of the 32 queries and the 32 CADs with the stand-in features (no descriptors: the candidates are given)."""
    cads = [synth.make_cloud(c, 15000)[:N_POINTS] for c in range(N_Q)]
    poses = [synth.random_pose(c, max_trans=0.0) for c in range(N_Q)]
    queries = [synth.apply_pose(synth.make_cloud(c, 15000)[15000 - N_POINTS:], poses[c], np.float32) for c in range(N_Q)]
    raw_off = (np.arange(N_Q + 1) * N_POINTS).tolist()
    out = []
    for clouds in (queries, cads):
        xyz = torch.from_numpy(np.concatenate(clouds)).to(dev)
        keep, _, off = B.voxelize(xyz, raw_off, VOXEL)
        out += [xyz[keep].contiguous(), [int(o) for o in off]]
    x0, off0, x1, off1 = out
    Ts = np.stack(poses)
    Rm = torch.from_numpy(Ts[:, :3, :3].astype(np.float32)).to(dev)
    t = torch.from_numpy(Ts[:, :3, 3].astype(np.float32)).to(dev)
    seg = torch.repeat_interleave(torch.arange(N_Q, device=dev), torch.as_tensor(np.diff(off0), device=dev),
                                  output_size=x0.shape[0])
    x_cad = torch.einsum("nj,njk->nk", x0 - t[seg], Rm[seg])                 # R^T (x - t): the bench's stand-in
    pad = torch.nn.functional.pad
    none = torch.zeros((N_Q, 0), dtype=torch.float32, device=dev)
    return (H.EmbeddedSet(pad(x_cad, (0, 13)).contiguous(), x0, off0, none),
            H.EmbeddedSet(pad(x1, (0, 13)).contiguous(), x1, off1, none), poses)


def wall_alternating(fns, reps, warmup=2):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4),
                "max_ms": round(float(max(v)), 4)} for k, v in ms.items()}


def device_ms(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return round(float(np.median(out)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    qs, cat, poses = step_sets(dev)
    syms = np.ones(N_Q, np.int32)
    syms[0] = 4
    pipe = H.Pipeline.__new__(H.Pipeline)            # the sets are embedded already: no network
    pipe.cfg, pipe.device, pipe.engine = H.Config(), dev, None
    cand = (np.arange(N_Q)[:, None] + np.arange(K)[None, :]) % N_Q
    q_of = np.repeat(np.arange(N_Q), K)
    c_of = cand.reshape(-1)
    batches = [np.arange(s, s + BATCH) for s in range(0, N_Q * K, BATCH)]
    sets = [(qs.gather(q_of[b]), cat.gather(c_of[b]), syms[c_of[b]], [(2 * int(i), 2 * int(i) + 1) for i in q_of[b]])
            for b in batches]
    first = (qs, cat.gather(cand[:, 0]), syms[cand[:, 0]], [(2 * i, 2 * i + 1) for i in range(N_Q)])

    def register(s):
        return pipe.register(s[0], s[1], s[2], anchor_ids=s[3], force_gate=True)

    kept = [register(s).T_best for s in sets]
    n = list(range(BATCH))

    def score():
        return [B.chamfer_2dir(s[0].origin, s[0].offsets, s[1].origin, s[1].offsets, n, n, T) for s, T in zip(sets, kept)]

    def stand_in():
        out = []
        for s, T in zip(sets, kept):
            fwd = B.chamfer_1dir(s[0].origin, s[0].offsets, s[1].origin, s[1].offsets, n, n, T)
            Ti = torch.from_numpy(np.linalg.inv(T.cpu().numpy().astype(np.float64)).astype(np.float32)).to(dev)
            out.append((fwd, B.chamfer_1dir(s[1].origin, s[1].offsets, s[0].origin, s[0].offsets, n, n, Ti)))
        return out

    fns = {"chamfer_2dir_x5": score, "two_chamfer_1dir_x5": stand_in,
           "register_k5": lambda: [register(s) for s in sets], "register_k1": lambda: register(first)}
    vox = np.diff(qs.offsets)
    res = {"device": torch.cuda.get_device_name(0), "queries": N_Q, "k": K, "pairs": N_Q * K, "batch_pairs": BATCH,
           "voxels_per_cloud": {"min": int(vox.min()), "mean": round(float(vox.mean()), 1), "max": int(vox.max())},
           "reps": a.reps, "wall_ms": wall_alternating(fns, a.reps)}
    w = res["wall_ms"]
    res["device_ms"] = {"chamfer_2dir_x5": device_ms(score, a.reps), "two_chamfer_1dir_x5": device_ms(stand_in, a.reps)}
    res["score_over_registration"] = round(w["chamfer_2dir_x5"]["median_ms"] / w["register_k5"]["median_ms"], 4)
    res["bar"] = 0.10
    res["bar_met"] = bool(res["score_over_registration"] <= 0.10)
    res["stand_in_over_chamfer_2dir"] = round(w["two_chamfer_1dir_x5"]["median_ms"] / w["chamfer_2dir_x5"]["median_ms"], 3)
    res["register_k5_over_k1"] = round(w["register_k5"]["median_ms"] / w["register_k1"]["median_ms"], 3)
    got = torch.cat(score()).cpu().numpy()
    alt = stand_in()
    alt_f = torch.cat([f for f, _ in alt]).cpu().numpy()
    alt_b = torch.cat([b for _, b in alt]).cpu().numpy()
    res["forward_max_rel_diff_vs_chamfer_1dir"] = float(np.max(np.abs(got[:, 0] - alt_f) / alt_f))
    res["backward_max_rel_diff_vs_inverted_f32_pose"] = float(np.max(np.abs(got[:, 1] - alt_b) / alt_b))
    order = H.verify_order(H.verify_scores(got, "symmetric").reshape(N_Q, K))
    res["true_cad_first_share"] = float(np.mean(order[:, 0] == 0))       # (column 0 is the query's own CAD)
    print(json.dumps(res))
    path = a.json or os.path.join(ROOT, "profiles", "verify_bench.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
