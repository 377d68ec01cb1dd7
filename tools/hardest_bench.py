"""Hardest-negative mining at the chair training shape: `python tools/hardest_bench.py [--json PATH]`.

The chair training batch of tools/triplet_batch.py (B = 32 triplets of 10 000-point synthetic clouds at voxel 0.03,
1 024 pairs per list and triplet, features of a real train-mode forward).  Median of --reps repetitions after warm-up,
device events (wall time of the call next to it):
 (a) losses.mine_hardest alone (three cs_hardest_negatives calls, the compaction and its one host wait), and the
     library's own kernel time of the three calls (profile family "hardneg");
 (b) a torch stand-in on the same GPU and batch, per slot: torch.cdist in f64 on the features, spatial cdist, mask,
     argmin -- what a user would otherwise write;
 (c) the whole training step with hardest_weight 0 and 1.
Also the shares of anchors the voucher sent to the exhaustive kernel (CS_HARDNEG_STATS=1, a run of its own).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import _lib, backend as B, losses, train as T  # noqa: E402
import triplet_batch as TB  # noqa: E402


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


def torch_mine(feats, data, radius):
    """The stand-in: per slot and list, f64 distance matrices, mask, argmin; the same three lists."""
    pip = data["PiP_pairs"].long()
    off = {k: data[k + "_off"].tolist() for k in ("base", "pos", "neg")}
    out = {"HN_bp_pairs": [], "HN_pb_pairs": [], "HN_bn_pairs": []}
    for key, q, t, col, r in (("HN_bp_pairs", "base", "pos", 0, radius), ("HN_pb_pairs", "pos", "base", 1, radius),
                              ("HN_bn_pairs", "base", "neg", 0, 0.0)):
        a_all = pip[:, col]
        for s in range(len(off[q]) - 1):
            a = a_all[(a_all >= off[q][s]) & (a_all < off[q][s + 1])]
            d = torch.cdist(feats[q][a].double(), feats[t][off[t][s]:off[t][s + 1]].double())
            if r > 0:
                sp = torch.cdist(data[q + "_canon"][a].double(), data[t + "_canon"][off[t][s]:off[t][s + 1]].double())
                d = d.masked_fill(sp < r, float("inf"))
            best = d.argmin(1)
            ok = torch.isfinite(d[torch.arange(len(a), device=d.device), best])
            pair = torch.stack([a, best + off[t][s]], 1)[ok]
            out[key].append(pair if col == 0 else pair.flip(1))
    return {k: torch.cat(v).int() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(batch_size=TB.N_BATCH, sample=TB.SAMPLE, voxel_size=TB.VOXEL, radius=TB.RADIUS, seed=31)
    cfg = T.TrainConfig(**kw)
    src, _ = TB.source(dev)
    model, head = T.build_model(cfg, dev)
    tr = T.Trainer(model, head, src, cfg)
    model.train()
    head.train()
    anchors = list(range(TB.N_BATCH))
    data = src.batch(anchors, 1, sample=TB.SAMPLE, mining=True)
    with torch.no_grad():
        feats, _ = tr._forward(data)
    feats = {k: v.detach() for k, v in feats.items()}
    radius = cfg.exclusion_radius
    res = {"device": torch.cuda.get_device_name(dev), "hip": torch.version.hip, "B": TB.N_BATCH,
           "rows": {k: int(v.shape[0]) for k, v in feats.items()}, "anchors": int(data["PiP_pairs"].shape[0]),
           "exclusion_radius": radius}

    # ---- (a) mine_hardest, (b) the torch stand-in -------------------------------------------------------------------
    res["mine_hip_ms"], res["mine_hip_wall_ms"] = timed(lambda: losses.mine_hardest(feats, data, radius), a.reps)
    res["mine_torch_ms"], res["mine_torch_wall_ms"] = timed(lambda: torch_mine(feats, data, radius), a.reps)
    res["torch_over_hip"] = round(res["mine_torch_ms"] / res["mine_hip_ms"], 2)
    got, want = losses.mine_hardest(feats, data, radius), torch_mine(feats, data, radius)
    res["lists_equal_torch"] = {k: bool(got[k].shape == want[k].shape and (got[k] == want[k]).float().mean() > 0.999)
                                for k in got}
    res["mined_pairs"] = {k: int(v.shape[0]) for k, v in got.items()}
    _lib.prof_enable(True)
    _lib.prof_reset()
    for _ in range(a.reps):
        losses.mine_hardest(feats, data, radius)
    torch.cuda.synchronize()
    ms, n, flop = _lib.prof_get("hardneg")
    _lib.prof_enable(False)
    res["hardneg_kernel_ms_per_mine"] = round(ms / a.reps, 4)
    res["hardneg_launch_groups_per_mine"] = n // a.reps
    res["hardneg_gflop_per_mine"] = round(flop / a.reps * 1e-9, 2)
    os.environ["CS_HARDNEG_STATS"] = "1"
    B.hardest_stats(reset=True)
    losses.mine_hardest(feats, data, radius)
    st = B.hardest_stats(reset=True)
    del os.environ["CS_HARDNEG_STATS"]
    res["fallback_share_step"] = round(st[1] / max(st[0], 1), 5)

    # ---- (c) the whole step -----------------------------------------------------------------------------------------
    for w in (0.0, 1.0):
        cfg_w = T.TrainConfig(hardest_weight=w, **kw)
        m, h = T.build_model(cfg_w, dev)
        t = T.Trainer(m, h, src, cfg_w)
        m.train()
        h.train()
        step = [0]

        def one():
            t.step(anchors, T.step_seed(cfg_w.seed, 0, step[0]))
            step[0] += 1

        res["step_ms_w%d" % int(w)], res["step_wall_ms_w%d" % int(w)] = timed(one, a.reps)
    res["step_w1_over_w0"] = round(res["step_ms_w1"] / res["step_ms_w0"], 4)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
