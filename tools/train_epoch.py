"""The loss alone and one training epoch at the chair shape: `python tools/train_epoch.py [--json PATH]`.

1. losses.pair_contrastive, forward + backward, on the chair training batch of tools/triplet_batch.py (B = 32 triplets of
   10 000-point clouds at voxel 0.03, 1 024 pairs per list and triplet, features of a real train-mode forward) against
   the equivalent torch expression (gather, norm, hinge, mean over PiP, PiN and NiN), the latter by default (float
   atomics in index_put's backward) and under torch.use_deterministic_algorithms(True).  Median of --reps repetitions
   after warm-up, device events.
2. One epoch over the 48 objects (Trainer.train_epoch's loop, instrumented): triplets per second and the shares of
   batch build / forward / loss / backward / optimizer.
Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from corsair_amd import losses, train as T  # noqa: E402
import triplet_batch as TB  # noqa: E402


def events_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def torch_pair_loss(feats, data, pos_margin=0.1, neg_margin=1.4):
    def d(key, other):
        p = data[key].long()
        return (feats["base"][p[:, 0]] - feats[other][p[:, 1]]).norm(dim=1)

    return (F.relu(d("PiP_pairs", "pos") - pos_margin).square().mean()
            + F.relu(neg_margin - d("PiN_pairs", "pos")).square().mean()
            + F.relu(neg_margin - d("NiN_pairs", "neg")).square().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = T.TrainConfig(batch_size=TB.N_BATCH, sample=TB.SAMPLE, voxel_size=TB.VOXEL, radius=TB.RADIUS, seed=31)
    src, _ = TB.source(dev)
    model, head = T.build_model(cfg, dev)
    tr = T.Trainer(model, head, src, cfg)
    model.train()
    head.train()

    # ---- 1. the loss alone ------------------------------------------------------------------------------------------
    data = src.batch(list(range(TB.N_BATCH)), 1, sample=TB.SAMPLE)
    with torch.no_grad():
        feats, _ = tr._forward(data)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in feats.items()}

    def run(fn):
        def once():
            for v in leaves.values():
                v.grad = None
            fn(leaves, data).backward()
        return once

    res = {"device": torch.cuda.get_device_name(dev), "hip": torch.version.hip, "B": TB.N_BATCH,
           "rows": {k: int(v.shape[0]) for k, v in feats.items()},
           "pairs": {k: int(data[k + "_pairs"].shape[0]) for k in ("PiP", "PiN", "NiN")}}
    res["loss_hip_ms"] = round(events_ms(run(losses.pair_contrastive), a.reps), 4)
    res["loss_torch_default_ms"] = round(events_ms(run(torch_pair_loss), a.reps), 4)
    torch.use_deterministic_algorithms(True)
    try:
        res["loss_torch_deterministic_ms"] = round(events_ms(run(torch_pair_loss), a.reps), 4)
    finally:
        torch.use_deterministic_algorithms(False)
    res["loss_value_hip_vs_torch"] = [float(losses.pair_contrastive(leaves, data).detach()),
                                      float(torch_pair_loss(leaves, data).detach())]

    # ---- 2. one epoch -----------------------------------------------------------------------------------------------
    names = ("build", "forward", "loss", "backward", "optimizer")

    def epoch(e):
        marks, n_trip = [], 0
        for s, anchors in enumerate(T.epoch_batches(len(src), cfg.batch_size, cfg.seed, e)):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            d = src.batch(anchors, T.step_seed(cfg.seed, e, s), radius=cfg.radius, sample=cfg.sample)
            ev[1].record()
            with T._deterministic():
                f, em = tr._forward(d)
                ev[2].record()
                loss, _ = tr._loss(f, em, d)
                ev[3].record()
                tr.opt.zero_grad()
                loss.backward()
                ev[4].record()
                tr.opt.step()
            ev[5].record()
            marks.append(ev)
            n_trip += len(anchors)
        torch.cuda.synchronize()
        ms = np.array([[m[i].elapsed_time(m[i + 1]) for i in range(5)] for m in marks]).sum(0)
        return ms, n_trip

    epoch(0)   # warm-up
    ms, n_trip = epoch(1)
    res["epoch_ms"] = round(float(ms.sum()), 2)
    res["epoch_triplets"] = n_trip
    res["triplets_per_s"] = round(n_trip / (ms.sum() * 1e-3), 1)
    res["epoch_shares"] = {k: round(float(v / ms.sum()), 4) for k, v in zip(names, ms)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
