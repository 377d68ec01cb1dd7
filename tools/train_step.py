"""One training step through the MinkowskiEngine shim, timed: `python tools/train_step.py [--json PATH]`.

ResUNetBN2C + conv1_max_embedding in train mode on two batches -- chair (32 clouds, 10 000 points at 0.03) and stress
(64 clouds, 15 000 points at 0.02) -- forward, backward and an SGD step (median of a few steps, whole-step wall time
with events), then every convolution of the step replayed on its own: forward (cs_conv_fwd), weight gradient
(cs_conv_wgrad) and data gradient (cs_conv_fwd on the reverse map), with wgrad's fraction of the f32 MFMA peak.
FLOP = 2 x pairs x Cin x Cout for all three (the same work).  For a kernel-level breakdown run it under
`rocprofv3 --kernel-trace --stats -d <dir> -o train -- python tools/train_step.py`."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shim"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corsair_amd import autograd as AG, backend as B, synth  # noqa: E402
from corsair_amd.model import fc, load_model  # noqa: E402
from oracle import sparse  # noqa: E402

F32_PEAK_TFLOPS = 157.3   # v_mfma_f32_32x32x2_f32 on MI355X (bench.py)
SHAPES = {"chair": (32, 10000, 0.03), "stress": (64, 15000, 0.02)}


def batch(n_clouds, n_points, voxel, dev):
    grids = [sparse.quantize_cloud(synth.make_cloud(c, 15000)[:n_points], voxel)[1] for c in range(n_clouds)]
    coords = torch.from_numpy(sparse.sparse_collate(grids)).to(dev)
    return coords, torch.ones((coords.shape[0], 1), device=dev)


def events(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def run(shape, dev, steps=5):
    import MinkowskiEngine as ME

    n_clouds, n_points, voxel = SHAPES[shape]
    sd, emb = synth.make_state_dicts(31)
    model = load_model("ResUNetBN2C")(1, 16, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=3).to(dev)
    head = fc.conv1_max_embedding(1024, 512, 256).to(dev)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in emb.items()})
    model.train()
    head.train()
    opt = torch.optim.SGD(list(model.parameters()) + list(head.parameters()), lr=1e-3, momentum=0.9)
    coords, feats = batch(n_clouds, n_points, voxel, dev)
    rng = np.random.default_rng(0)

    # record every convolution of the step (in call order) for the per-layer replay
    layers = []
    apply = AG.ConvFunction.apply

    def recording(x, weight, bias, kmap, rev):
        layers.append((x.detach(), weight.detach(), kmap, rev))
        return apply(x, weight, bias, kmap, rev)

    fwd, bwd, sgd = [], [], []
    try:
        for i in range(steps + 1):
            AG.ConvFunction.apply = recording if i == steps else apply
            x = ME.SparseTensor(feats, coords)   # a fresh manager: the maps are built inside the timed forward
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            out, feat = model(x)
            e = head(feat)
            loss = (out.F * out.F.detach().roll(1, 0)).sum() + e.square().sum()
            ev[1].record()
            opt.zero_grad()
            loss.backward()
            ev[2].record()
            opt.step()
            ev[3].record()
            torch.cuda.synchronize()
            if i:   # the first step warms up
                fwd.append(ev[0].elapsed_time(ev[1]))
                bwd.append(ev[1].elapsed_time(ev[2]))
                sgd.append(ev[2].elapsed_time(ev[3]))
    finally:
        AG.ConvFunction.apply = apply   # restored whatever happens in the steps

    rows = []
    for x, w, kmap, rev in layers:
        cin, cout = w.shape[-2], w.shape[-1]
        n_out = kmap.n_out if kmap is not None else x.shape[0]
        pairs = kmap.num_pairs if kmap is not None else x.shape[0]
        g = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32)).to(dev)
        r = rev() if kmap is not None and not kmap.stride1 else None
        t_f = events(lambda: B.conv_fwd(kmap, x, w), 5)
        t_w = events(lambda: B.conv_wgrad(kmap, x, g), 5)
        t_d = events(lambda: B.conv_dgrad(kmap, r, g, w), 5) if cin > 1 else 0.0   # conv1's input needs no gradient
        flop = 2.0 * pairs * cin * cout
        rows.append({"n_out": n_out, "cin": cin, "cout": cout, "pairs": pairs,
                     "kind": "1x1" if kmap is None else ("stride1" if kmap.stride1 else
                                                         ("transposed" if kmap.transposed else "strided")),
                     "fwd_us": round(t_f * 1e3, 1), "wgrad_us": round(t_w * 1e3, 1), "dgrad_us": round(t_d * 1e3, 1),
                     "wgrad_peak_frac": round(flop / (t_w * 1e-3) / 1e12 / F32_PEAK_TFLOPS, 3),
                     "fwd_peak_frac": round(flop / (t_f * 1e-3) / 1e12 / F32_PEAK_TFLOPS, 3)})
    tot = {k: round(sum(r[k] for r in rows) / 1e3, 3) for k in ("fwd_us", "wgrad_us", "dgrad_us")}
    return {"shape": shape, "device": torch.cuda.get_device_name(dev), "hip": torch.version.hip,
            "rows_s1": int(coords.shape[0]), "forward_ms": round(float(np.median(fwd)), 3),
            "backward_ms": round(float(np.median(bwd)), 3), "sgd_ms": round(float(np.median(sgd)), 3),
            "conv_totals_ms": {"fwd": tot["fwd_us"], "wgrad": tot["wgrad_us"], "dgrad": tot["dgrad_us"]},
            "layers": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the results to this file")
    ap.add_argument("--shapes", default="chair,stress")
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for shape in a.shapes.split(","):
        r = run(shape, dev, a.steps)
        res.append(r)
        print(f"[{shape}] s1 rows {r['rows_s1']}: forward {r['forward_ms']} ms, backward {r['backward_ms']} ms, "
              f"sgd {r['sgd_ms']} ms; conv replay fwd {r['conv_totals_ms']['fwd']} ms, "
              f"wgrad {r['conv_totals_ms']['wgrad']} ms, dgrad {r['conv_totals_ms']['dgrad']} ms "
              f"(wgrad / fwd {r['conv_totals_ms']['wgrad'] / r['conv_totals_ms']['fwd']:.2f}x; "
              f"{r['device']}, HIP {r['hip']})")
        for L in r["layers"]:
            print(f"  {L['kind']:10s} n_out={L['n_out']:7d} {L['cin']:4d}->{L['cout']:4d} pairs={L['pairs']:8d}  "
                  f"fwd {L['fwd_us']:8.1f} us ({L['fwd_peak_frac']:.2f})  wgrad {L['wgrad_us']:8.1f} us "
                  f"({L['wgrad_peak_frac']:.2f} of f32 peak)  dgrad {L['dgrad_us']:8.1f} us")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
