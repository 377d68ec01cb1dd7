"""Triplet-batch build vs the training step it feeds: `python tools/triplet_batch.py [--json PATH]`.

The chair training shape: B = 32 triplets of 10 000-point synthetic clouds at voxel 0.03.  Times
TripletSource.batch (device events, median of a few builds) and, on the same batch, one shim ResUNetBN2C +
conv1_max_embedding training step over base, positive and negative (forward, losses.corsair_loss, backward,
SGD).  Reports the pair search's algorithmic bytes (source rows read, candidate target rows probed, pairs and row
offsets written) over its kernel time as a share of HBM peak, and the same batch's pair mining done by a NumPy + SciPy
cKDTree.query_ball_point restatement on 16 threads -- a stand-in for the reference's per-point Open3D loop, which is not
available here.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "shim"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.spatial import cKDTree  # noqa: E402

from corsair_amd import backend as B, losses, synth, training as TR  # noqa: E402
from corsair_amd.model import fc, load_model  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak
N_OBJ, N_BATCH, N_POINTS, VOXEL, RADIUS, SAMPLE = 48, 32, 10000, 0.03, 0.03, 1024


def source(dev):
    clouds = [synth.make_cloud(c, 15000)[:N_POINTS] for c in range(N_OBJ)]
    rng = np.random.default_rng(5)
    a = rng.uniform(0.05, 0.4, (N_OBJ, N_OBJ))
    d = (a + a.T) / 2
    d[d < 0.15] = 0.3
    np.fill_diagonal(d, 0.0)
    for i in range(N_OBJ):
        for j in (i - 1, i + 1):
            d[i, j % N_OBJ] = d[j % N_OBJ, i] = 0.1
    return TR.TripletSource(clouds, d, VOXEL, 0.1, 0.5, device=dev), clouds


def timed(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def candidates(src, tgt, cell):
    """Target rows the 27-cell probe of every source row visits (the search's cell size)."""
    gt = np.floor(tgt / cell).astype(np.int64)
    keys, cnt = np.unique(gt, axis=0, return_counts=True)
    table = {tuple(k): c for k, c in zip(keys.tolist(), cnt.tolist())}
    gs = np.floor(src / cell).astype(np.int64)
    total = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                total += sum(table.get((x + dx, y + dy, z + dz), 0) for x, y, z in gs.tolist())
    return total


def scipy_restatement(clouds, data, seed):
    """Pair mining of the same batch on the host: per triplet a cKDTree radius query (16 threads), row sorting and
    the negative draws."""
    t0 = time.perf_counter()
    n_pairs = 0
    nb = data["base_idx"].shape[0]
    sizes = {k: np.bincount(data[k + "_coords"][:, 0].cpu().numpy(), minlength=nb) for k in ("base", "pos")}
    T = {k: data[k + "_T"].cpu().numpy().astype(np.float64) for k in ("base", "pos")}
    ids = {k: data[k + "_idx"].cpu().numpy() for k in ("base", "pos")}
    rng = np.random.default_rng(seed)
    for b in range(nb):
        kept = {}
        for k in ("base", "pos"):
            pc = clouds[ids[k][b]]
            x = pc.astype(np.float64) @ T[k][b][:3, :3].T + T[k][b][:3, 3]
            _, first = np.unique(np.floor(x / VOXEL).astype(np.int64), axis=0, return_index=True)
            kept[k] = pc[np.sort(first)]
        tree = cKDTree(kept["pos"].astype(np.float64))
        rows = tree.query_ball_point(kept["base"].astype(np.float64), RADIUS, workers=16, return_sorted=True)
        pip = np.array([(i, j) for i, r in enumerate(rows) for j in r], np.int64).reshape(-1, 2)
        n_pairs += len(pip)
        neg = np.floor(rng.random((len(pip), 2)) * np.array([[len(kept["base"]), len(kept["pos"])]])).astype(np.int64)
        dist = np.linalg.norm(kept["base"][neg[:, 0]] - kept["pos"][neg[:, 1]], 2, 1)
        neg = neg[dist > 0.1]
        rng.shuffle(pip)
        rng.shuffle(neg)
    return (time.perf_counter() - t0) * 1e3, n_pairs


def train_step(model, head, opt, data):
    import MinkowskiEngine as ME

    feats, embs = {}, {}
    for k in ("base", "pos", "neg"):
        out, feat = model(ME.SparseTensor(data[k + "_feat"], data[k + "_coords"]))
        feats[k], embs[k] = out.F, head(feat)
    loss, _ = losses.corsair_loss(feats, embs, data)   # PiP, PiN and NiN in the library + descriptor triplet
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    src, clouds = source(dev)
    anchors, seed = list(range(N_BATCH)), 1
    src.batch(anchors, seed, sample=SAMPLE)   # warm-up
    build_ms, data = timed(lambda: src.batch(anchors, seed, sample=SAMPLE), a.reps)
    stats = dict(src.last_stats)

    sd, emb = synth.make_state_dicts(31)
    model = load_model("ResUNetBN2C")(1, 16, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=3).to(dev)
    head = fc.conv1_max_embedding(1024, 512, 256).to(dev)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in emb.items()})
    model.train()
    head.train()
    opt = torch.optim.SGD(list(model.parameters()) + list(head.parameters()), lr=1e-3, momentum=0.9)
    train_step(model, head, opt, data)   # warm-up
    step_ms, _ = timed(lambda: train_step(model, head, opt, data), a.reps)

    # the pair search alone, on the batch's kept canonical clouds (count + fill kernels, one host wait between)
    base_o, pos_o = data["base_origin"], data["pos_origin"]
    nb = len(anchors)
    kept = {}
    for k in ("base", "pos"):
        sizes = np.bincount(data[k + "_coords"][:, 0].cpu().numpy(), minlength=nb)
        T = data[k + "_T"].cpu().numpy().astype(np.float64)
        ids = data[k + "_idx"].cpu().numpy()
        pcs = []
        for b in range(nb):
            pc = clouds[ids[b]]
            x = pc.astype(np.float64) @ T[b][:3, :3].T + T[b][:3, 3]
            _, first = np.unique(np.floor(x / VOXEL).astype(np.int64), axis=0, return_index=True)
            pcs.append(pc[np.sort(first)].astype(np.float64))
        assert [len(p) for p in pcs] == sizes.tolist()
        kept[k] = pcs
    segs = kept["base"] + kept["pos"]
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).tolist()
    xyz = torch.from_numpy(np.concatenate(segs, 0)).to(dev)
    rng_b, rng_p = list(range(nb)), list(range(nb, 2 * nb))
    search_ms, (row_ptr, idx) = timed(lambda: B.radius_pairs(xyz, off, xyz, off, rng_b, rng_p, RADIUS), a.reps)
    rows = off[nb]
    pairs = int(idx.numel())
    cand = sum(candidates(kept["base"][b], kept["pos"][b], RADIUS * (1.0 + 1.0 / 1024.0)) for b in range(nb))
    nbytes = rows * 24 + cand * (24 + 4) + pairs * 4 + (rows + 1) * 8
    res = {"shape": "chair", "B": nb, "points": N_POINTS, "voxel": VOXEL, "device": torch.cuda.get_device_name(dev),
           "hip": torch.version.hip, "build_ms": round(build_ms, 3), "step_ms": round(step_ms, 3),
           "build_over_step": round(build_ms / step_ms, 3), "rounds": stats["rounds"],
           "host_waits_per_round": stats["host_waits"] / stats["rounds"],
           "rows": {k: int(data[k + "_coords"].shape[0]) for k in ("base", "pos", "neg")},
           "pairs": {k: int(data[k + "_pairs"].shape[0]) for k in ("PiP", "PiN", "NiN")},
           "pip_full": pairs, "search_ms": round(search_ms, 3), "search_candidates": int(cand),
           "search_bytes": int(nbytes),
           "search_hbm_frac": round(nbytes / (search_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    if not a.no_scipy:
        ms, n = scipy_restatement(clouds, data, seed)
        res["scipy_stand_in_ms"] = round(ms, 1)
        res["scipy_stand_in_pip_full"] = int(n)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
