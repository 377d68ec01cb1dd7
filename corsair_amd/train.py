"""Epoch trainer with resume: `python -m corsair_amd.train`.

The reference ships the datasets and a checkpoint format with optimizer / scheduler / epoch entries
(utils/ckpts.py:21-63) but no training loop.  A step here is: TripletSource.batch, three shim
forwards (base, positive, negative), losses.corsair_loss, backward, SGD; the scheduler steps per epoch.  With
hardest_weight > 0 the step also mines FCGF's hardest negatives between the forward and the loss (losses.mine_hardest).

A run is a pure function of (data, seed, hyper-parameters): the anchor order of an epoch comes from a Philox generator
keyed by (seed, epoch), the batch seed of a step is a fixed function of (seed, epoch, step), the validation poses are
drawn once from (seed, "val"), the library's kernels are reproducible and torch runs under
use_deterministic_algorithms(True) inside a step.  Nothing reads NumPy's or torch's global generators.  So a resumed run
equals one that never stopped, bit for bit.
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys
import time
from contextlib import contextmanager
from dataclasses import dataclass

import numpy as np
import torch

from . import losses, training as TR
from .utils import ckpts

TIMING_FIELDS = ("seconds", "triplets_per_s")   # the fields of an epoch record that differ from run to run
PART_KEYS = ("pip", "pin", "nin", "triplet")
HN_PART_KEYS = ("hn_bp", "hn_pb", "hn_bn")       # logged as well when hardest_weight > 0


@dataclass
class TrainConfig:
    voxel_size: float = 0.03
    batch_size: int = 32
    epochs: int = 10                 # epochs run by one call of main (after --resume: that many MORE)
    lr: float = 1e-3
    momentum: float = 0.9
    weight_decay: float = 1e-4
    lr_step: int = 10                # StepLR: epochs per step
    lr_gamma: float = 0.5
    pos_ratio: float = 0.1           # CategoryDataset.py:89-90
    neg_ratio: float = 0.5
    radius: float = 0.03             # positive-pair radius
    sample: int = 1024               # pairs per list and triplet
    pos_margin: float = 0.1          # FCGF's defaults
    neg_margin: float = 1.4
    triplet_margin: float = 0.5
    pair_weights: tuple = (1.0, 1.0, 1.0)   # PiP, PiN, NiN
    triplet_weight: float = 1.0
    seed: int = 31
    val_period: int = 1              # validate every that many epochs (when there is a validation source)
    bn_momentum: float = 0.05
    hardest_weight: float = 0.0      # > 0: mine hardest negatives every step, all three HN terms weighted by it
    exclusion_radius: float = 0.1    # a row within that of the anchor (canonical frame) is no negative


_VAL_TAG = 1 << 62
_EPOCH_TAG = 1 << 63


def _philox(tag, seed):
    key = np.array([int(tag), int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    return np.random.Generator(np.random.Philox(key=key))


def epoch_batches(n, batch_size, seed, epoch):
    """The anchor batches of an epoch: a permutation of range(n) from a Philox generator keyed by (seed, epoch), cut
    into batches; the short last batch is kept."""
    if n < 0 or batch_size < 1 or epoch < 0:
        raise ValueError("epoch_batches: n >= 0, batch_size >= 1, epoch >= 0")
    perm = _philox(_EPOCH_TAG | int(epoch), seed).permutation(n)
    return [perm[i:i + batch_size].tolist() for i in range(0, n, batch_size)]


def step_seed(seed, epoch, step):
    """Batch seed of step `step` of epoch `epoch`: a splitmix64 finaliser of the three, below 2^63."""
    m = 0xFFFFFFFFFFFFFFFF
    x = (int(seed) + 0x9E3779B97F4A7C15 * (((int(epoch) & 0xFFFFFFFF) << 32 | (int(step) & 0xFFFFFFFF)) + 1)) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return (x ^ (x >> 31)) >> 1


def val_poses(n, seed):
    """Fixed validation poses f64 [n, 3, 4, 4] (base, positive, negative of every anchor), drawn once from
    (seed, "val")."""
    rng = _philox(_VAL_TAG, seed)
    return np.stack([np.stack([TR.random_pose(rng) for _ in range(3)]) for _ in range(n)]) if n else np.zeros((0, 3, 4, 4))


@contextmanager
def _deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev)


def _shim():
    try:
        import MinkowskiEngine as ME
    except ImportError:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shim"))
        import MinkowskiEngine as ME
    return ME


def build_model(cfg, device, state_dicts=None):
    """ResUNetBN2C + conv1_max_embedding on the shim.  state_dicts = (network, head) to start from; None = the
    Kaiming-normal initialisation of synth.make_state_dicts keyed by cfg.seed (not torch's global generator)."""
    from . import synth
    from .model import fc, load_model

    _shim()
    model = load_model("ResUNetBN2C")(1, 16, bn_momentum=cfg.bn_momentum, normalize_feature=True, conv1_kernel_size=3,
                                      D=3).to(device)
    head = fc.conv1_max_embedding(1024, 512, 256).to(device)
    sd, emb = state_dicts if state_dicts is not None else synth.make_state_dicts(cfg.seed)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    head.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in emb.items()})
    return model, head


class Trainer:
    def __init__(self, model, head, source, cfg, val_source=None):
        self.model, self.head, self.source, self.cfg, self.val_source = model, head, source, cfg, val_source
        self.ME = _shim()
        params = list(model.parameters()) + list(head.parameters())
        self.opt = torch.optim.SGD(params, lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay)
        self.sched = torch.optim.lr_scheduler.StepLR(self.opt, cfg.lr_step, cfg.lr_gamma)
        self._val_T = None
        self.log = []

    # ---- one batch ------------------------------------------------------------------------------------------------
    def _forward(self, data):
        feats, embs = {}, {}
        for k in ("base", "pos", "neg"):
            out, feat = self.model(self.ME.SparseTensor(data[k + "_feat"], data[k + "_coords"]))
            feats[k], embs[k] = out.F, self.head(feat)
        return feats, embs

    @property
    def mining(self):
        return self.cfg.hardest_weight > 0

    def _part_keys(self):
        return PART_KEYS + (HN_PART_KEYS if self.mining else ())

    def _loss(self, feats, embs, data, hardest=None):
        c = self.cfg
        if hardest is None:
            return losses.corsair_loss(feats, embs, data, c.pos_margin, c.neg_margin, tuple(c.pair_weights),
                                       c.triplet_margin, c.triplet_weight)
        return losses.corsair_loss(feats, embs, data, c.pos_margin, c.neg_margin, tuple(c.pair_weights),
                                   c.triplet_margin, c.triplet_weight, hardest=hardest,
                                   hardest_weights=(c.hardest_weight,) * 3)

    def _batch(self, src, anchors, seed, **kw):
        if self.mining:
            kw["mining"] = True
        return src.batch(anchors, seed, radius=self.cfg.radius, sample=self.cfg.sample, **kw)

    def _mine(self, feats, data):
        return losses.mine_hardest(feats, data, self.cfg.exclusion_radius) if self.mining else None

    def step(self, anchors, seed):
        """One training step on the anchors; returns (loss, parts) as detached device tensors (no host wait)."""
        data = self._batch(self.source, anchors, seed)
        with _deterministic():
            feats, embs = self._forward(data)
            loss, parts = self._loss(feats, embs, data, self._mine(feats, data))
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()
        return loss.detach(), parts

    # ---- epochs ---------------------------------------------------------------------------------------------------
    def train_epoch(self, epoch):
        """One pass over the source's anchors.  Returns the epoch record (without validation figures)."""
        c = self.cfg
        self.model.train()
        self.head.train()
        lr = float(self.opt.param_groups[0]["lr"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, n_trip = [], 0
        for s, anchors in enumerate(epoch_batches(len(self.source), c.batch_size, c.seed, epoch)):
            if len(anchors) < 2:   # the head's BatchNorm1d has no batch statistics of a single descriptor
                continue
            loss, parts = self.step(anchors, step_seed(c.seed, epoch, s))
            rows.append(torch.stack([loss.double()] + [parts[k].double() for k in self._part_keys()]))
            n_trip += len(anchors)
        self.sched.step()
        keys = self._part_keys()
        mean = torch.stack(rows).mean(0).cpu().tolist() if rows else [float("nan")] * (1 + len(keys))   # the epoch's host wait
        dt = time.perf_counter() - t0
        return {"epoch": int(epoch), "steps": len(rows), "loss": mean[0],
                "parts": dict(zip(keys, mean[1:])), "lr": lr,
                "seconds": dt, "triplets_per_s": n_trip / dt if dt > 0 else 0.0}

    def validate(self):
        """The validation source's anchors in order, FIXED poses, eval mode, no grad: mean loss over the batches, mean
        feature distance over PiP and over PiN + NiN, and the share of slots with |e_b - e_p| < |e_b - e_n| on the
        normalised descriptors.  With hardest_weight > 0 the loss includes the mined terms and val_hn_dist is the mean
        feature distance of the mined HN_bp pairs."""
        src, c = self.val_source, self.cfg
        if src is None:
            raise ValueError("validate: the trainer has no validation source")
        n = len(src)
        if self._val_T is None:
            self._val_T = val_poses(n, c.seed)
        was = self.model.training, self.head.training
        self.model.eval()
        self.head.eval()
        # loss, d_pos, n_pos, d_neg, n_neg, correct, d_hn, n_hn
        acc = torch.zeros(8, dtype=torch.float64, device=src.device)
        batches = 0
        with torch.no_grad():
            for s, i0 in enumerate(range(0, n, c.batch_size)):
                anchors = list(range(i0, min(n, i0 + c.batch_size)))
                data = self._batch(src, anchors, step_seed(c.seed, 0xFFFFFFFF, s), transforms=self._val_T[anchors])
                feats, embs = self._forward(data)
                hardest = self._mine(feats, data)
                loss, _ = self._loss(feats, embs, data, hardest)

                def dist(key, other, lists=data):
                    p = lists[key].long()
                    return (feats["base"][p[:, 0]] - feats[other][p[:, 1]]).norm(dim=1).double()

                dp = dist("PiP_pairs", "pos")
                dn = torch.cat([dist("PiN_pairs", "pos"), dist("NiN_pairs", "neg")])
                e = {k: torch.nn.functional.normalize(v, dim=1) for k, v in embs.items()}
                ok = (e["base"] - e["pos"]).norm(dim=1) < (e["base"] - e["neg"]).norm(dim=1)
                dh = dist("HN_bp_pairs", "pos", hardest) if hardest is not None else dp.new_zeros(0)
                acc += torch.stack([loss.double(), dp.sum(), dp.new_tensor(dp.numel()), dn.sum(),
                                    dn.new_tensor(dn.numel()), ok.sum().double(), dh.sum(),
                                    dh.new_tensor(dh.numel())])
                batches += 1
        self.model.train(was[0])
        self.head.train(was[1])
        a = acc.cpu().tolist()
        rec = {"val_loss": a[0] / max(batches, 1), "val_pos_dist": a[1] / max(a[2], 1.0),
               "val_neg_dist": a[3] / max(a[4], 1.0), "val_triplet_acc": a[5] / max(n, 1)}
        if self.mining:
            rec["val_hn_dist"] = a[6] / max(a[7], 1.0)
        return rec

    def fit(self, start_epoch, epochs, out_dir):
        """Epochs start_epoch .. start_epoch + epochs - 1.  After every epoch: epoch_%03d.pth and last.pth
        (utils/ckpts.py format) in out_dir, one JSON line on stdout and in out_dir/log.jsonl.  Returns the records."""
        os.makedirs(out_dir, exist_ok=True)
        recs = []
        for epoch in range(int(start_epoch), int(start_epoch) + int(epochs)):
            rec = self.train_epoch(epoch)
            if self.val_source is not None and self.cfg.val_period > 0 and (epoch + 1) % self.cfg.val_period == 0:
                rec.update(self.validate())
            for name in ("epoch_%03d.pth" % epoch, "last.pth"):
                ckpts.save_checkpoint(self.model, self.head, self.opt, self.sched, epoch, out_dir, name,
                                      config=dataclasses.asdict(self.cfg))
            line = json.dumps(rec)
            print(line, flush=True)
            with open(os.path.join(out_dir, "log.jsonl"), "a") as f:
                f.write(line + "\n")
            recs.append(rec)
        self.log += recs
        return recs

    def resume(self, path):
        """Network, head, optimizer (momentum buffers included) and scheduler of a checkpoint fit wrote; returns the
        epoch to continue at."""
        _, _, _, epoch = ckpts.load_checkpoint(self.model, self.head, self.opt, self.sched, path)
        return int(epoch) + 1


# ---- command line ---------------------------------------------------------------------------------------------------
def build_parser():
    import argparse

    d = TrainConfig()
    ap = argparse.ArgumentParser(
        prog="python -m corsair_amd.train",
        description="Metric-learning training of ResUNetBN2C + the descriptor head on the MI355X path from directories of "
                    ".npy clouds; writes checkpoints that `python -m corsair_amd.harness --checkpoint` loads.")
    ap.add_argument("--clouds-dir", required=True, help="training clouds, one [n,3] .npy each (sorted by name = object index)")
    ap.add_argument("--dist-mat", help=".npy f64 [n,n] pairwise Chamfer of the training clouds; default: computed from the "
                                       "first 2000 points of every cloud (utils/pc_dist.py) and saved as OUT/dist_mat.npy")
    ap.add_argument("--sym-labels", help="`<path> <label>` per line; default 1")
    ap.add_argument("--val-clouds-dir", help="validation clouds (default: no validation)")
    ap.add_argument("--val-dist-mat", help="as --dist-mat for the validation clouds (default: OUT/val_dist_mat.npy)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--init", metavar="CKPT", help="start from the weights of a checkpoint (network and head only)")
    g.add_argument("--resume", metavar="CKPT", help="continue a run: weights, optimizer, scheduler and epoch")
    ap.add_argument("--out", required=True, metavar="DIR", help="checkpoints, log.jsonl and computed distance matrices")
    ap.add_argument("--n-points", type=int, default=10000)
    ap.add_argument("--device", default="cuda", choices=["cuda"], help="there is no CPU path")
    for f in dataclasses.fields(TrainConfig):
        flag = "--" + f.name.replace("_", "-")
        v = getattr(d, f.name)
        if isinstance(v, tuple):
            ap.add_argument(flag, type=float, nargs=len(v), default=v)
        else:
            ap.add_argument(flag, type=type(v), default=v)
    return ap


def config_from_checkpoint(path):
    """The TrainConfig a checkpoint of fit was written with (None when the file stores none)."""
    d = ckpts.load_config(path)
    if d is None:
        return None
    names = {f.name for f in dataclasses.fields(TrainConfig)}
    kw = {k: tuple(v) if isinstance(v, list) else v for k, v in d.items() if k in names}
    return TrainConfig(**kw)


def config_from_args(a):
    kw = {f.name: getattr(a, f.name) for f in dataclasses.fields(TrainConfig)}
    kw["pair_weights"] = tuple(float(w) for w in kw["pair_weights"])
    return TrainConfig(**kw)


def _source_from_dir(path, dist_path, save_path, sym_path, cfg, a, what):
    from . import harness
    from .utils import pc_dist

    names, clouds = harness.load_cloud_dir(path, a.n_points, what)
    if dist_path:
        d = np.array(np.load(dist_path), np.float64)
    else:
        d = pc_dist.compute_dist([c[:2000] for c in clouds])
        np.save(save_path, d)
    np.fill_diagonal(d, 0.0)                                     # datasets/ScannetDataset.py:65-66
    if d.shape != (len(clouds), len(clouds)):
        raise SystemExit(f"{what}: distance matrix {d.shape} for {len(clouds)} clouds")
    sym = harness.read_sym_labels(sym_path, names) if sym_path else None
    clouds = [np.asarray(c, np.float32) for c in clouds]
    return TR.TripletSource(clouds, d, cfg.voxel_size, cfg.pos_ratio, cfg.neg_ratio, sym=sym, device=a.device)


def main(argv=None):
    """Returns the epoch records (and prints one JSON line per epoch)."""
    a = build_parser().parse_args(argv)
    cfg = config_from_args(a)
    os.makedirs(a.out, exist_ok=True)
    src = _source_from_dir(a.clouds_dir, a.dist_mat, os.path.join(a.out, "dist_mat.npy"), a.sym_labels, cfg, a, "clouds")
    val = None
    if a.val_clouds_dir:
        val = _source_from_dir(a.val_clouds_dir, a.val_dist_mat, os.path.join(a.out, "val_dist_mat.npy"), None, cfg, a,
                               "validation clouds")
    init = ckpts.load_state_dicts(a.init) if a.init else None
    if init is not None and init[1] is None:
        raise SystemExit("--init: the checkpoint has no embedding_state_dict")
    model, head = build_model(cfg, torch.device(a.device), init)
    tr = Trainer(model, head, src, cfg, val)
    start = tr.resume(a.resume) if a.resume else 0
    return tr.fit(start, cfg.epochs, a.out)


if __name__ == "__main__":
    main()
