"""Training triplet batches on the device: the counterpart of datasets/CategoryDataset.py:121-296 and the
collate of datasets/ChairDataset.py:130-237.

Per triplet the reference draws a positive and a negative instance from a Chamfer-distance matrix, poses and quantises
the three clouds, mines positive pairs with an Open3D radius query per point and random negative pairs, and redraws the
whole triplet when there are too few positive pairs; the collate then concatenates the samples.  Here the instance and
pose draws stay on the host (a few NumPy draws per slot), everything per point runs in the library for the whole batch at
once: cs_transform_f64, cs_voxelize_f64, cs_radius_pairs and cs_sample_pairs.  A round costs two host waits (the
quantiser's kept-row offsets and the pair counts); slots with too few positive pairs are redrawn in the next round.

Deliberate differences: filter_data returns its inputs when nothing is removed (the reference raises
UnboundLocalError there); randomness comes from generators keyed by (seed, slot, round) instead of NumPy's global state,
so a slot's triplet depends only on (seed, slot, anchor) and the source.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import backend as B
from .synth import euler2mat

MAX_ROUNDS = 16
POS_THRES = 0.15   # CategoryDataset.py:159 (and filter_data's default)
NEG_THRES = 0.2    # CategoryDataset.py:172


def filter_data(dist_mat_ref, pcs_ref, sym_ref=None, thres=0.15, num=3):
    """Drop, until nothing changes, the objects with fewer than `num` entries <= thres in their distance row
    (CategoryDataset.py:92-119).  Returns (dist_mat, pcs, sym, kept original indices)."""
    dist_mat = np.asarray(dist_mat_ref)
    pcs = list(pcs_ref)
    sym = None if sym_ref is None else list(sym_ref)
    kept = np.arange(len(dist_mat))
    while True:
        z = (dist_mat <= thres).sum(1)
        mask = (z >= num).nonzero()[0]
        if len(mask) == len(dist_mat):
            return dist_mat, pcs, sym, kept
        dist_mat = dist_mat[mask, :][:, mask].copy()
        pcs = [pcs[i] for i in mask]
        if sym is not None:
            sym = [sym[i] for i in mask]
        kept = kept[mask]


def rank_probabilities(topn):
    """The rank weights of CategoryDataset.py:161-162,174-175: rank q (0-based) has probability 2 (topn - q) /
    ((1 + topn) topn)."""
    prob = 2 * (np.arange(topn) + 1) / ((1 + topn) * topn)
    return np.flip(prob)


def positive_instance(dist_mat, idx, pos_n, rng):
    """generate_positive_inst (CategoryDataset.py:153-164).  As in the reference the ranking includes the anchor
    itself (distance 0 sorts first), so the anchor is its own most likely positive."""
    row = dist_mat[idx, :]
    dist_rank = np.argsort(row)
    valid = (row < POS_THRES).nonzero()[0]
    topn = max(min(pos_n, len(valid)), 1)
    return int(dist_rank[rng.choice(np.arange(topn), p=rank_probabilities(topn))])


def negative_instance(dist_mat, idx, neg_n, rng):
    """generate_negative_inst (CategoryDataset.py:166-177).  As in the reference the choice skips rank 0, the
    farthest object: ranks 1..topn are drawn."""
    row = dist_mat[idx, :]
    dist_rank = np.argsort(-row)
    valid = (row > NEG_THRES).nonzero()[0]
    topn = max(min(neg_n, len(valid) - 1), 1)
    return int(dist_rank[rng.choice(np.arange(topn), p=rank_probabilities(topn)) + 1])


def slot_rng(seed, slot, round_):
    """The host generator of one (seed, slot, round): Philox keyed by all three."""
    key = np.array([(int(slot) << 8) | int(round_), int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    return np.random.Generator(np.random.Philox(key=key))


def random_pose(rng):
    """random_rotation's pose (utils/preprocess.py:73-86): Euler angles U(0, 2 pi)^3 through euler2mat ('sxyz'),
    translation U(-0.5, 0.5)^3."""
    a = rng.uniform(0, 2 * np.pi, 3)
    T = np.eye(4)
    T[:3, :3] = euler2mat(a[0], a[1], a[2])
    T[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    return T


def draw_slot(dist_mat, anchor, pos_n, neg_n, seed, slot, round_, train):
    """Host draws of one slot in one round: (positive, negative, poses [3,4,4] or None)."""
    rng = slot_rng(seed, slot, round_)
    p = positive_instance(dist_mat, anchor, pos_n, rng)
    n = negative_instance(dist_mat, anchor, neg_n, rng)
    poses = np.stack([random_pose(rng) for _ in range(3)]) if train else None
    return p, n, poses


def _ranges(starts, lens, dev):
    """Device int64 index of the concatenated ranges [starts[i], starts[i] + lens[i])."""
    starts = np.asarray(starts, np.int64)
    lens = np.asarray(lens, np.int64)
    total = int(lens.sum())
    excl = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    delta = torch.from_numpy(starts - excl).to(dev)
    return torch.arange(total, device=dev) + torch.repeat_interleave(delta, torch.from_numpy(lens).to(dev),
                                                                     output_size=total)


class TripletSource:
    """The canonical clouds of a training split, resident on the device as one offset table (like
    harness.EmbeddedSet), with the reference dataset's instance statistics.

    clouds: list of f32 [n_i,3] arrays (already normalised, utils/preprocess.py:32-36); dist_mat: [n,n] Chamfer
    distances; sym: optional symmetry labels (1 for every object when None, CategoryDataset.py:199-206)."""

    def __init__(self, clouds, dist_mat, voxel_size, pos_ratio, neg_ratio, sym=None, device="cuda"):
        self.dist_mat, clouds, sym, self.kept = filter_data(np.asarray(dist_mat, np.float64), clouds, sym)
        self.voxel_size = float(voxel_size)
        self.device = torch.device(device)
        n = len(clouds)
        self.pos_n = int(n * pos_ratio)   # CategoryDataset.py:89-90
        self.neg_n = int(n * neg_ratio)
        self.sym = np.ones(n, np.int32) if sym is None else np.asarray(sym, np.int32)
        lens = [len(c) for c in clouds]
        self.offsets = [0] + np.cumsum(lens).tolist()
        xyz = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds], 0) if n else np.zeros((0, 3))
        self.xyz = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(self.device)
        self.last_stats = {}

    def __len__(self):
        return len(self.offsets) - 1

    def _round(self, slots, ids, poses, seed, rnd, radius, sample):
        """One round for the slots `slots` (instances ids [3, P]: base, positive, negative; poses [3, P, 4, 4])."""
        dev = self.device
        P = len(slots)
        seg = np.concatenate(ids).astype(np.int64)            # base 0..P-1, positive P..2P-1, negative 2P..3P-1
        Ts = np.concatenate(poses, 0).astype(np.float64)      # [3P, 4, 4]
        off = np.asarray(self.offsets, np.int64)
        lens = off[seg + 1] - off[seg]
        in_off = np.concatenate([[0], np.cumsum(lens)]).tolist()
        x64 = B.transform_f64(self.xyz, self.offsets, seg.tolist(), torch.from_numpy(Ts).to(dev))
        keep, grid, out_off = B.voxelize(x64, in_off, self.voxel_size)   # host wait 1
        # catalog row of every kept point: the transformed rows are the segments seg, concatenated
        delta = torch.from_numpy(off[seg] - np.asarray(in_off[:-1], np.int64)).to(dev)
        rows = keep + torch.repeat_interleave(delta, torch.from_numpy(lens).to(dev), output_size=int(in_off[-1]))[keep]
        canon = self.xyz[rows]
        origin = x64[keep].float()
        canon64 = canon.double()
        base_seg, pos_seg, neg_seg = list(range(P)), list(range(P, 2 * P)), list(range(2 * P, 3 * P))
        row_base = out_off[:P + 1]
        row_ptr, plan = B.radius_pairs_begin(canon64, out_off, canon64, out_off, base_seg, pos_seg, radius)
        bufs = B.sample_pairs(canon, out_off, base_seg, pos_seg, neg_seg, list(slots), row_base, row_ptr, None, 2,
                              seed, rnd, radius, sample)
        rb = torch.from_numpy(np.asarray(row_base, np.int64)).to(dev)
        h_ptr, h_counts = _lib.to_host(row_ptr[rb], bufs[3])             # host wait 2
        n_pos = np.diff(h_ptr)
        n0 = np.diff(out_off)[:P]
        n1 = np.diff(out_off)[P:2 * P]
        ok = ~(n_pos < 0.1 * np.minimum(n0, n1))                         # CategoryDataset.py:128-129
        tgt_idx = plan.fill(row_ptr, int(h_ptr[-1]))
        B.sample_pairs(canon, out_off, base_seg, pos_seg, neg_seg, list(slots), row_base, row_ptr, tgt_idx, 1, seed,
                       rnd, radius, sample, out=bufs)
        counts = np.stack([np.minimum(n_pos, sample), h_counts[:, 2], h_counts[:, 3]], 1)
        return {"ok": ok, "grid": grid, "origin": origin, "canon": canon, "out_off": np.asarray(out_off, np.int64), "pairs": bufs[:3],
                "counts": counts, "n_pos": n_pos}

    def batch(self, anchors, seed, transforms=None, radius=0.03, sample=1024, mining=False):
        """One training batch with collate_pair_fn's keys (datasets/ChairDataset.py:130-237), all on the device.

        anchors: object indices (after filter_data); transforms None = train mode (random poses), else f64/f32
        [B, 3, 4, 4] fixed poses (fix_trans[index] layout: base, positive, negative) used verbatim.

        mining=True adds what losses.mine_hardest needs: base_canon / pos_canon / neg_canon (f32 [n, 3] device: the
        kept CANONICAL points, rows as *_coords) and base_off / pos_off / neg_off (host int64 [B + 1]: the row offsets
        of the slots); every other entry is the same, and no host wait is added."""
        anchors = [int(a) for a in anchors]
        nb = len(anchors)
        if nb == 0:
            raise ValueError("TripletSource.batch: no anchors")
        if any(a < 0 or a >= len(self) for a in anchors):
            raise ValueError("TripletSource.batch: anchor out of range")
        train = transforms is None
        if not train:
            transforms = np.asarray(transforms, np.float64)
            if transforms.shape != (nb, 3, 4, 4):
                raise ValueError("transforms must be [B, 3, 4, 4]")
        dev = self.device
        done = {}            # slot -> (round result index, problem index, instances, poses)
        results = []
        pending = list(range(nb))
        waits = 0
        for rnd in range(MAX_ROUNDS):
            if not pending:
                break
            ids = np.zeros((3, len(pending)), np.int64)
            poses = np.zeros((3, len(pending), 4, 4))
            for q, b in enumerate(pending):   # host draws: a few NumPy calls per slot
                p, n, T = draw_slot(self.dist_mat, anchors[b], self.pos_n, self.neg_n, seed, b, rnd, train)
                ids[:, q] = (anchors[b], p, n)
                poses[:, q] = T if train else transforms[b]
            res = self._round(pending, ids, poses, seed, rnd, radius, sample)
            waits += 2
            results.append(res)
            for q, b in enumerate(pending):
                if res["ok"][q]:
                    done[b] = (len(results) - 1, q, ids[:, q], poses[:, q])
            pending = [b for b in pending if b not in done]
        if pending:
            raise ValueError(f"no triplet with enough positive pairs after {MAX_ROUNDS} rounds for anchors "
                             f"{[anchors[b] for b in pending]}")
        self.last_stats = {"rounds": len(results), "host_waits": waits,
                           "slot_round": [done[b][0] for b in range(nb)]}
        return self._assemble(results, done, nb, sample, mining)

    def _assemble(self, results, done, nb, sample, mining=False):
        dev = self.device
        row_off = np.concatenate([[0], np.cumsum([r["out_off"][-1] for r in results])]).astype(np.int64)
        grid = torch.cat([r["grid"] for r in results], 0)
        origin = torch.cat([r["origin"] for r in results], 0)
        canon = torch.cat([r["canon"] for r in results], 0) if mining else None
        pair_off = np.concatenate([[0], np.cumsum([r["pairs"][0].shape[0] for r in results])]).astype(np.int64)
        rr = np.array([done[b][0] for b in range(nb)])
        qq = np.array([done[b][1] for b in range(nb)])
        npb = np.array([(len(results[r]["out_off"]) - 1) // 3 for r in rr])   # problems of that round
        data = {}
        sizes = {}
        for k, name in enumerate(("base", "pos", "neg")):
            seg = k * npb + qq
            starts = np.array([row_off[r] + results[r]["out_off"][s] for r, s in zip(rr, seg)], np.int64)
            lens = np.array([results[r]["out_off"][s + 1] - results[r]["out_off"][s] for r, s in zip(rr, seg)],
                            np.int64)
            sizes[name] = lens
            idx = _ranges(starts, lens, dev)
            c = grid[idx]
            c[:, 0] = torch.repeat_interleave(torch.arange(nb, dtype=torch.int32, device=dev),
                                              torch.from_numpy(lens).to(dev), output_size=int(lens.sum()))
            data[name + "_coords"] = c
            data[name + "_feat"] = torch.ones((c.shape[0], 1), dtype=torch.float32, device=dev)
            data[name + "_origin"] = origin[idx]
            if mining:
                data[name + "_canon"] = canon[idx]
            data[name + "_T"] = torch.from_numpy(np.stack([done[b][3][k] for b in range(nb)]).astype(np.float32)).to(dev)
            data[name + "_idx"] = torch.from_numpy(
                np.array([done[b][2][k] for b in range(nb)], np.int32)).to(dev)
            data[name + "_sym"] = torch.from_numpy(self.sym[[int(done[b][2][k]) for b in range(nb)]].astype(np.int32)).to(dev)
        if mining:
            for name in sizes:
                data[name + "_off"] = np.concatenate([[0], np.cumsum(sizes[name])]).astype(np.int64)
        for li, (name, other) in enumerate((("PiP", "pos"), ("PiN", "pos"), ("NiN", "neg"))):
            buf = torch.cat([r["pairs"][li] for r in results], 0)
            cnt = np.array([results[r]["counts"][q, li] for r, q in zip(rr, qq)], np.int64)
            starts = pair_off[rr] + qq * sample
            idx = _ranges(starts, cnt, dev)
            shift = np.stack([np.concatenate([[0], np.cumsum(sizes["base"])[:-1]]),
                              np.concatenate([[0], np.cumsum(sizes[other])[:-1]])], 1).astype(np.int32)
            sh = torch.repeat_interleave(torch.from_numpy(shift).to(dev), torch.from_numpy(cnt).to(dev), dim=0,
                                         output_size=int(cnt.sum()))
            data[name + "_pairs"] = buf[idx] + sh
        return data
