"""Training batches on the device: radius pairs, pair sampling, the f64 transform and
TripletSource.batch against NumPy restatements (tests/pairs_ref.py), plus one SGD step through the shim."""
import os
import sys

import numpy as np
import pytest
import torch

from corsair_amd import backend as B, synth, training as TR
from tests import pairs_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _t(x, gpu, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu, dtype)


def _check_csr(row_ptr, idx, want):
    rp = row_ptr.cpu().numpy()
    ix = idx.cpu().numpy()
    assert len(rp) == len(want) + 1 and rp[-1] == len(ix)
    for i, w in enumerate(want):
        assert np.array_equal(ix[rp[i]:rp[i + 1]], w), i


def _cloud(c, n, voxel=None):
    pc = synth.make_cloud(c, 15000)[:n]
    if voxel is None:
        return pc
    keep, _ = PR.quantize_first(pc.astype(np.float64), voxel)
    return pc[keep]


@pytest.mark.parametrize("k", [None, 1, 3])
def test_radius_pairs_match_restatement(gpu, k):
    a = _cloud(0, 10000, 0.03)
    a2 = synth.make_cloud(0, 15000)[5000:15000]                       # the same shape resampled: many pairs
    b = _cloud(1, 10000, 0.03)
    dense = synth.make_cloud(2, 15000)[:6000]                         # dense targets: dozens of hits at 0.03 / 0.1
    segs = [a, a2, b, dense, np.zeros((0, 3), np.float32)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).tolist()
    xyz = _t(np.concatenate(segs, 0), gpu)
    for r in (0.03, 0.1):
        # problems: resampled, different clouds, dense self-search (distance-0 self pairs), empty target, empty source
        src_seg, tgt_seg = [0, 0, 3, 2, 4], [1, 2, 3, 4, 0]
        row_ptr, idx = B.radius_pairs(xyz, off, xyz, off, src_seg, tgt_seg, radius=r, k=k)
        want = []
        for s, t in zip(src_seg, tgt_seg):
            want += PR.radius_pairs(segs[s].astype(np.float64), segs[t].astype(np.float64), r, k)
        _check_csr(row_ptr, idx, want)
        if r == 0.1 and k is None:
            counts = np.diff(row_ptr.cpu().numpy())
            assert counts.max() > 32   # rows longer than the private-memory path
        if k is None:   # self pairs of the dense problem come first (distance 0)
            rp = row_ptr.cpu().numpy()
            base = len(a) * 2
            first = idx.cpu().numpy()[rp[base:base + len(dense)]]
            assert np.array_equal(first, np.arange(len(dense)))


def test_radius_pairs_boundary_and_zero_pairs(gpu):
    src = np.array([[0.0, 0.0, 0.0], [5.0, 5.0, 5.0]])
    tgt = np.array([[0.1, 0.0, 0.0], [0.0, 0.0999999, 0.0], [0.0, 0.0, -0.1], [1e6, -1e6, 3.0]])
    row_ptr, idx = B.radius_pairs(_t(src, gpu), [0, 2], _t(tgt, gpu), [0, 4], radius=0.1)
    _check_csr(row_ptr, idx, [np.array([1]), np.array([], np.int64)])   # exactly r is excluded
    row_ptr, idx = B.radius_pairs(_t(src, gpu), [0, 2], _t(tgt + 50.0, gpu), [0, 4], radius=0.1)
    assert row_ptr.cpu().numpy().tolist() == [0, 0, 0] and idx.numel() == 0


def test_radius_pairs_coincident_targets(gpu):
    # 300 targets within 1e-9 of each other: one long row, ordered by (d2, index)
    rng = np.random.default_rng(0)
    tgt = 0.2 + rng.uniform(-1e-9, 1e-9, (300, 3))
    tgt[::7] = tgt[0]
    src = np.array([[0.2, 0.2, 0.2], [0.21, 0.2, 0.2]])
    for k in (None, 5):
        row_ptr, idx = B.radius_pairs(_t(src, gpu), [0, 2], _t(tgt, gpu), [0, 300], radius=0.03, k=k)
        _check_csr(row_ptr, idx, PR.radius_pairs(src, tgt, 0.03, k))


def test_get_matching_indices(gpu):
    from corsair_amd.utils.preprocess import get_matching_indices

    a, b = _cloud(3, 4000, 0.03), _cloud(3, 4000, 0.03) + np.float32(0.01)
    for K in (None, 2):
        got = get_matching_indices(a, b, 0.03, K)
        want = PR.radius_pairs(a.astype(np.float64), b.astype(np.float64), 0.03, K)
        assert got == [(i, int(j)) for i, w in enumerate(want) for j in w]
        assert all(isinstance(i, int) and isinstance(j, int) for i, j in got[:5])


def test_sample_pairs_match_restatement(gpu):
    clouds = [_cloud(c, 10000, 0.03) for c in (4, 4, 5, 6, 6, 7)]
    clouds[1] = _cloud(4, 10000, 0.031)   # a different quantisation of the same shape
    clouds[4] = clouds[4][:50]            # a tiny positive: few pairs
    segs = clouds
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).tolist()
    xyz32 = _t(np.concatenate(segs, 0), gpu, torch.float32)
    base, pos, neg = [0, 3], [1, 4], [2, 5]
    slots, seed, rnd, r, sample = [5, 9], 1234, 2, 0.03, 256
    row_ptr, plan = B.radius_pairs_begin(xyz32.double(), off, xyz32.double(), off, base, pos, r)
    row_base = [0, off[1] - off[0], off[1] - off[0] + off[4] - off[3]]
    bufs = B.sample_pairs(xyz32, off, base, pos, neg, slots, row_base, row_ptr, None, 2, seed, rnd, r, sample)
    total = int(row_ptr[-1])
    tgt_idx = plan.fill(row_ptr, total)
    B.sample_pairs(xyz32, off, base, pos, neg, slots, row_base, row_ptr, tgt_idx, 1, seed, rnd, r, sample, out=bufs)
    pip, pin, nin, counts = [x.cpu().numpy() for x in bufs]
    for p in range(2):
        bs, ps, ns = segs[base[p]], segs[pos[p]], segs[neg[p]]
        rows = PR.radius_pairs(bs, ps, r)
        w_pip, w_pin, w_nin = PR.sample_slot(bs, ps, ns, rows, seed, slots[p], rnd, r, sample)
        n_pos = sum(len(x) for x in rows)
        assert counts[p].tolist() == [n_pos, len(w_pip), len(w_pin), len(w_nin)]
        g_pip = pip[p * sample:p * sample + len(w_pip)]
        g_pin = pin[p * sample:p * sample + len(w_pin)]
        g_nin = nin[p * sample:p * sample + len(w_nin)]
        assert np.array_equal(g_pip, w_pip) and np.array_equal(g_pin, w_pin) and np.array_equal(g_nin, w_nin)
        full = {(i, int(j)) for i, w in enumerate(rows) for j in w}
        assert {tuple(x) for x in g_pip.tolist()} <= full
        assert not ({tuple(x) for x in g_pin.tolist()} & full)
        assert np.all(np.linalg.norm(bs[g_pin[:, 0]] - ps[g_pin[:, 1]], 2, 1) > np.float32(0.1))
        assert np.all(np.linalg.norm(bs[g_nin[:, 0]] - ns[g_nin[:, 1]], 2, 1) > np.float32(0.1))
        assert not np.any((g_nin[:, 0] == 0) & (g_nin[:, 1] == 0))
        assert max(counts[p, 1:]) <= sample
    assert counts[0, 1] == sample and counts[1, 1] < sample   # one slot truncated, one below the cap


def test_transform_f64(gpu):
    pc = synth.make_cloud(8, 15000)[:3000]
    T = np.stack([synth.random_pose(3), synth.random_pose(4)])
    got = B.transform_f64(_t(pc, gpu, torch.float32), [0, 1000, 3000], [1, 0], _t(T, gpu)).cpu().numpy()
    want = np.concatenate([PR.transform(pc[1000:3000], T[0]), PR.transform(pc[:1000], T[1])], 0)
    assert np.array_equal(got, want)


# ---- TripletSource ---------------------------------------------------------------------------------------------
def _source(gpu, n=8, n_points=4000):
    clouds = [synth.make_cloud(c, 15000)[:n_points] for c in range(n)]
    rng = np.random.default_rng(5)
    a = rng.uniform(0.05, 0.4, (n, n))
    d = (a + a.T) / 2
    d[d < 0.15] = 0.3
    np.fill_diagonal(d, 0.0)
    for i in range(n):   # every object similar to its neighbours (filter_data keeps them all)
        for j in (i - 1, i + 1):
            d[i, j % n] = d[j % n, i] = 0.1
    return TR.TripletSource(clouds, d, 0.03, 0.3, 0.5, device=gpu), clouds, d


def test_batch_matches_restatement(gpu):
    src, clouds, d = _source(gpu)
    anchors, seed, sample = [0, 3, 5], 11, 256
    data = src.batch(anchors, seed, sample=sample)
    keys = {f"{k}_{f}" for k in ("base", "pos", "neg") for f in ("coords", "feat", "origin", "T", "idx", "sym")}
    keys |= {"PiP_pairs", "PiN_pairs", "NiN_pairs"}
    assert set(data) == keys
    for k in ("base", "pos", "neg"):
        assert data[k + "_coords"].dtype == torch.int32 and data[k + "_coords"].shape[1] == 4
        assert data[k + "_feat"].dtype == torch.float32 and torch.all(data[k + "_feat"] == 1)
        assert data[k + "_origin"].dtype == torch.float32 and data[k + "_T"].shape == (3, 4, 4)
        assert data[k + "_idx"].dtype == torch.int32 and data[k + "_sym"].tolist() == [1, 1, 1]
    for name in ("PiP", "PiN", "NiN"):
        assert data[name + "_pairs"].dtype == torch.int32 and data[name + "_pairs"].shape[1] == 2
    assert data["base_idx"].tolist() == anchors
    # per-slot rebuild from the dict's own instances and poses (the f32 T of a train batch is the f64 pose cast: redo
    # the draws to get the f64 poses)
    nb = {k: [] for k in ("base", "pos", "neg")}
    kept = {}
    for b, a in enumerate(anchors):
        rnd = src.last_stats["slot_round"][b]
        p, n, poses = TR.draw_slot(src.dist_mat, a, src.pos_n, src.neg_n, seed, b, rnd, True)
        assert [p, n] == [int(data["pos_idx"][b]), int(data["neg_idx"][b])]
        for k, inst, T in zip(("base", "pos", "neg"), (a, p, n), poses):
            assert np.array_equal(data[k + "_T"][b].cpu().numpy(), T.astype(np.float32))
            x64 = PR.transform(clouds[inst], T)
            keep, g = PR.quantize_first(x64, 0.03)
            kept[(b, k)] = (clouds[inst][keep], x64[keep].astype(np.float32), g)
            nb[k].append(len(keep))
    for k in ("base", "pos", "neg"):
        c = data[k + "_coords"].cpu().numpy()
        o = data[k + "_origin"].cpu().numpy()
        off = np.concatenate([[0], np.cumsum(nb[k])])
        for b in range(len(anchors)):
            canon, orig, g = kept[(b, k)]
            assert np.array_equal(c[off[b]:off[b + 1], 1:], g) and np.all(c[off[b]:off[b + 1], 0] == b)
            assert np.array_equal(o[off[b]:off[b + 1]], orig)
    # pairs: restated per slot, then shifted by the rows of the earlier slots
    for name, other in (("PiP", "pos"), ("PiN", "pos"), ("NiN", "neg")):
        got = data[name + "_pairs"].cpu().numpy()
        want = []
        sb = np.concatenate([[0], np.cumsum(nb["base"])])
        so = np.concatenate([[0], np.cumsum(nb[other])])
        for b in range(len(anchors)):
            rnd = src.last_stats["slot_round"][b]
            base, pos, neg = kept[(b, "base")][0], kept[(b, "pos")][0], kept[(b, "neg")][0]
            rows = PR.radius_pairs(base, pos, 0.03)
            lists = PR.sample_slot(base, pos, neg, rows, seed, b, rnd, 0.03, sample)
            li = {"PiP": 0, "PiN": 1, "NiN": 2}[name]
            want.append(lists[li] + np.array([sb[b], so[b]]))
        assert np.array_equal(got, np.concatenate(want, 0).astype(np.int32)), name


def test_batch_eval_mode_uses_transforms(gpu):
    src, clouds, _ = _source(gpu)
    T = np.stack([np.stack([synth.random_pose(10 * b + k, max_trans=0.5) for k in range(3)]) for b in range(2)])
    data = src.batch([1, 2], 3, transforms=T, sample=128)
    assert np.array_equal(data["base_T"].cpu().numpy(), T[:, 0].astype(np.float32))
    assert np.array_equal(data["neg_T"].cpu().numpy(), T[:, 2].astype(np.float32))
    x64 = PR.transform(clouds[1], T[0, 0])
    keep, g = PR.quantize_first(x64, 0.03)
    assert np.array_equal(data["base_coords"].cpu().numpy()[:len(keep), 1:], g)
    assert np.array_equal(data["base_origin"].cpu().numpy()[:len(keep)], x64[keep].astype(np.float32))


def test_batch_deterministic_and_slot_local(gpu):
    src, _, _ = _source(gpu)
    d1 = src.batch([0, 1, 2], 42, sample=128)
    d2 = src.batch([0, 1, 2], 42, sample=128)
    for k in d1:
        assert torch.equal(d1[k], d2[k]), k
    d3 = src.batch([0, 1, 5], 42, sample=128)
    n1 = {k: int((d1[k + "_coords"][:, 0] < 2).sum()) for k in ("base", "pos", "neg")}
    for k in ("base", "pos", "neg"):
        for f in ("coords", "origin"):
            assert torch.equal(d1[f"{k}_{f}"][:n1[k]], d3[f"{k}_{f}"][:n1[k]]), (k, f)
        assert torch.equal(d1[k + "_T"][:2], d3[k + "_T"][:2]) and torch.equal(d1[k + "_idx"][:2], d3[k + "_idx"][:2])
    for name, other in (("PiP", "pos"), ("PiN", "pos"), ("NiN", "neg")):
        a, b = d1[name + "_pairs"], d3[name + "_pairs"]
        m = int(((a[:, 0] < n1["base"]) & (a[:, 1] < n1[other])).sum())
        assert torch.equal(a[:m], b[:m]), name


def _third_neighbours(d):
    """filter_data keeps objects with >= 3 entries <= 0.15: 0.15 itself counts there but is no valid positive (< 0.15)."""
    d[0, 4] = d[4, 0] = d[1, 4] = d[4, 1] = 0.15
    for i, j in ((2, 3), (2, 4), (3, 4)):
        d[i, j] = d[j, i] = 0.1


def test_batch_redraws_slot_without_overlap(gpu):
    base = synth.make_cloud(0, 15000)[:3000]
    far = base + np.float32(10.0)   # the same shape translated out of reach: no pair in the canonical frame
    clouds = [base, far] + [synth.make_cloud(c, 15000)[:3000] for c in (1, 2, 3)]
    d = np.full((5, 5), 0.5)
    np.fill_diagonal(d, 0.0)
    d[0, 1] = d[1, 0] = 0.1
    _third_neighbours(d)
    src = TR.TripletSource(clouds, d, 0.03, 0.4, 0.4, device=gpu)
    assert src.pos_n == 2
    seen_redraw = False
    for seed in range(20):
        data = src.batch([0], seed, sample=64)
        assert int(data["pos_idx"][0]) == 0   # only the anchor itself overlaps
        seen_redraw |= src.last_stats["slot_round"][0] > 0
    assert seen_redraw


def test_batch_without_valid_positive_raises(gpu):
    base = synth.make_cloud(0, 15000)[:3000]
    clouds = [base, base + np.float32(10.0)] + [synth.make_cloud(c, 15000)[:3000] for c in (1, 2, 3)]
    d = np.full((5, 5), 0.5)
    np.fill_diagonal(d, 0.05)
    d[0, 1] = d[1, 0] = 0.0   # the far copy always ranks first, and pos_n = 1 leaves only it
    _third_neighbours(d)
    src = TR.TripletSource(clouds, d, 0.03, 0.2, 0.4, device=gpu)
    assert src.pos_n == 1
    with pytest.raises(ValueError, match=r"anchors \[0\]"):
        src.batch([0], 0, sample=64)


def test_sgd_step_on_batch(gpu):
    import torch.nn.functional as F

    sys.path.insert(0, os.path.join(ROOT, "shim"))
    import MinkowskiEngine as ME
    from corsair_amd.model import fc, load_model

    src, _, _ = _source(gpu, n_points=3000)
    data = src.batch([0, 2], 7, sample=256)
    sd, emb = synth.make_state_dicts(31)
    model = load_model("ResUNetBN2C")(1, 16, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=3).to(gpu)
    head = fc.conv1_max_embedding(1024, 512, 256).to(gpu)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in emb.items()})
    model.train()
    head.train()
    params = list(model.parameters()) + list(head.parameters())
    opt = torch.optim.SGD(params, lr=1e-3)
    outs, embs = {}, {}
    for k in ("base", "pos", "neg"):
        out, feat = model(ME.SparseTensor(data[k + "_feat"], data[k + "_coords"]))
        outs[k], embs[k] = out.F, F.normalize(head(feat), dim=1)
    pip, pin = data["PiP_pairs"].long(), data["PiN_pairs"].long()
    pos_d = (outs["base"][pip[:, 0]] - outs["pos"][pip[:, 1]]).norm(dim=1)
    neg_d = (outs["base"][pin[:, 0]] - outs["pos"][pin[:, 1]]).norm(dim=1)
    loss = pos_d.square().mean() + F.relu(1.4 - neg_d).square().mean()
    loss = loss + F.triplet_margin_loss(embs["base"], embs["pos"], embs["neg"], margin=0.5)
    opt.zero_grad()
    loss.backward()
    for p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    opt.step()
