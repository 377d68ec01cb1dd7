"""Training losses.  The reference ships datasets that mine PiP / PiN / NiN pair lists and no loss
(SURVEY 1); this is the FCGF-form contrastive loss those lists were mined for plus the triplet loss on the global
descriptors.

pair_contrastive runs in the library (cs_pair_loss_fwd / cs_pair_loss_bwd): value and feature gradients are integer
sums of fixed-point terms, bit-identical from run to run and independent of the order of the pairs.  embedding_triplet
is plain torch on 3 x B x 256 values (dense reductions only: deterministic as it is).

mine_hardest adds FCGF's hardest negatives: for every PiP pair the feature-nearest row of the other cloud that is not a
true correspondence (cs_hardest_negatives), as three more PUSH lists of the same cs_pair_loss_* call.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from . import backend as B
from .autograd import PairLossFunction

# (pair list, feature matrix of column 0, of column 1, kind): TripletSource.batch's lists, rows batch-global
PAIR_TERMS = (("PiP_pairs", "base", "pos", B.PAIR_PULL),
              ("PiN_pairs", "base", "pos", B.PAIR_PUSH),
              ("NiN_pairs", "base", "neg", B.PAIR_PUSH))


# (mined list, feature matrix of column 0, of column 1): mine_hardest's lists, all PUSH with neg_margin
HARDEST_TERMS = (("HN_bp_pairs", "base", "pos"), ("HN_pb_pairs", "base", "pos"), ("HN_bn_pairs", "base", "neg"))


def mine_hardest(feats, data, exclusion_radius=0.1):
    """The hardest negatives of every PiP pair of a batch made with TripletSource.batch(mining=True), on detached
    features under no_grad.  Returns {"HN_bp_pairs", "HN_pb_pairs", "HN_bn_pairs"}: int32 [n, 2] device, rows
    batch-global like the PiP / PiN / NiN lists:
      HN_bp: (the pair's base row, the feature-nearest row of the slot's positive cloud that is not within
             exclusion_radius of the base point in the canonical frame);
      HN_pb: (the feature-nearest such base row, the pair's positive row) -- the search runs positive -> base;
      HN_bn: (the pair's base row, the feature-nearest row of the slot's negative cloud) -- radius 0, every row counts.
    Anchors without an admissible row (-1) are dropped: the three lists' lengths are read in ONE download, the step's
    one extra host wait (the slot of an anchor and the slots' row offsets come from the batch column of *_coords on the
    device: nothing is uploaded)."""
    with torch.no_grad():
        f = {k: feats[k].detach() for k in ("base", "pos", "neg")}
        pip = data["PiP_pairs"]
        dev = pip.device
        bcol = {k: data[k + "_coords"][:, 0].contiguous() for k in ("base", "pos", "neg")}   # sorted: rows grouped by slot
        slots = torch.arange(len(data["base_off"]), dtype=bcol["base"].dtype, device=dev)
        off = {k: torch.searchsorted(bcol[k], slots) for k in bcol}                          # = *_off, on the device
        a_base, a_pos = pip[:, 0].contiguous(), pip[:, 1].contiguous()

        def search(q, t, anchors, radius):
            idx = B.hardest_negatives(f[q], data[q + "_canon"], data[q + "_off"], f[t], data[t + "_canon"],
                                      data[t + "_off"], anchors, radius)
            slot = bcol[q][anchors.long()].long()
            return idx, (idx.long() + off[t][slot]).int()

        i_bp, g_bp = search("base", "pos", a_base, exclusion_radius)
        i_pb, g_pb = search("pos", "base", a_pos, exclusion_radius)
        i_bn, g_bn = search("base", "neg", a_base, 0.0)
        keep = torch.stack([i_bp, i_pb, i_bn]) >= 0
        counts = _lib.to_host(keep.sum(1))[0]                             # the host wait
        lists = (torch.stack([a_base, g_bp], 1), torch.stack([g_pb, a_pos], 1), torch.stack([a_base, g_bn], 1))
        out = {}
        for l, (key, _, _) in enumerate(HARDEST_TERMS):
            # the kept pairs in list order: a stable sort of the drop flags, cut at the count (no second wait)
            order = torch.argsort((~keep[l]).to(torch.int8), stable=True)[:int(counts[l])]
            out[key] = lists[l][order].contiguous()
        return out


def pair_contrastive(feats, data, pos_margin=0.1, neg_margin=1.4, weights=(1, 1, 1), return_parts=False, hardest=None,
                     hardest_weights=(1, 1, 1)):
    """w0 mean_PiP max(d - pos_margin, 0)^2 + w1 mean_PiN max(neg_margin - d, 0)^2 + w2 mean_NiN max(neg_margin - d,
    0)^2 with d the feature distance of a pair.  feats = {"base": F, "pos": F, "neg": F} (f32 [n, C] device, rows of
    norm <= 8; the network's are unit vectors), data the batch dictionary of TripletSource.batch.  An empty list
    contributes 0.  FCGF's default margins.  hardest = mine_hardest's dictionary: its three lists enter the SAME
    library call as three more PUSH terms with neg_margin, weighted by hardest_weights = (w_bp, w_pb, w_bn).  Returns
    the f32 scalar (and the parts, f64 [3] detached -- [6] with hardest --, when return_parts)."""
    names = ("base", "pos", "neg")
    mats = [feats[k] for k in names]
    terms = [(names.index(a), names.index(b), data[key], kind, pos_margin if kind == B.PAIR_PULL else neg_margin, w)
             for (key, a, b, kind), w in zip(PAIR_TERMS, weights)]
    if hardest is not None:
        terms += [(names.index(a), names.index(b), hardest[key], B.PAIR_PUSH, neg_margin, w)
                  for (key, a, b), w in zip(HARDEST_TERMS, hardest_weights)]
    total, parts = PairLossFunction.apply(terms, *mats)
    return (total, parts) if return_parts else total


def embedding_triplet(e_base, e_pos, e_neg, margin=0.5):
    """Triplet margin loss on the L2-normalised global descriptors: mean_b max(|e_b - e_p| - |e_b - e_n| + margin,
    0) (torch's triplet_margin_loss, p = 2)."""
    e_base, e_pos, e_neg = (F.normalize(e, dim=1) for e in (e_base, e_pos, e_neg))
    return F.triplet_margin_loss(e_base, e_pos, e_neg, margin=margin)


def corsair_loss(feats, embs, data, pos_margin=0.1, neg_margin=1.4, weights=(1, 1, 1), triplet_margin=0.5,
                 triplet_weight=1.0, hardest=None, hardest_weights=(1, 1, 1)):
    """pair_contrastive(feats, data) + triplet_weight * embedding_triplet(embs).  embs = {"base": E, "pos": E,
    "neg": E} ([B, 256], not yet normalised).  Returns (scalar, parts): parts is a dict of detached device tensors
    {"pip", "pin", "nin", "triplet"} for logging -- reading them is the caller's host wait; with hardest (see
    pair_contrastive) also {"hn_bp", "hn_pb", "hn_bn"}."""
    pair, parts = pair_contrastive(feats, data, pos_margin, neg_margin, weights, return_parts=True, hardest=hardest,
                                   hardest_weights=hardest_weights)
    trip = embedding_triplet(embs["base"], embs["pos"], embs["neg"], triplet_margin)
    loss = pair + triplet_weight * trip
    out = {"pip": parts[0], "pin": parts[1], "nin": parts[2], "triplet": trip.detach()}
    if hardest is not None:
        out.update({"hn_bp": parts[3], "hn_pb": parts[4], "hn_bn": parts[5]})
    return loss, out
