"""Training losses.  The reference ships datasets that mine PiP / PiN / NiN pair lists and no loss
(SURVEY 1); this is the FCGF-form contrastive loss those lists were mined for plus the triplet loss on the global
descriptors.

pair_contrastive runs in the library (cs_pair_loss_fwd / cs_pair_loss_bwd): value and feature gradients are integer
sums of fixed-point terms, bit-identical from run to run and independent of the order of the pairs.  embedding_triplet
is plain torch on 3 x B x 256 values (dense reductions only: deterministic as it is).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import backend as B
from .autograd import PairLossFunction

# (pair list, feature matrix of column 0, of column 1, kind): TripletSource.batch's lists, rows batch-global
PAIR_TERMS = (("PiP_pairs", "base", "pos", B.PAIR_PULL),
              ("PiN_pairs", "base", "pos", B.PAIR_PUSH),
              ("NiN_pairs", "base", "neg", B.PAIR_PUSH))


def pair_contrastive(feats, data, pos_margin=0.1, neg_margin=1.4, weights=(1, 1, 1), return_parts=False):
    """w0 mean_PiP max(d - pos_margin, 0)^2 + w1 mean_PiN max(neg_margin - d, 0)^2 + w2 mean_NiN max(neg_margin - d,
    0)^2 with d the feature distance of a pair.  feats = {"base": F, "pos": F, "neg": F} (f32 [n, C] device, rows of
    norm <= 8; the network's are unit vectors), data the batch dictionary of TripletSource.batch.  An empty list
    contributes 0.  FCGF's default margins.  Returns the f32 scalar (and the three parts, f64 [3] detached, when
    return_parts)."""
    names = ("base", "pos", "neg")
    mats = [feats[k] for k in names]
    terms = [(names.index(a), names.index(b), data[key], kind, pos_margin if kind == B.PAIR_PULL else neg_margin, w)
             for (key, a, b, kind), w in zip(PAIR_TERMS, weights)]
    total, parts = PairLossFunction.apply(terms, *mats)
    return (total, parts) if return_parts else total


def embedding_triplet(e_base, e_pos, e_neg, margin=0.5):
    """Triplet margin loss on the L2-normalised global descriptors: mean_b max(|e_b - e_p| - |e_b - e_n| + margin,
    0) (torch's triplet_margin_loss, p = 2)."""
    e_base, e_pos, e_neg = (F.normalize(e, dim=1) for e in (e_base, e_pos, e_neg))
    return F.triplet_margin_loss(e_base, e_pos, e_neg, margin=margin)


def corsair_loss(feats, embs, data, pos_margin=0.1, neg_margin=1.4, weights=(1, 1, 1), triplet_margin=0.5,
                 triplet_weight=1.0):
    """pair_contrastive(feats, data) + triplet_weight * embedding_triplet(embs).  embs = {"base": E, "pos": E,
    "neg": E} ([B, 256], not yet normalised).  Returns (scalar, parts): parts is a dict of detached device tensors
    {"pip", "pin", "nin", "triplet"} for logging -- reading them is the caller's host wait."""
    pair, parts = pair_contrastive(feats, data, pos_margin, neg_margin, weights, return_parts=True)
    trip = embedding_triplet(embs["base"], embs["pos"], embs["neg"], triplet_margin)
    loss = pair + triplet_weight * trip
    return loss, {"pip": parts[0], "pin": parts[1], "nin": parts[2], "triplet": trip.detach()}
