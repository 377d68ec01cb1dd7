"""The stage-4 estimators of registration.sym_pose_batch, described once: one entry of TABLE per estimator, which
registration, shapenet_eval, harness and their command lines read instead of spelling the names out.  The table is static --
nothing registers at run time; a new estimator is a new entry, its checker and its runner here.

An entry's runner takes the estimator's checked options `o` (by keyword) and what the call assembled `c` (a namespace: src,
tgt, offs and m -- the correspondence lists of every hypothesis --, max_corr, max_iter, confidence, seed; for an estimator
that reads no descriptors the two clouds instead, see _run_ppf) and returns (T, inliers, rmse, iters) as its front end gives
them; run_stage4 brings them to the common form.  The front ends are looked up through their modules at call time (tools
swap backend.fgr_batch for a spy), and nothing here allocates an output tensor."""
from typing import Callable, NamedTuple, Optional

import numpy as np
import torch

from . import backend as B, featmatch as FM, ppf as PPF, sc2 as S2


def check_fm_options(ransac_n, edge_similarity, mutual, iterations, who="sym_pose_batch"):
    """The fm_* options of registration = "ransac_fm" as (ransac_n, edge_similarity, mutual, iterations), or ValueError."""
    if isinstance(ransac_n, bool) or ransac_n not in (3, 4):
        raise ValueError("%s: fm_ransac_n must be 3 or 4, got %r" % (who, ransac_n))
    if isinstance(edge_similarity, bool) or not isinstance(edge_similarity, (int, float)) or \
            not 0.0 <= edge_similarity <= 1.0:
        raise ValueError("%s: fm_edge_similarity must lie in [0, 1] (0 = no edge checker), got %r" % (who, edge_similarity))
    if not isinstance(mutual, (bool, np.bool_)):
        raise ValueError("%s: fm_mutual must be a bool, got %r" % (who, mutual))
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 1 <= iterations < 2 ** 31:
        raise ValueError("%s: fm_iterations must be an integer in [1, 2^31), got %r" % (who, iterations))
    return int(ransac_n), float(edge_similarity), bool(mutual), int(iterations)


def check_sc2_options(compat_dist, seeds, k, max_corr, who="sym_pose_batch"):
    """The sc2_* options of registration = "sc2" as (compat_dist, seeds, k), or ValueError.  compat_dist None = max_corr / 2
    (untuned)."""
    if compat_dist is None:
        compat_dist = 0.5 * max_corr
    if isinstance(compat_dist, bool) or not isinstance(compat_dist, (int, float, np.floating)) or \
            not 0.0 < compat_dist < float("inf"):
        raise ValueError("%s: sc2_compat_dist must be positive and finite, got %r" % (who, compat_dist))
    if isinstance(seeds, bool) or not isinstance(seeds, (int, np.integer)) or not 0 <= seeds < 2 ** 31:
        raise ValueError("%s: sc2_seeds must be an integer in [0, 2^31) (0 = every correspondence), got %r" % (who, seeds))
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 2 <= k <= 64:
        raise ValueError("%s: sc2_k must be an integer in [2, 64], got %r" % (who, k))
    return float(compat_dist), int(seeds), int(k)


def check_ppf_options(scene_side, dist_step, ref_step, n_cand, who="sym_pose_batch"):
    """The ppf_* options of registration = "ppf" as (scene_side, dist_step, ref_step, n_cand), or ValueError.  dist_step None
    = 0.05 of each model's bounding-box diagonal (untuned)."""
    if isinstance(scene_side, bool) or scene_side not in (0, 1):
        raise ValueError("%s: ppf_scene_side must be 0 or 1, got %r" % (who, scene_side))
    steps = dist_step if isinstance(dist_step, (list, tuple, np.ndarray)) else [dist_step]      # one per pair, or one for all
    for v in steps:
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.floating)) or
                              not 0.0 < v < float("inf")):
            raise ValueError("%s: ppf_dist_step must be positive and finite (None = 0.05 of the model's diagonal), got %r"
                             % (who, dist_step))
    if isinstance(ref_step, bool) or not isinstance(ref_step, (int, np.integer)) or not 1 <= ref_step < 2 ** 31:
        raise ValueError("%s: ppf_ref_step must be an integer in [1, 2^31), got %r" % (who, ref_step))
    if isinstance(n_cand, bool) or not isinstance(n_cand, (int, np.integer)) or not 1 <= n_cand <= 64:
        raise ValueError("%s: ppf_n_cand must be an integer in [1, 64], got %r" % (who, n_cand))
    if steps is not dist_step:
        dist_step = None if dist_step is None else float(dist_step)
    else:
        dist_step = [float(v) for v in steps]
    return int(scene_side), dist_step, int(ref_step), int(n_cand)


def _run_ransac(o, c):
    return B.ransac_batch(c.src, c.tgt, c.offs, c.max_corr, 10, c.max_iter, c.confidence, c.seed)


def _run_fgr(o, c):
    r = B.fgr_batch(c.src, c.tgt, c.offs, c.max_corr, mu_floor=o["fgr_mu_floor"], iteration_number=o["fgr_iterations"],
                    tuple_test=o["fgr_tuple_test"], seed=c.seed)
    return r.T, r.inliers, r.rmse, r.iters


def _run_fm(o, c):
    r = FM.ransac_fm_batch(c.src, c.tgt, c.offs, c.max_corr, m=c.m, ransac_n=o["fm_ransac_n"],
                           edge_similarity=o["fm_edge_similarity"], check_distance=True, iterations=o["fm_iterations"],
                           seed=c.seed)
    return r.T, r.inliers, r.rmse, r.n_valid


def _run_sc2(o, c):
    r = S2.sc2_batch(c.src, c.tgt, c.offs, c.max_corr, o["sc2_compat_dist"], n_seeds=o["sc2_seeds"], k_consensus=o["sc2_k"])
    return r.T, r.inliers, r.rmse, r.n_valid


def _run_ppf(o, c):
    """c: clouds, normals and offs as (scene, model), max_corr.  The pose is scene -> model, the inverse when the scene is
    the CAD side; inliers = the verification count, iters = the votes of the winner's peak."""
    pairs = list(range(len(c.offs[0]) - 1))
    steps = o["ppf_dist_step"] if o["ppf_dist_step"] is not None else PPF.default_dist_step(c.clouds[1], c.offs[1])
    r = PPF.ppf_batch(c.clouds[0], c.normals[0], c.offs[0], c.clouds[1], c.normals[1], c.offs[1], pairs, pairs, steps,
                      c.max_corr, o["ppf_ref_step"], o["ppf_n_cand"])
    return (r.T if o["ppf_scene_side"] == 0 else r.T_inv).reshape(-1, 4, 4), r.count, r.rmse, r.votes


class Estimator(NamedTuple):
    name: str
    what: str                           # as the refusals describe it
    design: int                         # the DESIGN section they quote
    options: dict                       # keyword of sym_pose_batch -> default, in the order the checker takes them
    check: Optional[Callable]           # (who, max_corr, *values in that order) -> the checked values in that order
    run: Callable                       # (o, c) -> (T, inliers, rmse, iters), see the module's documentation
    no_symmetry: Optional[str] = None   # why use_symmetry=True is refused, None = it is accepted
    descriptors: bool = True            # False: stages 1 - 3 are skipped, baseF / posF may be None
    k: Optional[int] = None             # the k of stage 1, None = k_nn
    wired: bool = False                 # the harness, the sharded evaluation and the cache format know it


TABLE = (
    Estimator("ransac", "the reference's correspondence RANSAC", 3, {}, None, _run_ransac, wired=True),
    Estimator("fgr", "Fast Global Registration", 17, dict(fgr_mu_floor=0.025, fgr_iterations=64, fgr_tuple_test=True), None,
              _run_fgr, wired=True),
    Estimator("ransac_fm", "feature-matching RANSAC", 25,
              dict(fm_ransac_n=3, fm_edge_similarity=0.9, fm_mutual=True, fm_iterations=100000),
              lambda who, max_corr, *v: check_fm_options(*v, who), _run_fm,
              no_symmetry="the part configurations are out of scope", k=1),
    Estimator("sc2", "the compatibility-graph estimator", 27, dict(sc2_compat_dist=None, sc2_seeds=1024, sc2_k=20),
              lambda who, max_corr, *v: check_sc2_options(*v, max_corr, who), _run_sc2),
    Estimator("ppf", "point-pair-feature voting", 28,
              dict(ppf_scene_side=0, ppf_dist_step=None, ppf_ref_step=5, ppf_n_cand=16, ppf_view_points=None),
              lambda who, max_corr, *v: check_ppf_options(*v[:4], who) + v[4:], _run_ppf,
              no_symmetry="symmetry hypotheses are out of scope", descriptors=False),
)
NAMES = tuple(e.name for e in TABLE)
WIRED = tuple(e.name for e in TABLE if e.wired)


def lookup(name, what, names=NAMES):
    """The entry called `name`; ValueError "`what` must be 'a', 'b' or 'c', got ..." when it is not one of `names`."""
    if name not in names:
        quoted = ["'%s'" % n for n in names]
        raise ValueError("%s must be %s or %s, got %r" % (what, ", ".join(quoted[:-1]), quoted[-1], name))
    return TABLE[NAMES.index(name)]


def checked_options(chosen, values, max_corr, who="sym_pose_batch"):
    """`chosen`'s options by keyword, checked.  values: keyword -> value, a missing one = the table's default.  The options of
    EVERY estimator are checked, in table order: an invalid fm_ransac_n is refused under "ransac" too."""
    out = {}
    for e in TABLE:
        v = tuple(values.get(key, default) for key, default in e.options.items())
        v = e.check(who, max_corr, *v) if e.check else v
        if e is chosen:
            out = dict(zip(e.options, v))
    return out


def run_stage4(entry, o, c):
    """entry's runner on c, as the quadruple sym_pose_batch's `finish` consumes: (T f32 [n,4,4], inliers int32, rmse, iters
    int32), the int32 columns contiguous."""
    T, inl, rmse, iters = entry.run(o, c)
    return T.to(torch.float32), inl.contiguous(), rmse, iters.contiguous()
