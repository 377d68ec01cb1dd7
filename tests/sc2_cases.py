"""Inputs shared by tests/test_sc2_cpu.py and tests/test_gpu_sc2.py: the batch of the GPU bit-equality test, the
defined cases of the header, and an independent float implementation of cs_sc2_batch (square-root lengths, a Kabsch / SVD fit
with the solver's acceptance rule evaluated from the singular values) that shares nothing with tests/sc2_ref.py but the tie
rules.  The planted problems come from tests/featmatch_cases.py."""
import numpy as np

from tests import featmatch_cases as FC

MAX_CORR = 0.02
TAU = 0.01


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---- the batch of the GPU bit-equality test ------------------------------------------------------------------------------
# 63, 64, 65, 129 and 4097 are the word and tile edges (4097 pairs need 65 words); the last problem: every seed invalid
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 129, 257, 1500, 4097, 200]
PAD = [0, 3, 0, 2, 0, 0, 5, 0, 70, 0, 7, 0, 1]                # slots past d_m[p]: the capacity is larger than the problem
INVALID = len(SIZES) - 1
INVALID_TAU = 1e-4
CAPS = [a + b for a, b in zip(SIZES, PAD)]
OFF = np.concatenate([[0], np.cumsum(CAPS)]).tolist()


def batch(seed):
    """{"src", "tgt" f32 [sum CAPS,3], "m" int32 [P]}: problem p holds SIZES[p] pairs in its first slots, the slots past them
    hold finite rows that would be compatible with each other (a translated copy) and that nothing may read."""
    rng = np.random.default_rng(seed)
    src, tgt = [], []
    for p, (m, pad) in enumerate(zip(SIZES, PAD)):
        share = 1.0 if (m <= 4 or p == INVALID) else (0.05 if m >= 1000 else 0.4)
        s, q, _, _, _ = FC.planted(m, share, 1000 * seed + p, noise=0.002)
        if p == INVALID:
            q = _f32(2.0 * q.astype(np.float64))
        filler = _f32(rng.uniform(-0.5, 0.5, (pad, 3)))
        src += [s, filler]
        tgt += [q, _f32(filler.astype(np.float64) + 0.25)]
    return {"src": np.concatenate(src), "tgt": np.concatenate(tgt), "m": np.asarray(SIZES, np.int32)}


def problem(d, p):
    return d["src"][OFF[p]:OFF[p] + SIZES[p]], d["tgt"][OFF[p]:OFF[p] + SIZES[p]]


# ---- the defined cases of the header -----------------------------------------------------------------------------------
def defined_cases():
    """name -> (src, tgt, kwargs of sc2_one); shared with the GPU test."""
    s, q, _, _, keep = FC.planted(40, 0.6, 5)
    order = np.concatenate([np.nonzero(keep)[0], np.nonzero(~keep)[0]])      # the planted pairs first
    s, q = s[order], q[order]
    line = _f32([[t, 2 * t, -t] for t in range(12)])
    bad_s, bad_q = s.copy(), q.copy()
    bad_s[3] = [np.nan, 0, 0]
    bad_q[7] = [0, np.inf, 0]
    bad_s[11], bad_q[11] = [np.inf] * 3, [np.inf] * 3
    bad_q[20] = [np.nan] * 3
    g, gq, _, _ = FC.two_clusters()
    # one source point with three targets (a 3-NN list), then planted pairs
    dup_s, dup_q = s.copy(), q.copy()
    dup_s[1], dup_s[2] = dup_s[0], dup_s[0]
    rng = np.random.default_rng(3)
    grid = _f32(rng.integers(-8, 9, (16, 3)))
    kw = dict(max_corr=MAX_CORR, compat_dist=TAU, n_seeds=0, k_consensus=20)
    cases = {"m%d" % m: (s[:m], q[:m], kw) for m in range(5)}
    cases.update({
        "copies": (np.tile(s[:1], (9, 1)), np.tile(q[:1], (9, 1)), kw),
        "collinear": (line, line + np.float32(1.0), dict(kw, max_corr=0.5, compat_dist=0.5)),
        "invalid": (s, _f32(2.0 * q.astype(np.float64)), dict(kw, compat_dist=1e-4)),
        "clusters": (g, gq, dict(kw, max_corr=0.5, compat_dist=1e-3)),
        "knn_duplicates": (dup_s, dup_q, kw),
        "nonfinite": (bad_s, bad_q, kw),
        "tau_overflow": (s, q, dict(kw, compat_dist=1e160)),
        "tau_underflow": (s, q, dict(kw, compat_dist=1e-170)),
        "corr_overflow": (s, q, dict(kw, max_corr=1e160)),
        "corr_underflow": (s, q, dict(kw, max_corr=1e-170)),
        "k_above_every_degree": (s, q, dict(kw, k_consensus=64)),
        "k2": (s, q, dict(kw, k_consensus=2)),
        "seeds1": (s, q, dict(kw, n_seeds=1)),
        "seeds_m": (s, q, dict(kw, n_seeds=len(s))),
        "seeds_m_plus_5": (s, q, dict(kw, n_seeds=len(s) + 5)),
        "all_compatible": (grid, grid.copy(), dict(kw, max_corr=0.5, compat_dist=0.5)),
    })
    return cases


# ---- the independent float implementation ----------------------------------------------------------------------------
def float_sc2(src, tgt, max_corr, compat_dist, n_seeds=1024, k_consensus=20):
    """cs_sc2_batch of one problem in plain float arithmetic.  Returns a dict: C bool [m,m], seeds (rows in rank order),
    sets {rank: sorted rows or None}, valid ranks, rank / row / count of the winner (-1 / -1 / 0 without one), its mask, its
    pose, and gap = the smallest relative distance of any comparison it made from its threshold."""
    s, q = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    m = len(s)
    gap = np.inf
    fin = np.isfinite(s).all(1) & np.isfinite(q).all(1)
    with np.errstate(all="ignore"):
        ls = np.sqrt(((s[:, None, :] - s[None, :, :]) ** 2).sum(2))
        lt = np.sqrt(((q[:, None, :] - q[None, :, :]) ** 2).sum(2))
        diff = np.abs(ls - lt)
        ok = fin[:, None] & fin[None, :] & (ls > 0) & (lt > 0) & np.isfinite(diff)
        C = ok & (diff < compat_dist)
        if ok.any() and np.isfinite(compat_dist):
            gap = min(gap, float(np.min(np.abs(diff[ok] - compat_dist) / np.maximum(diff[ok], compat_dist))))
    deg = C.sum(1)
    seeds = sorted(range(m), key=lambda i: (-int(deg[i]), i))
    S = m if n_seeds == 0 else min(n_seeds, m)
    sets, valid, poses = {}, [], {}
    best, r_best, best_inl = 0, -1, np.zeros(m, bool)
    for r in range(S):
        sd = seeds[r]
        cand = [int(j) for j in np.nonzero(C[sd])[0]]
        sc = {j: int((C[sd] & C[j]).sum()) for j in cand}
        take = sorted(cand, key=lambda j: (-sc[j], j))[:k_consensus]
        A = sorted([sd] + take)
        sets[r] = A if len(A) >= 3 else None
        if len(A) < 3:
            continue
        P, Q = s[A], q[A]
        cs, ct = P.mean(0), Q.mean(0)
        H = (P - cs).T @ (Q - ct)
        U, sv, Vt = np.linalg.svd(H)
        d = np.sign(np.linalg.det(Vt.T @ U.T))
        if sv[0] == 0 or d == 0:
            continue
        s1, s2, s3 = sv[0], sv[1], sv[2] * d
        lam = s1 + s2 + s3
        lhs, rhs = 8.0 * (s2 + s3) * (s1 + s3) * (s1 + s2), FC.HORN_ACCEPT * lam ** 3
        if lhs != rhs:
            gap = min(gap, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
        if not lhs >= rhs:
            continue
        R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
        tr = ct - R @ cs
        if not (np.isfinite(R).all() and np.isfinite(tr).all()):
            continue
        valid.append(r)
        poses[r] = (R, tr)
        with np.errstate(all="ignore"):
            dist = np.linalg.norm(s @ R.T + tr - q, axis=1)
        f = np.isfinite(dist)
        if f.any() and np.isfinite(max_corr):
            gap = min(gap, float(np.min(np.abs(dist[f] - max_corr) / np.maximum(dist[f], max_corr))))
        inl = f & (dist < max_corr)
        if int(inl.sum()) > best:
            best, r_best, best_inl = int(inl.sum()), r, inl
    if m < 3 or best < 3:
        best, r_best, best_inl = 0, -1, np.zeros(m, bool)
    return {"C": C, "seeds": seeds[:S], "sets": sets, "valid": valid, "rank": r_best, "row": seeds[r_best] if r_best >= 0 else -1,
            "count": best, "mask": best_inl, "pose": poses.get(r_best), "gap": gap, "deg": deg}


# ---- a smaller batch for the stream and stale-memory schedules -------------------------------------------------------
S_SIZES = [0, 3, 65, 257, 513]
S_PAD = [2, 0, 5, 0, 40]
S_OFF = np.concatenate([[0], np.cumsum([a + b for a, b in zip(S_SIZES, S_PAD)])]).tolist()


def stream_batch(seed):
    """batch() with S_SIZES / S_PAD: what the stream and stale-memory schedules run."""
    rng = np.random.default_rng(seed)
    src, tgt = [], []
    for p, (m, pad) in enumerate(zip(S_SIZES, S_PAD)):
        s, q, _, _, _ = FC.planted(m, 1.0 if m <= 4 else 0.4, 2000 * seed + p, noise=0.002)
        filler = _f32(rng.uniform(-0.5, 0.5, (pad, 3)))
        src += [s, filler]
        tgt += [q, _f32(filler.astype(np.float64) + 0.25)]
    return {"src": np.concatenate(src), "tgt": np.concatenate(tgt), "m": np.asarray(S_SIZES, np.int32)}
