"""Inputs shared by tests/test_featmatch_cpu.py and tests/test_gpu_featmatch.py: planted correspondence problems,
the batch of the GPU bit-equality test, 1-NN lists for the mutual filter, the defined cases of the header, and an independent
float implementation of cs_ransac_fm_batch (NumPy cross-covariance + SVD fit, plain norms) that shares nothing with
tests/featmatch_ref.py but the draws."""
import numpy as np

MAX_CORR = 0.02


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def pose(rng, max_trans=0.3):
    A = rng.normal(size=(3, 3))
    Q, _ = np.linalg.qr(A)
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q, rng.uniform(-max_trans, max_trans, 3)


def planted(m, share, seed, noise=0.0, half=0.5):
    """(src f32 [m,3], tgt f32 [m,3], R, t, planted bool [m]): round(share m) pairs obey q = R s + t (+ noise), the rest
    have a target drawn uniformly in the box of the posed cloud."""
    rng = np.random.default_rng(seed)
    s = _f32(rng.uniform(-half, half, (m, 3)))
    R, t = pose(rng)
    q = s.astype(np.float64) @ R.T + t
    if noise:
        q = q + rng.normal(0.0, noise, (m, 3))
    keep = np.zeros(m, bool)
    keep[rng.permutation(m)[:int(round(share * m))]] = True
    q[~keep] = rng.uniform(-half * 1.5, half * 1.5, (int((~keep).sum()), 3)) + t
    return s, _f32(q), R, t, keep


# ---- the batch of the GPU bit-equality test ------------------------------------------------------------------------------
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 257, 513, 1500, 200]      # the last one: every hypothesis rejected (target scaled by 2)
PAD = [0, 3, 0, 2, 0, 0, 5, 0, 1, 0, 7, 0]                    # slots past d_m[p]: the capacity is larger than the problem
REJECTED = len(SIZES) - 1
CAPS = [a + b for a, b in zip(SIZES, PAD)]
OFF = np.concatenate([[0], np.cumsum(CAPS)]).tolist()


def batch(seed):
    """{"src", "tgt" f32 [sum CAPS,3], "m" int32 [P]}: problem p holds SIZES[p] pairs in its first slots, the slots past them
    hold far-away finite rows that nothing may read."""
    rng = np.random.default_rng(seed)
    src, tgt = [], []
    for p, (m, pad) in enumerate(zip(SIZES, PAD)):
        share = 1.0 if m <= 4 else 0.4
        s, q, _, _, _ = planted(m, share, 1000 * seed + p, noise=0.002)
        if p == REJECTED:
            q = _f32(2.0 * q.astype(np.float64))
        src += [s, _f32(rng.uniform(50, 60, (pad, 3)))]
        tgt += [q, _f32(rng.uniform(-60, -50, (pad, 3)))]
    return {"src": np.concatenate(src), "tgt": np.concatenate(tgt), "m": np.asarray(SIZES, np.int32)}


def problem(d, p):
    return d["src"][OFF[p]:OFF[p] + SIZES[p]], d["tgt"][OFF[p]:OFF[p] + SIZES[p]]


# ---- 1-NN lists for the mutual filter --------------------------------------------------------------------------------------
M_OFF0 = [0, 300, 300, 340, 351, 363, 763]      # query rows: 300, 0 (an empty query), 40, 11, 12, 400
M_OFF1 = [0, 280, 330, 330, 350, 370, 720]      # CAD rows:   280, 50, 0 (an empty CAD), 20, 20, 350
M_MUTUAL = [120, 0, 0, 8, 9, 150]               # mutual matches planted per pair (ransac_n = 3: 8 falls back, 9 does not)


def mutual_lists(seed):
    """{"fwd" int32 [N0], "bwd" int32 [N1], "x0" f32 [N0,3], "x1" f32 [N1,3]}: per pair M_MUTUAL[p] mutual matches at random
    rows, the other forward entries point at CAD rows whose backward entry names another row (ties of a 1-NN search end
    like that), about one entry in ten is -1; the pair without CAD rows holds -1 only."""
    rng = np.random.default_rng(seed)
    fwd = np.full(M_OFF0[-1], -1, np.int32)
    bwd = np.full(M_OFF1[-1], -1, np.int32)
    for p, k in enumerate(M_MUTUAL):
        a0, n0, b0, n1 = M_OFF0[p], M_OFF0[p + 1] - M_OFF0[p], M_OFF1[p], M_OFF1[p + 1] - M_OFF1[p]
        if n0 == 0 or n1 == 0:
            continue
        qi = rng.permutation(n0)
        ci = rng.permutation(n1)
        for i, j in zip(qi[:k], ci[:k]):
            fwd[a0 + i], bwd[b0 + j] = j, i
        rest_c = ci[k:]
        for i in qi[k:]:
            if rng.random() < 0.1 or len(rest_c) == 0:
                continue                                      # stays -1
            fwd[a0 + i] = rng.choice(ci)                      # any CAD row, matched ones too: its backward entry is not i
        for j in rest_c:
            if rng.random() < 0.9:
                bwd[b0 + j] = rng.choice(qi[:max(k, 1)])      # points at a row whose forward entry is another CAD row
    return {"fwd": fwd, "bwd": bwd, "x0": _f32(rng.uniform(-1, 1, (M_OFF0[-1], 3))), "x1": _f32(rng.uniform(-1, 1, (M_OFF1[-1], 3)))}


# ---- the defined cases of the header -----------------------------------------------------------------------------------
def two_clusters():
    """Two exact pose clusters of 12 pairs each (integer coordinates, quarter turns: every product is exact) and 6 pairs that
    belong to neither."""
    rng = np.random.default_rng(11)
    g = _f32(rng.integers(-8, 9, (30, 3)))
    Ra = np.asarray([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    Rb = np.asarray([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)
    q = np.zeros((30, 3))
    q[:12] = g[:12].astype(np.float64) @ Ra.T + [1, 2, 3]
    q[12:24] = g[12:24].astype(np.float64) @ Rb.T + [-4, 0, 5]
    q[24:] = rng.integers(20, 40, (6, 3))
    perm = rng.permutation(30)
    return g[perm], _f32(q)[perm], np.isin(perm, np.arange(12)), np.isin(perm, np.arange(12, 24))


def defined_cases():
    """name -> (src, tgt, kwargs of ransac_fm_one); shared with the GPU test."""
    s, q, _, _, keep = planted(40, 0.6, 5)
    order = np.concatenate([np.nonzero(keep)[0], np.nonzero(~keep)[0]])      # the planted pairs first: m3 and m4 hold inliers only
    s, q = s[order], q[order]
    line = _f32([[t, 2 * t, -t] for t in range(12)])
    bad_s, bad_q = s.copy(), q.copy()
    bad_s[3] = [np.nan, 0, 0]
    bad_q[7] = [0, np.inf, 0]
    bad_s[11], bad_q[11] = [np.inf] * 3, [np.inf] * 3
    bad_q[20] = [np.nan] * 3
    g, gq, _, _ = two_clusters()
    kw = dict(max_corr=MAX_CORR, ransac_n=3, edge_similarity=0.9, check_distance=True, iterations=256, seed=0)
    cases = {"m%d" % m: (s[:m], q[:m], dict(kw, iterations=64)) for m in range(5)}
    cases.update({
        "m3_n4": (s[:3], q[:3], dict(kw, ransac_n=4, iterations=64)),
        "copies": (np.tile(s[:1], (9, 1)), np.tile(q[:1], (9, 1)), dict(kw, iterations=32)),
        "collinear": (line, line + np.float32(1.0), dict(kw, iterations=64)),
        "rejected": (s, _f32(2.0 * q.astype(np.float64)), kw),
        "clusters": (g, gq, dict(kw, max_corr=0.5, iterations=512, seed=2)),
        "nonfinite": (bad_s, bad_q, kw),
        "nonfinite_no_edge": (bad_s, bad_q, dict(kw, edge_similarity=0.0)),
        "corr_overflow": (s, q, dict(kw, max_corr=1e160, iterations=16)),
        "corr_underflow": (s, q, dict(kw, max_corr=1e-170, iterations=16)),
        "corr_underflow_no_check": (s, q, dict(kw, max_corr=1e-170, iterations=16, check_distance=False)),
        "edge0": (s, q, dict(kw, edge_similarity=0.0)),
        "edge1": (g, gq, dict(kw, max_corr=0.5, edge_similarity=1.0, iterations=512, seed=2)),
        "n4": (s, q, dict(kw, ransac_n=4)),
        "no_distance_check": (s, q, dict(kw, check_distance=False)),
        "iters1": (s, q, dict(kw, iterations=1, seed=5)),
    })
    return cases


# ---- the independent float implementation ----------------------------------------------------------------------------
HORN_ACCEPT = 0.02      # horn_qcp accepts a fit when P'(l) >= 0.02 l^3 at the largest eigenvalue l (corsair_amd/csrc/horn.h)


def float_ransac_fm(src, tgt, draws, max_corr, edge_similarity=0.9, check_distance=True):
    """cs_ransac_fm_batch of one problem in plain float arithmetic: norms with square roots, the rotation from the SVD of the
    cross-covariance (Kabsch), the solver's acceptance rule evaluated from the singular values.  draws: [K][n] row indices.
    Returns (t_best, count, inlier bool [m], valid t list, gap, poses) with gap = the smallest relative distance of any
    comparison it made from its threshold."""
    s, q = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    gap = np.inf
    best, t_best, best_inl, valid, poses = 0, -1, np.zeros(len(s), bool), [], {}

    def cmp_ge(a, b):                      # a >= b, and how close the call was
        nonlocal gap
        if a == b:                         # exact equality (zero lengths of a repeated draw): nothing to round
            return True
        gap = min(gap, abs(a - b) / max(abs(a), abs(b)))
        return a >= b

    for t, idx in enumerate(draws):
        S, Q = s[list(idx)], q[list(idx)]
        n = len(idx)
        if not (np.isfinite(S).all() and np.isfinite(Q).all()):
            continue
        ok = True
        if edge_similarity > 0:
            for a in range(n):
                for b in range(a + 1, n):
                    ls, lt = np.linalg.norm(S[a] - S[b]), np.linalg.norm(Q[a] - Q[b])
                    ok = ok and cmp_ge(ls, edge_similarity * lt) and cmp_ge(lt, edge_similarity * ls)
        if not ok:
            continue
        cs, ct = S.mean(0), Q.mean(0)
        H = (S - cs).T @ (Q - ct)
        U, sv, Vt = np.linalg.svd(H)
        d = np.sign(np.linalg.det(Vt.T @ U.T))
        if sv[0] == 0 or d == 0:
            continue
        s1, s2, s3 = sv[0], sv[1], sv[2] * d
        lam = s1 + s2 + s3
        if not cmp_ge(8.0 * (s2 + s3) * (s1 + s3) * (s1 + s2), HORN_ACCEPT * lam ** 3):
            continue
        R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
        tr = ct - R @ cs
        if check_distance and not all(cmp_ge(max_corr, np.linalg.norm(R @ S[j] + tr - Q[j])) and
                                      np.linalg.norm(R @ S[j] + tr - Q[j]) != max_corr for j in range(n)):
            continue
        valid.append(t)
        poses[t] = (R, tr)
        with np.errstate(all="ignore"):
            dist = np.linalg.norm(s @ R.T + tr - q, axis=1)
        fin = np.isfinite(dist)
        if fin.any():
            gap = min(gap, float(np.min(np.abs(dist[fin] - max_corr) / max_corr)))
        inl = fin & (dist < max_corr)
        if int(inl.sum()) > best:
            best, t_best, best_inl = int(inl.sum()), t, inl
    if best < len(draws[0]) if len(draws) else True:
        return -1, 0, np.zeros(len(s), bool), valid, gap, poses
    return t_best, best, best_inl, valid, gap, poses
