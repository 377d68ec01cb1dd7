"""NumPy / Python restatement of cs_icp_plane_robust_batch (include/corsair_hip.h), bit for bit.  Pose chain, association
and frame are those of tests/icp_ref.py, per-pair terms, normal equations, Cholesky solve, Cayley update and stop rules those
of tests/icp_plane_ref.py (imported, as the library shares the code); this file restates the weight of a kept pair, the 27
weighted sums, the 30th sum and wfitness.  Every plain Python float operation is one IEEE f64 operation."""
import math

import numpy as np

from tests.icp_plane_ref import MIN_CORR, PAIRS, _cls, plane_frame, terms_of, update
from tests.icp_ref import associate, fix, frame

NSUM = 30
L2, HUBER, CAUCHY, TUKEY = 0, 1, 2, 3
KERNELS = {"l2": L2, "huber": HUBER, "cauchy": CAUCHY, "tukey": TUKEY}


def weight(kernel, r, k):
    """w of one kept pair from its residual r and the scale k ([O3D-knowledge] Huber / Cauchy / TukeyLoss::Weight)."""
    a = abs(r)
    if kernel == HUBER:
        w = 1.0 if a <= k else k / a
    elif kernel == CAUCHY:
        q = r / k
        w = 1.0 / (1.0 + q * q)
    elif kernel == TUKEY:
        if not a < k:
            w = 0.0
        else:
            q = r / k
            e = 1.0 - q * q
            w = e * e
    else:
        w = 1.0
    return w if w == w else 0.0


def sums_of(corr, P, D, tgt, nrm, fr, kernel, k, watch=None):
    """The 30 integer sums over the kept pairs.  watch (a dict): records the largest |scaled weighted term| / clamp, the
    largest |sum| and the range of the weights seen."""
    S = [0] * NSUM
    for i, j in enumerate(corr):
        if j < 0:
            continue
        J, r = terms_of(P[i], tgt[j], nrm[j], fr)
        w = weight(kernel, r, k)
        S[0] += 1
        scaled = []
        with np.errstate(all="ignore"):
            for at, (a, b) in enumerate(PAIRS):
                sc = fr["sc_" + _cls(a, b)]
                x = (J[a] * J[b]) * w
                S[1 + at] += fix(x, sc, fr["clamp"])
                scaled.append(x * sc)
            for a in range(6):
                sc = fr["sc_rd"] if a < 3 else fr["sc_td"]
                x = (J[a] * r) * w
                S[22 + a] += fix(x, sc, fr["clamp"])
                scaled.append(x * sc)
        S[28] += fix(D[i], fr["sc2"], fr["clamp"])
        scaled.append(D[i] * fr["sc2"])
        S[29] += fix(w, fr["clamp"], fr["clamp"])
        if watch is not None:
            m = max(abs(v) if v == v else math.inf for v in scaled) / fr["clamp"]
            watch["term"] = max(watch.get("term", 0.0), m)
            watch["wmin"] = min(watch.get("wmin", 1.0), w)
            watch["wmax"] = max(watch.get("wmax", 0.0), w)
    if watch is not None:
        watch["sum"] = max(watch.get("sum", 0), max(abs(v) for v in S))
    assert all(abs(v) < 2 ** 62 for v in S)
    return S


def icp(src, tgt, nrm, T0, max_dist, max_iter=30, relative_fitness=1e-6, relative_rmse=1e-6, kernel=L2, kernel_scale=1.0,
        watch=None):
    """One problem.  Returns dict(T f64 [16], T32 f32 [16], fitness, rmse, wfitness, iters, ncorr, corr int32 [n_src],
    sums: the first 29 in cs_icp_plane_batch's layout)."""
    kernel = KERNELS.get(kernel, kernel)
    assert kernel in (L2, HUBER, CAUCHY, TUKEY)
    k = float(kernel_scale)
    assert kernel == L2 or (math.isfinite(k) and k > 0.0)
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
    assert nrm.shape == tgt.shape
    T = [float(v) for v in np.asarray(T0, np.float32).reshape(16)]
    fr = plane_frame(frame(tgt, len(src), max_dist))
    thr2 = float(max_dist) * float(max_dist)
    iters, fit, rm, rnd = 0, 0.0, 0.0, 0
    while True:
        corr, P, D = associate(T, src, tgt, thr2)
        S = sums_of(corr, P, D, tgt, nrm, fr, kernel, k, watch)
        n = S[0]
        pfit, prm = fit, rm
        fit = n / float(len(src)) if len(src) else 0.0
        rm = math.sqrt((float(S[28]) * fr["inv2"]) / float(n)) if n > 0 else 0.0
        wfit = (float(S[29]) * (1.0 / fr["clamp"])) / float(len(src)) if len(src) else 0.0
        stop = rnd == max_iter
        if rnd > 0 and abs(fit - pfit) < relative_fitness and abs(rm - prm) < relative_rmse:
            stop = True
        if n < MIN_CORR or not math.isfinite(fit) or not math.isfinite(rm):
            stop = True
        if not stop:
            Tn = update(T, S, fr)
            if Tn is None:
                stop = True
            else:
                T = Tn
                iters += 1
        if stop:
            break
        rnd += 1
    T64 = np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        T32 = T64.astype(np.float32)
    return {"T": T64, "T32": T32, "fitness": fit, "rmse": rm, "wfitness": wfit, "iters": iters, "ncorr": int(n),
            "corr": corr, "sums": S}


def icp_batch(src, soff, tgt, nrm, toff, src_seg, tgt_seg, T0, max_dist, max_iter=30, relative_fitness=1e-6,
              relative_rmse=1e-6, kernel=L2, kernel_scale=1.0):
    """The whole call: a list of per-problem results; problems with the same inputs are computed once."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
    T0 = np.asarray(T0, np.float32).reshape(-1, 16)
    out, memo = [], {}
    for p, (ss, ts) in enumerate(zip(src_seg, tgt_seg)):
        key = (ss, ts, T0[p].tobytes())
        if key not in memo:
            memo[key] = icp(src[soff[ss]:soff[ss + 1]], tgt[toff[ts]:toff[ts + 1]], nrm[toff[ts]:toff[ts + 1]], T0[p],
                            max_dist, max_iter, relative_fitness, relative_rmse, kernel, kernel_scale)
        out.append(memo[key])
    return out
