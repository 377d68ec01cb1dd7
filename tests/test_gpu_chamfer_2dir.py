"""cs_chamfer_2dir on the GPU against the NumPy restatement (tests/verify_ref.py) and against cs_chamfer_1dir.

Segment sizes on both sides come from {0, 1, 255, 256, 257, 513}: below, at and above the 256-row tile of either direction
and the 512-row LDS stage of the columns; every (source, target) combination is a problem, so every source segment is shared
by six problems with different poses and every target segment by six.  Further problems: a cloud against itself under the
identity (both values exactly 0), a target with one far outlier (backward > forward: the directions are not swapped), NaN and
infinite rows on either side, NaN entries of d_T.  The library has ONE path (exhaustive f64 on the vector unit; there is no
switch to test under): it is held to 1e-12 relative, the special values 0, +inf and NaN exactly."""
import numpy as np
import pytest
import torch

from tests import verify_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 257, 513)
REL = 1e-12


def _rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = q
    T[:3, 3] = rng.normal(scale=0.2, size=3)
    return T


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _assert_close(got, want, what):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    assert got.shape == want.shape
    for i, (g, w) in enumerate(zip(got, want)):
        if np.isnan(w):
            assert np.isnan(g), (what, i, g, w)
        elif np.isinf(w) or w == 0.0:
            assert g == w, (what, i, g, w)
        else:
            assert abs(g - w) <= REL * abs(w), (what, i, g, w)


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(2718)
    nan, inf = np.float32("nan"), np.float32("inf")
    src = [(0.5 * rng.normal(size=(n, 3))).astype(np.float32) for n in SIZES]
    tgt = [(0.5 * rng.normal(size=(n, 3))).astype(np.float32) for n in SIZES]
    src[4][5] = src[4][0]                                   # duplicate points on either side
    tgt[5][10] = tgt[5][3]
    tgt[5][300] = tgt[5][3]
    same = (0.5 * rng.normal(size=(300, 3))).astype(np.float32)
    src.append(same)                                        # source 6 == target 6
    tgt.append(same.copy())
    tgt.append(np.concatenate([same, [[40.0, -3.0, 2.0]]]).astype(np.float32))     # target 7: one far outlier
    s_nan = src[3].copy()                                   # source 7: a NaN row, source 8: an infinite row
    s_nan[17, 2] = nan
    s_inf = src[4].copy()
    s_inf[256, 0] = inf
    src += [s_nan, s_inf]
    t_nan = tgt[4].copy()                                   # target 8: a NaN row, target 9: an infinite row
    t_nan[0, 1] = nan
    t_inf = tgt[3].copy()
    t_inf[255, 2] = -inf
    tgt += [t_nan, t_inf]
    soff = np.concatenate([[0], np.cumsum([len(c) for c in src])]).tolist()
    toff = np.concatenate([[0], np.cumsum([len(c) for c in tgt])]).tolist()
    probs = [(i, j, _rigid(rng)) for i in range(len(SIZES)) for j in range(len(SIZES))]
    eye = np.eye(4, dtype=np.float32)
    probs += [(6, 6, eye), (6, 7, eye), (6, 7, _rigid(rng))]
    probs += [(7, 2, _rigid(rng)), (8, 3, _rigid(rng)), (2, 8, _rigid(rng)), (3, 9, _rigid(rng)), (7, 8, _rigid(rng)), (8, 0, eye),
              (0, 9, eye)]
    for i, j, entry in ((2, 3, (0, 3)), (4, 5, (1, 1)), (0, 3, (2, 0)), (3, 0, (0, 0)), (1, 1, (2, 3))):     # NaN entries of d_T
        T = _rigid(rng)
        T[entry] = nan
        probs.append((i, j, T))
    T_inf = _rigid(rng)
    T_inf[0, 3] = inf
    probs.append((2, 2, T_inf))
    sseg = [p[0] for p in probs]
    tseg = [p[1] for p in probs]
    Ts = np.stack([p[2] for p in probs])
    S, Tg = np.concatenate(src), np.concatenate(tgt)
    want = ref.chamfer_2dir_batch(S, soff, Tg, toff, sseg, tseg, Ts)
    return dict(S=S, Tg=Tg, soff=soff, toff=toff, sseg=sseg, tseg=tseg, Ts=Ts, want=want)


def _run(gpu, c, idx=None):
    from corsair_amd import backend as B

    idx = range(len(c["sseg"])) if idx is None else idx
    idx = [int(i) for i in idx]
    out = B.chamfer_2dir(torch.from_numpy(c["S"]).to(gpu), c["soff"], torch.from_numpy(c["Tg"]).to(gpu), c["toff"],
                         [c["sseg"][i] for i in idx], [c["tseg"][i] for i in idx], torch.from_numpy(c["Ts"][idx]).to(gpu))
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(idx), 2)
    return out.cpu().numpy()


def test_both_directions_match_the_restatement(gpu, case):
    want = case["want"]
    # the restatement itself sees every special value the problems were built for
    assert np.isnan(want).any() and np.isinf(want).any() and (want == 0.0).any() and np.isfinite(want).sum() > 50
    got = _run(gpu, case)
    _assert_close(got, want, "chamfer_2dir")
    n = len(SIZES) ** 2
    assert got[n].tolist() == [0.0, 0.0]                                      # a cloud against itself, identity
    assert got[n + 1][0] == 0.0 and got[n + 1][1] > 0.1                       # the outlier counts backward only
    assert got[n + 2][1] > got[n + 2][0] > 0.0
    empty_src = [p for p in range(n) if case["sseg"][p] == 0]
    empty_tgt = [p for p in range(n) if case["tseg"][p] == 0]
    assert np.isnan(got[empty_src, 0]).all() and np.isnan(got[empty_tgt, 1]).all()
    assert all(got[p, 1] == np.inf for p in empty_src if case["tseg"][p] != 0)
    assert all(got[p, 0] == np.inf for p in empty_tgt if case["sseg"][p] != 0)


def test_forward_is_chamfer_1dir(gpu, case):
    from corsair_amd import backend as B

    got = _run(gpu, case)
    one = B.chamfer_1dir(torch.from_numpy(case["S"]).to(gpu), case["soff"], torch.from_numpy(case["Tg"]).to(gpu), case["toff"],
                         case["sseg"], case["tseg"], torch.from_numpy(case["Ts"]).to(gpu)).cpu().numpy()
    _assert_close(got[:, 0], one, "forward against chamfer_1dir")


def test_bits_repeat_and_do_not_depend_on_the_other_problems(gpu, case):
    a = _run(gpu, case)
    b = _run(gpu, case)
    assert np.array_equal(_bits(a), _bits(b))
    perm = np.random.default_rng(9).permutation(len(case["sseg"]))
    c = _run(gpu, case, perm)
    assert np.array_equal(_bits(c), _bits(a[perm]))
    for p in (0, 7, 35, 36, 40, len(case["sseg"]) - 1):
        assert np.array_equal(_bits(_run(gpu, case, [p])), _bits(a[[p]])), p
    # the same problem twice in one call: each keeps its own column minima
    twice = _run(gpu, case, [35, 35, 37, 35])
    assert np.array_equal(_bits(twice), _bits(a[[35, 35, 37, 35]]))


def test_arguments_are_checked(gpu, case):
    from corsair_amd import backend as B

    S, Tg = torch.from_numpy(case["S"]).to(gpu), torch.from_numpy(case["Tg"]).to(gpu)
    eye = torch.eye(4, device=gpu).reshape(1, 4, 4)
    assert tuple(B.chamfer_2dir(S, case["soff"], Tg, case["toff"], [], [], eye[:0]).shape) == (0, 2)
    with pytest.raises(ValueError, match="offset table"):
        B.chamfer_2dir(S, case["soff"] + [len(S) + 1], Tg, case["toff"], [1], [1], eye)
    with pytest.raises(ValueError, match="segment id"):
        B.chamfer_2dir(S, case["soff"], Tg, case["toff"], [len(case["soff"]) - 1], [1], eye)
    with pytest.raises(ValueError, match="transform"):
        B.chamfer_2dir(S, case["soff"], Tg, case["toff"], [1, 2], [1, 2], eye)
