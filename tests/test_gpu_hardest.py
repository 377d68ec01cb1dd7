"""cs_hardest_negatives on the GPU: indices and f64 distances are BIT-EQUAL to tests/hardest_ref.py on every path (f16
matrix-core shortlist + voucher + fallback for 16-d, the exhaustive kernel for the rest and under CS_HARDNEG_MFMA=0).

`python -m tests.test_gpu_hardest OUT.npz` evaluates the battery of the switch test in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import hardest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SIZES_Q = (1, 31, 257, 5000, 12000)
SIZES_T = (257, 12000, 1, 31, 5000)
BIG_RADIUS = 10.0           # the clouds live in a unit cube: every row is excluded


def _unit_rows(rng, n, c):
    f = rng.standard_normal((n, c))
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def _case(seed, c, sizes_q=SIZES_Q, sizes_t=SIZES_T, per_seg=24):
    """Segments of mixed sizes, unit-norm random features, points in a unit cube, per_seg anchors from every query
    segment (global rows, duplicates possible), shuffled across the problems."""
    rng = np.random.default_rng(seed)
    qoff = np.concatenate([[0], np.cumsum(sizes_q)]).tolist()
    toff = np.concatenate([[0], np.cumsum(sizes_t)]).tolist()
    case = {"qf": _unit_rows(rng, qoff[-1], c), "tf": _unit_rows(rng, toff[-1], c),
            "qxyz": rng.uniform(-0.5, 0.5, (qoff[-1], 3)).astype(np.float32),
            "txyz": rng.uniform(-0.5, 0.5, (toff[-1], 3)).astype(np.float32), "qoff": qoff, "toff": toff}
    anchors = np.concatenate([rng.integers(qoff[s], qoff[s + 1], per_seg) for s in range(len(sizes_q)) if sizes_q[s]])
    case["anchors"] = rng.permutation(anchors).astype(np.int32)
    return case


def _padded(x, ld, dev):
    """The matrix as a device view with leading dimension ld (the padding holds NaN: it must never be read)."""
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :x.shape[1]] = torch.from_numpy(x).to(dev)
    return buf[:, :x.shape[1]]


def _run(case, radius, dev, ld=None, qseg=None, tseg=None):
    from corsair_amd import backend as B

    c = case["qf"].shape[1]
    ld = ld or c
    idx, dist = B.hardest_negatives(_padded(case["qf"], ld, dev), torch.from_numpy(case["qxyz"]).to(dev), case["qoff"],
                                    _padded(case["tf"], ld, dev), torch.from_numpy(case["txyz"]).to(dev), case["toff"],
                                    torch.from_numpy(case["anchors"]).to(dev), radius, qseg, tseg,
                                    return_distance=True)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _want(case, radius, qseg=None, tseg=None):
    return ref.hardest_batch(case["qf"], case["qxyz"], case["qoff"], case["tf"], case["txyz"], case["toff"],
                             case["anchors"], radius, qseg, tseg)


def _assert_bit_equal(got, want):
    assert np.array_equal(got[0], want[0])
    assert got[1].dtype == np.float64 and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))


@pytest.mark.parametrize("c,ld", [(3, 3), (3, 48), (3, 10), (16, 16), (16, 48), (16, 23), (32, 32), (32, 48), (32, 39),
                                  (256, 256), (256, 263)])
def test_bit_equal_to_reference(gpu, c, ld):
    case = _case(100 + c, c)
    for radius in (0.0, 0.03, 0.1, BIG_RADIUS):
        got = _run(case, radius, gpu, ld)
        _assert_bit_equal(got, _want(case, radius))
        if radius == BIG_RADIUS:
            assert np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
        else:
            assert np.all(got[0] >= 0)


def test_empty_segments_no_anchors_duplicates_and_permutation(gpu):
    from corsair_amd import backend as B

    case = _case(7, 16, sizes_q=(300, 40, 0, 500), sizes_t=(0, 700, 50, 2000), per_seg=1)
    rng = np.random.default_rng(8)
    qoff = case["qoff"]
    anchors = np.concatenate([rng.integers(0, 300, 50), rng.integers(300, 340, 30), rng.integers(340, 840, 300)])
    anchors = np.concatenate([anchors, anchors[:40], np.array([5, 5, 5, 339, 339])]).astype(np.int32)   # duplicates
    case["anchors"] = anchors
    got = _run(case, 0.1, gpu)
    _assert_bit_equal(got, _want(case, 0.1))
    in_first = anchors < qoff[1]
    assert np.all(got[0][in_first] == -1) and np.all(np.isposinf(got[1][in_first]))      # empty target segment
    assert np.all(got[0][~in_first] >= 0)
    # a permuted anchor list: the results permute with it
    perm = rng.permutation(len(anchors))
    case_p = dict(case, anchors=anchors[perm])
    got_p = _run(case_p, 0.1, gpu)
    _assert_bit_equal(got_p, (got[0][perm], got[1][perm]))
    # a subset of the problems, in another order; the anchors of segments that are in no problem get -1 / +inf
    got_s = _run(case, 0.1, gpu, qseg=[3, 1], tseg=[1, 3])
    _assert_bit_equal(got_s, _want(case, 0.1, [3, 1], [1, 3]))
    assert np.all(got_s[0][in_first] == -1) and np.all(got_s[0][~in_first] >= 0)
    # A = 0 and n_prob = 0
    case_0 = dict(case, anchors=np.zeros(0, np.int32))
    i0, d0 = _run(case_0, 0.1, gpu)
    assert i0.shape == (0,) and d0.shape == (0,)
    got_n = _run(case, 0.1, gpu, qseg=[], tseg=[])
    assert np.all(got_n[0] == -1) and np.all(np.isposinf(got_n[1]))
    # without the distance output
    dev = gpu
    idx = B.hardest_negatives(torch.from_numpy(case["qf"]).to(dev), torch.from_numpy(case["qxyz"]).to(dev), qoff,
                              torch.from_numpy(case["tf"]).to(dev), torch.from_numpy(case["txyz"]).to(dev),
                              case["toff"], torch.from_numpy(anchors).to(dev), 0.1)
    assert np.array_equal(idx.cpu().numpy(), got[0])


def test_same_matrix_finds_itself_or_a_smaller_duplicate(gpu):
    rng = np.random.default_rng(21)
    for c in (16, 32):
        f = _unit_rows(rng, 3000, c)
        f[1500:1600] = f[100:200]          # duplicated rows: the smaller index wins
        xyz = rng.uniform(-0.5, 0.5, (3000, 3)).astype(np.float32)
        anchors = np.arange(3000, dtype=np.int32)
        case = {"qf": f, "tf": f, "qxyz": xyz, "txyz": xyz, "qoff": [0, 3000], "toff": [0, 3000], "anchors": anchors}
        idx, dist = _run(case, 0.0, gpu)
        want = anchors.copy()
        want[1500:1600] = np.arange(100, 200)
        assert np.array_equal(idx, want) and np.all(dist == 0.0)
        _assert_bit_equal((idx[::7], dist[::7]), _want(dict(case, anchors=anchors[::7]), 0.0))


def _smooth_case(seed=5, n=5000, n_seg=2, per_seg=400):
    """The adversarial case of a shortlist: features are a fixed linear map of the canonical coordinates to 16-d (plus
    a constant vector, so that the normalisation does not fold the rays through the origin onto one feature) plus 1e-3
    noise, row-normalised: every anchor's feature-nearest rows lie inside its exclusion ball."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((3, 16))
    b = rng.standard_normal(16)
    b /= np.linalg.norm(b)
    off = (np.arange(n_seg + 1) * n).tolist()

    def cloud():
        xyz = rng.uniform(-0.5, 0.5, (n * n_seg, 3)).astype(np.float32)
        f = xyz.astype(np.float64) @ m + b + 1e-3 * rng.standard_normal((n * n_seg, 16))
        return xyz, (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)

    qxyz, qf = cloud()
    txyz, tf = cloud()
    anchors = np.concatenate([rng.integers(off[s], off[s + 1], per_seg) for s in range(n_seg)]).astype(np.int32)
    return {"qf": qf, "tf": tf, "qxyz": qxyz, "txyz": txyz, "qoff": off, "toff": off, "anchors": rng.permutation(anchors)}


def test_smooth_features(gpu, monkeypatch):
    from corsair_amd import backend as B

    case = _smooth_case()
    want = _want(case, 0.1)
    # the case is what it claims: without the exclusion the nearest row is a spatial neighbour
    near = _want(case, 0.0)
    assert np.mean(near[0] != want[0]) > 0.9
    monkeypatch.setenv("CS_HARDNEG_STATS", "1")
    B.hardest_stats(reset=True)
    got = _run(case, 0.1, gpu)
    answered, recomputed = B.hardest_stats(reset=True)
    print("smooth features: anchors %d, recomputed exhaustively %d (share %.4f)"
          % (answered, recomputed, recomputed / max(answered, 1)))
    _assert_bit_equal(got, want)
    assert answered == len(case["anchors"])


def test_fallback_share_on_random_features(gpu, monkeypatch):
    """32 problems x 1 024 anchors x 5 000 rows of i.i.d. unit-norm 16-d features, exclusion radius 0.1: the voucher
    must accept at least 90 % of the anchors (the k-NN path recomputes none on such data), and the answers are those
    of a torch brute force."""
    from corsair_amd import backend as B

    g = torch.Generator(device=gpu)
    g.manual_seed(77)
    n_prob, n, per = 32, 5000, 1024
    off = (np.arange(n_prob + 1) * n).tolist()

    def rows(k):
        return torch.nn.functional.normalize(torch.randn((n_prob * n, k), generator=g, device=gpu), dim=1)

    qf, tf = rows(16), rows(16)
    qxyz = torch.rand((n_prob * n, 3), generator=g, device=gpu) - 0.5
    txyz = torch.rand((n_prob * n, 3), generator=g, device=gpu) - 0.5
    anchors = (torch.randint(0, n, (n_prob, per), generator=g, device=gpu) +
               torch.arange(n_prob, device=gpu)[:, None] * n).reshape(-1).int()
    anchors = anchors[torch.randperm(anchors.numel(), generator=g, device=gpu)]
    monkeypatch.setenv("CS_HARDNEG_STATS", "1")
    B.hardest_stats(reset=True)
    idx, dist = B.hardest_negatives(qf, qxyz, off, tf, txyz, off, anchors, 0.1, return_distance=True)
    answered, recomputed = B.hardest_stats(reset=True)
    share = recomputed / max(answered, 1)
    print("random features: anchors %d, recomputed exhaustively %d (share %.4f)" % (answered, recomputed, share))
    assert answered == n_prob * per
    assert share < 0.10
    for p in range(0, n_prob, 5):
        sel = torch.nonzero((anchors >= off[p]) & (anchors < off[p + 1]))[:, 0]
        a = anchors[sel].long()
        d = torch.cdist(qf[a].double(), tf[off[p]:off[p + 1]].double())
        s = torch.cdist(qxyz[a].double(), txyz[off[p]:off[p + 1]].double())
        d[s < 0.1 - 1e-9] = float("inf")
        d_excl = d.clone()
        d_excl[(s - 0.1).abs() <= 1e-9] = float("inf")      # (rows on the sphere to within rounding: either answer)
        best = d.argmin(1)
        ok = (idx[sel].long() == best) | (idx[sel].long() == d_excl.argmin(1))
        assert bool(ok.all())
        assert torch.allclose(dist[sel], d[torch.arange(len(a), device=gpu), idx[sel].long()], rtol=1e-12, atol=0)


def _raw_call(lib, qf, ld_q, qxyz, qoff, tf, ld_t, txyz, toff, qseg, tseg, c, anchors, radius, idx, dist):
    from corsair_amd._lib import i32_array, i64_array, ptr, stream_ptr

    return lib.cs_hardest_negatives(ptr(qf), ld_q, ptr(qxyz), i64_array(qoff), ptr(tf), ld_t, ptr(txyz),
                                    i64_array(toff), i32_array(qseg), i32_array(tseg), len(qseg), c, ptr(anchors),
                                    anchors.shape[0], float(radius), ptr(idx), ptr(dist), stream_ptr())


def test_refused_arguments_leave_outputs_untouched(gpu):
    from corsair_amd import _lib, backend as B

    lib = _lib.load()
    case = _case(9, 16, sizes_q=(100, 200), sizes_t=(300, 400), per_seg=10)
    t = {k: torch.from_numpy(np.asarray(case[k])).to(gpu) for k in ("qf", "tf", "qxyz", "txyz", "anchors")}
    idx = torch.full((20,), -7, dtype=torch.int32, device=gpu)
    dist = torch.full((20,), -7.0, dtype=torch.float64, device=gpu)
    qoff, toff = case["qoff"], case["toff"]

    def call(ld_q=16, ld_t=16, qseg=(0, 1), tseg=(0, 1), c=16, qoff=qoff, toff=toff, radius=0.1):
        return _raw_call(lib, t["qf"], ld_q, t["qxyz"], qoff, t["tf"], ld_t, t["txyz"], toff, list(qseg), list(tseg), c,
                         t["anchors"], radius, idx, dist)

    for kw in (dict(ld_q=15), dict(ld_t=8), dict(c=0), dict(c=257, ld_q=300, ld_t=300), dict(qseg=(0, 0)),
               dict(qseg=(0, -1)), dict(tseg=(-2, 1)), dict(qoff=[0, 200, 100]), dict(toff=[0, 300, 100]),
               dict(radius=float("nan"))):
        assert call(**kw) < 0, kw
        assert lib.cs_last_error()
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((dist == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    _assert_bit_equal((idx.cpu().numpy(), dist.cpu().numpy()), _want(case, 0.1))
    with pytest.raises(_lib.CorsairHipError):
        B.hardest_negatives(t["qf"], t["qxyz"], qoff, t["tf"], t["txyz"], toff, t["anchors"], 0.1, [0, 0], [0, 1])
    with pytest.raises(ValueError):
        B.hardest_negatives(t["qf"], t["qxyz"], qoff, t["tf"][:, :8], t["txyz"], toff, t["anchors"], 0.1)
    with pytest.raises(TypeError):
        B.hardest_negatives(t["qf"], t["qxyz"], qoff, t["tf"], t["txyz"], toff, t["anchors"].long(), 0.1)


# ---- CS_HARDNEG_MFMA=0 against the default, a fresh process per setting ------------------------------------------------
def _battery(dev):
    out = {}
    case = _case(116, 16)
    for radius in (0.0, 0.1):
        out["mixed_i_%g" % radius], out["mixed_d_%g" % radius] = _run(case, radius, dev, 23)
    out["smooth_i"], out["smooth_d"] = _run(_smooth_case(), 0.1, dev)
    return out


def test_switch_selects_the_exhaustive_kernel_with_equal_results(gpu, tmp_path):
    res = {}
    for setting in ("default", "0"):
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), CS_HARDNEG_STATS="1")
        env.pop("CS_HARDNEG_MFMA", None)
        if setting == "0":
            env["CS_HARDNEG_MFMA"] = "0"
        path = str(tmp_path / ("out_%s.npz" % setting))
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_hardest", path], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[setting] = dict(np.load(path))
    a, b = res["default"], res["0"]
    assert a.keys() == b.keys()
    for k in a:
        if k != "stats":
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k],
                                                               b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]), k
    # the switch did select another path: under it every anchor is "recomputed", by default (nearly) none of the mixed ones
    assert b["stats"][0] == b["stats"][1] == a["stats"][0]
    assert a["stats"][1] < a["stats"][0]
    case = _case(116, 16)
    _assert_bit_equal((a["mixed_i_0.1"], a["mixed_d_0.1"]), _want(case, 0.1))


if __name__ == "__main__":
    from corsair_amd import backend as _B

    _B.hardest_stats(reset=True)
    _out = _battery(torch.device("cuda:0"))
    _out["stats"] = np.array(_B.hardest_stats(), np.int64)
    np.savez(sys.argv[1], **_out)
