"""Hardest-negative mining without a GPU: the NumPy restatement against an independent brute force, the library's
exports, the trainer's new options, and the unchanged pair terms."""
import ctypes

import numpy as np
from scipy.spatial.distance import cdist

from tests import hardest_ref as ref


def _unit_rows(rng, n, c):
    f = rng.standard_normal((n, c))
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def _brute(qf, qxyz, tf, txyz, radius):
    """SciPy's f64 distance matrices, mask, argmin."""
    d = cdist(qf.astype(np.float64), tf.astype(np.float64))
    if radius > 0:
        s = cdist(qxyz.astype(np.float64), txyz.astype(np.float64), "sqeuclidean")
        d[s < radius * radius] = np.inf
    idx = d.argmin(1).astype(np.int32)
    val = d[np.arange(len(d)), idx]
    idx[~np.isfinite(val)] = -1
    return idx, val


def test_restatement_equals_brute_force():
    rng = np.random.default_rng(11)
    for c, nq, nt, radius in ((16, 200, 3000, 0.1), (3, 50, 700, 0.03), (32, 64, 1000, 0.0), (256, 20, 300, 0.2),
                              (16, 40, 500, 5.0)):
        qf, tf = _unit_rows(rng, nq, c), _unit_rows(rng, nt, c)
        qxyz = rng.uniform(-0.5, 0.5, (nq, 3)).astype(np.float32)
        txyz = rng.uniform(-0.5, 0.5, (nt, 3)).astype(np.float32)
        idx, dist = ref.hardest(qf, qxyz, tf, txyz, radius)
        bidx, bdist = _brute(qf, qxyz, tf, txyz, radius)
        assert np.array_equal(idx, bidx)
        ok = idx >= 0
        assert np.all(np.abs(dist[ok] - bdist[ok]) <= 1e-12 * bdist[ok])
        assert np.all(np.isinf(dist[~ok]))
        if radius == 5.0:
            assert not ok.any()
        else:
            assert ok.all()


def test_fma_is_the_fused_operation():
    # a product whose low half decides the rounding of the sum: the unfused form gives another result
    a = 1.0 + 2.0 ** -30
    c = -(1.0 + 2.0 ** -29)
    assert ref.fma(a, a, c) == 2.0 ** -60 and a * a + c == 0.0
    assert ref.chain(np.float32([1.0, 2.0]), np.float32([0.0, 0.0])) == 5.0


def test_exact_ties_go_to_the_smaller_admissible_row():
    rng = np.random.default_rng(12)
    tf = _unit_rows(rng, 50, 16)
    txyz = rng.uniform(-0.5, 0.5, (50, 3)).astype(np.float32)
    qf = tf[7:8] + np.float32(1e-3)
    qxyz = np.zeros((1, 3), np.float32)
    # rows 3, 20 and 41 are copies of row 7; row 3 lies inside the exclusion ball of the query, the others outside
    for j in (3, 20, 41):
        tf[j] = tf[7]
    txyz[3] = (0.01, 0.0, 0.0)
    for j in (7, 20, 41):
        txyz[j] = (0.3, 0.0, 0.0)
    idx, dist = ref.hardest(qf, qxyz, tf, txyz, 0.1)
    assert idx[0] == 7
    idx0, dist0 = ref.hardest(qf, qxyz, tf, txyz, 0.0)
    assert idx0[0] == 3 and dist0[0] == dist[0]
    # a point at exactly r is admissible (the test is strict)
    txyz[3] = (0.5, 0.0, 0.0)
    assert ref.hardest(qf, qxyz, tf, txyz, 0.5)[0][0] == 3
    bidx, _ = ref.hardest_batch(qf, qxyz, [0, 1], tf, txyz, [0, 50], [0, 0, 5], 0.1)
    assert bidx.tolist() == [3, 3, -1]          # duplicates; an anchor outside every segment


def test_library_exports_and_header():
    from corsair_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cs_hardest_negatives", "cs_hardest_stats"):
        assert hasattr(lib, name)
        assert name in _lib.header_symbols()
    out = (ctypes.c_uint64 * 2)(7, 7)
    lib.cs_hardest_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    lib.cs_hardest_stats.restype = None
    lib.cs_hardest_stats(out, 1)
    assert list(out) == [0, 0]
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for word in ("CS_HARDNEG_MFMA", "CS_HARDNEG_STATS", '"hardneg"'):
        assert word in text


def test_trainer_options():
    from corsair_amd import train as T

    cfg = T.TrainConfig()
    assert cfg.hardest_weight == 0.0 and cfg.exclusion_radius == 0.1
    ap = T.build_parser()
    a = ap.parse_args(["--clouds-dir", "x", "--out", "y"])
    assert a.hardest_weight == 0.0 and a.exclusion_radius == 0.1
    a = ap.parse_args(["--clouds-dir", "x", "--out", "y", "--hardest-weight", "1", "--exclusion-radius", "0.2"])
    cfg = T.config_from_args(a)
    assert cfg.hardest_weight == 1.0 and cfg.exclusion_radius == 0.2


def test_pair_terms_unchanged():
    from corsair_amd import backend as B, losses

    assert losses.PAIR_TERMS == (("PiP_pairs", "base", "pos", B.PAIR_PULL), ("PiN_pairs", "base", "pos", B.PAIR_PUSH),
                                 ("NiN_pairs", "base", "neg", B.PAIR_PUSH))
