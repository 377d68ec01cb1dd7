"""Host side of the training batches (corsair_amd/training.py): instance selection follows
CategoryDataset.py:153-177, filter_data follows :92-119, and the NumPy generator restates the header's formula."""
import os
import re

import numpy as np
import pytest
from scipy import stats

from corsair_amd import training as TR
from tests import pairs_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dist(n=8, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.02, 0.5, (n, n))
    d = (a + a.T) / 2
    np.fill_diagonal(d, 0.0)
    return d


def test_rank_probabilities():
    p = TR.rank_probabilities(4)
    assert np.allclose(p, [0.4, 0.3, 0.2, 0.1]) and abs(p.sum() - 1) < 1e-12


def test_positive_selection_chi_square():
    d = _dist()
    d[0] = d[:, 0] = [0.0, 0.01, 0.05, 0.12, 0.14, 0.3, 0.4, 0.5]
    rng = np.random.default_rng(1)
    draws = np.array([TR.positive_instance(d, 0, 4, rng) for _ in range(20000)])
    rank = np.argsort(d[0])
    want = TR.rank_probabilities(4)
    obs = np.array([(draws == rank[q]).sum() for q in range(4)])
    assert obs.sum() == len(draws)   # nothing outside the top 4
    assert stats.chisquare(obs, want * len(draws)).pvalue > 1e-3
    assert (draws == 0).sum() > 0.3 * len(draws)   # the anchor itself is the most likely positive (reference quirk)


def test_positive_selection_caps_at_valid():
    d = _dist()
    d[0] = d[:, 0] = [0.0, 0.01, 0.3, 0.3, 0.3, 0.3, 0.4, 0.5]
    rng = np.random.default_rng(2)
    assert {TR.positive_instance(d, 0, 6, rng) for _ in range(500)} <= {0, 1}


def test_negative_selection_skips_rank0_chi_square():
    d = _dist()
    d[0] = d[:, 0] = [0.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.25, 0.1]
    rng = np.random.default_rng(3)
    draws = np.array([TR.negative_instance(d, 0, 3, rng) for _ in range(20000)])
    assert not np.any(draws == 1)   # rank 0 (the farthest) is never drawn (reference quirk)
    want = TR.rank_probabilities(3)
    obs = np.array([(draws == c).sum() for c in (2, 3, 4)])
    assert obs.sum() == len(draws)
    assert stats.chisquare(obs, want * len(draws)).pvalue > 1e-3


def test_filter_data_shrinks():
    d = np.full((5, 5), 0.5)
    np.fill_diagonal(d, 0.0)
    d[0, 1] = d[1, 0] = d[0, 2] = d[2, 0] = d[1, 2] = d[2, 1] = 0.1
    d[3, 4] = d[4, 3] = 0.1   # 3 and 4 have only two entries <= 0.15 each
    pcs = [np.full((2, 3), i, np.float32) for i in range(5)]
    dm, p, sym, kept = TR.filter_data(d, pcs, [1, 2, 3, 4, 5])
    assert kept.tolist() == [0, 1, 2] and dm.shape == (3, 3) and sym == [1, 2, 3]
    assert [int(x[0, 0]) for x in p] == [0, 1, 2]


def test_filter_data_unchanged():
    d = np.zeros((4, 4))
    pcs = [np.zeros((1, 3), np.float32)] * 4
    dm, p, sym, kept = TR.filter_data(d, pcs, None)   # the reference raises UnboundLocalError here
    assert dm is not None and np.array_equal(dm, d) and len(p) == 4 and sym is None and kept.tolist() == [0, 1, 2, 3]


def test_slot_generator_is_keyed():
    a = TR.slot_rng(7, 3, 0).uniform(size=4)
    assert np.array_equal(a, TR.slot_rng(7, 3, 0).uniform(size=4))
    assert not np.array_equal(a, TR.slot_rng(7, 3, 1).uniform(size=4))
    assert not np.array_equal(a, TR.slot_rng(7, 4, 0).uniform(size=4))
    assert not np.array_equal(a, TR.slot_rng(8, 3, 0).uniform(size=4))


def test_counter_generator_matches_header_formula():
    with open(os.path.join(ROOT, "include", "corsair_hip.h")) as f:
        header = f.read()
    for const in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB",
                  "slot << 40 | round << 36 | stream << 32 | ctr"):
        assert const in header
    with open(os.path.join(ROOT, "corsair_amd", "csrc", "common.h")) as f:
        common = f.read()
    assert re.search(r"x \^ \(x >> 30\)\) \* 0xBF58476D1CE4E5B9", common)
    for seed, slot, rnd, stream in [(0, 0, 0, 0), (12345, 31, 15, 2), ((1 << 64) - 1, (1 << 24) - 1, 3, 1)]:
        ctr = np.array([0, 1, 2, 1000, (1 << 32) - 1], np.uint64)
        got = PR.rng_u64(seed, slot, rnd, stream, ctr)
        for c, g in zip(ctr.tolist(), got.tolist()):
            j = (slot << 40) | (rnd << 36) | (stream << 32) | c
            assert g == PR.rng_u64_int(seed, j)


def test_random_pose_is_rigid():
    T = TR.random_pose(TR.slot_rng(1, 2, 3))
    R = T[:3, :3]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1) < 1e-12
    assert np.all(np.abs(T[:3, 3]) <= 0.5) and np.array_equal(T[3], [0, 0, 0, 1])


@pytest.mark.parametrize("name", ["cs_radius_pairs", "cs_radius_pairs_fill", "cs_radius_plan_free", "cs_sample_pairs",
                                  "cs_transform_f64"])
def test_new_symbols_declared(name):
    from corsair_amd import _lib

    assert name in _lib.header_symbols()
