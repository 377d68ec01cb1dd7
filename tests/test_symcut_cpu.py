"""The part cut's oracle off its default path (CPU only): which Lloyd branch each input of tests/symcut_cases.py takes
(branch census of oracle/corsair_oracle.c), that counting changes no result, that the tie builders select what they
intend, and the pin against sklearn's KMeans away from n_init = 10, max_iter = 300, 50 points.  The kernels are
compared with this oracle, on the same arrays, by tests/test_gpu_symcut.py."""
import warnings

import numpy as np
import pytest

from tests import symcut_cases as C

RELOC, LABELS, TOL, CAP, SWITCH, REJECT = range(6)


def _census(native, f, x, anchors, K, n_nn=50, n_init=10, max_iter=300):
    native.symcut_census(reset=True)
    native.symcut_fit(f, x, anchors, K, n_nn, n_init, max_iter)
    return native.symcut_census(reset=True)


def test_census_counts_restarts(oracle_native):
    """Every restart leaves through exactly one of the three stops; a read without reset keeps the counts."""
    f, x, a = C.uniform()
    c = _census(oracle_native, f, x, a, 4, 50, 7, 300)
    assert c.dtype == np.int64 and c.shape == (6,)
    assert c[LABELS] + c[TOL] + c[CAP] == len(a) * 7
    assert c[SWITCH] + c[REJECT] <= len(a) * 6
    assert not oracle_native.symcut_census().any()                 # _census reset them
    oracle_native.symcut_fit(f, x, a[:3], 2, 50, 10, 300)
    first = oracle_native.symcut_census()
    assert first[LABELS] + first[TOL] + first[CAP] == 30
    assert np.array_equal(oracle_native.symcut_census(reset=True), first)
    assert not oracle_native.symcut_census().any()


def test_census_is_neutral(oracle_native):
    """Counting changes no output: the same call before a reset, after it, and with the counters far from zero."""
    f, x, a = C.three_positions()
    before = oracle_native.symcut_fit(f, x, a, 4)
    oracle_native.symcut_census(reset=True)
    after = oracle_native.symcut_fit(f, x, a, 4)
    again = oracle_native.symcut_fit(f, x, a, 4)
    assert oracle_native.symcut_census()[RELOC] > 0
    for u, v, w in zip(before, after, again):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    rows = oracle_native.symcut_nn_rows(f, x, int(a[0]), 4)
    oracle_native.symcut_census(reset=True)
    assert np.array_equal(rows, oracle_native.symcut_nn_rows(f, x, int(a[0]), 4))


# (case, K, (n_nn, n_init, max_iter), branches that must fire): what tests/test_gpu_symcut.py relies on
DEFAULT = (50, 10, 300)
CONDITIONS = [
    ("uniform16", 2, DEFAULT, (LABELS, SWITCH)), ("uniform16", 4, DEFAULT, (LABELS, SWITCH)),
    ("uniform32", 2, DEFAULT, (LABELS, SWITCH)), ("uniform32", 4, DEFAULT, (LABELS, SWITCH)),
    ("uniform16", 2, (50, 10, 1), (CAP, REJECT)), ("uniform16", 2, (50, 10, 2), (CAP, REJECT)),
    ("uniform16", 2, (50, 10, 3), (CAP, REJECT)), ("uniform32", 2, (50, 10, 1), (CAP, REJECT)),
    ("uniform16", 4, (50, 10, 1), (CAP,)), ("uniform16", 4, (50, 10, 2), (CAP,)), ("uniform16", 4, (50, 10, 3), (CAP,)),
    ("uniform16", 2, (4, 10, 300), (LABELS,)), ("uniform16", 4, (4, 10, 300), (TOL,)),
    ("uniform16", 4, (64, 10, 300), (LABELS,)), ("uniform16", 4, (7, 3, 300), (LABELS,)),
    ("uniform16", 4, (50, 1, 300), (LABELS,)), ("uniform16", 4, (50, 7, 300), (LABELS, SWITCH)),
    ("three_positions", 4, DEFAULT, (RELOC, TOL)), ("three_positions", 2, DEFAULT, (LABELS,)),
    ("identical", 2, DEFAULT, (RELOC, TOL)), ("identical", 4, DEFAULT, (RELOC, TOL)),
    ("blobs", 4, DEFAULT, (TOL, LABELS)), ("blobs_tight", 4, DEFAULT, (TOL,)),
    ("exactly_2", 2, DEFAULT, (TOL,)), ("exactly_4", 4, DEFAULT, (TOL,)),
    ("ring_and_core", 4, (50, 1, 300), (RELOC, LABELS)), ("ring_and_core", 4, DEFAULT, (RELOC, LABELS)),
]


def _case(name):
    return {"uniform16": lambda: C.uniform(dim=16), "uniform32": lambda: C.uniform(dim=32),
            "three_positions": C.three_positions, "identical": C.identical, "blobs": C.blobs,
            "blobs_tight": lambda: C.blobs(sd=3e-4), "exactly_2": lambda: C.exactly_K(2),
            "exactly_4": lambda: C.exactly_K(4), "ring_and_core": C.ring_and_core}[name]()


@pytest.mark.parametrize("name,K,cfg,fires", CONDITIONS, ids=lambda v: str(v).replace(" ", ""))
def test_census_conditions(oracle_native, name, K, cfg, fires):
    f, x, a = _case(name)
    c = _census(oracle_native, f, x, a, K, *cfg)
    print(name, K, cfg, dict(zip(oracle_native.CENSUS_EVENTS, c.tolist())))
    for b in fires:
        assert c[b] > 0, (oracle_native.CENSUS_EVENTS[b], c.tolist())
    if name == "identical":                      # K - 1 relocations in every restart, every restart stops on tol = 0
        assert c[RELOC] == (K - 1) * len(a) * cfg[1] and c[TOL] == len(a) * cfg[1]
    if name == "three_positions" and K == 4:
        assert c[RELOC] >= len(a) * cfg[1]
    if name == "ring_and_core":                  # a relocation although no two points coincide
        assert len(np.unique(x, axis=0)) == len(x) and c[RELOC] == 1


def test_degenerate_models_are_rejected_by_the_gate(oracle_native):
    """Fewer distinct positions than K: two centres coincide (min centre distance exactly 0, the reference's gate
    `> 0.15` refuses the model), every centre is finite, and with ONE position the clusters without a member at the
    final assignment make max error +inf."""
    for name, K in (("three_positions", 4), ("identical", 2), ("identical", 4)):
        f, x, a = _case(name)
        cen, cnt, mcd, mer = oracle_native.symcut_fit(f, x, a, K)
        assert np.isfinite(cen).all() and (mcd == 0.0).all(), name
        assert (cnt.sum(1) == len(x)).all()
        if name == "identical":
            assert np.isposinf(mer).all()
            assert (cnt[:, 0] == len(x)).all()
            assert np.array_equal(cen[:, :K], np.broadcast_to(x[0].astype(np.float64), (len(a), K, 3)))


@pytest.mark.parametrize("n_init", [1, 10])
def test_relocation_agrees_with_sklearn(oracle_native, n_init):
    """ring_and_core relocates an emptied cluster to a point that ties with no other (sklearn's argpartition is then
    well defined): the oracle's "farthest point from its centre" is sklearn's _relocate_empty_clusters_dense."""
    cluster = pytest.importorskip("sklearn.cluster")
    f, x, a = C.ring_and_core()
    assert _census(oracle_native, f, x, a, 4, 50, n_init, 300)[RELOC] == 1
    cen = oracle_native.symcut_fit(f, x, a, 4, 50, n_init, 300)[0][0]
    own = np.argmin(((x[:, None, :].astype(np.float64) - cen[None]) ** 2).sum(2), axis=1)
    km = cluster.KMeans(n_clusters=4, random_state=0, n_init=n_init).fit(x)
    assert np.array_equal(own, km.predict(x))
    assert np.abs(km.cluster_centers_ - cen).max() < 1e-6          # sklearn computes in f32


TIE_PARAMS = [(n, n_nn, v) for n in (256, 8193) for n_nn in (50, 20) for v in ("q2", "q1")]


@pytest.mark.parametrize("n,n_nn,variant", TIE_PARAMS)
def test_tie_blocks_select_the_intended_rows(oracle_native, n, n_nn, variant):
    """The builder's intended selection is the oracle's: ties go to the smaller row across the quarter boundaries."""
    t = C.tie_blocks(n, n_nn, variant)
    q = C.wave_quarter(n)
    rows = oracle_native.symcut_nn_rows(t.feat, t.xyz, int(t.anchors[0]), 4, n_nn)
    assert np.array_equal(rows, t.rows)
    taken = np.isin(t.block, rows)
    assert taken[t.block < q].all() and not taken[t.block >= 3 * q].any()     # quarter 0 whole, quarter 3 nothing
    in_q2 = (t.block >= 2 * q) & (t.block < 3 * q)
    assert in_q2.any() and (taken[in_q2].any() == (variant == "q2")) and not taken[in_q2].all()
    # anchor 1 sits inside the block: its n_nn nearest are the first n_nn block rows
    rows1 = oracle_native.symcut_nn_rows(t.feat, t.xyz, int(t.anchors[1]), 4, n_nn)
    assert np.array_equal(rows1, t.block[:n_nn])


def test_wide_keys_spread_over_the_first_radix_digit(oracle_native):
    f, x, a = C.wide_keys()
    d = oracle_native.dist2_matrix(f[a], f)
    assert np.isfinite(d).all()
    bins = [len(np.unique(row.view(np.uint64) >> np.uint64(56))) for row in d]
    print("occupied bins of the first radix pass per anchor:", bins)
    assert max(bins) >= 10 and (d[0] == 0.0).sum() == 6            # anchor 0 and its five copies


# ---- sklearn pin off the defaults ---------------------------------------------------------------------------------------
PIN_CONFIGS = ([("random50", 50, n_init, max_iter) for n_init, max_iter in
                ((1, 300), (3, 300), (7, 300), (10, 1), (10, 2), (10, 3))]
               + [("random%d" % m, m, 10, 300) for m in (4, 7, 50, 64)] + [("blobs", 50, 10, 300)])
N_SETS = 60


def _point_set(kind, m, i):
    rng = np.random.default_rng([11, m, i])
    if kind == "blobs":
        return C.blobs(n=m, seed=100 + i)[1]
    return rng.uniform(-0.5, 0.5, (m, 3)).astype(np.float32)


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("kind,m,n_init,max_iter", PIN_CONFIGS, ids=lambda v: str(v))
def test_symcut_kmeans_agrees_with_sklearn_off_the_defaults(oracle_native, kind, m, n_init, max_iter, K):
    """60 point sets per configuration, n_nn = n so that the selection is the whole cloud: the partition of the oracle's
    centres against KMeans(n_clusters=K, random_state=0, n_init, max_iter).fit(points).predict(points), with the
    cluster numbering, in >= 0.99 of the fits (the threshold of test_symcut_kmeans_agrees_with_sklearn; only near-ties
    may differ, sklearn computing in f32 on centred points).  Inputs with exact duplicates are not pinned: sklearn's
    relocation picks among exact ties by argpartition, which defines no order -- there the oracle's "first farthest"
    is the definition."""
    cluster = pytest.importorskip("sklearn.cluster")
    from sklearn.exceptions import ConvergenceWarning

    n_same = n_numbered = 0
    for i in range(N_SETS):
        pts = _point_set(kind, m, i)
        f = np.zeros((m, 16), np.float32)
        f[:, 0] = 1.0
        cen = oracle_native.symcut_fit(f, pts, np.zeros(1, np.int32), K, m, n_init, max_iter)[0][0, :K]
        own = np.argmin(((pts[:, None, :].astype(np.float64) - cen[None]) ** 2).sum(2), axis=1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            km = cluster.KMeans(n_clusters=K, random_state=0, n_init=n_init, max_iter=max_iter).fit(pts)
            ref = km.predict(pts)
        n_same += int(np.array_equal(own[:, None] == own[None, :], ref[:, None] == ref[None, :]))
        n_numbered += int(np.array_equal(own, ref))
    print("sklearn pin %s m=%d n_init=%d max_iter=%d K=%d: same partition %d/%d, same numbering %d/%d"
          % (kind, m, n_init, max_iter, K, n_same, N_SETS, n_numbered, N_SETS))
    assert n_numbered / N_SETS >= 0.99
