"""CPU-side checks of the FPFH specification (include/corsair_hip.h: cs_fpfh, cs_orient_normals) through its
restatement tests/fpfh_ref.py: against an independent float implementation (cKDTree, arctan2, np.add.at) written here, the
invariance the orientation entry exists for, the edge cases of the header, and the ABI."""
import math
import os

import numpy as np
import pytest

from tests import fpfh_ref as FR
from tests.icp_ref import fma

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _voxelize(pc, voxel):
    """first point per voxel, input order"""
    g = np.floor(pc.astype(np.float64) / voxel).astype(np.int64)
    _, idx = np.unique(g, axis=0, return_index=True)
    return pc[np.sort(idx)]


def _real_cloud(i, voxel):
    z = np.load(os.path.join(GOLD, "real_clouds10.npz"))
    pc = z["clouds"][i].astype(np.float32)
    pc = pc - pc.mean(0)
    pc = (pc / np.max(np.linalg.norm(pc, 2, 1))).astype(np.float32)
    return _voxelize(pc, voxel)


def _shapes():
    """a box, a sphere and a cylinder, a few hundred surface points each"""
    rng = np.random.default_rng(5)
    n = 400
    face = rng.integers(0, 6, n)
    u = rng.uniform(-0.5, 0.5, (n, 3))
    box = u.copy()
    box[np.arange(n), face % 3] = np.where(face < 3, -0.5, 0.5)
    box *= (1.0, 0.6, 0.4)
    v = rng.normal(size=(n, 3))
    sphere = 0.5 * v / np.linalg.norm(v, axis=1, keepdims=True)
    th, h = rng.uniform(0, 2 * np.pi, n), rng.uniform(-0.5, 0.5, n)
    cyl = np.stack([0.3 * np.cos(th), h, 0.3 * np.sin(th)], 1)
    return {"box": box.astype(np.float32), "sphere": sphere.astype(np.float32), "cylinder": cyl.astype(np.float32)}


def _pca_normals(pc, k=12):
    """plain float normals (smallest eigenvector of the k-NN covariance), oriented away from the centroid"""
    from scipy.spatial import cKDTree

    p = pc.astype(np.float64)
    _, nb = cKDTree(p).query(p, k)
    q = p[nb] - p[nb].mean(1, keepdims=True)
    _, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", q, q))
    nrm = vec[:, :, 0]
    flip = np.einsum("ni,ni->n", nrm, p - p.mean(0)) < 0
    nrm[flip] = -nrm[flip]
    return nrm.astype(np.float32)


# ---- the independent float implementation: not derived from the restatement ---------------------------------------------
def float_neighbours(pc, radius, max_nn):
    from scipy.spatial import cKDTree

    p = pc.astype(np.float64)
    tree = cKDTree(p)
    lists = []
    for i, nb in enumerate(tree.query_ball_point(p, radius * (1 + 1e-9))):
        nb = np.asarray([j for j in nb if j != i], np.int64)
        d2 = ((p[nb] - p[i]) ** 2).sum(1) if len(nb) else np.zeros(0)
        keep = d2 < radius * radius
        nb, d2 = nb[keep], d2[keep]
        o = np.lexsort((nb, d2))[:max_nn - 1]
        lists.append((nb[o], d2[o]))
    return lists


def float_fpfh(pc, nrm, radius, max_nn):
    p, n = pc.astype(np.float64), nrm.astype(np.float64)
    lists = float_neighbours(pc, radius, max_nn)
    N = len(p)
    I = np.concatenate([np.full(len(nb), i) for i, (nb, _) in enumerate(lists)]).astype(np.int64)
    J = np.concatenate([nb for nb, _ in lists]).astype(np.int64)
    D2 = np.concatenate([d for _, d in lists])
    dp = p[J] - p[I]
    ln = np.sqrt(D2)
    with np.errstate(all="ignore"):
        a1 = np.einsum("ni,ni->n", n[I], dp) / ln
        a2 = np.einsum("ni,ni->n", n[J], dp) / ln
        sw = np.arccos(np.clip(np.abs(a1), 0, 1)) > np.arccos(np.clip(np.abs(a2), 0, 1))
        n1 = np.where(sw[:, None], n[J], n[I])
        n2 = np.where(sw[:, None], n[I], n[J])
        dp = np.where(sw[:, None], -dp, dp)
        f2 = np.where(sw, -a2, a1)
        v = np.cross(dp, n1)
        vl = np.linalg.norm(v, axis=1)
        v = v / vl[:, None]
        w = np.cross(n1, v)
        f1 = np.einsum("ni,ni->n", v, n2)
        f0 = np.arctan2(np.einsum("ni,ni->n", w, n2), np.einsum("ni,ni->n", n1, n2))
    bad = ~((ln > 0) & (vl > 0) & np.isfinite(f0) & np.isfinite(f1) & np.isfinite(f2))
    f0, f1, f2 = (np.where(bad, 0.0, f) for f in (f0, f1, f2))
    b0 = np.clip(np.floor(11 * (f0 + np.pi) / (2 * np.pi)), 0, 10).astype(np.int64)
    b1 = np.clip(np.floor(11 * (f1 + 1.0) * 0.5), 0, 10).astype(np.int64)
    b2 = np.clip(np.floor(11 * (f2 + 1.0) * 0.5), 0, 10).astype(np.int64)
    m = np.bincount(I, minlength=N).astype(np.float64)
    spfh = np.zeros((N, 33))
    inc = 100.0 / m[I]
    np.add.at(spfh, (I, b0), inc)
    np.add.at(spfh, (I, 11 + b1), inc)
    np.add.at(spfh, (I, 22 + b2), inc)
    acc = np.zeros((N, 33))
    on = D2 > 0
    np.add.at(acc, I[on], spfh[J[on]] / D2[on, None])
    s = acc.reshape(N, 3, 11).sum(2)
    scale = np.where(s != 0, 100.0 / np.where(s != 0, s, 1.0), 1.0)
    return acc * np.repeat(scale, 11, axis=1) + spfh, lists


def _compare(pc, nrm, radius, max_nn):
    """(share of rows with an element off by more than 1e-6 relative, rows); asserts the lists and the 1e-9 bound"""
    want, lists = float_fpfh(pc, nrm, radius, max_nn)
    ref_lists = [FR.neighbours(pc, i, radius, max_nn) for i in range(len(pc))]
    for i, (nb, _) in enumerate(lists):
        assert [j for _, j in ref_lists[i]] == nb.tolist(), i
    # the restatement before its one cast, element by element relative to the float implementation's value (a bin both
    # leave empty is an exact zero on both sides; 1e-12 absolute covers the sums' last bits on the near-empty ones)
    got = FR.fpfh_segment(pc, nrm, radius, max_nn, ref_lists, cast=False)
    err = np.abs(got - want)
    off = (err > 1e-6 * np.abs(want) + 1e-12).any(axis=1)
    assert (err[~off] <= 1e-9 * np.abs(want[~off]) + 1e-12).all()
    return float(off.mean()), len(pc)


@pytest.mark.parametrize("max_nn", [32, 128])
def test_restatement_matches_float_implementation_on_a_real_cloud(max_nn):
    pc = _real_cloud(3, 0.05)            # 1836 rows, the smallest of the ten at this voxel size
    share, n = _compare(pc, _pca_normals(pc), 0.2, max_nn)
    print("real cloud: rows %d, share of rows off by more than 1e-6: %.5f" % (n, share))
    assert share <= 0.001


@pytest.mark.parametrize("name", ["box", "sphere", "cylinder"])
def test_restatement_matches_float_implementation_on_shapes(name):
    pc = _shapes()[name]
    share, n = _compare(pc, _pca_normals(pc), 0.2, 32)
    print("%s: rows %d, share %.5f" % (name, n, share))
    assert share <= 0.001


def test_exact_fma_is_the_rational_fma():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        a, b, c = rng.normal(size=3) * 10.0 ** rng.integers(-6, 6, 3)
        assert FR.exact_fma(a, b, c) == fma(a, b, c)
    for a, b, c in [(0.1, 0.1, -0.01), (1e-200, 1e-200, 1.0), (3.0, 0.0, -0.0), (1 + 2 ** -30, 1 - 2 ** -30, -1.0)]:
        assert FR.exact_fma(a, b, c) == fma(a, b, c)


def test_angle_bins_equal_atan2_bins():
    rng = np.random.default_rng(1)
    x, y = rng.normal(size=200000), rng.normal(size=200000)
    got = FR._bin_angle(x, y)
    want = np.clip(np.floor(11 * (np.arctan2(y, x) + np.pi) / (2 * np.pi)), 0, 10).astype(np.int64)
    assert (got != want).mean() < 1e-5              # they differ only within an ulp of a boundary
    # the stated cases
    assert FR._bin_angle(np.array([1.0, -1.0, -1.0, 0.0]), np.array([0.0, 0.0, -0.0, 0.0])).tolist() == [5, 10, 10, 5]
    # on a boundary direction itself: the boundary is not above the angle
    c, s = FR.BOUNDS[2]
    assert FR._bin_angle(np.array([c]), np.array([s]))[0] in (2, 3)


# ---- invariance: why cs_orient_normals exists ----------------------------------------------------------------------------
def test_descriptor_is_invariant_with_centroid_oriented_normals_only():
    from tests import normals_ref as NR

    pc = _real_cloud(1, 0.06)[:700]
    # a signed permutation matrix (a proper rotation) and a dyadic translation: the moved coordinates are exact
    Rm = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float32)
    assert round(float(np.linalg.det(Rm))) == 1
    t = np.array([0.25, -0.5, 0.125], np.float32)
    moved = (pc @ Rm.T + t).astype(np.float32)
    off = [0, len(pc)]
    n0 = NR.estimate_normals(pc, off, 12)
    n1 = NR.estimate_normals(moved, off, 12)
    f0 = FR.fpfh(pc, FR.orient_normals(pc, off, n0), off, 0.25, 64)
    f1 = FR.fpfh(moved, FR.orient_normals(moved, off, n1), off, 0.25, 64)
    assert np.abs(f0 - f1).max() <= 1e-4 * 200.0          # 1e-4 of the descriptor's range [0, 200]
    g0 = FR.fpfh(pc, n0, off, 0.25, 64)
    g1 = FR.fpfh(moved, n1, off, 0.25, 64)
    assert np.abs(g0 - g1).max() > 10.0                   # the pose-dependent sign rule: not the same descriptor


# ---- edge cases ----------------------------------------------------------------------------------------------------------
def _lattice(n):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_strict_threshold_on_an_integer_lattice():
    pc = _lattice(4)
    centre = int(np.nonzero((pc == (1, 1, 1)).all(1))[0][0])
    assert len(FR.neighbours(pc, centre, 1.0, 128)) == 0           # the six rows AT the radius do not qualify
    assert len(FR.neighbours(pc, centre, 1.0 + 2 ** -20, 128)) == 6
    nb = FR.neighbours(pc, centre, 1.5, 128)                        # 6 at d2 = 1, 12 at d2 = 2; ties by the row
    assert [d for d, _ in nb] == [1.0] * 6 + [2.0] * 12
    assert [j for _, j in nb[:6]] == sorted(j for _, j in nb[:6])


def test_max_nn_truncates_to_the_nearest():
    pc = _lattice(4)
    centre = int(np.nonzero((pc == (1, 1, 1)).all(1))[0][0])
    full = FR.neighbours(pc, centre, 1.5, 128)
    assert FR.neighbours(pc, centre, 1.5, 4) == full[:3]
    assert FR.neighbours(pc, centre, 1.5, 9) == full[:8]


def test_degenerate_pairs_and_lonely_rows():
    pc = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [50, 0, 0], [0.5, 0.5, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 1], [np.nan, 0, 0]], np.float32)
    lists = [FR.neighbours(pc, i, 2.0, 16) for i in range(5)]
    counts, m = FR.spfh_counts(pc, nrm, lists)
    assert m.tolist() == [3, 3, 3, 0, 3]
    # row 0: the duplicate (d2 = 0) and the NaN normal are degenerate: bins 5 / 5 / 5
    assert counts[0, 5] >= 2 and counts[0, 16] >= 2 and counts[0, 27] >= 2
    # row 2 against rows 0 / 1: dp is parallel to its normal n1 = (1, 0, 0): |dp x n1| = 0, degenerate
    assert counts[2, 5] == 3
    out = FR.fpfh(pc, nrm, [0, 5], 2.0, 16)
    assert np.isfinite(out).all()
    assert (out[3] == 0).all()                                     # no neighbour: zeros
    assert abs(float(out[0, :11].sum()) - 200.0) < 1e-3            # 100 from the weighted sum, 100 of its own


def test_centroid_is_exact_and_order_free():
    rng = np.random.default_rng(2)
    pc = (rng.normal(size=(500, 3)) * 3).astype(np.float32)
    pc[7] = (np.nan, 0, 0)
    pc[9] = (40000.0, 0, 0)
    c = FR.centroid(pc)
    assert FR.centroid(pc[rng.permutation(500)]) == c
    ok = np.delete(np.arange(500), [7, 9])
    assert np.allclose(c, pc[ok].astype(np.float64).mean(0), atol=2e-5)
    assert FR.centroid(np.full((3, 3), np.inf, np.float32)) is None


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_are_exported_and_declared():
    from corsair_amd import _lib

    declared = _lib.header_symbols()
    lib = _lib.load()
    for name in ("cs_orient_normals", "cs_fpfh", "cs_fpfh_stats"):
        assert name in declared, name
        assert hasattr(lib, name), name
