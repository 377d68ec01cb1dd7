"""DBSCAN on raw scans, the part that needs no GPU: tests/dbscan_ref.py -- the restatement the GPU tests compare
with -- against scikit-learn, the patch fixture's numbers, the canonical numbering, the edge cases of the rule, the
configuration and the source layout."""
import glob
import os
import re

import numpy as np
import pytest

from tests import dbscan_cases as DC
from tests import dbscan_ref as ref
from tests import outlier_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = DC.VOXEL
PARAMS = ((2.5, 5), (2.5, 10), (2.0, 6))           # (eps in voxels, min_points)
_runs = {}


def _run(i, eps_v, mp):
    """the restatement on fixture i, computed once"""
    key = (i, eps_v, mp)
    if key not in _runs:
        xyz, _ = DC.patch_cloud(i)
        _runs[key] = ref.dbscan(xyz, [0, len(xyz)], eps_v * V, mp)
    return _runs[key]


@pytest.mark.parametrize("i", DC.CLOUDS)
def test_restatement_against_sklearn(i):
    from scipy.spatial import cKDTree
    from sklearn.cluster import DBSCAN

    xyz, _ = DC.patch_cloud(i)
    c = xyz.astype(np.float64)
    tree = cKDTree(c)
    for eps_v, mp in PARAMS:
        eps = eps_v * V
        # the gap that makes the comparison safe: no pair distance within 1e-8 of eps, so sklearn's d <= eps (1 - 1e-9) and
        # the header's d2 < eps * eps select the same pairs
        pairs = tree.query_pairs(eps * 1.01, output_type="ndarray")
        dist = np.linalg.norm(c[pairs[:, 0]] - c[pairs[:, 1]], axis=1)
        gap = float(np.abs(dist - eps).min())
        print("cloud %d eps %.1f voxels: smallest gap of a pair distance to eps %.3g" % (i, eps_v, gap))
        assert gap > 1e-8
        sk = DBSCAN(eps=eps * (1 - 1e-9), min_samples=mp).fit(c)
        label, count, core = _run(i, eps_v, mp)
        sk_core = np.zeros(len(c), bool)
        sk_core[sk.core_sample_indices_] = True
        assert np.array_equal(core, sk_core)
        assert ref.same_partition(label[core], sk.labels_[core]) and (label[core] >= 0).all()
        # border rows: the rule differs from sklearn's on purpose.  Each one's cluster is that of its NEAREST core row
        # inside eps; a row without a core row inside eps is noise in both
        nbr = ref.neighbours(xyz, eps)
        for r in np.nonzero(~core)[0]:
            cores = [j for j in nbr[r] if core[j]]
            assert (label[r] >= 0) == bool(cores) == (sk.labels_[r] >= 0)
            if cores:
                d2 = [oref.d2_exact(c, r, j) for j in cores]
                assert max(d2) < eps * eps
                assert label[r] == label[cores[int(np.argmin(d2))]]        # argmin: the first minimum, the smaller row


@pytest.mark.parametrize("i", DC.CLOUDS)
def test_patch_fixture_table(i):
    """The numbers of the fixture: the radius filter keeps every patch row, the largest cluster keeps the real rows alone."""
    xyz, kind = DC.patch_cloud(i)
    n = len(xyz)
    assert n == DC.ROWS[i] and (kind == DC.REAL).sum() == DC.OC.ROWS[i][0] and (kind == DC.CLUTTER).sum() == DC.OC.ROWS[i][1]
    sizes, noise, border, border10 = DC.TABLE[i]
    assert (kind == DC.PATCH).sum() == sizes[1] == int(0.12 * sizes[0])
    from scipy.spatial import cKDTree

    gap = cKDTree(xyz[kind == DC.REAL].astype(np.float64)).query(xyz[kind == DC.PATCH].astype(np.float64))[0].min() / V
    print("cloud %d: the patch lies %.2f voxels from the real rows" % (i, gap))
    assert 5.9 < gap < 7.1
    rkeep, _ = oref.outlier_radius(xyz, [0, n], 2.5 * V, 4)
    assert rkeep[kind == DC.PATCH].all()                                   # the reason for the feature
    label, count, core = _run(i, 2.5, 5)
    assert np.array_equal(count, oref.radius_count(xyz, [0, n], 2.5 * V))
    assert tuple(np.bincount(label[label >= 0])) in (sizes, sizes[::-1])
    assert (label < 0).sum() == noise and ((label >= 0) & ~core).sum() == border
    keep, stat = ref.cluster_largest(label, [0, n])
    assert stat.tolist() == [[2, int(label[kind == DC.REAL][0]), sizes[0]]]
    assert keep[kind == DC.REAL].all() and not keep[kind != DC.REAL].any()
    label10, _, core10 = _run(i, 2.5, 10)
    assert ((label10 >= 0) & ~core10).sum() == border10
    if i == 5:
        assert sorted(np.bincount(label10[label10 >= 0]).tolist()) == [5, 184, 1530]


def test_canonical_numbering_and_permutation():
    xyz, _ = DC.patch_cloud(5)
    n = len(xyz)
    label, count, core = _run(5, 2.5, 10)
    first = [int(np.nonzero(core & (label == c))[0][0]) for c in range(int(label.max()) + 1)]
    assert first == sorted(first) and len(first) == 3           # ids ascend with the smallest core row
    perm = np.random.default_rng(3).permutation(n)
    plabel, pcount, pcore = ref.dbscan(xyz[perm], [0, n], 2.5 * V, 10)
    assert np.array_equal(pcount, count[perm]) and np.array_equal(pcore, core[perm])
    assert ref.same_partition(plabel, label[perm])              # (no border row of this fixture sits at an exact tie)
    rlabel, _, rcore = ref.dbscan(xyz[::-1], [0, n], 2.5 * V, 10)
    assert ref.same_partition(rlabel, label[::-1])
    rfirst = [int(np.nonzero(rcore & (rlabel == c))[0][0]) for c in range(3)]
    assert rfirst == sorted(rfirst)
    # a reversed segment renumbers the clusters: the cluster that holds the first core row is cluster 0
    # (fixture 3 at 2.5 / 5 has no border row and its noise rows see no core row: leaving them out changes no count)
    xyz, _ = DC.patch_cloud(3)
    label, _, _ = _run(3, 2.5, 5)
    small, big = (1, 0) if (label == 0).sum() == 1082 else (0, 1)
    two = np.concatenate([xyz[label == small], xyz[label == big]])
    tlabel, _, _ = ref.dbscan(two, [0, len(two)], 2.5 * V, 5)
    assert tlabel.tolist() == [0] * 129 + [1] * 1082
    tlabel, _, _ = ref.dbscan(two[::-1], [0, len(two)], 2.5 * V, 5)
    assert tlabel.tolist() == [0] * 1082 + [1] * 129


def _lattice(m, spacing):
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)
    return (g * spacing).astype(np.float32)


def tie_case(a_first):
    """(f32 [14,3], labels at eps 1.1 / 4 points).  Unit stars: X1 = (-1, 0, 0) and A = (0, 0, 0) are linked core rows, B =
    (2, 0, 0) is the core row of a second cluster and row 9 = (1, 0, 0) lies at d2 = 1 exactly from A and from B; every
    other row is a border row of one star.  X1 is row 0, so its cluster is 0; B is row 4 and A row 10, or with a_first the
    other way round."""
    x1 = [[-1, 0, 0], [-2, 0, 0], [-1, 1, 0], [-1, -1, 0]]
    a = [[0, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]]
    b = [[2, 0, 0], [3, 0, 0], [2, 1, 0], [2, -1, 0], [2, 0, 1]]
    mid = [[1, 0, 0]]
    if a_first:
        return np.float32(x1 + a + [[0, 0, -1]] + mid + b[:4]), [0] * 10 + [1] * 4
    return np.float32(x1 + b + mid + a), [0] * 4 + [1] * 5 + [1] + [0] * 4


def test_edge_cases_of_the_rule():
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 1, (60, 3)).astype(np.float32)
    pts[17] = [9, 9, 9]
    label, count, core = ref.dbscan(pts, [0, 60], 0.3, 1)       # min_points = 1: every finite row is core
    assert core.all() and (label >= 0).all() and count[17] == 1
    assert (label == label[17]).sum() == 1                      # the isolated row is its own cluster
    label, count, core = ref.dbscan(pts, [0, 60], 0.3, 61)      # more than the segment holds
    assert not core.any() and (label == -1).all()
    dup = np.tile(np.float32([[0.25, -1.0, 3.0]]), (7, 1))      # k copies of one point
    label, count, core = ref.dbscan(dup, [0, 7], 1e-3, 7)
    assert count.tolist() == [7] * 7 and label.tolist() == [0] * 7
    label, _, _ = ref.dbscan(dup, [0, 7], 1e-3, 8)
    assert label.tolist() == [-1] * 7
    lat = _lattice(4, 0.5)                                      # spacing exactly eps: the threshold is strict
    label, count, core = ref.dbscan(lat, [0, 64], 0.5, 1)
    assert count.tolist() == [1] * 64 and label.tolist() == list(range(64))
    label, count, core = ref.dbscan(lat, [0, 64], 0.5 * (1 + 2.0 ** -20), 2)
    assert count.max() == 7 and count.min() == 4 and label.tolist() == [0] * 64
    # a border row at equal d2 from core rows of two clusters takes the smaller ROW's cluster, not the smaller id's
    both, want = tie_case(False)
    label, count, core = ref.dbscan(both, [0, len(both)], 1.1, 4)
    assert np.nonzero(core)[0].tolist() == [0, 4, 10] and count[9] == 3
    assert label.tolist() == want and label[9] == 1             # row 4 (cluster 1) beats row 10 (cluster 0)
    both, want = tie_case(True)
    label, _, _ = ref.dbscan(both, [0, len(both)], 1.1, 4)
    assert label.tolist() == want and label[9] == 0
    a = np.float32([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0]])          # four rows that see one another
    bad = np.concatenate([a, np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0.25, 0.25, -np.inf]])])
    label, count, core = ref.dbscan(bad, [0, 7], 1.3, 4)
    assert label.tolist() == [0] * 4 + [-1] * 3 and count.tolist() == [4] * 4 + [0] * 3
    label, count, _ = ref.dbscan(bad, [0, 7], 1e160, 4)         # eps * eps overflows: every finite row is linked
    assert label.tolist() == [0] * 4 + [-1] * 3 and count.tolist() == [4] * 4 + [0] * 3
    label, count, _ = ref.dbscan(bad, [0, 7], 1e-170, 1)        # eps * eps underflows: not even the row itself
    assert label.tolist() == [-1] * 7 and not count.any()
    # cluster_largest: ties go to the smaller id, labels out of range count as -1, no cluster gives (0, -1, 0)
    lab = np.int32([1, 1, 0, 0, -1, 2, 8, -5] + [-1, -1] + [] + [3, 3, 3, 0])
    keep, stat = ref.cluster_largest(lab, [0, 8, 10, 10, 14])
    assert stat.tolist() == [[3, 0, 2], [0, -1, 0], [0, -1, 0], [2, 3, 3]]
    assert keep.tolist() == [False, False, True, True, False, False, False, False, False, False, True, True, True, False]


def test_config_parser_and_readme():
    from corsair_amd import harness as H

    assert H.SCAN_FILTERS == ("none", "statistical", "radius", "cluster")
    c = H.Config()
    assert (c.scan_filter, c.scan_filter_eps, c.scan_filter_min_points) == ("none", 2.5, 5)
    assert c.scan_filter_eps == c.scan_filter_radius and c.scan_filter_min_points == c.scan_filter_min_nb + 1
    H.Config(scan_filter="cluster", scan_filter_eps=0.5, scan_filter_min_points=1).check_scan_filter()
    for kw, word in ((dict(scan_filter_eps=0.0), "scan_filter_eps"), (dict(scan_filter_eps=-1.0), "scan_filter_eps"),
                     (dict(scan_filter_eps=float("nan")), "scan_filter_eps"),
                     (dict(scan_filter_eps=float("inf")), "scan_filter_eps"),
                     (dict(scan_filter_min_points=0), "scan_filter_min_points"),
                     (dict(scan_filter_min_points=2.5), "scan_filter_min_points"),
                     (dict(scan_filter_min_points=True), "scan_filter_min_points")):
        with pytest.raises(ValueError, match=word):
            H.Config(**kw).check_scan_filter()
    base = ["--checkpoint", "c", "--catalog-dir", "a", "--query-dir", "b"]
    a = H.build_parser().parse_args(base)
    assert (a.scan_filter, a.scan_filter_eps, a.scan_filter_min_points) == ("none", 2.5, 5)
    a = H.build_parser().parse_args(base + ["--scan-filter", "cluster", "--scan-filter-eps", "3", "--scan-filter-min-points", "8"])
    assert (a.scan_filter, a.scan_filter_eps, a.scan_filter_min_points) == ("cluster", 3.0, 8)
    help_text = " ".join(H.build_parser().format_help().split())
    assert help_text.count("untuned, no real scan measured") >= 2
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "--scan-filter cluster" in readme and "untuned" in readme
    at = readme.index("--scan-filter cluster")
    assert "untuned, no real scan measured" in readme[at:at + 3000]


def assert_one_cell_grid():
    """dbscan.hip probes the grid that normals.hip builds through the shared headers: it defines no probe, no table
    builder and no distance chain or count kernel of its own, and the count kernels are defined once, in outlier_count.h."""
    csrc = os.path.join(ROOT, "corsair_amd", "csrc")
    text = {os.path.basename(p): open(p).read() for ext in ("*.h", "*.hip") for p in glob.glob(os.path.join(csrc, ext))}
    db = text["dbscan.hip"]
    for inc in ('#include "cellgrid.h"', '#include "normals_grid.h"', '#include "outlier_count.h"'):
        assert inc in db
    assert "nrm_grid_build(" in db and db.count("cg_probe<3>(") == 2 and "k_out_count_grid" in db
    for word in ("cg_lookup", "cg_cell", "hash64", "pack_key", "kEmptyKey", "DeviceRadixSort", "cellgrid_insert_ranges",
                 "cellgrid_table_fill", "floor("):
        assert word not in db, word
    kernels = re.findall(r"^__global__ [^\n]*?void (k_\w+)\(", db, flags=re.M)
    assert sorted(kernels) == sorted(["k_db_init", "k_db_hook", "k_db_hook_grid", "k_db_compress", "k_db_number",
                                      "k_db_border", "k_db_border_grid", "k_cl_sizes", "k_cl_max", "k_cl_finish",
                                      "k_cl_keep"])
    defs = {n: re.findall(r"void (k_out_count\w*)\(", t) for n, t in text.items()}
    assert {n: d for n, d in defs.items() if d} == {"outlier_count.h": ["k_out_count", "k_out_count_grid"]}
    assert {n for n, t in text.items() if re.search(r"double out_d2\(", t)} == {"outlier_count.h"}
    # no thread waits for another: no cooperative launch, no grid-wide barrier
    for word in ("hipLaunchCooperativeKernel", "cooperative_groups", "grid.sync", "__threadfence"):
        assert word not in db, word
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "dbscan.hip" in make and "dbscan.o: nn_common.h cellgrid.h normals_grid.h outlier_count.h" in make
    assert "outlier.o: outlier_count.h" in make


def test_source_layout():
    assert_one_cell_grid()
    header = open(os.path.join(ROOT, "include", "corsair_hip.h")).read()
    for name in ("int cs_dbscan(", "int cs_cluster_largest(", "void cs_dbscan_stats("):
        assert name in header
    assert "DELIBERATE DIFFERENCE" in header and '"cluster"' in header
