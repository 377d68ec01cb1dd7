"""The stale-memory schedules and their edge cases (tests/test_gpu_stale_memory.py; the proxy alone:
tests/test_stale_proxy_cpu.py).

The suite calls every operator repeatedly at the same shapes, so a recycled scratch block and a recycled torch allocation
usually hold a VALID result of the same problem: a counter that is not cleared, a table that is not filled with its empty
marker, an output element that is never written all go unnoticed.  Three kinds of schedule make such a mistake change the
result.  Each runs a whole case of tests/stream_cases.py -- its set-up stage included -- on the default stream and must
give the bits of the plain schedule (SC.run_plain):

  scratch-00 / scratch-ff   cs_pool_poison(0x00 / 0xFF): every block the library's pool hands out is filled with the byte
                            first.  The two values are the ones scratch is legitimately initialised to (0x00: a cleared
                            counter or flag; 0xFF: kEmptyKey, -1, a NaN), so whatever byte a kernel expects to find differs
                            from at least one of them.
  outputs-00 / outputs-ff   corsair_amd.backend sees a `torch` whose empty / empty_like fill the new tensor with the byte:
                            an output element the kernels do not write differs under at least one of the two.
  decoy-first               the whole case runs once on its decoy draw (seed + 1000: the same shapes, other valid values)
                            and the result is dropped; then the plain schedule.  Whatever survives a call -- pool blocks,
                            download buffers, count slots, counters -- now holds values of ANOTHER problem.

The edge cases at the end exist for this module alone: variants of the stream cases in which a kernel legitimately writes
nothing for a part of the batch (an empty segment, a problem without pairs, an anchor without an admissible row).  No oracle
pins their bits, so each carries a metamorphic relation: the live parts equal, bit for bit, the same call on the batch
without the empty parts, and the empty parts hold what include/corsair_hip.h documents.
"""
import contextlib
import ctypes

import numpy as np
import torch

from tests import stream_cases as SC

PATTERNS = {"00": 0x00, "ff": 0xFF}
SCHEDULES = ["scratch-00", "scratch-ff", "outputs-00", "outputs-ff", "decoy-first"]


# ---- the pool hooks ----------------------------------------------------------------------------------------------
def _lib():
    from corsair_amd import _lib as L

    return L.load()


@contextlib.contextmanager
def pool_poison(pattern):
    """cs_pool_poison(pattern) for the block, off again afterwards whatever happens."""
    lib = _lib()
    lib.cs_pool_poison(int(pattern))
    try:
        yield
    finally:
        lib.cs_pool_poison(-1)


def poison_stats(reset=False):
    """(blocks, bytes) poisoned since the last reset."""
    out = (ctypes.c_uint64 * 2)()
    _lib().cs_pool_poison_stats(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


def pool_peek(nbytes, device):
    """The bytes a kernel would find in a scratch block of `nbytes` (uint8 ndarray)."""
    from corsair_amd import _lib as L

    out = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    L.check(_lib().cs_pool_peek(nbytes, L.ptr(out), L.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- the torch proxy ---------------------------------------------------------------------------------------------
class PoisonTorch:
    """Stands in for the module `torch` inside corsair_amd.backend: every attribute is torch's own, except empty and
    empty_like, which fill the bytes of the tensor they return with `pattern` (on the current stream for a device tensor),
    whatever its dtype and also when it has no element.  Counts what it poisoned."""

    def __init__(self, pattern):
        assert 0 <= int(pattern) <= 255
        self._pattern, self.count, self.bytes = int(pattern), 0, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def _poison(self, t):
        # a uint8 view of the new tensor's whole storage: any dtype, any layout, 0-d and zero-size tensors alike
        raw = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
        assert raw.numel() >= t.numel() * t.element_size()
        raw.fill_(self._pattern)
        self.count += 1
        self.bytes += raw.numel()
        return t

    def empty(self, *args, **kwargs):
        return self._poison(torch.empty(*args, **kwargs))

    def empty_like(self, *args, **kwargs):
        return self._poison(torch.empty_like(*args, **kwargs))


@contextlib.contextmanager
def poisoned_outputs(monkeypatch, B, pattern):
    """B.torch is a PoisonTorch for the block (and nothing else is patched); yields the proxy."""
    proxy = PoisonTorch(pattern)
    with monkeypatch.context() as m:
        m.setattr(B, "torch", proxy)
        yield proxy


# ---- the schedules -----------------------------------------------------------------------------------------------
def decoy_of(case):
    """The same case on its decoy draw."""
    return SC.Case(case.name, case.make, case.op, case.env, case.seed + 1000, case.setup, case.ready)


def run_schedule(B, case, device, schedule, monkeypatch):
    """(snapshot, info) of the case under `schedule`; info = {"blocks", "bytes"} poisoned in the pool for a scratch
    schedule, {"allocations", "bytes"} poisoned by the proxy for an outputs schedule, {} for decoy-first."""
    kind, _, pat = schedule.partition("-")
    if kind == "scratch":
        poison_stats(reset=True)
        with pool_poison(PATTERNS[pat]):
            snap, _ = SC.run_plain(B, case, device)
        blocks, nbytes = poison_stats(reset=True)
        return snap, {"blocks": blocks, "bytes": nbytes}
    if kind == "outputs":
        with poisoned_outputs(monkeypatch, B, PATTERNS[pat]) as proxy:
            snap, _ = SC.run_plain(B, case, device)
        return snap, {"allocations": proxy.count, "bytes": proxy.bytes}
    assert schedule == "decoy-first", schedule
    SC.run_plain(B, decoy_of(case), device)
    snap, _ = SC.run_plain(B, case, device)
    return snap, {}


def returns_device_tensor(snap):
    return any(leaf[0] != "host" for leaf in snap)


# Cases that take nothing from the pool, set-up stage included, settled from the code: cs_affine_act, cs_row_l2_normalize
# and cs_segmented_max (rowops.hip: only cs_instance_norm has PoolBuf scratch) and the four list helpers of sympose.hip,
# which has no pool allocation at all.  Checked both ways: these report exactly 0 poisoned blocks, every other case more.
SCRATCH_FREE = ["affine_act", "row_l2_normalize", "segmented_max", "partition_by_label", "cfg_bad", "rows_nonfinite",
                "corr_assemble"]

# Cases whose wrappers never call torch.empty / torch.empty_like, so the proxy has nothing to poison: orient_normals works
# in place on the caller's tensor; the others allocate every output INITIALISED (torch.zeros / torch.full: masks of which
# the kernels write the set bytes only, labels that start at -1).  Checked both ways like SCRATCH_FREE: exactly 0 poisoned
# allocations here, more than 0 for every other case that returns a tensor.
NO_EMPTY_OUTPUTS = ["orient_normals", "fpfh", "outlier_radius", "dbscan", "cluster_largest", "segment_plane"]


# ---- edge cases ----------------------------------------------------------------------------------------------------
class EdgeCase(SC.Case):
    """A case with a part for which a kernel writes nothing, its twin without that part, and `relate(full, twin)`,
    which asserts the metamorphic relation on the two outputs (tensors on the device)."""

    def __init__(self, name, make, op, twin, relate, env=None, seed=1):
        super().__init__(name, make, op, env, seed)
        self.twin, self.relate = twin, relate


def _bits(t):
    t = t.detach().contiguous().cpu()
    return str(t.dtype), tuple(t.shape), t.numpy().tobytes()


def same(a, b, what):
    """Bitwise equality of two tensors or of two nests of them."""
    sa, sb = SC.snapshot(a), SC.snapshot(b)
    diff = SC.first_difference(sa, sb)
    assert diff is None, "%s: %s" % (what, diff)


def holds(t, want, what):
    """Every row of t equals `want` (NaN matches NaN of any payload)."""
    got = t.detach().cpu().numpy()
    want = np.broadcast_to(np.asarray(want, dtype=got.dtype), got.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), "%s: %r, documented %r" % (what, got, want)


# -- scan family: an empty segment first and in the middle
E_SCAN_OFF, E_SCAN_LIVE, E_SCAN_EMPTY = [0, 0, 1100, 1100, 1500], [1, 3], [0, 2]
assert [E_SCAN_OFF[s] for s in E_SCAN_LIVE] + [E_SCAN_OFF[-1]] == SC.SCAN_OFF


def _scan(call):
    """(op, twin) of a scan entry point `call(B, d, off)`."""
    return (lambda B, d: call(B, d, E_SCAN_OFF)), (lambda B, d: call(B, d, SC.SCAN_OFF))


def _view(d, off):
    """A view point per segment: the draw's two for the live segments, the origin for the empty ones."""
    if len(off) - 1 == 2:
        return d["view"]
    v = torch.zeros((len(off) - 1, 3), dtype=d["view"].dtype, device=d["view"].device)
    v[E_SCAN_LIVE] = d["view"]
    return v


def _orient(B, d, off):
    return (B.orient_normals(d["xyz"], off, d["nrm"].clone()),
            B.orient_normals(d["xyz"], off, d["nrm"].clone(), _view(d, off), away=False))


def _dbscan(B, d, off):
    label, count = B.dbscan(d["xyz"], off, 0.08, 5)
    return label, count, B.cluster_largest(label, off)


def _rows_only(full, twin):
    same(full, twin, "the rows of the live segments")


def _per_segment(table_of, empty_rows):
    """Relation of an output with per-row tensors and per-segment tables: `table_of(out)` -> (rows part, [tables]);
    empty_rows[i] = the documented row of table i for an empty segment."""
    def relate(full, twin):
        (frows, ftabs), (trows, ttabs) = table_of(full), table_of(twin)
        same(frows, trows, "the rows of the live segments")
        for i, (ft, tt) in enumerate(zip(ftabs, ttabs)):
            same(ft[E_SCAN_LIVE], tt, "table %d, live segments" % i)
            holds(ft[E_SCAN_EMPTY], empty_rows[i], "table %d, empty segments" % i)
    return relate


# -- voxelize: an empty segment in the middle and one at the end
E_VOX_OFF, E_VOX_LIVE = [0, 800, 800, 2000, 2000], [0, 2]


def _vox_relate(full, twin):
    (fk, fg, fo), (tk, tg, to) = full, twin
    same(fk, tk, "kept rows")
    same(fg[:, 1:], tg[:, 1:], "grid cells")
    seg = torch.as_tensor(E_VOX_LIVE, dtype=fg.dtype, device=fg.device)
    same(fg[:, 0], seg[tg[:, 0].long()], "the batch column names the segment of the FULL table")
    assert fo == [to[0], to[1], to[1], to[2], to[2]], (fo, to)


# -- distances and ICP: an empty source (problem 1) and an empty target (problem 2) between two ordinary problems
E_REG_SOFF, E_REG_TOFF = [0, 500, 500, 800], [0, 700, 700, 1300]
E_REG_SSEG, E_REG_TSEG = [0, 1, 0, 2], [0, 0, 1, 2]
E_REG_LIVE = [0, 3]


def mk_reg4(seed):
    d = SC.mk_reg(seed)
    d["T0"] = np.ascontiguousarray(d["T0"][[0, 1, 0, 1]])
    return d


def _dist(fn):
    op = lambda B, d: getattr(B, fn)(d["src"], E_REG_SOFF, d["tgt"], E_REG_TOFF, E_REG_SSEG, E_REG_TSEG, d["T0"])
    twin = lambda B, d: getattr(B, fn)(d["src"], SC.REG_SOFF, d["tgt"], SC.REG_TOFF, [0, 1], [0, 1],
                                       d["T0"][E_REG_LIVE].contiguous())
    return op, twin


def _dist_relate(empty_src, empty_tgt):
    def relate(full, twin):
        same(full[E_REG_LIVE], twin, "ordinary problems")
        holds(full[1], empty_src, "empty source")
        holds(full[2], empty_tgt, "empty target")
    return relate


def _icp(**kw):
    def call(B, d, soff, toff, sseg, tseg, T0):
        args = {k: (d[v] if isinstance(v, str) and v in d else v) for k, v in kw.items()}
        r = B.icp_batch(d["src"], soff, d["tgt"], toff, sseg, tseg, T0, 0.1, max_iter=8, return_corr=True, **args)
        return r
    op = lambda B, d: _icp_out(call(B, d, E_REG_SOFF, E_REG_TOFF, E_REG_SSEG, E_REG_TSEG, d["T0"]))
    twin = lambda B, d: _icp_out(call(B, d, SC.REG_SOFF, SC.REG_TOFF, [0, 1], [0, 1], d["T0"][E_REG_LIVE].contiguous()))
    return op, twin


def _icp_out(r):
    """Per-problem fields by name (None where the estimation has none), then corr and its offsets."""
    return {"T": r.T, "T32": r.T32, "fitness": r.fitness, "rmse": r.rmse, "iters": r.iters, "ncorr": r.ncorr,
            "wfitness": r.wfitness, "scale": r.scale, "mrmse": r.mrmse, "corr": r.corr, "corr_off": r.corr_off}


ICP_EMPTY = {"fitness": 0.0, "rmse": 0.0, "iters": 0, "ncorr": 0, "wfitness": 0.0, "scale": 1.0, "mrmse": 0.0}


def _icp_relate(full, twin):
    """cs_icp_batch: "Empty source or target segment: answered with fitness 0, rmse 0, T = T0, 0 iterations" (scale 1,
    mrmse 0, wfitness 0, no pair)."""
    for k in ("T", "T32", "fitness", "rmse", "iters", "ncorr", "wfitness", "scale", "mrmse"):
        if full[k] is None:
            assert twin[k] is None
            continue
        same(full[k][E_REG_LIVE], twin[k], "%s of the ordinary problems" % k)
        if k in ICP_EMPTY:
            holds(full[k][[1, 2]], ICP_EMPTY[k], "%s of the empty problems" % k)
    assert full["corr_off"] == [0, 500, 500, 1000, 1300] and twin["corr_off"] == [0, 500, 800]
    same(full["corr"][:500], twin["corr"][:500], "corr of problem 0")
    same(full["corr"][1000:], twin["corr"][500:], "corr of problem 3")
    holds(full["corr"][500:1000], -1, "corr of the problem with the empty target")


def _icp_t0_relate(full, twin, d):
    T0 = d["T0"]
    same(full["T32"][[1, 2]], T0[[1, 2]], "T32 of the empty problems is T0")
    same(full["T"][[1, 2]], T0[[1, 2]].double(), "T of the empty problems is T0")


# -- feature k-NN: an empty query segment
E_KNN_QOFF = [0, 700, 700, 1000]


def _knn(B, d):
    return B.knn_feat(d["q"], E_KNN_QOFF, d["t"], SC.KNN_TOFF, 5, qseg=[0, 1, 2], tseg=[0, 0, 1], return_distance=True)


def _knn_twin(B, d):
    return B.knn_feat(d["q"], SC.KNN_QOFF, d["t"], SC.KNN_TOFF, 5, return_distance=True)


# -- hardest negatives: an anchor without an admissible row; no anchor at all
HN_LONE = 300                      # the first query row of problem 1


def mk_hardneg_lone(seed):
    """mk_hardneg with the whole target segment of problem 1 within 0.02 of query row HN_LONE (radius 0.1): that anchor
    has no admissible row.  The other anchors of problem 1 are moved out of reach of it, and the lone anchor comes
    third."""
    d = SC.mk_hardneg(seed)
    rng = np.random.default_rng(seed + 77)
    lo, hi = SC.HN_TOFF[1], SC.HN_TOFF[2]
    centre = np.array([0.3, 0.3, 0.3], np.float32)
    d["qxyz"][HN_LONE] = centre
    d["txyz"][lo:hi] = centre + SC._f32(rng.uniform(-0.01, 0.01, (hi - lo, 3)))
    a = np.where(d["anchors"] == HN_LONE, HN_LONE + 1, d["anchors"])
    d["anchors"] = np.concatenate([a[:2], [HN_LONE], a[2:]]).astype(np.int32)
    far = np.setdiff1d(np.arange(SC.HN_QOFF[1], SC.HN_QOFF[2]), [HN_LONE])
    d["qxyz"][far] = SC._f32(rng.uniform(-0.5, 0.1, (far.size, 3)))        # at least 0.19 from every target row
    return d


def _hn(B, d, anchors):
    return B.hardest_negatives(d["qf"], d["qxyz"], SC.HN_QOFF, d["tf"], d["txyz"], SC.HN_TOFF, anchors, 0.1,
                               return_distance=True)


def _hn_lone_relate(full, twin):
    keep = [i for i in range(full[0].shape[0]) if i != 2]
    same((full[0][keep], full[1][keep]), twin, "the other anchors")
    holds(full[0][2], -1, "index of the anchor without an admissible row")
    holds(full[1][2], np.inf, "distance of the anchor without an admissible row")
    assert int((twin[0] >= 0).sum()) == twin[0].numel(), "every other anchor has an admissible row"


def _hn_none_relate(full, twin):
    assert tuple(full[0].shape) == (0,) and tuple(full[1].shape) == (0,)
    assert full[0].dtype == torch.int32 and full[1].dtype == torch.float64


# -- registration: a zero-size problem in the middle
E_RANSAC_SIZES, E_RANSAC_INLIERS = [10, 191, 0, 192, 193, 700, 0], [0.5, 0.3, 0.0, 0.2, 0.4, 0.25, 0.0]
E_FGR_SIZES, E_FGR_INLIERS = [193, 0, 700, 64], [0.5, 0.0, 0.3, 0.6]


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).tolist()


def _live(sizes):
    return [i for i, m in enumerate(sizes) if m]


def _ransac(sizes):
    call = lambda B, d, off: B.ransac_batch(d["src"], d["tgt"], off, 0.2, 10, SC.RANSAC_ITER, 0.999, 7)
    return (lambda B, d: call(B, d, _offsets(sizes))), (lambda B, d: call(B, d, _offsets([m for m in sizes if m])))


def _fgr(sizes):
    call = lambda B, d, off: tuple(B.fgr_batch(d["src"], d["tgt"], off, 0.2, seed=5))
    return (lambda B, d: call(B, d, _offsets(sizes))), (lambda B, d: call(B, d, _offsets([m for m in sizes if m])))


EYE4 = np.eye(4)


def _ransac_relate(full, twin):
    """cs_ransac_batch: "A problem with no finite pair returns the identity, 0 inliers and rmse 0"; an empty problem
    consumes 0 iterations."""
    live, dead = _live(E_RANSAC_SIZES), [i for i, m in enumerate(E_RANSAC_SIZES) if not m]
    same([t[live] for t in full], list(twin), "problems with pairs")
    T, inl, rmse, iters = full
    holds(T[dead], EYE4, "T of an empty problem")
    holds(inl[dead], 0, "inliers of an empty problem")
    holds(rmse[dead], 0.0, "rmse of an empty problem")
    holds(iters[dead], 0, "iterations of an empty problem")


def _fgr_relate(full, twin):
    """cs_fgr_batch: "Empty problems are legal (identity, 0 inliers)"; a degenerate frame (m = 0) gives 0 updates, rmse 0
    without an inlier and n_tuple = 0 with the test on."""
    live, dead = _live(E_FGR_SIZES), [i for i, m in enumerate(E_FGR_SIZES) if not m]
    same([t[live] for t in full], list(twin), "problems with pairs")
    T, T64, inl, rmse, iters, n_tuple = full
    holds(T[dead], EYE4, "T of an empty problem")
    holds(T64[dead], EYE4, "T64 of an empty problem")
    for t, name in ((inl, "inliers"), (rmse, "rmse"), (iters, "iters"), (n_tuple, "n_tuple")):
        holds(t[dead], 0, "%s of an empty problem" % name)


# -- training: a problem without a pair, a term without a pair
def mk_pairs_apart(seed):
    """mk_pairs with the positive cloud of problem 1 moved ten units away: no pair within any radius used here."""
    d = SC.mk_pairs(seed)
    d["xyz"][SC.PAIR_OFF[4]:SC.PAIR_OFF[5], 0] += 10.0
    return d


def _radius(B, d, base, pos, neg):
    xyz = d["xyz"].double()
    row_ptr, plan = B.radius_pairs_begin(xyz, SC.PAIR_OFF, xyz, SC.PAIR_OFF, base, pos, 0.03)
    total = int(row_ptr[-1])
    return row_ptr, total, plan.fill(row_ptr, total), B.radius_pairs(xyz, SC.PAIR_OFF, xyz, SC.PAIR_OFF, base, pos, 0.05, k=3)


def _radius_relate(full, twin):
    (frp, ftot, fidx, (frp3, fidx3)), (trp, ttot, tidx, (trp3, tidx3)) = full, twin
    assert ftot == ttot and ttot > 0
    for f, t, what in ((frp, trp, "row_ptr"), (frp3, trp3, "row_ptr, k = 3")):
        same(f[:401], t, what + " of the problem with pairs")
        holds(f[401:], int(t[-1]), what + " of the problem without pairs")
    same((fidx, fidx3), (tidx, tidx3), "target indices")


def _loss_terms(B, d, with_empty):
    none = d["pin"][:0]
    terms = [(0, 1, d["pip"], B.PAIR_PULL, 0.1, 1.0), (0, 2, none, B.PAIR_PUSH, 1.4, 0.75),
             (0, 1, d["pin"], B.PAIR_PUSH, 1.4, 1.0), (0, 2, d["nin"], B.PAIR_PUSH, 1.4, 0.5)]
    return [d["base"], d["pos"], d["neg"]], (terms if with_empty else terms[:1] + terms[2:])


def _loss_fwd_relate(full, twin):
    """cs_pair_loss_fwd: "h_npairs[t] = 0 is legal: the term is 0 and contributes no gradient"."""
    same(full[0][[0, 2, 3]], twin[0], "terms with pairs")
    holds(full[0][1], 0.0, "the term without pairs")
    same(full[1], twin[1], "total (an exact zero added)")


# -- the list
def _edge_cases():
    cases = []

    def add(name, make, pair, relate, env=None):
        cases.append(EdgeCase("edge_" + name, make, pair[0], pair[1], relate, env))

    add("normals_knn", SC.mk_scan, _scan(lambda B, d, off: B.estimate_normals(d["xyz"], off, 16)), _rows_only)
    add("normals_hybrid", SC.mk_scan, _scan(lambda B, d, off: B.estimate_normals(d["xyz"], off, 16, radius=0.1)), _rows_only)
    add("orient_normals", SC.mk_scan, _scan(_orient), _rows_only)
    add("fpfh", SC.mk_scan, _scan(lambda B, d, off: B.fpfh(d["xyz"], off, d["nrm"], 0.12, 50)), _rows_only)
    add("knn_mean_dist", SC.mk_scan, _scan(lambda B, d, off: B.knn_mean_dist(d["xyz"], off, 20)), _rows_only)
    # cs_outlier_statistical: an empty segment has n_valid = 0, for which the header gives mu = sigma = 0 and tau = 0
    add("outlier_statistical", SC.mk_scan, _scan(lambda B, d, off: B.outlier_statistical(d["xyz"], off, 20, 2.0)),
        _per_segment(lambda o: (o[0], [o[1]]), [[0.0, 0.0, 0.0, 0.0]]))
    add("outlier_radius", SC.mk_scan, _scan(lambda B, d, off: B.outlier_radius(d["xyz"], off, 0.1, 8)), _rows_only)
    # cs_cluster_largest: "a segment without a cluster gives (0, -1, 0)"
    add("dbscan", SC.mk_scan, _scan(_dbscan), _per_segment(lambda o: ((o[0], o[1], o[2][0]), [o[2][1]]), [[0, -1, 0]]))
    # cs_segment_plane: "an empty segment writes the NO-PLANE row": a zero plane and stat (0, -1, 0, 0, 0, 0, 0, rows_finite)
    add("segment_plane", SC.mk_scan, _scan(lambda B, d, off: B.segment_plane(d["xyz"], off, 0.01, 256, 3)),
        _per_segment(lambda o: (o[0], [o[1], o[2]]), [[0.0, 0.0, 0.0, 0.0], [0, -1, 0, 0, 0, 0, 0, 0]]))
    for name, make in (("voxelize_f32", SC.mk_voxel), ("voxelize_f64", lambda seed: SC.mk_voxel(seed, np.float64))):
        add(name, make, (lambda B, d: B.voxelize(d["xyz"], E_VOX_OFF, 0.05), lambda B, d: B.voxelize(d["xyz"], SC.VOX_OFF, 0.05)),
            _vox_relate)
    nan, inf = np.nan, np.inf
    add("chamfer_1dir", mk_reg4, _dist("chamfer_1dir"), _dist_relate(nan, inf))
    add("chamfer_2dir", mk_reg4, _dist("chamfer_2dir"), _dist_relate([nan, inf], [inf, nan]))
    # cs_hausdorff_1dir shares cs_chamfer_1dir's rules: NaN for an empty source alone, +inf without a finite target row
    add("hausdorff_1dir", mk_reg4, _dist("hausdorff_1dir"), _dist_relate(nan, inf))
    add("icp_point", mk_reg4, _icp(), _icp_relate)
    add("icp_plane", mk_reg4, _icp(tgt_normals="tn"), _icp_relate)
    add("icp_robust", mk_reg4, _icp(tgt_normals="tn", kernel="huber", kernel_scale=0.02), _icp_relate)
    add("icp_scale", mk_reg4, _icp(with_scaling=True), _icp_relate)
    add("icp_gicp", mk_reg4, _icp(tgt_normals="tn", src_normals="sn", estimation="gicp"), _icp_relate)
    add("knn_feat", SC.mk_knn, (_knn, _knn_twin), _rows_only)
    add("knn_feat_exhaustive", SC.mk_knn, (_knn, _knn_twin), _rows_only, {"CS_KNN_MFMA": "0"})
    add("hardneg_lone_anchor", mk_hardneg_lone,
        (lambda B, d: _hn(B, d, d["anchors"]), lambda B, d: _hn(B, d, torch.cat([d["anchors"][:2], d["anchors"][3:]]))),
        _hn_lone_relate)
    add("hardneg_no_anchor", SC.mk_hardneg, (lambda B, d: _hn(B, d, d["anchors"][:0]),) * 2, _hn_none_relate)
    add("ransac", lambda seed: SC.mk_corr(seed, E_RANSAC_SIZES, E_RANSAC_INLIERS), _ransac(E_RANSAC_SIZES), _ransac_relate)
    add("fgr", lambda seed: SC.mk_corr(seed, E_FGR_SIZES, E_FGR_INLIERS), _fgr(E_FGR_SIZES), _fgr_relate)
    add("radius_pairs", mk_pairs_apart, (lambda B, d: _radius(B, d, [0, 3], [1, 4], None),
                                         lambda B, d: _radius(B, d, [0], [1], None)), _radius_relate)
    add("pair_loss_fwd", SC.mk_loss, (lambda B, d: B.pair_loss_fwd(*_loss_terms(B, d, True)),
                                      lambda B, d: B.pair_loss_fwd(*_loss_terms(B, d, False))), _loss_fwd_relate)
    add("pair_loss_bwd", SC.mk_loss, (lambda B, d: B.pair_loss_bwd(*_loss_terms(B, d, True), d["g"]),
                                      lambda B, d: B.pair_loss_bwd(*_loss_terms(B, d, False), d["g"])), _rows_only)
    return cases


EDGE_CASES = _edge_cases()
ICP_EDGES = [c.name for c in EDGE_CASES if c.name.startswith("edge_icp_")]


def check_relation(B, case, device):
    """Runs the edge case and its twin on the real draw (plain schedule) and asserts the relation."""
    d = SC.ready_inputs(B, case, device)
    with SC.environment(case.env):
        full, twin = case.op(B, d), case.twin(B, d)
    torch.cuda.synchronize()
    case.relate(full, twin)
    if case.name in ICP_EDGES:
        _icp_t0_relate(full, twin, d)
