"""The late-input schedule and its cases (tests/test_gpu_streams.py).

A case is an `op(B, d) -> outputs` over corsair_amd.backend and a generator `make(seed) -> {name: ndarray}` of its device
inputs.  Two draws of one generator have the same shapes and dtypes and different values; index-typed inputs are drawn in
range, so the second draw (the DECOY) is a valid input: an operator that reads it computes wrong numbers, never a fault.

The late schedule on a caller stream `st` (LateRun): the inputs are allocated on st and filled with the decoy; a delay
is enqueued on st, then the copy of the real data over the decoys; a tiny reduction of one input on the OTHER stream
(the positive control) must still see the decoy; then the operator is called with st current.  Whatever the call enqueues
anywhere but behind st -- a launch on the null stream, a fork that does not wait for st -- runs during the delay, reads
the decoy and changes the outputs.  The outputs are compared bit for bit with the plain schedule: the same op on the
default stream, inputs ready, device idle.  No oracle and no tolerance: the plain schedule is what the operators' own
suites pin.

A call that waits for the device ends the late part of its op: whatever the op calls afterwards sees finished inputs on an
idle device.  An entry point that works on a handle (a kernel map for the convolutions, a catalog for l2_topk) therefore
gets the handle from a SET-UP stage: `setup(B, d)` runs on the caller's stream before the delay, on the inputs named in
`ready` (real data, complete), and its result reaches the op as d["ctx"]; only the other inputs arrive late.  What the
late part cannot reach is listed in DESIGN.md (section 4, "Stream contract").
"""
import contextlib
import os
import time

import numpy as np
import torch

MIN_DELAY_MS = 20.0


# ---- outputs ---------------------------------------------------------------------------------------------------
def _leaves(out, acc):
    if isinstance(out, torch.Tensor):
        acc.append(out)
    elif isinstance(out, (tuple, list)):
        for o in out:
            _leaves(o, acc)
    elif isinstance(out, dict):
        for k in sorted(out):
            _leaves(out[k], acc)
    else:
        assert out is None or isinstance(out, (bool, int, float, str, np.integer, np.floating)), type(out)
        acc.append(out)
    return acc


def snapshot(out):
    """Host copy of every leaf of `out` (call after a synchronise): device tensors as (dtype, shape, bytes), host
    values as they are."""
    snap = []
    for leaf in _leaves(out, []):
        if isinstance(leaf, torch.Tensor):
            t = leaf.detach().contiguous().cpu()
            snap.append((str(t.dtype), tuple(t.shape), t.numpy().tobytes()))
        else:
            snap.append(("host", leaf))
    return snap


def first_difference(got, want):
    """None when the snapshots are equal bit for bit, otherwise a description of the first leaf that differs."""
    if len(got) != len(want):
        return "%d outputs, plain schedule %d" % (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g[:-1] != w[:-1]:
            return "output %d: %r, plain schedule %r" % (i, g[:-1], w[:-1])
        if g[-1] != w[-1]:
            if g[0] == "host":
                return "host output %d: %r, plain schedule %r" % (i, g[1], w[1])
            a, b = np.frombuffer(g[2], np.uint8), np.frombuffer(w[2], np.uint8)
            return "output %d (%s %s): %d of %d bytes differ" % (i, g[0], g[1], int((a != b).sum()), a.size)
    return None


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in (env or {})}
    try:
        for k, v in (env or {}).items():
            os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- the delay -------------------------------------------------------------------------------------------------
def _timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


class Delay:
    """A device-side delay on the current stream: torch.cuda._sleep where it behaves (its duration is measured once, with
    events, and must double with the cycle count), otherwise a chain of f64 matrix products."""

    def __init__(self, device):
        self.kind, self.per_ms, self.probe_ms = "matmul", None, None
        c0 = 20_000_000
        try:
            torch.cuda._sleep(1000)
            m1 = _timed_ms(lambda: torch.cuda._sleep(c0))
            m2 = _timed_ms(lambda: torch.cuda._sleep(2 * c0))
            if 1.0 < m1 < 5000.0 and 1.5 < m2 / m1 < 2.5:
                self.kind, self.per_ms, self.probe_ms = "sleep", c0 / m1, m1
        except (AttributeError, RuntimeError):
            pass
        if self.kind == "matmul":
            self.a = torch.randn((1536, 1536), dtype=torch.float64, device=device)
            self.b = torch.empty_like(self.a)
            torch.mm(self.a, self.a, out=self.b)
            self.probe_ms = _timed_ms(lambda: torch.mm(self.a, self.a, out=self.b))
            self.per_ms = 1.0 / max(self.probe_ms, 1e-3)

    def enqueue(self, ms):
        if self.kind == "sleep":
            torch.cuda._sleep(int(ms * self.per_ms))
        else:
            for _ in range(int(np.ceil(ms * self.per_ms))):
                torch.mm(self.a, self.a, out=self.b)

    def measure(self, ms):
        return _timed_ms(lambda: self.enqueue(ms))


# ---- streams that really run side by side ----------------------------------------------------------------------
# The runtime maps its streams onto a few hardware queues (four by default), and two streams on one
# queue run one after the other: work sent to the wrong one of them would wait behind the delay, see the real data and
# hide the mistake, and the positive control would report the real data.  The schedule therefore takes fresh streams
# until it has one whose work overlaps with the default stream's (and with the other chosen ones'), which it measures.
_overlap = {}


def overlaps(a, b, delay):
    """Whether work on stream b runs while stream a is busy (measured once per pair of streams, 5 ms)."""
    key = tuple(sorted((a.cuda_stream, b.cuda_stream)))
    if key not in _overlap:
        torch.cuda.synchronize()
        with torch.cuda.stream(a):
            delay.enqueue(5.0)
            end = torch.cuda.Event()
            end.record(a)
        with torch.cuda.stream(b):
            torch.zeros(1, device=a.device).add_(1)
            ev = torch.cuda.Event()
            ev.record(b)
        ev.synchronize()
        _overlap[key] = not end.query()
        torch.cuda.synchronize()
    return _overlap[key]


def fresh_streams(device, delay, n=1):
    """n fresh torch streams whose work overlaps with the default stream's and with each other's."""
    chosen = [torch.cuda.default_stream(device)]
    for _ in range(64):
        c = torch.cuda.Stream(device=device)
        if all(c.cuda_stream != x.cuda_stream and overlaps(x, c, delay) for x in chosen):
            chosen.append(c)
            if len(chosen) == n + 1:
                return chosen[1:]
    raise AssertionError("no %d streams that run beside the default stream and each other among 64 fresh ones" % n)


# ---- the two schedules -----------------------------------------------------------------------------------------
def _reduce(t):
    return t.sum(dtype=torch.float64) if t.dtype.is_floating_point else t.sum(dtype=torch.int64)


def _bits(t):
    return t.cpu().numpy().tobytes()


def _staged(case, seed, device):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in case.make(seed).items()}


def ready_inputs(B, case, device):
    """The real inputs on the device and, for a case with a set-up stage, its result under "ctx" (current stream)."""
    d = _staged(case, case.seed, device)
    if case.setup is not None:
        with environment(case.env):
            d["ctx"] = case.setup(B, d)
    return d


def run_plain(B, case, device):
    """(snapshot, host enqueue time in ms) of the op on the default stream, inputs ready, device synchronised."""
    d = ready_inputs(B, case, device)
    torch.cuda.synchronize()
    with environment(case.env):
        t0 = time.perf_counter()
        out = case.op(B, d)
        ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return snapshot(out), ms


class LateRun:
    """One operator call under the late-input schedule, in steps, so that two runs can be interleaved on one thread:
    prepare() -> arm() -> call() -> [torch.cuda.synchronize()] -> finish()."""

    def __init__(self, B, case, device, st, delay, delay_ms):
        self.B, self.case, self.device, self.st, self.delay, self.delay_ms = B, case, device, st, delay, delay_ms
        default = torch.cuda.default_stream(device)
        # the other stream: the default stream for a side stream, a fresh side stream for the default stream
        self.other = default if st != default else fresh_streams(device, delay)[0]
        self.out = None

    def prepare(self):
        real, decoy = _staged(self.case, self.case.seed, self.device), _staged(self.case, self.case.seed + 1000, self.device)
        assert real.keys() == decoy.keys()
        # the control reads the input whose reduction tells the two draws apart
        self.ctrl_key = None
        self.late = [k for k in real if k not in self.case.ready]
        for k in self.late:
            assert real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype, k
            if self.ctrl_key is None and real[k].numel() and _bits(_reduce(real[k])) != _bits(_reduce(decoy[k])):
                self.ctrl_key = k
        assert self.ctrl_key is not None, "the decoy draw equals the real one"
        self.want_real, self.want_decoy = _bits(_reduce(real[self.ctrl_key])), _bits(_reduce(decoy[self.ctrl_key]))
        self.real = real
        with torch.cuda.stream(self.st):
            self.bufs = {k: torch.empty_like(real[k]) for k in self.late}
            for k in self.late:
                self.bufs[k].copy_(decoy[k])
            for k in self.case.ready:                 # real and complete before the delay: the set-up stage reads them
                self.bufs[k] = real[k]
            torch.cuda.synchronize()
            if self.case.setup is not None:
                with environment(self.case.env):
                    self.bufs["ctx"] = self.case.setup(self.B, self.bufs)
        torch.cuda.synchronize()
        return self

    def arm(self):
        with torch.cuda.stream(self.st):
            self.delay.enqueue(self.delay_ms)
            for k in self.late:
                self.bufs[k].copy_(self.real[k])
            self.e_ready = torch.cuda.Event()
            self.e_ready.record(self.st)
        with torch.cuda.stream(self.other):
            self.ctrl = _reduce(self.bufs[self.ctrl_key])
        return self

    def call(self):
        with torch.cuda.stream(self.st), environment(self.case.env):
            self.out = self.case.op(self.B, self.bufs)
            self.host_early = not self.e_ready.query()
        return self

    def finish(self):
        """After torch.cuda.synchronize(): (snapshot, what the control saw: 'decoy', 'real' or 'mixed')."""
        got = _bits(self.ctrl)
        saw = "decoy" if got == self.want_decoy else ("real" if got == self.want_real else "mixed")
        return snapshot(self.out), saw


def run_late(B, case, device, st, delay, delay_ms):
    run = LateRun(B, case, device, st, delay, delay_ms).prepare().arm().call()
    torch.cuda.synchronize()
    snap, saw = run.finish()
    return snap, saw, run.host_early


# ---- input generators ------------------------------------------------------------------------------------------
def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def _unit(rng, n, c):
    x = rng.standard_normal((n, c))
    return _f32(x / np.linalg.norm(x, axis=1, keepdims=True))


def _cube(rng, n, half=0.5):
    return _f32(rng.uniform(-half, half, (n, 3)))


def _shell(rng, n):
    """Points near a sphere of radius 0.5: a surface, so that radius searches of 0.1 find a dozen neighbours."""
    return _f32(0.5 * _unit(rng, n, 3).astype(np.float64) + rng.normal(0, 0.004, (n, 3)))


def _pose(rng, angle=0.15, trans=0.03):
    """A rigid 4x4 (f64) of a small random rotation and translation."""
    w = rng.standard_normal(3)
    w *= angle * rng.uniform(0.5, 1.0) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = rng.uniform(-trans, trans, 3)
    return T


def _apply(T, x):
    return x.astype(np.float64) @ T[:3, :3].T + T[:3, 3]


COORD_ROWS = (700, 500)   # voxels per sample: 5 % and 3.6 % of a 24^3 box, so most voxels have neighbours


def _coords(rng):
    """int32 [1200, 4] (batch, x, y, z): distinct voxels of a 24^3 box per sample, rows grouped by sample."""
    rows = []
    for b, n in enumerate(COORD_ROWS):
        cell = rng.choice(24 ** 3, n, replace=False)
        xyz = np.stack(np.unravel_index(cell, (24, 24, 24)), 1) - 12
        rows.append(np.concatenate([np.full((n, 1), b), xyz], 1))
    return np.concatenate(rows).astype(np.int32)


N_VOX = sum(COORD_ROWS)


def mk_coords(seed):
    return {"coords": _coords(np.random.default_rng(seed))}


def mk_conv(seed):
    rng = np.random.default_rng(seed)
    return {"coords": _coords(rng), "x": _f32(rng.standard_normal((N_VOX, 32))),
            "w": _f32(rng.standard_normal((27, 32, 64)) * 0.1), "w1": _f32(rng.standard_normal((32, 64)) * 0.1),
            "scale": _f32(rng.uniform(-1.5, 1.5, 64)), "shift": _f32(rng.standard_normal(64)),
            "res": _f32(rng.standard_normal((N_VOX, 64))), "g": _f32(rng.standard_normal((N_VOX, 64)))}


def mk_rows(seed):
    rng = np.random.default_rng(seed)
    n, c = 1237, 48      # no multiple of a 64-lane wave or of a 256-row block
    a = int(rng.integers(100, n - 100))
    coords = rng.integers(-12, 12, (n, 4))
    coords[:, 0] = np.arange(n) >= a           # sample 0 = rows [0, a), sample 1 the rest: `seg` says the same
    return {"x": _f32(rng.standard_normal((n, c))), "scale": _f32(rng.uniform(-1.5, 1.5, c)),
            "shift": _f32(rng.standard_normal(c)), "res": _f32(rng.standard_normal((n, c))), "coords": coords.astype(np.int32),
            "seg": np.array([0, a, n], np.int32), "gamma": _f32(rng.uniform(0.5, 1.5, c)), "beta": _f32(rng.standard_normal(c))}


VOX_OFF = [0, 800, 2000]


def mk_voxel(seed, dtype=np.float32):
    return {"xyz": np.ascontiguousarray(np.random.default_rng(seed).uniform(-0.5, 0.5, (2000, 3)), dtype=dtype)}


def mk_topk(seed):
    rng = np.random.default_rng(seed)
    return {"q": _unit(rng, 37, 256), "x": _unit(rng, 5000, 256)}


KNN_QOFF, KNN_TOFF = [0, 700, 1000], [0, 900, 1156]


def mk_knn(seed):
    rng = np.random.default_rng(seed)
    perm = np.array([list(rng.permutation(4)) + [-3] * 4 for _ in range(3)], np.int32)
    return {"q": _unit(rng, KNN_QOFF[-1], 16), "t": _unit(rng, KNN_TOFF[-1], 16),
            "qlabel": rng.integers(0, 4, KNN_QOFF[-1]).astype(np.int32),
            "tlabel": rng.integers(0, 4, KNN_TOFF[-1]).astype(np.int32), "perm": perm}


HN_QOFF, HN_TOFF = [0, 300, 500], [0, 400, 650]


def mk_hardneg(seed):
    rng = np.random.default_rng(seed)
    anchors = np.concatenate([rng.integers(HN_QOFF[s], HN_QOFF[s + 1], 24) for s in range(2)])
    return {"qf": _unit(rng, 500, 16), "qxyz": _cube(rng, 500), "tf": _unit(rng, 650, 16), "txyz": _cube(rng, 650),
            "anchors": rng.permutation(anchors).astype(np.int32)}


REG_SOFF, REG_TOFF = [0, 500, 800], [0, 700, 1300]


def mk_reg(seed):
    """Two problems: the source is a posed, noisy part of its target (points near a sphere), with unit normals for both."""
    rng = np.random.default_rng(seed)
    tgt = [_shell(rng, 700), _shell(rng, 600)]
    src, T0 = [], []
    for t, n in zip(tgt, (500, 300)):
        src.append(_f32(_apply(_pose(rng), t[:n]) + rng.normal(0, 0.002, (n, 3))))
        T0.append(_pose(rng, 0.02, 0.005))
    tgt, src = np.concatenate(tgt), np.concatenate(src)
    unit = lambda x: _f32(x / np.linalg.norm(x, axis=1, keepdims=True))
    return {"src": src, "tgt": tgt, "T0": _f32(np.stack(T0)), "tn": unit(tgt.astype(np.float64)),
            "sn": unit(src.astype(np.float64))}


SCAN_OFF = [0, 1100, 1500]   # one segment above every cell-grid threshold (513, 1 025 rows), one below


def mk_scan(seed):
    rng = np.random.default_rng(seed)
    xyz = _shell(rng, 1500)
    xyz[1100:1300, 2] = _f32(0.1 + rng.normal(0, 0.003, 200))    # a plane in the small segment
    xyz[:400, 1] = _f32(-0.2 + rng.normal(0, 0.003, 400))        # and one in the large segment
    nrm = _unit(rng, 1500, 3)
    return {"xyz": xyz, "nrm": nrm, "view": rng.uniform(-2, 2, (2, 3))}


RANSAC_SIZES = [10, 191, 192, 193, 700, 0]     # the batch of tests/test_gpu_ransac_front.py
RANSAC_INLIERS = [0.5, 0.3, 0.2, 0.4, 0.25, 0.0]
RANSAC_OFF = np.concatenate([[0], np.cumsum(RANSAC_SIZES)]).tolist()
# The smallest max_iter that puts a front half on the internal side stream: cs_ransac_batch enqueues the front half of
# the round starting at it1 on the side stream when the current round and that one are both prefiltered
# (RansacCall::prefiltered: it0 >= first_chunk = 64) and it1 < max_iter.  chunk_of gives the rounds [0, 64), [64, 512),
# [512, 1024), ...: the first prefiltered round is [64, 512), the first one behind a prefiltered round starts at 512, so
# max_iter >= 513.  2 048 (three such rounds, the value of test_gpu_ransac_front.py) makes the side stream's work count.
RANSAC_MIN_SIDE_ITER = 513
RANSAC_ITER = 2048


def mk_corr(seed, sizes=RANSAC_SIZES, inliers=RANSAC_INLIERS):
    rng = np.random.default_rng(seed)
    src, tgt = [], []
    for m, f in zip(sizes, inliers):
        s = _f32(rng.uniform(-0.8, 0.8, (m, 3)))
        t = _f32(_apply(_pose(rng, 1.0, 0.5), s) + rng.normal(0, 0.01, (m, 3)))
        bad = rng.random(m) > f
        t[bad] = _f32(rng.uniform(-1.2, 1.2, (int(bad.sum()), 3)))
        src.append(s)
        tgt.append(t)
    return {"src": np.concatenate(src), "tgt": np.concatenate(tgt)}


FGR_SIZES, FGR_INLIERS = [193, 700, 64], [0.5, 0.3, 0.6]
FGR_OFF = np.concatenate([[0], np.cumsum(FGR_SIZES)]).tolist()

SYM_OFF, SYM_KS = [0, 400, 1000], [2, 4]


def mk_symcut(seed):
    from tests.helpers import legged_object

    x0, f0 = legged_object(seed, 2, 200)
    x1, f1 = legged_object(seed + 1, 4, 150)
    rng = np.random.default_rng(seed)
    return {"feat": np.concatenate([f0, f1]), "xyz": np.concatenate([x0, x1]),
            "anchors": rng.integers(0, 400, (2, 12)).astype(np.int32),
            "centres": rng.uniform(-0.4, 0.4, (2, 4, 3))}


def mk_lists(seed):
    rng = np.random.default_rng(seed)
    a = int(rng.integers(150, 550))
    first = np.sort(np.concatenate([[0, 3, 3, 700], rng.integers(0, 700, 3)])).astype(np.int64)   # one empty range
    nn = rng.integers(0, 50, (700, 5)).astype(np.int32)
    x = _f32(rng.standard_normal((700, 16)))
    for r in rng.integers(0, 700, 3):       # a few dirty ranges; which ones depends on the draw
        nn[r, rng.integers(0, 5)] = -1
    if seed < 1000:                         # non-finite elements in the real draw only: a decoy never holds one
        x[rng.integers(0, 700), 3] = np.nan
        x[rng.integers(0, 700), 9] = -np.inf
    else:
        x[rng.integers(0, 700), 3] = 1e30
    return {"label": rng.integers(0, 4, 700).astype(np.int32), "off": np.array([0, a, 700], np.int64), "nn": nn,
            "first": first, "x": x}


def mk_assemble(seed):
    rng = np.random.default_rng(seed)
    return {"x0": _cube(rng, 400), "x1": _cube(rng, 300), "nn": rng.integers(0, 300, (400, 5)).astype(np.int32),
            "rows": rng.permutation(400).astype(np.int64)}


PAIR_OFF = [0, 400, 800, 1200, 1600, 2000, 2400]   # base, positive, negative of two problems


def mk_pairs(seed):
    rng = np.random.default_rng(seed)
    segs = []
    for _ in range(2):
        base = _cube(rng, 400, 0.2)
        pos = _f32(base[rng.permutation(400)] + rng.normal(0, 0.004, (400, 3)))
        segs += [base, pos, _cube(rng, 400, 0.2)]
    T = np.stack([_pose(rng), _pose(rng)])
    return {"xyz": np.concatenate(segs), "T": T}


def mk_loss(seed):
    rng = np.random.default_rng(seed)
    n = (500, 450, 400)
    base, pos, neg = (_unit(rng, k, 16) for k in n)
    pos[:300] = _f32(base[:300] + 0.05 * rng.standard_normal((300, 16)))
    pairs = lambda na, nb, p: np.stack([rng.integers(0, na, p), rng.integers(0, nb, p)], 1).astype(np.int32)
    pip = pairs(300, 300, 3000)
    pip[:, 1] = pip[:, 0]
    return {"base": base, "pos": pos, "neg": neg, "pip": pip, "pin": pairs(n[0], n[1], 3300), "nin": pairs(n[0], n[2], 3100),
            "g": _f32([rng.uniform(0.2, 0.9)])}


# ---- operators -------------------------------------------------------------------------------------------------
def _map_out(m):
    return m.n, m.tensor_stride, m.coords


def _kmap_out(km, export=True):
    out = [km.n_out, km.n_in, km.table(), km.num_pairs]
    return out + list(km.export()) if export else out


def op_coordmap(B, d):
    m = B.CoordMap.create(d["coords"])
    s = m.stride(2)
    return _map_out(m), _map_out(s), _map_out(s.stride(2))


def op_pyramid(B, d):
    return [_map_out(m) for m in B.CoordMap.pyramid(d["coords"], 4, len(COORD_ROWS))]


def op_kmap_build(B, d):
    m = B.CoordMap.create(d["coords"])
    s = m.stride(2)
    return [_kmap_out(B.KernelMap.build(m, m)), _kmap_out(B.KernelMap.build(m, s)),
            _kmap_out(B.KernelMap.build(s, m, 3, True))]


def build_all_maps(B, coords):
    """The ten kernel maps of a forward pass in one build_many, as engine.BatchMaps asks for them."""
    c1, c2, c4, c8 = B.CoordMap.pyramid(coords, 4, len(COORD_ROWS))
    specs = [(c1, c1), (c1, c2), (c2, c2), (c2, c4), (c4, c4), (c4, c8), (c8, c8), (c8, c4, 3, True), (c4, c2, 3, True),
             (c2, c1, 3, True)]
    return B.KernelMap.build_many(specs)


def op_kmap_many(B, d):
    return [_kmap_out(km, export=False) for km in build_all_maps(B, d["coords"])]


def _stride1_map(B, d):
    m = B.CoordMap.create(d["coords"])
    return B.KernelMap.build(m, m)


def op_conv_fwd(B, d):
    km = d["ctx"]
    return (B.conv_fwd(km, d["x"], d["w"], d["scale"], d["shift"], d["res"], relu=True), B.conv_fwd(km, d["x"], d["w"]),
            B.conv_fwd(None, d["x"], d["w1"], shift=d["shift"]))


def op_conv_wgrad(B, d):
    return B.conv_wgrad(d["ctx"], d["x"], d["g"]), B.conv_wgrad(None, d["x"], d["g"])


def op_conv_dgrad(B, d):
    return B.conv_dgrad(d["ctx"], None, d["g"], d["w"]), B.conv_dgrad(None, None, d["g"], d["w1"])


def op_affine_act(B, d):
    return B.affine_act(d["x"], d["scale"], d["shift"], d["res"], relu=True), B.affine_act(d["x"], None, d["shift"])


def op_row_l2(B, d):
    return B.row_l2_normalize(d["x"], 1e-12)


def op_segmented_max(B, d):
    return B.segmented_max(d["x"], d["coords"], 2)


def op_instance_norm(B, d):
    return B.instance_norm(d["x"], d["seg"], d["gamma"], d["beta"]), B.instance_norm(d["x"], d["seg"])


def op_voxelize(B, d):
    return B.voxelize(d["xyz"], VOX_OFF, 0.05)


def op_topk(B, d):
    return B.l2_topk(d["q"], d["x"], 10, True), B.l2_topk(d["q"], d["x"], 10, True, squared=True)


def op_topk_catalog_create(B, d):
    cat = B.TopkCatalog(d["x"])                      # the catalog rows arrive late
    return B.l2_topk(d["q"], cat, 10, True)


def op_topk_catalog(B, d):
    cat = d["ctx"]                                   # made from ready rows; the queries arrive late
    return B.l2_topk(d["q"], cat, 10, True), B.l2_topk(d["q"], cat, 3)


def op_knn(B, d):
    return B.knn_feat(d["q"], KNN_QOFF, d["t"], KNN_TOFF, 5, return_distance=True)


def op_knn_labels(B, d):
    return B.knn_feat(d["q"], KNN_QOFF, d["t"], KNN_TOFF, 5, qseg=[0, 0, 1], tseg=[0, 0, 1], qlabel=d["qlabel"],
                      tlabel=d["tlabel"], perm=d["perm"])


def op_hardneg(B, d):
    return B.hardest_negatives(d["qf"], d["qxyz"], HN_QOFF, d["tf"], d["txyz"], HN_TOFF, d["anchors"], 0.1,
                               return_distance=True)


def _reg(fn):
    return lambda B, d: getattr(B, fn)(d["src"], REG_SOFF, d["tgt"], REG_TOFF, [0, 1], [0, 1], d["T0"])


def _icp(**kw):
    def op(B, d):
        args = {k: (d[v] if isinstance(v, str) and v in d else v) for k, v in kw.items()}
        r = B.icp_batch(d["src"], REG_SOFF, d["tgt"], REG_TOFF, [0, 1], [0, 1], d["T0"], 0.1, max_iter=8, return_corr=True,
                        **args)
        return tuple(r), r.mrmse
    return op


def op_normals(B, d):
    return B.estimate_normals(d["xyz"], SCAN_OFF, 16)


def op_normals_hybrid(B, d):
    return B.estimate_normals(d["xyz"], SCAN_OFF, 16, radius=0.1)


def op_orient(B, d):
    return (B.orient_normals(d["xyz"], SCAN_OFF, d["nrm"].clone()),
            B.orient_normals(d["xyz"], SCAN_OFF, d["nrm"].clone(), d["view"], away=False))


def op_fpfh(B, d):
    return B.fpfh(d["xyz"], SCAN_OFF, d["nrm"], 0.12, 50)


def op_knn_mean(B, d):
    return B.knn_mean_dist(d["xyz"], SCAN_OFF, 20)


def op_outlier_stat(B, d):
    return B.outlier_statistical(d["xyz"], SCAN_OFF, 20, 2.0)


def op_outlier_radius(B, d):
    return B.outlier_radius(d["xyz"], SCAN_OFF, 0.1, 8)


def op_dbscan(B, d):
    label, count = B.dbscan(d["xyz"], SCAN_OFF, 0.08, 5)
    return label, count, B.cluster_largest(label, SCAN_OFF)


def mk_labels(seed):
    """int32 [1500]: labels as cs_dbscan writes them, -1 or a small cluster id, per row of SCAN_OFF's segments."""
    return {"label": np.random.default_rng(seed).integers(-1, 6, SCAN_OFF[-1]).astype(np.int32)}


def op_cluster_largest(B, d):
    return B.cluster_largest(d["label"], SCAN_OFF)


def op_plane(B, d):
    return B.segment_plane(d["xyz"], SCAN_OFF, 0.01, 256, 3)


def op_ransac(B, d):
    return B.ransac_batch(d["src"], d["tgt"], RANSAC_OFF, 0.2, 10, RANSAC_ITER, 0.999, 7)


def op_fgr(B, d):
    return tuple(B.fgr_batch(d["src"], d["tgt"], FGR_OFF, 0.2, seed=5))


def op_symcut_fit(B, d):
    return B.symcut_fit(d["feat"], d["xyz"], SYM_OFF, d["anchors"], SYM_KS, 50, 10, 300)


def op_symcut_labels(B, d):
    return B.symcut_labels(d["xyz"], SYM_OFF, SYM_KS, d["centres"])


def op_partition(B, d):
    return B.partition_by_label(d["label"], d["off"], 2)


def op_cfg_bad(B, d):
    return B.cfg_bad(d["nn"], d["first"], 6)


def op_rows_nonfinite(B, d):
    return B.rows_nonfinite(d["x"], d["first"], 6)


def op_assemble(B, d):
    desc = np.asarray([[0, 0, 0, 150, 0], [150, 150, 0, 250, 150]], dtype=np.int64)
    return B.corr_assemble(d["x0"], d["x1"], None, d["nn"], desc, 400, 250), \
        B.corr_assemble(d["x0"], d["x1"], d["rows"], d["nn"], desc, 400, 250)


def op_radius_pairs(B, d):
    xyz = d["xyz"].double()
    row_ptr, plan = B.radius_pairs_begin(xyz, PAIR_OFF, xyz, PAIR_OFF, [0, 3], [1, 4], 0.03)
    total = int(row_ptr[-1])
    return row_ptr, total, plan.fill(row_ptr, total), B.radius_pairs(xyz, PAIR_OFF, xyz, PAIR_OFF, [0, 3], [2, 4], 0.05, k=3)


def op_sample_pairs(B, d):
    xyz = d["xyz"]
    base, pos, neg, slots = [0, 3], [1, 4], [2, 5], [5, 9]
    row_ptr, plan = B.radius_pairs_begin(xyz.double(), PAIR_OFF, xyz.double(), PAIR_OFF, base, pos, 0.03)
    row_base = [0, 400, 800]
    bufs = B.sample_pairs(xyz, PAIR_OFF, base, pos, neg, slots, row_base, row_ptr, None, 2, 1234, 2, 0.03, 64)
    total = int(row_ptr[-1])
    tgt_idx = plan.fill(row_ptr, total)
    B.sample_pairs(xyz, PAIR_OFF, base, pos, neg, slots, row_base, row_ptr, tgt_idx, 1, 1234, 2, 0.03, 64, out=bufs)
    return bufs, total


def op_transform(B, d):
    return B.transform_f64(d["xyz"], PAIR_OFF, [4, 1], d["T"])


def _loss_terms(B, d):
    return [d["base"], d["pos"], d["neg"]], [(0, 1, d["pip"], B.PAIR_PULL, 0.1, 1.0), (0, 1, d["pin"], B.PAIR_PUSH, 1.4, 1.0),
                                             (0, 2, d["nin"], B.PAIR_PUSH, 1.4, 0.5)]


def op_loss_fwd(B, d):
    return B.pair_loss_fwd(*_loss_terms(B, d))


def op_loss_bwd(B, d):
    mats, terms = _loss_terms(B, d)
    return B.pair_loss_bwd(mats, terms, d["g"])


# ---- the cases -------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, make, op, env=None, seed=1, setup=None, ready=()):
        self.name, self.make, self.op, self.env, self.seed = name, make, op, env, seed
        self.setup, self.ready = setup, tuple(ready)     # the set-up stage and the inputs it reads (never late)

    def __repr__(self):
        return self.name


_mk_corr_fgr = lambda seed: mk_corr(seed, FGR_SIZES, FGR_INLIERS)

CASES = [
    # sparse maps and convolution
    Case("coordmap", mk_coords, op_coordmap),
    Case("pyramid", mk_coords, op_pyramid),
    Case("kmap_build", mk_coords, op_kmap_build),
    Case("kmap_many", mk_coords, op_kmap_many),                                   # four streams (the default)
    Case("kmap_many_1stream", mk_coords, op_kmap_many, {"CS_KMAP_STREAMS": "1"}),
    Case("conv_fwd", mk_conv, op_conv_fwd, setup=_stride1_map, ready=("coords",)),
    Case("conv_wgrad", mk_conv, op_conv_wgrad, setup=_stride1_map, ready=("coords",)),
    Case("conv_dgrad", mk_conv, op_conv_dgrad, setup=_stride1_map, ready=("coords",)),
    Case("affine_act", mk_rows, op_affine_act),
    Case("row_l2_normalize", mk_rows, op_row_l2),
    Case("segmented_max", mk_rows, op_segmented_max),
    Case("instance_norm", mk_rows, op_instance_norm),
    # retrieval and search
    Case("voxelize_f32", mk_voxel, op_voxelize),
    Case("voxelize_f64", lambda seed: mk_voxel(seed, np.float64), op_voxelize),
    Case("topk", mk_topk, op_topk),                                               # the path the size selects
    Case("topk_slab", mk_topk, op_topk, {"CS_TOPK_MFMA": "0"}),
    Case("topk_f64", mk_topk, op_topk, {"CS_TOPK_MFMA": "1"}),
    Case("topk_f16", mk_topk, op_topk, {"CS_TOPK_MFMA": "16"}),
    Case("topk_catalog_create", mk_topk, op_topk_catalog_create, {"CS_TOPK_MFMA": "16"}),
    Case("topk_catalog", mk_topk, op_topk_catalog, {"CS_TOPK_MFMA": "16"}, setup=lambda B, d: B.TopkCatalog(d["x"]), ready=("x",)),
    Case("knn_f16", mk_knn, op_knn),
    Case("knn_exhaustive", mk_knn, op_knn, {"CS_KNN_MFMA": "0"}),
    Case("knn_labels", mk_knn, op_knn_labels),
    Case("hardest_negatives", mk_hardneg, op_hardneg),
    # distances and ICP
    Case("chamfer_1dir", mk_reg, _reg("chamfer_1dir")),
    Case("chamfer_2dir", mk_reg, _reg("chamfer_2dir")),
    Case("hausdorff_1dir", mk_reg, _reg("hausdorff_1dir")),
    Case("icp_point", mk_reg, _icp()),
    Case("icp_plane", mk_reg, _icp(tgt_normals="tn")),
    Case("icp_robust", mk_reg, _icp(tgt_normals="tn", kernel="huber", kernel_scale=0.02)),
    Case("icp_scale", mk_reg, _icp(with_scaling=True)),
    Case("icp_gicp", mk_reg, _icp(tgt_normals="tn", src_normals="sn", estimation="gicp")),
    # scan preparation
    Case("normals_knn", mk_scan, op_normals),
    Case("normals_hybrid", mk_scan, op_normals_hybrid),
    Case("orient_normals", mk_scan, op_orient),
    Case("fpfh", mk_scan, op_fpfh),
    Case("knn_mean_dist", mk_scan, op_knn_mean),
    Case("outlier_statistical", mk_scan, op_outlier_stat),
    Case("outlier_radius", mk_scan, op_outlier_radius),
    Case("dbscan", mk_scan, op_dbscan),
    Case("cluster_largest", mk_labels, op_cluster_largest),
    Case("segment_plane", mk_scan, op_plane),
    # registration
    Case("ransac_overlap", mk_corr, op_ransac),                                   # the default: CS_RANSAC_OVERLAP unset = on
    Case("ransac_serial", mk_corr, op_ransac, {"CS_RANSAC_OVERLAP": "0"}),
    Case("fgr", _mk_corr_fgr, op_fgr),
    Case("symcut_fit", mk_symcut, op_symcut_fit),
    Case("symcut_labels", mk_symcut, op_symcut_labels),
    Case("partition_by_label", mk_lists, op_partition),
    Case("cfg_bad", mk_lists, op_cfg_bad),
    Case("rows_nonfinite", mk_lists, op_rows_nonfinite),
    Case("corr_assemble", mk_assemble, op_assemble),
    # training
    Case("radius_pairs", mk_pairs, op_radius_pairs),
    Case("sample_pairs", mk_pairs, op_sample_pairs),
    Case("transform_f64", mk_pairs, op_transform),
    Case("pair_loss_fwd", mk_loss, op_loss_fwd),
    Case("pair_loss_bwd", mk_loss, op_loss_bwd),
]
BY_NAME = {c.name: c for c in CASES}

# Entry point of backend.py -> the cases that call it.  tests/test_gpu_streams.py checks that every public function and
# class member of backend.py is a key here or in EXCLUDED: a new operator needs a stream case.
ENTRY_CASES = {
    "CoordMap.create": ["coordmap"], "CoordMap.stride": ["coordmap"], "CoordMap.pyramid": ["pyramid"],
    "CoordMap.coords": ["coordmap", "pyramid"],
    "KernelMap.build": ["kmap_build"], "KernelMap.build_many": ["kmap_many", "kmap_many_1stream"],
    "KernelMap.num_pairs": ["kmap_build", "kmap_many"], "KernelMap.export": ["kmap_build"],
    "KernelMap.table": ["kmap_build", "kmap_many"],
    "conv_fwd": ["conv_fwd"], "conv_wgrad": ["conv_wgrad"], "conv_dgrad": ["conv_dgrad"], "dgrad_weight": ["conv_dgrad"],
    "affine_act": ["affine_act"], "row_l2_normalize": ["row_l2_normalize"], "segmented_max": ["segmented_max"],
    "instance_norm": ["instance_norm"],
    "voxelize": ["voxelize_f32", "voxelize_f64"],
    "l2_topk": ["topk", "topk_slab", "topk_f64", "topk_f16", "topk_catalog"], "TopkCatalog": ["topk_catalog_create"],
    "knn_feat": ["knn_f16", "knn_exhaustive", "knn_labels"], "hardest_negatives": ["hardest_negatives"],
    "chamfer_1dir": ["chamfer_1dir"], "chamfer_2dir": ["chamfer_2dir"], "hausdorff_1dir": ["hausdorff_1dir"],
    "icp_batch": ["icp_point", "icp_plane", "icp_robust", "icp_scale", "icp_gicp"],
    "estimate_normals": ["normals_knn", "normals_hybrid"], "orient_normals": ["orient_normals"], "fpfh": ["fpfh"],
    "knn_mean_dist": ["knn_mean_dist"], "outlier_statistical": ["outlier_statistical"],
    "outlier_radius": ["outlier_radius"], "dbscan": ["dbscan"], "cluster_largest": ["cluster_largest", "dbscan"],
    "segment_plane": ["segment_plane"],
    "ransac_batch": ["ransac_overlap", "ransac_serial"], "fgr_batch": ["fgr"],
    "symcut_fit": ["symcut_fit"], "symcut_labels": ["symcut_labels"], "partition_by_label": ["partition_by_label"],
    "cfg_bad": ["cfg_bad"], "rows_nonfinite": ["rows_nonfinite"], "corr_assemble": ["corr_assemble"],
    "radius_pairs_begin": ["radius_pairs", "sample_pairs"], "RadiusPlan.fill": ["radius_pairs", "sample_pairs"],
    "radius_pairs": ["radius_pairs"], "sample_pairs": ["sample_pairs"], "transform_f64": ["transform_f64"],
    "pair_loss_fwd": ["pair_loss_fwd"], "pair_loss_bwd": ["pair_loss_bwd"],
}

# Public names of backend.py without a stream case, and why.
EXCLUDED = {
    # host-side counters of the library: no stream argument, nothing is enqueued
    "hardest_stats": "stats getter", "fpfh_stats": "stats getter", "normals_stats": "stats getter",
    "outlier_stats": "stats getter", "dbscan_stats": "stats getter", "icp_stats": "stats getter",
    # plain torch on the current stream, no library call
    "select_rows": "plain torch",
    # result containers
    "IcpResult": "result tuple", "GicpResult": "result tuple", "FgrResult": "result tuple",
}


def public_entries(backend):
    """The public functions of backend.py and, per class, its public members (the class itself when it has none)."""
    names = []
    for name, obj in vars(backend).items():
        if name.startswith("_") or getattr(obj, "__module__", None) != backend.__name__:
            continue
        if isinstance(obj, type):
            if issubclass(obj, tuple):
                names.append(name)
                continue
            members = [m for m, v in vars(obj).items() if not m.startswith("_")
                       and (callable(v) or isinstance(v, (classmethod, staticmethod, property)))]
            names += ["%s.%s" % (name, m) for m in members] or [name]
        elif callable(obj):
            names.append(name)
    return sorted(names)


def missing_entries(backend, table=None, excluded=None):
    table = ENTRY_CASES if table is None else table
    excluded = EXCLUDED if excluded is None else excluded
    return [n for n in public_entries(backend) if n not in table and n not in excluded]
