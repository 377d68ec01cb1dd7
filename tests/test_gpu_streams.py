"""The stream contract of include/corsair_hip.h (the Conventions block), for every entry point of backend.py, off the
default stream:

  1. the work of a call is enqueued on the stream the call is given, in stream order;
  2. scratch is cached per host thread and handed out again in stream order (a thread that switches streams drains the
     old one first);
  3. different threads may drive different streams concurrently.

Every case of tests/stream_cases.py runs under the late-input schedule described there, with a fresh side stream and with
the default stream as the caller's stream, and must give the bits of the plain schedule (default stream, ready inputs,
idle device).  The positive control of a run must have seen the decoy; otherwise the delay was too short, the run proves
nothing and the test FAILS.  The delay is three times the longest host-side enqueue time of any plain call of the module,
at least 20 ms; it is printed with every case, together with whether the host returned from the call before the inputs
were ready.
"""
import threading

import numpy as np
import pytest
import torch

from tests import stream_cases as SC

pytestmark = pytest.mark.gpu


def test_every_backend_entry_point_has_a_stream_case():
    """Needs no device: every public function and class member of backend.py is a key of ENTRY_CASES or of the commented
    exclusion list, the table names existing cases only, and every case is in the table."""
    from corsair_amd import backend

    assert SC.missing_entries(backend) == []
    entries = set(SC.public_entries(backend))
    assert [n for n in list(SC.ENTRY_CASES) + list(SC.EXCLUDED) if n not in entries] == []
    assert not set(SC.ENTRY_CASES) & set(SC.EXCLUDED)
    named = {c for cases in SC.ENTRY_CASES.values() for c in cases}
    assert named == set(SC.BY_NAME) and len(SC.BY_NAME) == len(SC.CASES)
    # the check bites: without its entry an operator is reported
    pruned = {k: v for k, v in SC.ENTRY_CASES.items() if k != "segment_plane"}
    assert SC.missing_entries(backend, table=pruned) == ["segment_plane"]
    assert SC.RANSAC_ITER >= SC.RANSAC_MIN_SIDE_ITER


@pytest.fixture(scope="module")
def plain(gpu):
    """The plain schedule of every case, run twice (the first call of an operator loads its kernels and fills the scratch
    pool; the second is timed, and both must agree: a case that differs from itself would prove nothing about streams),
    and the delay derived from the longest host-side enqueue time."""
    from corsair_amd import backend as B

    snaps, times = {}, {}
    for case in SC.CASES:
        first, _ = SC.run_plain(B, case, gpu)
        snaps[case.name], times[case.name] = SC.run_plain(B, case, gpu)
        diff = SC.first_difference(first, snaps[case.name])
        assert diff is None, "%s: two plain runs differ: %s" % (case.name, diff)
    slowest = max(times, key=times.get)
    delay = SC.Delay(gpu)
    delay_ms = max(SC.MIN_DELAY_MS, 3.0 * times[slowest])
    measured = delay.measure(delay_ms)
    print("stream cases: longest plain enqueue %.2f ms (%s); delay asked %.1f ms, measured %.1f ms (%s, probe %.2f ms)"
          % (times[slowest], slowest, delay_ms, measured, delay.kind, delay.probe_ms))
    assert measured >= 0.8 * delay_ms, "the delay is shorter than asked for"
    return {"B": B, "snaps": snaps, "times": times, "delay": delay, "delay_ms": delay_ms}


def _stream(kind, gpu, plain):
    return SC.fresh_streams(gpu, plain["delay"])[0] if kind == "side" else torch.cuda.default_stream(gpu)


def _judge(name, kind, plain, snap, saw, host_early, want=None):
    print("stream case %-20s st=%-7s delay %.1f ms  control saw the %s  host returned %s the inputs were ready"
          % (name, kind, plain["delay_ms"], saw, "BEFORE" if host_early else "after"))
    assert saw == "decoy", ("%s on the %s stream is inconclusive: the positive control saw the %s data, so the delay of "
                            "%.1f ms was too short to expose a misordered launch" % (name, kind, saw, plain["delay_ms"]))
    diff = SC.first_difference(snap, plain["snaps"][name] if want is None else want)
    assert diff is None, "%s with the %s stream as caller differs from the plain schedule: %s" % (name, kind, diff)


@pytest.mark.parametrize("kind", ["side", "default"])
@pytest.mark.parametrize("case", SC.CASES, ids=repr)
def test_late_inputs_give_the_plain_bits(gpu, plain, case, kind):
    """Contract line 1.  A launch, memset, copy or library call that misses the caller's stream, and a fork onto the
    internal side streams that does not wait for it, run during the delay and read the decoy."""
    snap, saw, early = SC.run_late(plain["B"], case, gpu, _stream(kind, gpu, plain), plain["delay"], plain["delay_ms"])
    _judge(case.name, kind, plain, snap, saw, early)


def _wrong_stream_case(name, kind, gpu, plain):
    """The case `name` with its operator launched on purpose on the stream the caller did NOT give: the mistake the
    module looks for."""
    wrong = torch.cuda.default_stream(gpu) if kind == "side" else SC.fresh_streams(gpu, plain["delay"])[0]
    case = SC.BY_NAME[name]

    def op(B, d):
        with torch.cuda.stream(wrong):
            return case.op(B, d)

    return SC.Case(name, case.make, op, case.env, case.seed, case.setup, case.ready)


@pytest.mark.parametrize("kind", ["side", "default"])
@pytest.mark.parametrize("name", ["row_l2_normalize", "conv_fwd", "conv_dgrad"])
def test_the_schedule_catches_a_launch_on_the_wrong_stream(gpu, plain, name, kind):
    """The method's own control, for a row operator and for the convolutions, whose kernel map comes from the set-up
    stage: sent to the other stream, the operator reads the decoy (valid data: wrong numbers, no fault), the positive
    control is conclusive, and the outputs differ from the plain schedule's.  (Entry points that take scratch from the
    pool cannot serve here: given another stream they drain the old one first, as the contract says, and so wait for the
    real data; the mistake the module looks for is a single launch inside a call, which no test can stage from outside.)"""
    case = _wrong_stream_case(name, kind, gpu, plain)
    snap, saw, _ = SC.run_late(plain["B"], case, gpu, _stream(kind, gpu, plain), plain["delay"], plain["delay_ms"])
    assert saw == "decoy"
    diff = SC.first_difference(snap, plain["snaps"][name])
    print("wrong stream, %s, st=%s: %s" % (name, kind, diff))
    assert diff is not None, "a launch on the wrong stream went unnoticed"


def _pair(gpu, plain, case_a, st_a, case_b, st_b, tag):
    """case_a under the late schedule on st_a, then AT ONCE case_b under the late schedule on st_b: same thread, no
    synchronise in between.  Both are armed before either is called, so their kernels become runnable at about the same
    time: a scratch block that changed hands without the old stream being drained would be used by both."""
    B = plain["B"]
    a = SC.LateRun(B, case_a, gpu, st_a, plain["delay"], plain["delay_ms"]).prepare()
    b = SC.LateRun(B, case_b, gpu, st_b, plain["delay"], plain["delay_ms"]).prepare()
    a.arm()
    b.arm()
    a.call()
    b.call()
    torch.cuda.synchronize()
    for run, which in ((a, "first"), (b, "second")):
        snap, saw = run.finish()
        _judge(run.case.name, "%s:%s" % (tag, which), plain, snap, saw, run.host_early)


@pytest.mark.parametrize("name", ["segment_plane", "knn_f16"])
def test_switching_streams_on_one_thread(gpu, plain, name):
    """Contract line 2: the same operator on the same shapes, hence the same scratch size classes, on stream A and at once
    on stream B, then the other way round (B first)."""
    case = SC.BY_NAME[name]
    sa, sb = SC.fresh_streams(gpu, plain["delay"], 2)
    _pair(gpu, plain, case, sa, case, sb, "A,B")
    _pair(gpu, plain, case, sb, case, sa, "B,A")
    _pair(gpu, plain, case, sa, case, torch.cuda.default_stream(gpu), "A,default")


def test_build_many_then_conv_on_another_stream(gpu, plain):
    """Contract line 2 around the fork of cs_kernelmap_build_many (pool_defer): the ten maps are built on stream A under the
    late schedule and a convolution over the first of them follows at once on stream B, ordered behind the build by an
    event, as the engine orders them."""
    from corsair_amd import backend as B

    conv_stream = {"st": None}

    def op(B, d):
        kms = SC.build_all_maps(B, d["coords"])
        ev = torch.cuda.Event()
        ev.record()                                    # on the building stream; the copies of x and w precede it there
        st = conv_stream["st"] or torch.cuda.current_stream()
        with torch.cuda.stream(st):
            st.wait_event(ev)
            y = B.conv_fwd(kms[0], d["x"], d["w"], d["scale"], d["shift"], d["res"], relu=True)
        return [SC._kmap_out(km, export=False) for km in kms], y

    case = SC.Case("maps_then_conv", SC.mk_conv, op)
    want, _ = SC.run_plain(B, case, gpu)
    for kind in ("side", "default"):
        st, conv_stream["st"] = SC.fresh_streams(gpu, plain["delay"], 2)
        try:
            snap, saw, early = SC.run_late(B, case, gpu, st if kind == "side" else _stream(kind, gpu, plain), plain["delay"],
                                           plain["delay_ms"])
        finally:
            conv_stream["st"] = None
        _judge(case.name, kind, plain, snap, saw, early, want=want)


def _mk_busy(seed):
    return {"coords": SC.mk_coords(1)["coords"], "probe": SC._f32(np.random.default_rng(seed).standard_normal(64))}


def _specs(c1, c2, c4, c8):
    return [(c1, c1), (c1, c2), (c2, c2), (c2, c4), (c4, c4), (c4, c8), (c8, c8), (c8, c4, 3, True), (c4, c2, 3, True),
            (c2, c1, 3, True)]


BUSY = {   # the call on finished handles; its outputs
    "CoordMap.stride": lambda B, c: SC._map_out(c[0].stride(2)),
    "KernelMap.build": lambda B, c: [SC._kmap_out(B.KernelMap.build(c[0], c[0])), SC._kmap_out(B.KernelMap.build(c[0], c[1])),
                                     SC._kmap_out(B.KernelMap.build(c[1], c[0], 3, True))],
    "KernelMap.build_many": lambda B, c: [SC._kmap_out(km, export=False) for km in B.KernelMap.build_many(_specs(*c))],
}


@pytest.mark.parametrize("kind", ["side", "default"])
@pytest.mark.parametrize("entry", sorted(BUSY))
def test_calls_on_handles_behind_a_busy_caller_stream(gpu, plain, entry, kind):
    """CoordMap.stride, KernelMap.build and build_many take coordinate maps, which are complete when the call that made
    them returns (it waits for the device): no input of theirs can arrive late.  What can be late is the caller's stream.
    The maps come from the set-up stage; the op makes the call once (this leaves the maps' lazily made per-sample segments
    in place and VALID results of the same problem in the scratch blocks the pool hands out again), enqueues the delay on the
    caller's stream and makes the call again.  Each launch of the second call depends on the launches before it (cleared
    counters, keys, the sort): one that missed the caller's stream, or a builder on a side stream that did not wait for
    the fork, would run ahead of them, during the delay, on the stale values -- wrong numbers, never unwritten memory."""
    def op(B, d):
        BUSY[entry](B, d["ctx"])
        plain["delay"].enqueue(plain["delay_ms"])
        return BUSY[entry](B, d["ctx"])

    case = SC.Case(entry, _mk_busy, op, setup=lambda B, d: B.CoordMap.pyramid(d["coords"], 4, len(SC.COORD_ROWS)),
                   ready=("coords",))
    want, _ = SC.run_plain(plain["B"], case, gpu)
    snap, saw, early = SC.run_late(plain["B"], case, gpu, _stream(kind, gpu, plain), plain["delay"], plain["delay_ms"])
    _judge(case.name, kind + ":busy", plain, snap, saw, early, want=want)


MAP_HEAVY = ["coordmap", "pyramid", "kmap_build", "kmap_many", "conv_fwd", "conv_wgrad"]
SEARCH_HEAVY = ["knn_f16", "topk", "chamfer_2dir", "normals_knn", "ransac_overlap", "segment_plane"]


def test_two_threads_two_streams(gpu, plain):
    """Contract line 3: two worker threads start on a barrier, each with its own stream, one running six map-heavy
    operators three times over, the other six search-heavy ones; every result equals the serial plain-schedule bits.
    This case hunts a race between the threads (the pool's shared table, the per-thread caches and side streams, the
    kernel-map count slots): it CANNOT be made deterministic -- a pass shows that this run did not hit one, not that
    there is none.  It stays because line 3 of the contract has no other test.  One process, two threads, no retry."""
    from corsair_amd import backend as B

    assert all(SC.BY_NAME[n].env is None for n in MAP_HEAVY + SEARCH_HEAVY)   # the environment is the process's, not a thread's
    lists = [[SC.BY_NAME[n] for n in names] for names in (MAP_HEAVY, SEARCH_HEAVY)]
    inputs = [[SC._staged(c, c.seed, gpu) for c in cases] for cases in lists]
    torch.cuda.synchronize()
    streams = SC.fresh_streams(gpu, plain["delay"], 2)   # two that run side by side
    barrier = threading.Barrier(2)
    results, errors = [None, None], [None, None]

    def worker(w):
        try:
            torch.cuda.set_device(gpu)
            st = streams[w]
            outs = []
            barrier.wait(timeout=60)
            with torch.cuda.stream(st):
                for case, d in zip(lists[w], inputs[w]):
                    if case.setup is not None:      # the handles of a case are made by the thread that uses them
                        d["ctx"] = case.setup(B, d)
                for rep in range(3):
                    for case, d in zip(lists[w], inputs[w]):
                        outs.append((case.name, rep, case.op(B, d)))
                st.synchronize()
                results[w] = [(name, rep, SC.snapshot(out)) for name, rep, out in outs]
        except BaseException as e:   # reported by the main thread
            errors[w] = e
            barrier.abort()

    threads = [threading.Thread(target=worker, args=(w,)) for w in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for e in errors:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    assert all(e is None for e in errors), errors
    for w in range(2):
        assert len(results[w]) == 18
        for name, rep, snap in results[w]:
            diff = SC.first_difference(snap, plain["snaps"][name])
            assert diff is None, "thread %d, %s, repetition %d differs from the serial plain schedule: %s" % (w, name, rep, diff)
