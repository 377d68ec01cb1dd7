"""No result may depend on stale scratch, on unwritten outputs or on what ran before (tests/stale_cases.py has the
method).  Every case of tests/stream_cases.py and every edge case of tests/stale_cases.py runs under five schedules --
the pool poisoned with 0x00 and 0xFF, the outputs poisoned with 0x00 and 0xFF, a decoy problem of the same shapes first --
and must give the bits of the plain schedule.  The controls show that a pass means something: the poison reaches fresh
and recycled blocks, recycling is real, every case that has scratch got poisoned scratch, every case whose wrapper
allocates uninitialised outputs got poisoned outputs, and an output that is not written is reported.
"""
import numpy as np
import pytest
import torch

from tests import stale_cases as ST
from tests import stream_cases as SC

pytestmark = pytest.mark.gpu

ALL_CASES = SC.CASES + ST.EDGE_CASES


@pytest.fixture(scope="module")
def plain(gpu):
    """plain(case) -> the snapshot of the plain schedule, made once per case."""
    from corsair_amd import backend as B

    snaps = {}

    def get(case):
        if case.name not in snaps:
            snaps[case.name], _ = SC.run_plain(B, case, gpu)
        return snaps[case.name]

    get.B = B
    return get


@pytest.mark.parametrize("schedule", ST.SCHEDULES)
@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_schedule_gives_the_plain_bits(gpu, plain, monkeypatch, case, schedule):
    want = plain(case)
    snap, info = ST.run_schedule(plain.B, case, gpu, schedule, monkeypatch)
    print("stale case %-26s %-11s %s" % (case.name, schedule, info))
    diff = SC.first_difference(snap, want)
    assert diff is None, "%s under %s differs from the plain schedule: %s" % (case.name, schedule, diff)
    listed = case in SC.CASES      # the two count controls name stream cases; an edge case's counts are printed only
    if schedule.startswith("scratch") and listed:
        if case.name in ST.SCRATCH_FREE:
            assert info["blocks"] == 0, "%s is listed as scratch-free and took %d pool blocks" % (case.name, info["blocks"])
        else:
            assert info["blocks"] > 0, "%s took no pool block: the schedule proves nothing about it" % case.name
    if schedule.startswith("outputs") and listed and ST.returns_device_tensor(snap):
        if case.name in ST.NO_EMPTY_OUTPUTS:
            assert info["allocations"] == 0, "%s is listed as allocating nothing through torch.empty" % case.name
        else:
            assert info["allocations"] > 0, "%s allocated nothing through torch.empty: the schedule proves nothing" % case.name


def test_every_stream_case_runs_under_all_five_schedules():
    """Needs no device: the parametrisation above is the product of the five schedules and a list that holds every case
    of SC.CASES (a new operator's stream case is covered without a change here) and every edge case."""
    marks = {m.args[0]: list(m.args[1]) for m in test_schedule_gives_the_plain_bits.pytestmark if m.name == "parametrize"}
    assert marks["schedule"] == ["scratch-00", "scratch-ff", "outputs-00", "outputs-ff", "decoy-first"]
    assert len(SC.CASES) > 0 and all(any(c is p for p in marks["case"]) for c in SC.CASES)
    assert all(any(c is p for p in marks["case"]) for c in ST.EDGE_CASES)
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    for listed in (ST.SCRATCH_FREE, ST.NO_EMPTY_OUTPUTS):
        assert len(set(listed)) == len(listed) and set(listed) <= set(SC.BY_NAME)


@pytest.mark.parametrize("case", ST.EDGE_CASES, ids=repr)
def test_edge_case_relation(gpu, plain, case):
    """The live parts equal the same call on the batch without the empty parts, bit for bit; the empty parts hold what the
    header documents."""
    ST.check_relation(plain.B, case, gpu)


# ---- controls ------------------------------------------------------------------------------------------------------
PEEK_BYTES = 3 << 20          # a 4 MiB size class


def test_pool_peek_sees_the_poison_in_fresh_and_recycled_blocks(gpu):
    from corsair_amd import _lib

    lib = _lib.load()
    torch.cuda.synchronize()
    lib.cs_pool_trim()        # the thread's cache is empty: the next block of any class is fresh from the driver
    ST.poison_stats(reset=True)
    with ST.pool_poison(0xA5):
        got = ST.pool_peek(PEEK_BYTES, gpu)
        assert got.size == PEEK_BYTES and (got == 0xA5).all(), "a fresh block was not poisoned"
        assert ST.poison_stats() == (1, 4 << 20), "one block, poisoned over its whole size class"
    # hook off: the block freed holding 0xA5 comes back holding it -- recycling is real, and nothing is filled any more
    got = ST.pool_peek(PEEK_BYTES, gpu)
    assert (got == 0xA5).all(), "the pool did not hand the freed block out again"
    assert ST.poison_stats() == (1, 4 << 20)
    for pattern in (0x00, 0xFF):      # the same class again, cached with other contents
        with ST.pool_poison(pattern):
            got = ST.pool_peek(PEEK_BYTES, gpu)
        assert (got == pattern).all(), "a recycled block was not poisoned with 0x%02x" % pattern
    assert ST.poison_stats(reset=True) == (3, 3 * (4 << 20))
    got = ST.pool_peek(PEEK_BYTES, gpu)
    assert (got == 0xFF).all() and ST.poison_stats() == (0, 0), "the hook is still on after cs_pool_poison(-1)"


def _mk_copy(seed):
    """f32 [37, 5]; no byte of it is 0x00 or 0xFF (1.23f = 0x3F9D70A4, the decoy 4.56f = 0x4091EB85)."""
    return {"x": np.full((37, 5), 1.23 if seed < 1000 else 4.56, np.float32)}


def _copy_written(B, d):
    out = B.torch.empty(d["x"].shape, dtype=d["x"].dtype, device=d["x"].device)
    out.copy_(d["x"])
    return out


def _copy_unwritten(B, d):
    return B.torch.empty(d["x"].shape, dtype=d["x"].dtype, device=d["x"].device)


def _copy_but_last_row(B, d):
    out = B.torch.empty(d["x"].shape, dtype=d["x"].dtype, device=d["x"].device)
    out[:-1].copy_(d["x"][:-1])
    return out


@pytest.mark.parametrize("schedule", ["outputs-00", "outputs-ff"])
def test_an_unwritten_output_is_reported(gpu, monkeypatch, schedule):
    """The check bites: wrappers that allocate through B.torch.empty as backend.py does and leave the tensor, or its last
    row, unwritten differ from the wrapper that writes everything -- under BOTH patterns, with the right byte count."""
    from corsair_amd import backend as B

    want, _ = SC.run_plain(B, SC.Case("copy", _mk_copy, _copy_written), gpu)
    snap, info = ST.run_schedule(B, SC.Case("copy", _mk_copy, _copy_written), gpu, schedule, monkeypatch)
    assert SC.first_difference(snap, want) is None and info["allocations"] == 1 and info["bytes"] == 37 * 5 * 4
    snap, info = ST.run_schedule(B, SC.Case("copy", _mk_copy, _copy_unwritten), gpu, schedule, monkeypatch)
    assert SC.first_difference(snap, want) == "output 0 (torch.float32 (37, 5)): 740 of 740 bytes differ"
    snap, info = ST.run_schedule(B, SC.Case("copy", _mk_copy, _copy_but_last_row), gpu, schedule, monkeypatch)
    assert SC.first_difference(snap, want) == "output 0 (torch.float32 (37, 5)): 20 of 740 bytes differ"
    assert B.torch is torch
