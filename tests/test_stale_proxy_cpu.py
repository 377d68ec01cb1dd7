"""The torch proxy of the stale-memory schedules (tests/stale_cases.py) on CPU tensors: what the outputs-00 / outputs-ff
schedules of tests/test_gpu_stale_memory.py rely on."""
import re

import numpy as np
import pytest
import torch

from tests import stale_cases as ST

DTYPES = [torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8]   # what backend.py allocates


def _bytes(t):
    return np.frombuffer(t.contiguous().numpy().tobytes(), np.uint8)


def test_the_dtypes_are_those_backend_allocates():
    import corsair_amd.backend as B

    with open(B.__file__) as f:
        text = f.read()
    used = set()
    for call in re.findall(r"torch\.empty\((?:[^()]|\([^()]*\))*\)", text):
        m = re.search(r"dtype=torch\.(\w+)", call)
        assert m, call
        used.add(getattr(torch, m.group(1)))
    assert used and used <= set(DTYPES), used


@pytest.mark.parametrize("pattern", [0x00, 0xFF, 0xA5])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_empty_is_filled_byte_for_byte(dtype, pattern):
    proxy = ST.PoisonTorch(pattern)
    for shape in [(7,), (3, 5), (2, 4, 4), (0,), (0, 4), ()]:
        t = proxy.empty(shape, dtype=dtype)
        assert t.dtype == dtype and tuple(t.shape) == shape
        raw = _bytes(t)
        assert raw.size == t.numel() * t.element_size() and (raw == pattern).all(), (shape, raw)
    t = proxy.empty(6, dtype=dtype)                       # sizes as positional integers, as torch.empty takes them
    assert tuple(t.shape) == (6,) and (_bytes(t) == pattern).all()


def test_empty_like_is_filled_and_keeps_the_layout():
    proxy = ST.PoisonTorch(0xFF)
    src = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    t = proxy.empty_like(src)
    assert t.shape == src.shape and t.dtype == src.dtype and t.data_ptr() != src.data_ptr()
    assert (_bytes(t) == 0xFF).all() and torch.isnan(t).all()
    assert src[3, 5] == 23                                # the model is left alone
    tt = proxy.empty_like(src.t())                        # a dense, permuted model: torch keeps its strides
    assert tt.stride() == src.t().stride() and (_bytes(tt) == 0xFF).all()
    z = proxy.empty_like(torch.zeros((0, 3), dtype=torch.int64))
    assert tuple(z.shape) == (0, 3) and z.dtype == torch.int64
    i = proxy.empty_like(src, dtype=torch.int32)
    assert i.dtype == torch.int32 and (i == -1).all()


def test_the_counter_counts():
    proxy = ST.PoisonTorch(0)
    assert (proxy.count, proxy.bytes) == (0, 0)
    proxy.empty((3, 5), dtype=torch.float64)
    proxy.empty((0,), dtype=torch.int32)
    proxy.empty_like(torch.zeros(4, dtype=torch.uint8))
    assert (proxy.count, proxy.bytes) == (3, 3 * 5 * 8 + 0 + 4)
    proxy.zeros(9)                                        # forwarded: initialised allocations are not counted
    proxy.full((2,), -1)
    assert proxy.count == 3


def test_other_attributes_are_torchs_own():
    proxy = ST.PoisonTorch(0xFF)
    for name in ("zeros", "full", "float32", "int64", "Tensor", "is_tensor", "cuda", "as_tensor", "cat", "is_grad_enabled"):
        assert getattr(proxy, name) is getattr(torch, name), name
    assert isinstance(proxy.zeros(2), proxy.Tensor) and proxy.zeros(2).sum() == 0
    with pytest.raises(AttributeError):
        proxy.no_such_attribute
    with pytest.raises(AssertionError):
        ST.PoisonTorch(256)


def test_backend_torch_is_patched_for_the_block_only(monkeypatch):
    import corsair_amd.backend as B
    import corsair_amd._lib as L

    assert B.torch is torch
    with ST.poisoned_outputs(monkeypatch, B, 0xFF) as proxy:
        assert B.torch is proxy and L.__dict__.get("torch", torch) is torch
        t = B.torch.empty((2, 3), dtype=torch.int32)
        assert (t == -1).all() and proxy.count == 1
        assert torch.empty is not proxy.empty             # the module torch itself is untouched
    assert B.torch is torch
    with pytest.raises(RuntimeError):
        with ST.poisoned_outputs(monkeypatch, B, 0x00):
            raise RuntimeError("a failing case")
    assert B.torch is torch


def test_schedules_and_lists_name_existing_cases():
    from tests import stream_cases as SC

    assert ST.SCHEDULES == ["scratch-00", "scratch-ff", "outputs-00", "outputs-ff", "decoy-first"]
    assert set(ST.SCRATCH_FREE) | set(ST.NO_EMPTY_OUTPUTS) <= set(SC.BY_NAME)
    names = [c.name for c in ST.EDGE_CASES]
    assert len(set(names)) == len(names) and not set(names) & set(SC.BY_NAME)
    for case in ST.EDGE_CASES:                            # the generators run without a device, twice, with equal shapes
        a, b = case.make(case.seed), case.make(case.seed + 1000)
        assert a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
        assert any(a[k].tobytes() != b[k].tobytes() for k in a)
