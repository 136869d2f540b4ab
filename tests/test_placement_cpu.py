"""``beat._device.place_buffer``'s fallbacks by Python fault injection, on a host stand-in for the device context: an allocation
that runs out of memory once candidates are held, a probe that refuses the layout, a layout the probe cannot take, a device
without room for a second candidate.  The probe's rates are injected too; the routine's real run is tests/test_gpu_kernels.py."""

import types

import pytest
import torch

from beat import _device, _hip

NUMEL = 1 << 18  # 2 MiB: above the lowered threshold


class FakeContext:
    """What place_buffer uses of a Context: ``zeros``, ``torch.cuda.mem_get_info`` / ``empty_cache`` and ``device``."""

    def __init__(self, oom_on_call=None, free_bytes=1 << 40):
        self.device = None
        self.allocated = []
        self.emptied = 0
        self.oom_on_call = oom_on_call
        cuda = types.SimpleNamespace(mem_get_info=lambda device: (free_bytes, 1 << 40), empty_cache=self._empty_cache)
        self.torch = types.SimpleNamespace(cuda=cuda)

    def _empty_cache(self):
        self.emptied += 1

    def zeros(self, n):
        if len(self.allocated) + 1 == self.oom_on_call:
            raise RuntimeError("HIP out of memory (injected)")
        self.allocated.append(torch.zeros(int(n), dtype=torch.float64))
        return self.allocated[-1]


@pytest.fixture
def probe(monkeypatch):
    """The probe's results, one per call: a rate in GB/s, or an exception to raise."""
    results, calls = [], []

    def fake(ctx, buf, offset, n, rows, ld):
        calls.append((offset, n, rows, ld))
        r = results[len(calls) - 1]
        if isinstance(r, Exception):
            raise r
        return r

    monkeypatch.setenv("BEAT_STATE_PLACE_MIN_BYTES", str(1 << 20))
    monkeypatch.setattr(_device, "_probe_rate", fake)
    return types.SimpleNamespace(results=results, calls=calls)


def place(ctx, offset=4096, ld=4096 * 3, tries=3):
    return _device.place_buffer(ctx, NUMEL, offset=offset, n=4096, rows=4, ld=ld, tries=tries)


def assert_usable(buf):
    assert buf.numel() == NUMEL and float(buf.abs().max()) == 0.0


def test_keeps_the_fastest_candidate(probe):
    probe.results[:] = [3.0, 7.04, 5.0]
    ctx = FakeContext()
    buf, rec = place(ctx)
    assert rec == {"candidates": [3.0, 7.0, 5.0], "chosen": 1, "rows_probed": 4, "unit": "GB/s"}
    assert buf is ctx.allocated[1] and ctx.emptied == 1
    assert probe.calls == [(4096, 4096, 4, 4096 * 3)] * 3


def test_below_threshold_or_off_is_one_plain_allocation(probe, monkeypatch):
    for tries in (0, 1):
        ctx = FakeContext()
        buf, rec = place(ctx, tries=tries)
        assert rec is None and len(ctx.allocated) == 1
    monkeypatch.setenv("BEAT_STATE_PLACE_MIN_BYTES", str(8 * NUMEL + 8))
    ctx = FakeContext()
    buf, rec = place(ctx)
    assert rec is None and len(ctx.allocated) == 1 and not probe.calls and ctx.emptied == 0
    assert_usable(buf)


def test_out_of_memory_on_a_later_candidate_chooses_among_those_held(probe):
    probe.results[:] = [4.0, 9.0]
    ctx = FakeContext(oom_on_call=3)
    buf, rec = place(ctx)
    assert rec["candidates"] == [4.0, 9.0] and rec["chosen"] == 1 and buf is ctx.allocated[1] and ctx.emptied == 1
    probe.calls.clear()
    ctx = FakeContext(oom_on_call=2)
    buf, rec = place(ctx)
    assert rec["candidates"] == [4.0] and rec["chosen"] == 0 and ctx.emptied == 0
    assert_usable(buf)


def test_out_of_memory_on_the_first_allocation_propagates(probe):
    with pytest.raises(RuntimeError, match="out of memory"):
        place(FakeContext(oom_on_call=1))


def test_no_room_for_a_second_candidate(probe):
    probe.results[:] = [4.0]
    ctx = FakeContext(free_bytes=2 * 8 * NUMEL - 1)
    buf, rec = place(ctx)
    assert rec["candidates"] == [4.0] and len(ctx.allocated) == 1 and ctx.emptied == 0
    assert_usable(buf)


def test_probe_refusal_keeps_the_first_candidate(probe):
    probe.results[:] = [6.0, _hip.BeatHipError("libbeat_hip error -2: injected")]
    ctx = FakeContext()
    buf, rec = place(ctx)
    assert list(rec) == ["skipped"] and "injected" in rec["skipped"]
    assert buf is ctx.allocated[0] and len(ctx.allocated) == 2 and ctx.emptied == 1
    assert_usable(buf)
    probe.calls.clear()
    probe.results[:] = [_hip.BeatHipError("libbeat_hip error -2: injected")]
    ctx = FakeContext()
    buf, rec = place(ctx)
    assert list(rec) == ["skipped"] and buf is ctx.allocated[0] and len(ctx.allocated) == 1 and ctx.emptied == 0


@pytest.mark.parametrize("offset, ld", [(4095, 4096 * 3), (4096, 4096 * 3 + 1)])
def test_a_layout_the_probe_cannot_take_is_not_probed(probe, offset, ld):
    ctx = FakeContext()
    buf, rec = place(ctx, offset=offset, ld=ld)
    assert list(rec) == ["skipped"] and "16-byte" in rec["skipped"]
    assert len(ctx.allocated) == 1 and not probe.calls and ctx.emptied == 0
    assert_usable(buf)
