"""GPU tests of the paired-lane forms of the fp32 2^20 persistent kernel (csrc/fft_col2.hpp PAIR_IN / PAIR_OUT, csrc/fft_fused2.hpp,
docs/persistent.md): lanes i and i + 32 of a wave own adjacent columns, fetch 16 bytes of two different rows and trade halves, so a
stream moves 16 bytes per lane on the 16-column tile.  Only the lane that computes a point changes, never the operations on it: every
form the library holds -- selected through MIFFT_DEBUG_PAIR_LANES, the default included -- must give the plain chain's bits over whole
arrays, forward and inverse, in and out of place, at a batch that is ragged against the smallest ring (29 against 14 slots) and one
that wraps it more than twice (57).  (Up to the cache size per side a plan runs the chain on its own, so the batch of 29 -- 232 MiB --
asks for the persistent launch with PYFFT_AMD_STRATEGY=fused: lag 7, ring 14; 57 is the planner's own choice, lag 14, ring 28.)
That covers the first and last tile of a transform, slot wrap-around, the upper half-wave's
offsets and the operand order of the trade.

Bases that are not 16-byte aligned: the C ABI refuses them at every entry point (include/mifft.h; tests/test_host.py pins
mifft_launch_fused2's refusal of exactly this launch), so a paired form never sees one -- the launcher's own fall-back to form 0 is a
second line behind that check.  What the tests hold the plan to is that such an execute is refused before anything is enqueued: a
ValueError, the output and its guards untouched, for every form."""
import numpy
import pytest

import pyfft_oracle as oracle
from helpers import EPS_F, MAX_F, GuardedBuffer, _execute, _test_data

pytestmark = pytest.mark.gpu

N20 = 1 << 20
# values of the switch: 0 = the default form of the shape, n = form n - 1.  The library holds form 0 (8-byte lanes on every stream: the
# fallback) and form 3 (16-byte lanes on every stream); forms 1 and 2 (the ring side alone) were measured and not kept
SWITCH_VALUES = (0, 1, 4)
NO_SUCH_FORMS = (2, 3, 5, -1)
_cache = {}


def _data(batch):
    if "data" not in _cache:
        _cache["data"] = _test_data((N20,), numpy.complex64, 57, 20)
        _cache["data"].setflags(write=False)
    return _cache["data"][:batch * N20]


def _chain(ctx, monkeypatch, batch, inverse):
    """the chain's result for the first `batch` transforms of the data set (computed once per direction, at batch 57: the chain runs
    every transform on its own, so a shorter batch is a prefix)"""
    key = ("chain", inverse)
    if key not in _cache:
        monkeypatch.setenv("PYFFT_AMD_STRATEGY", "chain")
        _cache[key] = _execute(ctx, (N20,), numpy.complex64, 57, _data(57), inverse=inverse, expect="chain")
        _cache[key].setflags(write=False)
        monkeypatch.setenv("PYFFT_AMD_STRATEGY", "auto")
    return _cache[key][:batch * N20]


def _persistent(monkeypatch, batch):
    """the persistent launch for this batch: the planner's own choice where it is one, on request below the cache size"""
    monkeypatch.setenv("PYFFT_AMD_STRATEGY", "auto" if batch * N20 * 8 > (256 << 20) else "fused")


class _Form(object):
    """MIFFT_DEBUG_PAIR_LANES = value on this thread for the block"""

    def __init__(self, ctx, value):
        self.N, self.value = ctx.hip.N, value

    def __enter__(self):
        self.N.check(self.N.lib.mifft_debug_set(self.N.DEBUG_PAIR_LANES, self.value), "debug_set")
        return self

    def __exit__(self, *exc):
        self.N.check(self.N.lib.mifft_debug_set(self.N.DEBUG_PAIR_LANES, 0), "debug_set")


def _form_taken(ctx, value):
    """the form a launch under switch value `value` reports: the asked one, or whatever the default is"""
    got = ctx.hip.N.lib.mifft_debug_last_pair_lanes_form()
    assert got >= 0 and (value == 0 or got == value - 1), (value, got)
    return got


@pytest.mark.parametrize("batch", [29, 57])
@pytest.mark.parametrize("value", SWITCH_VALUES)
def test_every_form_gives_the_chains_bits(ctx, monkeypatch, value, batch):
    data = _data(batch)
    for inverse in (False, True):
        want = _chain(ctx, monkeypatch, batch, inverse)
        _persistent(monkeypatch, batch)
        with _Form(ctx, value):
            for inplace in (False, True):
                got = _execute(ctx, (N20,), numpy.complex64, batch, data, inplace=inplace, inverse=inverse, expect="fused2")
                _form_taken(ctx, value)
                assert numpy.array_equal(got, want), (value, batch, inverse, inplace)


def test_default_form_is_the_one_the_switch_names(ctx, monkeypatch):
    """value 0 runs one of the forms the other values name, and the getter says which"""
    data = _data(29)
    _persistent(monkeypatch, 29)
    with _Form(ctx, 0):
        _execute(ctx, (N20,), numpy.complex64, 29, data, expect="fused2")
        default = _form_taken(ctx, 0)
    assert default + 1 in SWITCH_VALUES


def test_a_form_the_library_lacks_is_refused(ctx, monkeypatch):
    """asking for a form without an instance raises (MIFFT_E_UNSUPPORTED): never another kernel"""
    data = _data(29)
    _persistent(monkeypatch, 29)
    plan = ctx.getPlan((N20,), dtype=numpy.complex64)
    assert plan.strategy(29)[0] == "fused2"
    a, b = ctx.toGpu(data), ctx.allocate(data.shape, data.dtype)
    for value in NO_SUCH_FORMS:
        with _Form(ctx, value):
            with pytest.raises(RuntimeError, match="no kernel"):
                plan.execute(a, b, batch=29)
    plan.execute(a, b, batch=29)               # and the plan works again
    assert numpy.array_equal(a.get(), data)


@pytest.mark.parametrize("off_in,off_out", [(8, 0), (0, 8), (8, 8)])
def test_bases_one_element_past_a_16_byte_boundary_are_refused_untouched(ctx, monkeypatch, off_in, off_out):
    """the input, the output or both one complex64 (8 bytes) into a larger allocation: refused by the entry point with a ValueError
    before anything is enqueued, whatever form the switch asks for -- the output keeps its pre-filled bytes, both guards theirs, and no
    launch is recorded"""
    N = ctx.hip.N
    batch = 29
    data = _data(batch)
    _persistent(monkeypatch, batch)
    plan = ctx.getPlan((N20,), dtype=numpy.complex64)
    assert plan.strategy(batch)[0] == "fused2"
    gin, gout = GuardedBuffer(data.nbytes, off_in, align=8), GuardedBuffer(data.nbytes, off_out, align=8)
    try:
        N.check(N.lib.mifft_memcpy_h2d(gin.ptr, data.ctypes.data, data.nbytes, None), "mifft_memcpy_h2d")
        N.check(N.lib.mifft_memset(gout.ptr, 0xff, data.nbytes, None), "mifft_memset")
        before = N.lib.mifft_debug_last_pair_lanes_form()
        for value in SWITCH_VALUES:
            with _Form(ctx, value):
                with pytest.raises(ValueError, match="16-byte aligned"):
                    plan.execute(gin.ptr, gout.ptr, batch=batch)
        N.check(N.lib.mifft_device_sync(), "mifft_device_sync")
        assert N.lib.mifft_debug_last_pair_lanes_form() == before
        got = numpy.empty(data.nbytes // 4, numpy.uint32)
        N.check(N.lib.mifft_memcpy_d2h(got.ctypes.data, gout.ptr, data.nbytes, None), "mifft_memcpy_d2h")
        assert (got == 0xffffffff).all()
        gin.check_guards("input")
        gout.check_guards("output")
    finally:
        gin.free()
        gout.free()


def test_accuracy_unchanged(ctx, monkeypatch):
    """three transforms of the batch-29 output of the default form against numpy.fft.fft in complex128, the reference's thresholds"""
    data = _data(29)
    _persistent(monkeypatch, 29)
    got = _execute(ctx, (N20,), numpy.complex64, 29, data, expect="fused2")
    for j in (0, 14, 28):
        ref = numpy.fft.fft(data[j * N20:(j + 1) * N20].astype(numpy.complex128))
        out = got[j * N20:(j + 1) * N20]
        assert oracle.difference(ref, out, 1) < EPS_F
        assert numpy.abs(ref - out).max() / numpy.abs(ref).max() < MAX_F
