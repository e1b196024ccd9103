"""The host state behind a plan's scratch, without a device (docs/parity.md, "Plan lifecycle").

Every plan class that owns batch-sized scratch is built on PooledFakeContext (helpers.py) and driven through the step that
(re)allocates it -- _prepare, for FFTPlan _prepare + _ensure_scratch -- at batch B1, then at B2 with the k-th allocation of the
step failing, for every k the step has, then at B2 again with a healthy pool:

  * after the failure the plan is in the state close() leaves: no scratch, batch 0 (a plan that believed its old scratch fitted the
    new batch would run the next execute of that batch on it: an out-of-range device write when the new batch is larger);
  * the retry requests every allocation again, at B2's size;
  * scratch a recorded graph replays on stays in _capture_keepalive;
  * scratch that came from a pool is let go of only after wait_scratch(), and never waited for once a graph keeps it.

GenericFFTPlan also refuses, on a context that is capturing, an execute that would allocate: before the pool is asked.
FirPlan's step is filter_spectrum's (its execute needs no scratch).  HalfFFTPlan owns no scratch and has no such step.
"""
import numpy
import pytest

from helpers import FailingPool, PooledFakeContext
from kernel_coverage import full_machine, long_limits, _smooth_upto

B1, B2 = 3, 5


class _Drive(object):
    """One plan kind: how to build it, how to run the allocating step, what it then holds and what it must have asked the pool for."""

    def __init__(self, name, build, sizes, step=None, scratch=("_scratch",), batch_attr="_last_batch", setup=None, batches=(B1, B2)):
        self.name, self.build, self.sizes, self.scratch, self.batch_attr, self.setup = name, build, sizes, scratch, batch_attr, setup
        self.b1, self.b2 = batches
        self.step = step or (lambda plan, batch: plan._prepare(batch))

    def held(self, plan):
        return [getattr(plan, a) for a in self.scratch]

    def batch(self, plan):
        return getattr(plan, self.batch_attr)

    def assert_closed(self, plan, what):
        assert self.batch(plan) == 0, "%s: the plan believes it is prepared for batch %d" % (what, self.batch(plan))
        assert all(h is None for h in self.held(plan)), "%s: the plan still holds %s" % (what, self.held(plan))
        if hasattr(plan, "_scratch_ready"):
            assert not plan._scratch_ready, what


def _fft_step(plan, batch):
    plan._prepare(batch)
    plan._ensure_scratch()


def _fft(shape, dtype):
    from pyfft_amd.plan import FFTPlan
    return lambda ctx: FFTPlan(ctx, shape, dtype=dtype)


def _generic(shape, dtype, parent=None):
    def build(ctx):
        from pyfft_amd import generic
        kw = {"parent_shape": parent} if parent is not None else {"any_size": True}
        saved = generic._unit_roots, generic._chirp, generic._bluestein_spectrum      # (tables go nowhere: kernel_coverage.ext_plan)
        generic._unit_roots = lambda count, step, period: numpy.zeros(count, numpy.complex128)
        generic._chirp = lambda n, *a: numpy.zeros(n, numpy.complex128)
        generic._bluestein_spectrum = lambda n, m: numpy.zeros(m, numpy.complex128)
        try:
            return generic.GenericFFTPlan(ctx, shape, dtype=dtype, **kw)
        finally:
            generic._unit_roots, generic._chirp, generic._bluestein_spectrum = saved
    return build


def _real(shape, dtype):
    from pyfft_amd.real import RealFFTPlan
    return lambda ctx: RealFFTPlan(ctx, shape, dtype=dtype)


def _conv(shape, dtype):
    from pyfft_amd.conv import ConvPlan
    return lambda ctx: ConvPlan(ctx, shape, dtype=dtype, real=True)


def _r2r(shape, dtype):
    from pyfft_amd.r2r import R2RPlan
    return lambda ctx: R2RPlan(ctx, shape, dtype=dtype, r2r="dct")


def _fir(dtype, real=False):
    from pyfft_amd.fir import FirPlan
    return lambda ctx: FirPlan(ctx, 256, dtype=dtype, real=real, taps=33)


def _smallest_long():
    top = long_limits(numpy.complex64)[0]
    import ctypes
    from pyfft_amd import _native as N
    a, b = ctypes.c_int32(0), ctypes.c_int32(0)
    return min(n for n in _smooth_upto(top) if n > 4096 and N.lib.mifft_mixed_long_split(N.F32, n, ctypes.byref(a), ctypes.byref(b)) == 0)


class _DeviceObject(object):
    def take(self):         # (ErrorWord: nothing reported)
        return 0


def _force(strategy, pipe_mb=None):
    def setup(monkeypatch):
        import pyfft_amd.hip as hip
        monkeypatch.setenv("PYFFT_AMD_STRATEGY", strategy)
        if pipe_mb is not None:
            monkeypatch.setenv("PYFFT_AMD_PIPE_MB", str(pipe_mb))
        # what _ensure_scratch creates next to its allocations needs a device: stand-ins
        for name in ("ErrorWord", "Stream", "Event"):
            monkeypatch.setattr(hip, name, _DeviceObject)
    return setup


def _fused2_sizes(batch):
    from pyfft_amd import _native as N
    from pyfft_amd.plan import FFTPlan
    plan = FFTPlan(PooledFakeContext(full_machine()), (1 << 16,), dtype=numpy.complex64)
    strat = plan._select_strategy(batch)
    assert strat[0] == "fused2", strat
    return [3 * N.fused2_counter_bytes(batch), strat[2] * (1 << 16) * 8]


def _pipelined_sizes(batch):
    from pyfft_amd.plan import FFTPlan
    plan = FFTPlan(PooledFakeContext(full_machine()), (1 << 16,), dtype=numpy.complex64)
    strat = plan._select_strategy(batch)
    assert strat[0] == "pipelined", strat
    return [strat[1] * strat[2] * (1 << 16) * 8]


_FFT_STATE = dict(step=_fft_step, scratch=("_tempmemobj", "_counters"), batch_attr="_last_batch_size")
# 16411: the smallest prime whose padded rows (65536 points) are beyond the one-launch Bluestein kernel, so that an interleaved 1-D plan
# has work arrays (4099 complex64 runs that kernel straight on the user's buffers); (17, 4): axis lengths 4 (x, a power of two, m = 4) and 17 (y, Bluestein in one launch, m = 17): rows = the work array's size
DRIVES = [
    _Drive("fft-chain-temp-c64", _fft((1 << 17,), numpy.complex64), lambda b: [b * (1 << 17) * 8], **_FFT_STATE),
    _Drive("fft-chain-temp-f32-planes", _fft((1 << 17,), numpy.float32), lambda b: [b * (1 << 17) * 8], **_FFT_STATE),
    _Drive("fft-fused2", _fft((1 << 16,), numpy.complex64), _fused2_sizes, setup=_force("fused"), batches=(9, 13), **_FFT_STATE),
    _Drive("fft-pipelined", _fft((1 << 16,), numpy.complex64), _pipelined_sizes, setup=_force("pipelined", 1), batches=(9, 13), **_FFT_STATE),
    _Drive("generic-work-f32-planes", _generic((17, 4), numpy.float32), lambda b: [b * 68 * 8, b * 68 * 8], scratch=("_work", "_rows")),
    _Drive("generic-work-c64", _generic((16411,), numpy.complex64), lambda b: [b * 16411 * 8, b * 65536 * 8], scratch=("_work", "_rows")),
    _Drive("generic-tiles-gather", _generic((16, 4), numpy.complex64, parent=(64, 64)), lambda b: [b * 4096 * 8, b * 4096 * 8],
           scratch=("_work", "_rows")),
    _Drive("generic-long-in-place", lambda ctx: _generic((_smallest_long(),), numpy.complex64)(ctx),
           lambda b: [b * _smallest_long() * 8], step=lambda plan, b: plan._prepare(b, long_scratch=True), scratch=("_work", "_rows")),
    _Drive("real-composed", _real((8, 16), numpy.float32), lambda b: [b * 64 * 8]),
    _Drive("real-composed-f64", _real((1 << 17,), numpy.float64), lambda b: [b * (1 << 16) * 16]),
    _Drive("conv-real-composed", _conv((8, 16), numpy.float32), lambda b: [b * 8 * 9 * 8]),
    _Drive("r2r-composed", _r2r((8, 8), numpy.float64), lambda b: [b * 64 * 8]),
    _Drive("fir-filter-spectrum-c64", _fir(numpy.complex64), lambda b: [b * 256 * 8]),
    _Drive("fir-filter-spectrum-f32-real", _fir(numpy.float32, real=True), lambda b: [b * 256 * 4]),
]


@pytest.fixture(params=DRIVES, ids=[d.name for d in DRIVES])
def drive(request, monkeypatch):
    d = request.param
    if d.setup is not None:
        d.setup(monkeypatch)
    return d


def _fresh(drive):
    ctx = PooledFakeContext(full_machine())
    plan = drive.build(ctx)
    ctx.pool.arm(None)
    return ctx, plan


def test_the_step_asks_for_the_batch_it_runs(drive):
    ctx, plan = _fresh(drive)
    for batch in (drive.b1, drive.b1, drive.b2, drive.b1):
        ctx.pool.arm(None)
        was = drive.batch(plan)
        drive.step(plan, batch)
        assert ctx.pool.requests == ([] if batch == was else drive.sizes(batch)), (drive.name, batch)
        assert drive.batch(plan) == batch
        # what the plan holds is what this step (or the one that prepared the batch) was given: one block per request, of its size
        assert sorted(h.nbytes for h in drive.held(plan) if h is not None) == sorted(drive.sizes(batch)), (drive.name, batch)


@pytest.mark.parametrize("grow", [True, False], ids=["grow", "shrink"])
def test_failed_allocation_leaves_the_closed_state_and_the_retry_allocates_again(drive, grow):
    b_from, b_to = (drive.b1, drive.b2) if grow else (drive.b2, drive.b1)
    steps = len(drive.sizes(b_to))
    for k in range(1, steps + 1):
        ctx, plan = _fresh(drive)
        drive.step(plan, b_from)
        assert drive.batch(plan) == b_from and ctx.waits == 0
        ctx.pool.arm(k)
        with pytest.raises(MemoryError):
            drive.step(plan, b_to)
        what = "%s: allocation %d of %d at batch %d failed" % (drive.name, k, steps, b_to)
        assert ctx.pool.requests == drive.sizes(b_to)[:k], what
        drive.assert_closed(plan, what)
        assert plan._capture_keepalive == [], what
        assert ctx.waits >= 1, what + ": pooled scratch of batch %d was let go of without waiting for the plan's stream" % b_from
        ctx.pool.arm(None)
        drive.step(plan, b_to)
        assert ctx.pool.requests == drive.sizes(b_to), what + ", retry: the plan did not ask for every allocation again at the new size"
        assert drive.batch(plan) == b_to
        assert sorted(h.nbytes for h in drive.held(plan) if h is not None) == sorted(drive.sizes(b_to)), what


def test_failed_allocation_keeps_what_a_recorded_graph_replays_on(drive):
    ctx, plan = _fresh(drive)
    drive.step(plan, drive.b1)
    recorded = [h for h in drive.held(plan) if h is not None]
    plan._captured = True             # (what an execute on a capturing stream leaves behind)
    ctx.pool.arm(1)
    with pytest.raises(MemoryError):
        drive.step(plan, drive.b2)
    drive.assert_closed(plan, drive.name)
    kept = []
    for entry in plan._capture_keepalive:
        kept += list(entry) if isinstance(entry, tuple) else [entry]
    assert all(any(k is r for k in kept) for r in recorded), (drive.name, plan._capture_keepalive)
    assert len(plan._capture_keepalive) == 1
    assert ctx.waits == 0, "scratch that is kept alive is not released: nothing to wait for"


def test_close_waits_before_pooled_scratch_goes_back(drive):
    ctx, plan = _fresh(drive)
    drive.step(plan, drive.b1)
    plan.close()
    drive.assert_closed(plan, drive.name + " after close()")
    assert ctx.syncs >= 1 and ctx.waits >= 1
    ctx.pool.arm(None)
    drive.step(plan, drive.b1)
    assert ctx.pool.requests == drive.sizes(drive.b1)


def test_scratch_allocated_lazily_after_an_out_of_place_execute_fails_into_the_closed_state():
    """(16, 2048) float32 planes: out of place the plan takes the one-launch route, which needs no scratch, so an out-of-place execute of
    a new batch only commits the batch (_prepare); the temp buffer of the chain is allocated by the first IN-PLACE execute of that batch
    (_ensure_scratch alone).  That allocation failing must not leave a plan that believes the batch is ready."""
    from pyfft_amd.plan import FFTPlan
    ctx = PooledFakeContext(full_machine())
    plan = FFTPlan(ctx, (16, 2048), dtype=numpy.float32)
    assert plan._temp_buffer_needed and plan.strategy(B1, inplace=False) == ("nd_oop",) and plan.strategy(B1)[0] == "chain"
    size = lambda b: [b * 16 * 2048 * 8]
    ctx.pool.arm(None)
    plan._prepare(B2)                       # an out-of-place execute of a new batch: nothing asked for
    assert ctx.pool.requests == [] and plan._last_batch_size == B2 and plan._tempmemobj is None and not plan._scratch_ready
    plan._ensure_scratch()                  # the first in-place one
    assert ctx.pool.requests == size(B2) and plan._scratch_ready
    held = plan._tempmemobj
    plan._prepare(B1)                       # out of place at another batch: the temp buffer goes, after the wait
    assert ctx.waits == 1 and plan._tempmemobj is None and not plan._scratch_ready and plan._last_batch_size == B1
    ctx.pool.arm(1)
    with pytest.raises(MemoryError):
        plan._ensure_scratch()
    assert plan._last_batch_size == 0 and plan._tempmemobj is None and not plan._scratch_ready
    ctx.pool.arm(None)
    plan._prepare(B1)
    plan._ensure_scratch()
    assert ctx.pool.requests == size(B1) and plan._tempmemobj is not held and plan._tempmemobj.nbytes == size(B1)[0]
    plan.close()
    assert plan._tempmemobj is None and plan._last_batch_size == 0 and ctx.waits == 2


# ---- GenericFFTPlan on a capturing stream -------------------------------------------------------------------------------------------
GENERIC_CAPTURE = [("work-f32-planes", (17, 4), numpy.float32, None, False), ("work-c64", (16411,), numpy.complex64, None, False),
                   ("tiles-gather", (16, 4), numpy.complex64, (64, 64), False), ("long-in-place", None, numpy.complex64, None, True)]


@pytest.mark.parametrize("name,shape,dtype,parent,inplace", GENERIC_CAPTURE, ids=[c[0] for c in GENERIC_CAPTURE])
@pytest.mark.parametrize("prepared", [False, True], ids=["never-run", "other-batch-run"])
def test_generic_plan_refuses_to_allocate_on_a_capturing_stream(name, shape, dtype, parent, inplace, prepared):
    shape = shape if shape is not None else (_smallest_long(),)
    ctx = PooledFakeContext(full_machine())
    plan = _generic(shape, dtype, parent)(ctx)
    if prepared:
        plan._prepare(B1, long_scratch=True) if inplace else plan._prepare(B1)
    held = (plan._work, plan._rows, plan._last_batch)
    ctx.pool.arm(None)
    ctx.is_capturing = True
    planes = 2 if numpy.dtype(dtype).kind == "f" else 1
    src = [FailingPool.Block(0) for _ in range(planes)]
    dst = src if inplace else [FailingPool.Block(0) for _ in range(planes)]
    with pytest.raises(RuntimeError, match="needs one eager execute\\(\\) of the same batch first"):
        if inplace:
            plan.execute(*src, batch=B2, wait_for_finish=False)
        else:
            plan.execute(*(src + dst), batch=B2, wait_for_finish=False)
    assert ctx.pool.requests == [], "the plan asked the pool for %s inside a capture" % ctx.pool.requests
    assert (plan._work, plan._rows, plan._last_batch) == held, "the refusal changed the plan's state"
    assert plan._capture_keepalive == [] and not plan._captured and ctx.waits == 0


def test_generic_long_plan_out_of_place_records_without_scratch():
    """out of place the long smooth transform needs no scratch: a capture at a new batch allocates nothing, releases nothing (the
    in-place scratch of the other batch moves to the keep-alive list) and goes on to its launch"""
    ctx = PooledFakeContext(full_machine())
    plan = _generic((_smallest_long(),), numpy.complex64)(ctx)
    plan._prepare(B1, long_scratch=True)
    scratch = plan._work
    ctx.pool.arm(None)
    ctx.is_capturing = True
    with pytest.raises(AssertionError, match="went on to a launch"):
        plan.execute(FailingPool.Block(0), FailingPool.Block(0), batch=B2, wait_for_finish=False)
    assert ctx.pool.requests == [] and ctx.waits == 0
    assert plan._work is None and plan._capture_keepalive == [(scratch, None)]
