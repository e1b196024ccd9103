"""Real-input transforms on the device: Plan(shape, dtype=float32 | float64, real=True) against an extended-precision reference of
numpy's rfftn / irfftn, held to the project's per-item accuracy bound (helpers.accuracy_bound, n_points = prod(shape)), with guard
bands, a poisoned neighbour item, the plan's semantics and its stream / graph interop."""
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import real_model as M                                               # noqa: E402
from helpers import GuardedBuffer, accuracy_bound, item_error, sampled_items   # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = numpy.float32, numpy.float64
CDT = {F32: numpy.complex64, F64: numpy.complex128}


def _hip():
    import pyfft_amd.hip as hip
    if hip.device_count() < 1:
        pytest.fail("no HIP device")
    return hip


def _real_data(shape, dtype, batch, seed):
    r = numpy.random.default_rng(seed)
    return r.standard_normal((batch,) + tuple(shape)).astype(dtype)


def _spec_data(shape, dtype, batch, seed):
    r = numpy.random.default_rng(seed)
    s = (batch,) + tuple(shape[:-1]) + (shape[-1] // 2 + 1,)
    return (r.standard_normal(s) + 1j * r.standard_normal(s)).astype(CDT[dtype])


def _check(shape, dtype, batch, inp, got, inverse, normalize=True, scale=1.0, what=""):
    double = dtype == F64
    n = int(numpy.prod(shape))
    l1b, mxb = accuracy_bound(dtype, n)
    for j in sampled_items(batch, n):
        if inverse:
            ref = M.irfftn_exact(inp[j], shape, double) * ((1.0 if normalize else n) / scale)
        else:
            ref = M.rfftn_exact(inp[j], double) * scale
        l1, mx = item_error(got[j], ref)
        assert l1 <= l1b and mx <= mxb, "%s %s %s item %d %s: L1 %.3g (bound %.3g) max %.3g (bound %.3g)" % (
            what, shape, numpy.dtype(dtype).name, j, "inverse" if inverse else "forward", l1, l1b, mx, mxb)


def _run_guarded(hip, shape, dtype, batch, inverse, seed=7, poison=None):
    """One execute between guard bands; item `poison` of the input holds NaNs, which must not reach its neighbours."""
    plan = hip.Plan(shape, dtype=dtype, real=True)
    inp = _spec_data(shape, dtype, batch, seed) if inverse else _real_data(shape, dtype, batch, seed)
    if poison is not None:
        inp[poison] = numpy.nan
    out_dtype = dtype if inverse else CDT[dtype]
    out_shape = (batch,) + (tuple(shape) if inverse else tuple(shape[:-1]) + (shape[-1] // 2 + 1,))
    nb_out = int(numpy.prod(out_shape)) * numpy.dtype(out_dtype).itemsize
    gi = GuardedBuffer(inp.nbytes, 16)
    go = GuardedBuffer(nb_out, 48)
    from pyfft_amd import _native as N
    N.check(N.lib.mifft_memcpy_h2d(gi.ptr, inp.ctypes.data, inp.nbytes, None), "h2d")
    plan.execute(gi.ptr, go.ptr, inverse=inverse, batch=batch)
    got = numpy.empty(out_shape, out_dtype)
    N.check(N.lib.mifft_memcpy_d2h(got.ctypes.data, go.ptr, nb_out, None), "d2h")
    back = numpy.empty_like(inp)
    N.check(N.lib.mifft_memcpy_d2h(back.ctypes.data, gi.ptr, inp.nbytes, None), "d2h")
    gi.check_guards("input")
    go.check_guards("output")
    assert numpy.array_equal(back, inp, equal_nan=True), "the input was modified"
    gi.free()
    go.free()
    return inp, got


FUSED = [(dt, 1 << e) for dt, top in ((F32, 16), (F64, 15)) for e in range(2, top + 1)]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dtype,n", FUSED, ids=["%s-%d" % (numpy.dtype(d).name, n) for d, n in FUSED])
def test_real_fused_row_instance(dtype, n, inverse):
    """One case per one-launch real-row instance: guard bands, a ragged last work-group (67 rows: never a multiple of the rows per
    work-group), a poisoned item that must not reach its neighbours, the accuracy bound of an n-point transform."""
    hip = _hip()
    plan = hip.Plan((n,), dtype=dtype, real=True)
    assert plan._real_form == "fused_row" and plan.inner_plan is None
    batch = 67 if n <= 2048 else 3
    inp, got = _run_guarded(hip, (n,), dtype, batch, inverse, seed=n, poison=1)
    keep = numpy.array([j for j in range(batch) if j != 1])
    assert numpy.isfinite(got[keep]).all(), "a poisoned item leaked into its neighbours"
    _check((n,), dtype, len(keep), inp[keep], got[keep], inverse, what="fused_row")


COMPOSED = [(1 << 17,), (1 << 20,), (1 << 21,), (1 << 22,), (16, 16), (1024, 1024), (2048, 2048), (4096, 8), (16, 16, 16),
            (64, 64, 64), (256, 256, 256), (2,), (8, 2), (1024,), (32, 4)]


def _batch_for(shape, dtype):
    n = int(numpy.prod(shape)) * numpy.dtype(dtype).itemsize
    return 3 if n <= (64 << 20) else 1


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", COMPOSED, ids=str)
def test_real_composed(shape, dtype, inverse):
    hip = _hip()
    batch = _batch_for(shape, dtype)
    poison = 1 if batch >= 3 else None
    inp, got = _run_guarded(hip, shape, dtype, batch, inverse, poison=poison)
    items = [j for j in range(batch) if j != poison]
    if poison is not None:
        assert numpy.isfinite(got[[0, 2]]).all(), "a poisoned item leaked into its neighbours"
    keep = numpy.array(items)
    _check(shape, dtype, len(items), inp[keep], got[keep], inverse, what="composed")


def test_real_persistent_and_pipelined_inner_strategies():
    """2^22 fp32 real rows: the inner 2^21 complex plan runs its persistent / pipelined strategies at a big batch."""
    hip = _hip()
    shape = (1 << 22,)
    plan = hip.Plan(shape, dtype=F32, real=True)
    batch = 48
    strat = plan.inner_plan.strategy(batch, inplace=False)
    x = _real_data(shape, F32, batch, 3)
    gx = hip.to_gpu(x)
    gs = hip.DeviceArray((batch, (1 << 21) + 1), numpy.complex64)
    plan.execute(gx, gs, batch=batch)
    got = gs.get()
    _check(shape, F32, batch, x, got, False, what="strategy %s" % (strat[0],))
    gy = hip.DeviceArray((batch,) + shape, F32)
    plan.execute(gs, gy, inverse=True, batch=batch)
    y = gy.get()
    for j in sampled_items(batch, 1 << 22):
        assert numpy.abs(y[j] - x[j]).max() <= 1e-4 * numpy.abs(x[j]).max()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", [(256,), (8, 32), (4, 4, 8), (2,)], ids=str)
def test_real_normalize_scale(shape, normalize):
    hip = _hip()
    for dtype in (F32, F64):
        plan = hip.Plan(shape, dtype=dtype, real=True, normalize=normalize, scale=3.5)
        x = _real_data(shape, dtype, 2, 5)
        gs = hip.DeviceArray((2,) + tuple(shape[:-1]) + (shape[-1] // 2 + 1,), CDT[dtype])
        plan.execute(hip.to_gpu(x), gs, batch=2)
        _check(shape, dtype, 2, x, gs.get(), False, normalize, 3.5)
        X = _spec_data(shape, dtype, 2, 6)
        gy = hip.DeviceArray((2,) + tuple(shape), dtype)
        plan.execute(hip.to_gpu(X), gy, inverse=True, batch=2)
        _check(shape, dtype, 2, X, gy.get(), True, normalize, 3.5)


@pytest.mark.parametrize("shape", [(2,), (64,), (1 << 16,), (16, 8), (8, 4, 16)], ids=str)
def test_real_round_trip_and_numpy(shape):
    hip = _hip()
    for dtype, tol in ((F32, 2e-5), (F64, 1e-12)):
        plan = hip.Plan(shape, dtype=dtype, real=True)
        x = _real_data(shape, dtype, 1, 9)
        gx = hip.to_gpu(x)
        gs = hip.DeviceArray((1,) + tuple(shape[:-1]) + (shape[-1] // 2 + 1,), CDT[dtype])
        plan.execute(gx, gs)
        ref = numpy.fft.rfftn(x[0].astype(numpy.float64))
        assert numpy.abs(gs.get()[0] - ref).max() <= tol * numpy.abs(ref).max() * 10
        gy = hip.DeviceArray((1,) + tuple(shape), dtype)
        plan.execute(gs, gy, inverse=True)
        assert numpy.abs(gy.get() - x).max() <= tol * max(1.0, numpy.abs(x).max()) * 10
        # non-Hermitian edge planes: what numpy.fft.irfftn makes of them
        X = _spec_data(shape, dtype, 1, 10)
        plan.execute(hip.to_gpu(X), gy, inverse=True)
        ref = numpy.fft.irfftn(X[0].astype(numpy.complex128), s=shape, axes=tuple(range(len(shape))))
        assert numpy.abs(gy.get()[0] - ref).max() <= tol * max(1.0, numpy.abs(ref).max()) * 10


def test_real_torch_interop_stream_and_graph():
    hip = _hip()
    import torch
    shape = (64, 256)
    dev = torch.device("cuda:0")
    x = torch.randn((3,) + shape, device=dev, dtype=torch.float32)
    spec = torch.empty((3, 64, 129), device=dev, dtype=torch.complex64)
    plan = hip.Plan(shape, dtype=F32, real=True)
    plan.execute(x, spec, batch=3)
    ref = torch.fft.rfftn(x.double(), dim=(1, 2))
    assert (spec.cdouble() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    # asynchronous on a side torch stream, no host sync before the stream's own
    s = torch.cuda.Stream(device=dev)
    aplan = hip.Plan(shape, dtype=F32, real=True, stream=s)
    out = torch.empty_like(spec)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        ret = aplan.execute(x, out, batch=3)
    assert ret is not None
    s.synchronize()
    assert torch.equal(out, spec)
    # capture into a torch graph, replayed twice: bit-identical to the eager execute
    gplan = hip.Plan(shape, dtype=F32, real=True, stream=s)
    xs = x.clone()
    o1 = torch.empty_like(spec)
    y1 = torch.empty_like(x)
    with torch.cuda.stream(s):
        gplan.execute(xs, o1, batch=3)
        gplan.execute(o1, y1, inverse=True, batch=3)
    s.synchronize()
    eager_o, eager_y = o1.clone(), y1.clone()
    o1.zero_()
    y1.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gplan.execute(xs, o1, batch=3, wait_for_finish=False)
        gplan.execute(o1, y1, inverse=True, batch=3, wait_for_finish=False)
    for _ in range(2):
        o1.zero_()
        y1.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o1, eager_o) and torch.equal(y1, eager_y)
    assert (y1 - x).abs().max().item() <= 1e-4 * x.abs().max().item()


def test_real_hip_graph_capture():
    hip = _hip()
    s = hip.Stream()
    shape = (1 << 18,)
    plan = hip.Plan(shape, dtype=F64, real=True, stream=s)
    x = _real_data(shape, F64, 2, 11)
    gx = hip.to_gpu(x)
    gs = hip.DeviceArray((2, (1 << 17) + 1), numpy.complex128)
    plan.execute(gx, gs, batch=2)
    s.synchronize()
    eager = gs.get()
    gs.set(numpy.zeros_like(eager))
    with hip.Graph(s) as g:
        plan.execute(gx, gs, batch=2)
    g.launch()
    g.launch()
    s.synchronize()
    assert numpy.array_equal(gs.get(), eager)


def test_real_second_device():
    hip = _hip()
    if hip.device_count() < 2:
        pytest.skip("one device visible")
    import torch
    shape = (32, 64)
    plan = hip.Plan(shape, dtype=F32, real=True, context=1)
    x = torch.randn((2,) + shape, device="cuda:1")
    spec = torch.empty((2, 32, 33), dtype=torch.complex64, device="cuda:1")
    plan.execute(x, spec, batch=2)
    ref = torch.fft.rfftn(x.double(), dim=(1, 2))
    assert (spec.cdouble() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
