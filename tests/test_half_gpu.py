"""Half-precision (complex32) transforms on the device: every complex32 kernel instance against an extended-precision reference of its
fp16 input and against the complex64 plan's result rounded to fp16, with guard bands and a poisoned neighbour item; then the plan's
semantics (in place, normalize / scale, overflow, streams, graphs, torch tensors).  docs/extensions.md, "Half-precision transforms"."""
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import GuardedBuffer, accuracy_bound, reference_fft   # noqa: E402

pytestmark = pytest.mark.gpu

F16_UNIT = 2.0 ** -11            # unit roundoff of fp16: the one rounding at the store


def _hip():
    import pyfft_amd.hip as hip
    if hip.device_count() < 1:
        pytest.fail("no HIP device")
    return hip


def _instances():
    """{kernel instance: first numpy-order shape that runs it}, from mifft_half_supported over the shape set."""
    from pyfft_amd import _native as N
    from pyfft_amd.half import half_kernel
    found = {}
    for lx in range(1, 16):
        if N.lib.mifft_half_supported(1 << lx, 1, 1) == 0:
            found.setdefault(half_kernel((1 << lx, 1, 1)), (1 << lx,))
    for lx in range(1, 16):
        for ly in range(1, 16 - lx):
            for lz in range(0, 16 - lx - ly):
                x, y, z = 1 << lx, 1 << ly, 1 << lz
                if N.lib.mifft_half_supported(x, y, z) == 0:
                    found.setdefault(half_kernel((x, y, z)), (y, x) if z == 1 else (z, y, x))
    return found


INSTANCES = sorted(_instances().items(), key=lambda kv: (int(numpy.prod(kv[1])), kv[0]))


def _half_data(shape, batch, seed, scale=1.0):
    """batch items of complex32 data as float16 pairs, shape (batch,) + shape + (2,)"""
    r = numpy.random.default_rng(seed)
    return (r.standard_normal((batch,) + tuple(shape) + (2,)) * scale).astype(numpy.float16)


def _as_complex(h):
    h = numpy.asarray(h, numpy.float16).astype(numpy.float64)
    return h[..., 0] + 1j * h[..., 1]


def _to_half(c):
    """complex64 values rounded to complex32 (float16 pairs), to nearest even"""
    c = numpy.asarray(c, numpy.complex64)
    return numpy.stack([c.real, c.imag], axis=-1).astype(numpy.float16)


def _upload(ptr, host):
    from pyfft_amd import _native as N
    host = numpy.ascontiguousarray(host)
    N.check(N.lib.mifft_memcpy_h2d(ptr, host.ctypes.data, host.nbytes, None), "mifft_memcpy_h2d")


def _download(ptr, shape):
    from pyfft_amd import _native as N
    host = numpy.empty(shape, numpy.float16)
    N.check(N.lib.mifft_memcpy_d2h(host.ctypes.data, ptr, host.nbytes, None), "mifft_memcpy_d2h")
    return host


def _c64_rounded(hip, shape, x, batch, inverse, normalize=True, scale=1.0):
    """The complex64 plan's result of the fp16 input `x` (items [0, batch)) rounded to complex32.  In place and with the wave kernel
    switched off, the complex64 plan runs the fp32 kernel each complex32 kernel is the twin of, so the two agree bit for bit."""
    from pyfft_amd import _native as N
    prev = N.lib.mifft_debug_get(N.DEBUG_NO_WAVE)
    N.check(N.lib.mifft_debug_set(N.DEBUG_NO_WAVE, 1), "mifft_debug_set")
    try:
        c64 = hip.Plan(shape, dtype=numpy.complex64, normalize=normalize, scale=scale)
        gc = hip.to_gpu(_as_complex(x[:batch]).astype(numpy.complex64))
        c64.execute(gc, batch=batch, inverse=inverse)
        return _to_half(gc.get())
    finally:
        N.check(N.lib.mifft_debug_set(N.DEBUG_NO_WAVE, prev), "mifft_debug_set")


def _check_item(shape, got_h, inp_h, want_h, inverse, normalize=True, scale=1.0, what=""):
    """got_h: the plan's complex32 result of one item; inp_h its input; want_h the complex64 plan's result rounded to fp16."""
    n = int(numpy.prod(shape))
    ref = reference_fft(_as_complex(inp_h), shape, numpy.complex64, inverse, normalize, scale)
    got = _as_complex(got_h).reshape(-1)
    l1b, mxb = accuracy_bound(numpy.complex64, n)
    mag = numpy.abs(ref)
    rms = float(numpy.sqrt(numpy.mean(mag * mag)))
    diff = numpy.abs(got - ref)
    l1 = float(diff.sum() / mag.sum())
    mx = float(diff.max())
    assert l1 <= F16_UNIT + l1b and mx <= F16_UNIT * float(mag.max()) + mxb * rms, \
        "%s %s: L1-relative %.3g (bound %.3g), max|err| %.3g (bound %.3g)" % (what, shape, l1, F16_UNIT + l1b, mx,
                                                                             F16_UNIT * float(mag.max()) + mxb * rms)
    # against the complex64 plan rounded once: every element within one fp16 ulp of it (the ulp of that element), most bit-identical
    g = got_h.reshape(-1).astype(numpy.float64)
    w = want_h.reshape(-1).astype(numpy.float64)
    ulp = numpy.spacing(numpy.abs(want_h.reshape(-1))).astype(numpy.float64)
    far = numpy.abs(g - w) > ulp
    assert not far.any(), "%s %s: %d elements more than one fp16 ulp from the complex64 plan's rounded result" % (what, shape, far.sum())
    same = float(numpy.mean(got_h.reshape(-1).view(numpy.uint16) == want_h.reshape(-1).view(numpy.uint16)))
    assert same >= 0.99, "%s %s: only %.4f of the elements are bit-identical to the complex64 plan's rounded result" % (what, shape, same)


@pytest.mark.parametrize("kernel,shape", INSTANCES, ids=["%s-%s" % kv for kv in INSTANCES])
def test_half_instance(kernel, shape, monkeypatch):
    """One case per complex32 kernel instance: forward and inverse, out of place between guard bands (16-byte aligned, not 64-byte),
    batch 4 with a NaN-poisoned last item that must not leak into the others, against the reference and the complex64 plan.  Both
    plans run variant 0 here (the "nd_generic" rule off), so that every fixed-shape twin is reached; test_half_nd_generic_shapes
    covers the rule."""
    monkeypatch.setenv("PYFFT_AMD_NO_ND_GENERIC", "1")
    hip = _hip()
    plan = hip.Plan(shape, dtype="complex32")
    assert plan.kernel == kernel
    batch, poison = 4, 3
    n = int(numpy.prod(shape))
    nbytes = batch * n * 4
    for inverse in (False, True):
        x = _half_data(shape, batch, 17 + inverse)
        x[poison] = numpy.float16("nan")
        gin, gout = GuardedBuffer(nbytes, 48), GuardedBuffer(nbytes, 16)
        try:
            _upload(gin.ptr, x)
            _upload(gout.ptr, numpy.zeros_like(x))
            plan.execute(gin.ptr, gout.ptr, inverse=inverse, batch=batch)
            got = _download(gout.ptr, x.shape)
            assert numpy.array_equal(_download(gin.ptr, x.shape).view(numpy.uint16), x.view(numpy.uint16)), "input changed"
            gin.check_guards("%s input" % kernel)
            gout.check_guards("%s output" % kernel)
        finally:
            gin.free()
            gout.free()
        want = _c64_rounded(hip, shape, x, poison, inverse)
        for j in range(poison):
            _check_item(shape, got[j], x[j], want[j], inverse, what="%s item %d %s" % (kernel, j, "inverse" if inverse else "forward"))
        assert numpy.isnan(got[poison].astype(numpy.float32)).any()


def test_half_nd_generic_shapes():
    """Shapes of the tuning table's "nd_generic" list run the run-time-shaped twin, as the complex64 plan does, and agree with it."""
    hip = _hip()
    for shape in ((4, 4), (2, 2), (16, 4)):
        plan = hip.Plan(shape, dtype="complex32")
        assert plan.kernel == "nd:4096", (shape, plan.kernel)
        x = _half_data(shape, 3, 31)
        for inverse in (False, True):
            a = hip.to_gpu(x)
            plan.execute(a, inverse=inverse, batch=3)
            got = a.get()
            want = _c64_rounded(hip, shape, x, 3, inverse)
            for j in range(3):
                _check_item(shape, got[j], x[j], want[j], inverse, what="nd_generic item %d" % j)


def test_half_refuses_buffers_of_another_dtype():
    hip = _hip()
    plan = hip.Plan((64,), dtype="complex32")
    with pytest.raises(ValueError, match="dtype"):
        plan.execute(hip.DeviceArray((64,), numpy.complex64))


@pytest.mark.parametrize("shape", [(64,), (1024,), (32768,), (64, 64), (16, 8, 2), (32, 32, 32)], ids=str)
def test_half_in_place_equals_out_of_place(shape):
    hip = _hip()
    plan = hip.Plan(shape, dtype="complex32")
    x = _half_data(shape, 3, 5)
    for inverse in (False, True):
        a = hip.to_gpu(x)
        b = hip.DeviceArray(x.shape, numpy.float16)
        plan.execute(a, b, inverse=inverse, batch=3)
        plan.execute(a, inverse=inverse, batch=3)
        assert numpy.array_equal(a.get().view(numpy.uint16), b.get().view(numpy.uint16)), (shape, inverse)


def test_half_normalize_and_scale():
    hip = _hip()
    shape = (32, 64)
    x = _half_data(shape, 2, 9)
    for normalize, scale in ((True, 1.0), (False, 1.0), (False, 4.0), (True, 0.25)):
        plan = hip.Plan(shape, dtype="complex32", normalize=normalize, scale=scale)
        for inverse in (False, True):
            data = x if not inverse else _half_data(shape, 2, 10, 1.0 / 64)
            a = hip.to_gpu(data)
            plan.execute(a, inverse=inverse, batch=2)
            got = a.get()
            want = _c64_rounded(hip, shape, data, 2, inverse, normalize, scale)
            for j in range(2):
                _check_item(shape, got[j], data[j], want[j], inverse, normalize, scale, what="normalize %s scale %g" % (normalize, scale))


def test_half_overflow_and_scale_keep_range():
    """n = 32768 forward of constant 4: DC = 131072 > 65504 rounds to +inf; with scale = 1/32 it is 4096, exact, and all else 0."""
    hip = _hip()
    n = 32768
    x = numpy.zeros((n, 2), numpy.float16)
    x[:, 0] = 4
    a = hip.to_gpu(x)
    hip.Plan((n,), dtype="complex32").execute(a)
    got = a.get().astype(numpy.float32)
    assert numpy.isposinf(got[0, 0]) and got[0, 1] == 0
    assert numpy.all(got[1:] == 0)
    a = hip.to_gpu(x)
    hip.Plan((n,), dtype="complex32", scale=1.0 / 32).execute(a)
    got = a.get().astype(numpy.float32)
    assert got[0, 0] == 4096 and got[0, 1] == 0 and numpy.all(got[1:] == 0)


def test_half_stream_and_hip_graph():
    hip = _hip()
    shape = (128, 128)
    s = hip.Stream()
    plan = hip.Plan(shape, dtype="complex32", stream=s)
    x = _half_data(shape, 3, 21)
    a = hip.to_gpu(x)
    b = hip.DeviceArray(x.shape, numpy.float16)
    assert plan.execute(a, b, batch=3) is not None
    s.synchronize()
    eager = b.get()
    sync = hip.Plan(shape, dtype="complex32")
    c = hip.to_gpu(x)
    sync.execute(c, batch=3)
    assert numpy.array_equal(c.get().view(numpy.uint16), eager.view(numpy.uint16))
    b.set(numpy.zeros_like(eager))
    with hip.Graph(s) as g:
        plan.execute(a, b, batch=3)
    for _ in range(2):
        b.set(numpy.zeros_like(eager))
        g.launch()
        s.synchronize()
        assert numpy.array_equal(b.get().view(numpy.uint16), eager.view(numpy.uint16))


def test_half_torch_tensors_stream_and_graph():
    hip = _hip()
    import torch
    dev = torch.device("cuda:0")
    shape = (64, 256)
    xr = torch.randn((3,) + shape + (2,), device=dev).half()             # float16 with a trailing axis of 2
    xc = torch.view_as_complex(xr.float()).to(torch.complex32)           # the same values as complex32
    plan = hip.Plan(shape, dtype=torch.complex32)
    o1 = torch.empty_like(xr)
    plan.execute(xr, o1, batch=3)
    o2 = torch.empty_like(xc)
    plan.execute(xc, o2, batch=3)
    assert torch.equal(torch.view_as_real(o2.to(torch.complex64)).half(), o1)
    ref = torch.fft.fftn(torch.view_as_complex(xr.double()), dim=(1, 2))
    got = torch.view_as_complex(o1.double())
    assert (got - ref).abs().max().item() <= 2 * F16_UNIT * ref.abs().max().item()
    with pytest.raises(ValueError, match="needs"):
        plan.execute(xr[:2], o1, batch=3)
    # a torch side stream and a torch graph, replayed twice: bit-identical to the eager execute
    s = torch.cuda.Stream(device=dev)
    gplan = hip.Plan(shape, dtype="complex32", stream=s)
    o3 = torch.empty_like(xr)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        gplan.execute(xr, o3, batch=3)
    s.synchronize()
    assert torch.equal(o3, o1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gplan.execute(xr, o3, batch=3, wait_for_finish=False)
    for _ in range(2):
        o3.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o3, o1)
