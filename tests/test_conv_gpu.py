"""Convolution plans on the device (docs/extensions.md, "Convolution plans"): one case per one-launch instance (guard bands, a ragged last
work-group, a poisoned item, shared and per-item spectra, correlation, in place and out of place), the composed forms, the scale rule,
filter_spectrum, graph capture and torch interop, each against an extended-precision reference within helpers.accuracy_bound with
L = 2 log2 N + 1 (two transforms and a product)."""
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as C                                                   # noqa: E402
from helpers import GuardedBuffer, accuracy_bound, item_error, unit_roundoff   # noqa: E402

pytestmark = pytest.mark.gpu

CDT = {C.F32: numpy.complex64, C.F64: numpy.complex128, numpy.complex64: numpy.complex64, numpy.complex128: numpy.complex128}


def _hip():
    import pyfft_amd.hip as hip
    if hip.device_count() < 1:
        pytest.fail("no HIP device")
    return hip


def _N():
    from pyfft_amd import _native as N
    return N


def _ext(a, dtype):
    return numpy.asarray(a).astype(numpy.clongdouble if unit_roundoff(dtype) < 2.0 ** -30 else numpy.complex128)


def reference(x, S, shape, dtype, real, normalize=True, scale=1.0):
    """scale * IFFTN(FFTN(x) * S) of one item in extended precision (clongdouble for fp64, complex128 for fp32); real plans with numpy's
    irfftn rule (the half spectrum's Hermitian extension; edge planes through their Hermitian parts)."""
    shape = tuple(shape)
    n = int(numpy.prod(shape))
    X = numpy.fft.fftn(_ext(x, dtype).reshape(shape))
    if not real:
        y = numpy.fft.ifftn(X * _ext(S, dtype).reshape(shape))
    else:
        nx = shape[-1]
        H = _ext(S, dtype).reshape(shape[:-1] + (nx // 2 + 1,))
        Yh = X[..., :nx // 2 + 1] * H
        # Hermitian extension over all axes: F[k] = Yh[k] for kx <= nx/2, conj(Yh[-k]) otherwise; edge planes by their Hermitian parts
        F = numpy.zeros(shape, Yh.dtype)
        F[..., :nx // 2 + 1] = Yh
        idx = [(-numpy.arange(m)) % m for m in shape[:-1]]
        def mirror(a):
            for ax, ii in enumerate(idx):
                a = numpy.take(a, ii, axis=ax)
            return a
        for e in (0, nx // 2):
            plane = Yh[..., e]
            F[..., e] = 0.5 * (plane + numpy.conj(mirror(plane)))
        for kx in range(nx // 2 + 1, nx):
            F[..., kx] = numpy.conj(mirror(F[..., nx - kx]))
        y = numpy.fft.ifftn(F).real
    if not normalize:
        y = y * n
    return (y * scale).reshape(-1)


def bound(dtype, n):
    return accuracy_bound(dtype, n, levels=2 * (int(n).bit_length() - 1) + 1)


def _data(shape, dtype, real, batch, seed):
    r = numpy.random.default_rng(seed)
    s = (batch,) + tuple(shape)
    if real:
        return r.standard_normal(s).astype(dtype)
    return (r.standard_normal(s) + 1j * r.standard_normal(s)).astype(CDT[dtype])


def _unit_spectrum(sshape, dtype, count, seed):
    r = numpy.random.default_rng(seed + 1)
    return numpy.exp(2j * numpy.pi * r.random((count,) + tuple(sshape))).astype(CDT[dtype])


def _sshape(shape, real):
    return tuple(shape[:-1]) + (shape[-1] // 2 + 1,) if real else tuple(shape)


def _h2d(ptr, host):
    _N().check(_N().lib.mifft_memcpy_h2d(ptr, host.ctypes.data, host.nbytes, None), "h2d")


def _d2h(host, ptr):
    _N().check(_N().lib.mifft_memcpy_d2h(host.ctypes.data, ptr, host.nbytes, None), "d2h")
    return host


def _check(x, S, got, shape, dtype, real, items, per_item, correlate, normalize=True, scale=1.0, what=""):
    n = int(numpy.prod(shape))
    l1b, mxb = bound(dtype, n)
    for j in items:
        s = S[j if per_item else 0]
        if correlate:
            s = numpy.conj(s)
        ref = reference(x[j], s, shape, dtype, real, normalize, scale)
        l1, mx = item_error(got[j], ref)
        assert l1 <= l1b and mx <= mxb, "%s %s item %d: L1 %.3g (bound %.3g) max %.3g (bound %.3g)" % (what, shape, j, l1, l1b, mx, mxb)


def run_guarded(hip, plan, shape, dtype, real, batch, in_place, per_item, correlate, seed, poison=None):
    x = _data(shape, dtype, real, batch, seed)
    if poison is not None:
        x[poison] = numpy.nan
    S = _unit_spectrum(_sshape(shape, real), dtype, batch if per_item else 1, seed)
    gx = GuardedBuffer(x.nbytes, 16)
    gs = GuardedBuffer(S.nbytes, 80)
    gy = gx if in_place else GuardedBuffer(x.nbytes, 48)
    _h2d(gx.ptr, x)
    _h2d(gs.ptr, S)
    if in_place:
        plan.execute(gx.ptr, spectrum=gs.ptr, batch=batch, correlate=correlate, spectrum_batch=batch if per_item else 1)
    else:
        plan.execute(gx.ptr, gy.ptr, spectrum=gs.ptr, batch=batch, correlate=correlate, spectrum_batch=batch if per_item else 1)
    got = _d2h(numpy.empty_like(x), gy.ptr)
    assert numpy.array_equal(_d2h(numpy.empty_like(S), gs.ptr), S), "the spectrum was written"
    if not in_place:
        assert numpy.array_equal(_d2h(numpy.empty_like(x), gx.ptr), x, equal_nan=True), "the input was modified"
    for g, w in ((gx, "x"), (gy, "y"), (gs, "spectrum")):
        g.check_guards(w)
    for g in {id(b): b for b in (gx, gy, gs)}.values():
        g.free()
    return x, S, got


@pytest.mark.parametrize("in_place", [False, True], ids=["oop", "inplace"])
@pytest.mark.parametrize("case", C.FUSED, ids=[C.case_id(c) for c in C.FUSED])
def test_conv_fused_row_instance(case, in_place):
    """One case per one-launch instance: a ragged last work-group (67 rows), guard bands around y, an untouched spectrum, a poisoned item
    that must not reach its neighbours; a shared spectrum, then a per-item spectrum with correlation."""
    dtype, real, n = case
    hip = _hip()
    pdt = dtype if real else CDT[dtype]
    plan = hip.Plan((n,), dtype=pdt, convolve=True, real=real)
    assert plan.conv_form == "fused_row"
    assert plan.kernel == ("conv_row_real_kernel" if real else "conv_row_kernel")
    batch = 67 if n <= 2048 else 3
    keep = [j for j in range(batch) if j != 1]
    for per_item, correlate in ((False, False), (True, True)):
        x, S, got = run_guarded(hip, plan, (n,), dtype if real else CDT[dtype], real, batch, in_place, per_item, correlate, seed=n + real,
                                poison=1)
        assert numpy.isfinite(got[keep]).all(), "a poisoned item leaked into its neighbours"
        _check(x, S, got, (n,), dtype, real, keep, per_item, correlate, what=C.case_id(case))


@pytest.mark.parametrize("per_item", [False, True], ids=["shared", "per_item"])
@pytest.mark.parametrize("case", C.COMPOSED, ids=[C.case_id(c) for c in C.COMPOSED])
def test_conv_composed(case, per_item):
    dtype, real, shape = case
    hip = _hip()
    plan = hip.Plan(shape, dtype=dtype, convolve=True, real=real)
    assert plan.conv_form == "composed" and plan.kernel == "composed"
    nbytes = int(numpy.prod(shape)) * numpy.dtype(dtype).itemsize
    batch = 3 if nbytes <= (64 << 20) else 1
    poison = 1 if batch == 3 else None
    x, S, got = run_guarded(hip, plan, shape, dtype, real, batch, False, per_item, per_item, seed=len(shape) + batch, poison=poison)
    items = [j for j in range(batch) if j != poison]
    assert numpy.isfinite(got[items]).all()
    _check(x, S, got, shape, dtype, real, items, per_item, per_item, what="composed")


@pytest.mark.parametrize("shape,dtype,real", [((1024,), numpy.complex64, False), ((64, 64), numpy.complex64, False),
                                              ((4096,), numpy.float32, True), ((256,), numpy.float64, True)], ids=str)
def test_conv_normalize_and_scale(shape, dtype, real):
    hip = _hip()
    plan = hip.Plan(shape, dtype=dtype, convolve=True, real=real, normalize=False, scale=3.0)
    x, S, got = run_guarded(hip, plan, shape, dtype, real, 2, False, False, False, seed=5)
    _check(x, S, got, shape, dtype, real, [0, 1], False, False, normalize=False, scale=3.0, what="scale")


@pytest.mark.parametrize("shape,dtype,real", [((4096,), numpy.float32, True), ((256, 256), numpy.float32, True),
                                              ((1024,), numpy.complex64, False), ((512,), numpy.float64, True)], ids=str)
def test_gaussian_blur_through_filter_spectrum(shape, dtype, real):
    hip = _hip()
    plan = hip.Plan(shape, dtype=dtype, convolve=True, real=real)
    grids = numpy.meshgrid(*[numpy.minimum(numpy.arange(m), m - numpy.arange(m)) for m in shape], indexing="ij")
    g = numpy.exp(-sum(v.astype(float) ** 2 for v in grids) / (2 * 3.0 ** 2))
    g = (g / g.sum()).astype(dtype if real else numpy.float64)
    h = g if real else g.astype(dtype)
    x = _data(shape, dtype, real, 1, 11)[0]
    hd, xd = hip.to_gpu(h), hip.to_gpu(x)
    Hd = hip.DeviceArray(_sshape(shape, real), CDT[numpy.dtype(dtype).type])
    plan.filter_spectrum(hd, Hd)
    plan.execute(xd, spectrum=Hd)
    got = xd.get()
    if real:
        want = numpy.fft.irfftn(numpy.fft.rfftn(x.astype(float)) * numpy.fft.rfftn(g.astype(float)), s=shape, axes=tuple(range(len(shape))))
    else:
        want = numpy.fft.ifftn(numpy.fft.fftn(x) * numpy.fft.fftn(g))
    tol = 1e-12 if numpy.dtype(dtype) in (numpy.dtype(numpy.float64), numpy.dtype(numpy.complex128)) else 2e-6
    assert numpy.abs(got - want).max() <= tol * numpy.abs(want).max() * 10


@pytest.mark.parametrize("shape,dtype,real", [((1024,), numpy.complex64, False), ((64, 64), numpy.complex128, False),
                                              ((2048,), numpy.float32, True), ((16, 32), numpy.float64, True)], ids=str)
def test_filter_spectrum_is_the_plain_forward(shape, dtype, real):
    hip = _hip()
    plan = hip.Plan(shape, dtype=dtype, convolve=True, real=real)
    plain = hip.Plan(shape, dtype=dtype, real=True) if real else hip.Plan(shape, dtype=dtype)
    h = _data(shape, dtype, real, 3, 2)
    hd = hip.to_gpu(h)
    a = hip.DeviceArray((3,) + _sshape(shape, real), CDT[numpy.dtype(dtype).type])
    b = hip.DeviceArray((3,) + _sshape(shape, real), CDT[numpy.dtype(dtype).type])
    plan.filter_spectrum(hd, a, batch=3)
    plain.execute(hd, b, batch=3)
    assert numpy.array_equal(a.get(), b.get())


@pytest.mark.parametrize("shape,dtype,real", [((4096,), numpy.complex64, False), ((64, 64), numpy.complex64, False),
                                              ((1024,), numpy.float32, True), ((16, 64), numpy.float32, True)], ids=str)
def test_conv_hip_graph_capture(shape, dtype, real):
    hip = _hip()
    s = hip.Stream()
    plan = hip.Plan(shape, dtype=dtype, convolve=True, real=real, stream=s)
    x = _data(shape, dtype, real, 4, 3)
    S = _unit_spectrum(_sshape(shape, real), dtype if real else dtype, 1, 3)
    xd, Sd = hip.to_gpu(x), hip.to_gpu(S)
    yd = hip.DeviceArray(x.shape, x.dtype)
    plan.execute(xd, yd, spectrum=Sd, batch=4)
    s.synchronize()
    eager = yd.get()
    yd.set(numpy.zeros_like(x))
    with hip.Graph(s) as g:
        plan.execute(xd, yd, spectrum=Sd, batch=4)
    g.launch()
    g.launch()
    s.synchronize()
    assert numpy.array_equal(yd.get(), eager)


def test_conv_torch_tensors_stream_and_graph():
    torch = pytest.importorskip("torch")
    hip = _hip()
    dev = torch.device("cuda:0")
    for shape, real, dt, tdt in (((2048,), False, numpy.complex64, torch.complex64), ((4096,), True, numpy.float32, torch.float32),
                                 ((128, 128), False, numpy.complex64, torch.complex64)):
        plan = hip.Plan(shape, dtype=dt, convolve=True, real=real)
        x = _data(shape, dt, real, 2, 9)
        S = _unit_spectrum(_sshape(shape, real), dt, 1, 9)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            xt = torch.from_numpy(x).to(dev)
            St = torch.from_numpy(S).to(dev)
            yt = torch.empty_like(xt)
            plan.execute(xt, yt, spectrum=St, batch=2)
            st.synchronize()
            got = yt.cpu().numpy()
        _check(x, S, got, shape, dt, real, [0, 1], False, False, what="torch")
        # torch.cuda.graph capture, replayed
        g = torch.cuda.CUDAGraph()
        yt2 = torch.zeros_like(xt)
        s2 = torch.cuda.Stream()
        s2.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s2):
            plan.execute(xt, yt2, spectrum=St, batch=2, wait_for_finish=False)
            s2.synchronize()
            with torch.cuda.graph(g, stream=s2):
                plan.execute(xt, yt2, spectrum=St, batch=2, wait_for_finish=False)
        yt2.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert numpy.array_equal(yt2.cpu().numpy(), got)
