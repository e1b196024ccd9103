"""Convolution plans without a device (docs/extensions.md, "Convolution plans"): the refusals of Plan(..., convolve=True), the form
selection against the library's query, the coverage rule of the GPU cases, and numpy models of the two one-launch algorithms of
csrc/fft_conv_row.hpp (the real rows' pair-local separation / product / packing, and the complex rows' conjugate-forward inverse)."""
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as C                        # noqa: E402
from helpers import FakeContext               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _native():
    from pyfft_amd import _native as N
    return N


def _prec(dt):
    N = _native()
    return N.F64 if numpy.dtype(dt) in (numpy.dtype(numpy.float64), numpy.dtype(numpy.complex128)) else N.F32


# ---- refusals: ValueError naming convolve, before any device call ---------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import pyfft_amd.hip as hip

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(hip, "device_count", touched)
    monkeypatch.setattr(hip, "Context", touched)
    return hip


@pytest.mark.parametrize("kw", [dict(dtype=numpy.float32), dict(dtype=numpy.float64), dict(dtype="complex32"),
                                dict(dtype=numpy.complex64, any_size=True), dict(dtype=numpy.complex64, parent_shape=(2048,)),
                                dict(dtype=numpy.float32, real=True, any_size=True), dict(dtype=numpy.complex64, shape=(12,)),
                                dict(dtype=numpy.float32, real=True, shape=(24,)), dict(dtype=numpy.int32)], ids=str)
def test_refusals_before_the_device(no_device, kw):
    kw = dict(kw)
    shape = kw.pop("shape", (1024,))
    with pytest.raises(ValueError, match="convolve"):
        no_device.Plan(shape, convolve=True, **kw)


def test_torch_complex32_refused(no_device):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="convolve"):
        no_device.Plan((1024,), dtype=torch.complex32, convolve=True)


class _Obj(int):
    """A device address that knows its size (FakeContext.pointer_of passes buffers through as they are)."""
    def __new__(cls, ptr, nbytes):
        o = int.__new__(cls, ptr)
        o.nbytes = nbytes
        return o


def _fake(shape, dtype=numpy.complex64, real=False):
    from pyfft_amd.conv import ConvPlan
    from kernel_coverage import full_machine
    return ConvPlan(FakeContext(full_machine()), shape, dtype=dtype, real=real)


@pytest.mark.parametrize("shape,dtype,real", [((1024,), numpy.complex64, False), ((64, 64), numpy.complex128, False),
                                              ((4096,), numpy.float32, True), ((16, 32), numpy.float64, True)], ids=str)
def test_buffer_refusals(shape, dtype, real):
    p = _fake(shape, dtype, real)
    n = int(numpy.prod(shape))
    item = n * numpy.dtype(dtype).itemsize
    sp = int(numpy.prod(p.spectrum_shape())) * (numpy.dtype(dtype).itemsize * (2 if real else 1))
    x = _Obj(1 << 30, 4 * item)
    y = _Obj(1 << 31, 4 * item)
    with pytest.raises(ValueError, match="convolve.*spectrum"):
        p.execute(x, y, spectrum=_Obj(1 << 32, sp - 16), batch=4)
    with pytest.raises(ValueError, match="convolve.*spectrum"):
        p.execute(x, y, spectrum=_Obj(1 << 32, 3 * sp), batch=4, spectrum_batch=4)
    with pytest.raises(ValueError, match="convolve.*spectrum"):
        p.execute(x, y, spectrum=_Obj((1 << 30) + item, sp), batch=4)
    with pytest.raises(ValueError, match="convolve.*spectrum"):
        p.execute(x, spectrum=_Obj((1 << 30) + 4 * item - 16, sp), batch=4)      # in place on x: the spectrum starts inside x
    with pytest.raises(ValueError, match="convolve.*spectrum_batch"):
        p.execute(x, y, spectrum=_Obj(1 << 32, 4 * sp), batch=4, spectrum_batch=2)
    with pytest.raises(ValueError, match="convolve.*overlap"):
        p.execute(x, _Obj((1 << 30) + 16, 4 * item), spectrum=_Obj(1 << 32, sp), batch=4)
    with pytest.raises(ValueError, match="convolve.*spectrum"):
        p.execute(x, y, batch=4)


def test_sharded_plan_has_no_convolution_form():
    from pyfft_amd.sharded import ShardedPlan
    import inspect
    assert "convolve" not in inspect.signature(ShardedPlan.__init__).parameters


# ---- form selection and coverage ----------------------------------------------------------------------------------------------
def _accepted():
    from pyfft_amd import passes
    N = _native()
    out = set()
    for dt in (C.F32, C.F64):
        prec = _prec(dt)
        for real in (False, True):
            for e in range(1, 18):
                n = 1 << e
                if N.lib.mifft_conv_row_supported(prec, 1 if real else 0, n) == 0:
                    out.add((dt, real, n))
                    if real:
                        assert N.lib.mifft_real_row_supported(prec, n) == 0, (dt, n)
                    else:
                        assert n <= passes.row_max(prec, interleaved=True), (dt, n)
    return out


def test_coverage_every_instance_has_a_gpu_case():
    assert _accepted() == set(C.FUSED)


def test_left_out_lengths_are_recorded():
    """Every length with a row (complex) or real-row (real) kernel is either a one-launch instance or listed in conv_cases.LEFT_OUT with the
    log line that records why it was dropped."""
    from pyfft_amd import passes
    N = _native()
    log = open(os.path.join(ROOT, "profiles", "r07_conv_transforms.log")).read()
    accepted = _accepted()
    for dt in (C.F32, C.F64):
        prec = _prec(dt)
        for e in range(1, 18):
            n = 1 << e
            cands = []
            if n <= passes.row_max(prec, interleaved=True):
                cands.append(False)
            if n >= 4 and N.lib.mifft_real_row_supported(prec, n) == 0:
                cands.append(True)
            for real in cands:
                key = (dt, real, n)
                if key in accepted:
                    assert key not in C.LEFT_OUT
                else:
                    assert key in C.LEFT_OUT, key
                    assert C.LEFT_OUT[key] in log, (key, C.LEFT_OUT[key])


@pytest.mark.parametrize("shape,dtype,real", [((n,), dt if not real else dt, real) for dt, real, n in C.FUSED[::5]] +
                         [((1 << 16,), numpy.complex64, False), ((64, 64), numpy.complex64, False), ((32768,), numpy.float32, True),
                          ((16, 16), numpy.float64, True), ((8192, 2), numpy.complex128, False)], ids=str)
def test_form_follows_the_library(shape, dtype, real):
    if not real:
        dtype = {C.F32: numpy.complex64, C.F64: numpy.complex128}.get(dtype, dtype)
    p = _fake(shape, dtype, real)
    N = _native()
    fused = len(shape) == 1 and N.lib.mifft_conv_row_supported(_prec(dtype), 1 if real else 0, shape[0]) == 0
    assert p.conv_form == ("fused_row" if fused else "composed")
    assert p.kernel == (("conv_row_real_kernel" if real else "conv_row_kernel") if fused else "composed")


def test_abi_argument_errors():
    import ctypes
    N = _native()
    lib = N.lib
    a = ctypes.c_void_p(1 << 20)
    b = ctypes.c_void_p(1 << 24)
    s = ctypes.c_void_p(1 << 28)
    assert lib.mifft_launch_conv_row(N.F32, 0, 12, 1, a, b, s, 0, 0, s, None, 1.0, None) == N.E_INVALID
    assert lib.mifft_launch_conv_row(7, 0, 16, 1, a, b, s, 0, 0, s, None, 1.0, None) == N.E_INVALID
    assert lib.mifft_launch_conv_row(N.F32, 0, 16, 1, a, b, s, 0, 2, s, None, 1.0, None) == N.E_INVALID
    assert lib.mifft_launch_conv_row(N.F32, 0, 16, 1, a, b, s, 3, 0, s, None, 1.0, None) == N.E_INVALID          # pitch < n
    assert lib.mifft_launch_conv_row(N.F32, 1, 16, 1, a, b, s, 0, 0, s, None, 1.0, None) == N.E_INVALID          # no tw_sep
    assert lib.mifft_launch_conv_row(N.F32, 0, 16, 4, a, ctypes.c_void_p((1 << 20) + 8), s, 0, 0, s, None, 1.0, None) == N.E_INVALID
    assert lib.mifft_launch_conv_row(N.F32, 0, 16, 4, a, b, ctypes.c_void_p((1 << 20) + 64), 0, 0, s, None, 1.0, None) == N.E_INVALID
    assert lib.mifft_launch_conv_row(N.F64, 0, 16384, 1, a, b, s, 0, 0, s, None, 1.0, None) == N.E_UNSUPPORTED
    assert lib.mifft_conv_row_supported(N.F32, 0, 12) == N.E_UNSUPPORTED
    assert lib.mifft_conv_row_supported(N.F32, 1, 2) == N.E_UNSUPPORTED
    assert lib.mifft_aux_mul_spectrum(N.F32, a, s, 1, 16, 8, 0, 1.0, None) == N.E_INVALID
    assert lib.mifft_aux_mul_spectrum(N.F32, None, s, 1, 16, 0, 0, 1.0, None) == N.E_INVALID


# ---- numpy models of the one-launch algorithms ---------------------------------------------------------------------------------
def conv_real_row_model(x, S, edge_rule=True):
    """csrc/fft_conv_row.hpp, real rows: packed forward, pair-local X[k] / X[L - k], products, packing, conjugate-forward inverse."""
    n = x.size
    L = n // 2
    z = x[0::2] + 1j * x[1::2]
    Z = numpy.fft.fft(z)
    w = numpy.exp(-2j * numpy.pi * numpy.arange(L + 1) / n)
    Zp = numpy.empty(L, complex)
    for k in range(L):
        p, q = Z[k], Z[(L - k) % L]
        s, d = p + numpy.conj(q), p - numpy.conj(q)
        t = w[k] * d
        y1 = 0.5 * (s - 1j * t) * S[k]
        y2 = numpy.conj(0.5 * (s + 1j * t)) * S[L - k]
        if k == 0 and edge_rule:
            y1, y2 = y1.real, y2.real
        Zp[k] = (y1 + numpy.conj(y2)) + 1j * numpy.conj(w[k]) * (y1 - numpy.conj(y2))
    r = numpy.conj(numpy.fft.fft(numpy.conj(Zp))) / n          # IFFT as the conjugate's forward transform
    out = numpy.empty(n)
    out[0::2], out[1::2] = r.real, r.imag
    return out


def conv_complex_row_model(x, S):
    Y = numpy.fft.fft(x) * S
    return numpy.conj(numpy.fft.fft(numpy.conj(Y))) / x.size


@pytest.mark.parametrize("n", [4, 8, 16, 64, 256, 2048])
def test_real_row_model(n):
    r = numpy.random.default_rng(n)
    x = r.standard_normal(n)
    S = r.standard_normal(n // 2 + 1) + 1j * r.standard_normal(n // 2 + 1)      # not Hermitian on the edge entries
    ref = numpy.fft.irfftn(numpy.fft.rfftn(x) * S, s=(n,), axes=(0,))
    numpy.testing.assert_allclose(conv_real_row_model(x, S), ref, rtol=0, atol=1e-12)
    numpy.testing.assert_allclose(conv_real_row_model(x, numpy.conj(S)), numpy.fft.irfftn(numpy.fft.rfftn(x) * numpy.conj(S), s=(n,), axes=(0,)),
                                  rtol=0, atol=1e-12)
    # the mutant without the edge rule is wrong on exactly these spectra
    assert not numpy.allclose(conv_real_row_model(x, S, edge_rule=False), ref, rtol=0, atol=1e-6)


@pytest.mark.parametrize("n", [2, 8, 128, 4096])
def test_complex_row_model(n):
    r = numpy.random.default_rng(n)
    x = r.standard_normal(n) + 1j * r.standard_normal(n)
    S = numpy.exp(2j * numpy.pi * r.random(n))
    numpy.testing.assert_allclose(conv_complex_row_model(x, S), numpy.fft.ifft(numpy.fft.fft(x) * S), rtol=0, atol=1e-12)
    # a unit-modulus spectrum keeps the norm (the GPU cases rely on it)
    numpy.testing.assert_allclose(numpy.linalg.norm(conv_complex_row_model(x, S)), numpy.linalg.norm(x), rtol=1e-12)
