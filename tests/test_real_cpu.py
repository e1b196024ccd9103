"""Real-input transforms without a device: the packing identity (numpy model of csrc/fft_real.hip), argument handling of
Plan(..., real=True), the planner's form and the C ABI's argument errors (docs/extensions.md, "Real-input transforms")."""
import ctypes
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import real_model as M                        # noqa: E402
from helpers import FakeContext               # noqa: E402

SHAPES = [(2,), (4,), (8,), (1024,), (1, 2), (8, 2), (1, 16), (16, 2), (4, 16), (16, 64), (1, 1, 8), (2, 4, 2), (4, 8, 16), (8, 1, 4)]


def _rng(shape):
    return numpy.random.default_rng(abs(hash(shape)) % (1 << 32))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_packing_identity_forward(shape):
    x = _rng(shape).standard_normal(shape)
    numpy.testing.assert_allclose(M.rfftn_model(x), numpy.fft.rfftn(x), rtol=0, atol=1e-12 * max(1, x.size))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_packing_identity_inverse_non_hermitian_edges(shape):
    """Random half spectra are not Hermitian on the kx = 0 and kx = nx / 2 planes: numpy drops the imaginary parts there after the
    leading inverse transforms, which the packing step reproduces through the planes' Hermitian parts -- and only through them."""
    r = _rng(shape)
    sshape = shape[:-1] + (shape[-1] // 2 + 1,)
    X = r.standard_normal(sshape) + 1j * r.standard_normal(sshape)
    ref = numpy.fft.irfftn(X, s=shape, axes=tuple(range(len(shape))))
    numpy.testing.assert_allclose(M.irfftn_model(X, shape), ref, rtol=0, atol=1e-12)
    numpy.testing.assert_allclose(M.irfftn_exact(X, shape, True).astype(numpy.float64), ref, rtol=0, atol=1e-12)
    # the naive rule (edge planes as they are) is wrong on exactly this input
    assert not numpy.allclose(M.irfftn_model(X, shape, hermitian=False), ref, rtol=0, atol=1e-6)


@pytest.mark.parametrize("shape", [(2,), (64,), (8, 2), (4, 8, 16)], ids=str)
def test_packing_identity_hermitian_input_needs_no_correction(shape):
    x = _rng(shape).standard_normal(shape)
    X = numpy.fft.rfftn(x)
    numpy.testing.assert_allclose(M.irfftn_model(X, shape, hermitian=False), x, rtol=0, atol=1e-12)
    numpy.testing.assert_allclose(M.irfftn_model(X, shape), x, rtol=0, atol=1e-12)


# ---- argument handling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", [((1024,), numpy.float32), ((16, 16), numpy.float64), ((4, 8, 2), numpy.complex64),
                                         ((2,), numpy.complex128), (64, numpy.float32)])
def test_real_params_accepted(shape, dtype):
    from pyfft_amd.real import RealFFTPlan, real_params, spectrum_shape
    RealFFTPlan.validate(shape, dtype=dtype)
    s, prec, rdt, cdt = real_params(shape, dtype)
    assert rdt.itemsize * 2 == cdt.itemsize
    assert spectrum_shape(s)[-1] == s[-1] // 2 + 1


@pytest.mark.parametrize("shape,dtype", [((12,), numpy.float32), ((16, 24), numpy.float32), ((1,), numpy.float32), ((8, 1), numpy.float64),
                                         ((2, 2, 2, 2), numpy.float32), ((0,), numpy.float32), ((16,), numpy.int32), ((16,), numpy.float16)])
def test_real_params_refused(shape, dtype):
    from pyfft_amd import hip
    with pytest.raises(ValueError):
        hip.Plan(shape, dtype=dtype, real=True)


@pytest.mark.parametrize("extra", [{"any_size": True}, {"parent_shape": (64, 64)}])
def test_real_refuses_extensions(extra):
    from pyfft_amd import hip
    with pytest.raises(ValueError, match="real=True"):
        hip.Plan((16, 16), dtype=numpy.float32, real=True, **extra)


def _fake_plan(shape, dtype=numpy.float32):
    from pyfft_amd.real import RealFFTPlan
    from kernel_coverage import full_machine
    return RealFFTPlan(FakeContext(full_machine()), shape, dtype=dtype)


def test_in_place_and_split_planes_refused():
    p = _fake_plan((64,))
    with pytest.raises(ValueError, match="out of place"):
        p.execute(4096)
    with pytest.raises(ValueError, match="out of place"):
        p.execute(4096, 4096)
    with pytest.raises(ValueError, match="split planes"):
        p.execute(4096, 8192, 12288, 16384)


# ---- planner -----------------------------------------------------------------------------------------------------------------
def test_planner_forms_follow_the_library():
    """1-D rows take the one-launch form exactly where the library has a real-row kernel, which is every n / 2 with a ROW kernel
    (n >= 4): no instance is dead and no plan asks for a missing one."""
    from pyfft_amd import _native as N
    from pyfft_amd import passes as P
    for dtype, prec in ((numpy.float32, N.F32), (numpy.float64, N.F64)):
        row_max = P.row_max(prec, interleaved=True)
        n = 2
        while n <= 4 * row_max:
            have = N.lib.mifft_real_row_supported(prec, n) == 0
            assert have == (4 <= n <= 2 * row_max), (dtype, n)
            p = _fake_plan((n,), dtype)
            assert p._real_form == ("fused_row" if have else "composed"), (dtype, n)
            assert (p.inner_plan is None) == (have or n == 2)
            n *= 2
    assert P.row_max(N.F32, interleaved=True) == 32768 and P.row_max(N.F64, interleaved=True) == 16384


@pytest.mark.parametrize("shape,packed", [((2,), None), ((1, 2), None), ((1, 1, 2), None), ((1 << 17,), (1 << 16,)), ((1 << 21,), (1 << 20,)),
                                          ((8, 2), (8, 1)), ((2048, 2048), (2048, 1024)), ((256, 256, 256), (256, 256, 128)),
                                          ((4096, 8), (4096, 4)), ((1, 64), (1, 32))], ids=str)
def test_planner_composed_form(shape, packed):
    p = _fake_plan(shape)
    assert p._real_form == "composed"
    if packed is None:
        assert p.inner_plan is None              # a single packed point: the inner transform is the identity and is skipped
    else:
        inner = p.inner_plan
        assert inner is not None and inner._normalize is False and inner._scale == 1.0
        from pyfft_amd.plan import normalize_shape
        assert (inner._params.x, inner._params.y, inner._params.z) == normalize_shape(packed if len(packed) > 1 else packed[0])[1]


def test_overlapping_buffers_refused():
    p = _fake_plan((64,))
    with pytest.raises(ValueError, match="overlap"):
        p.execute(4096, 4096 + 64)               # 64 reals = 256 bytes of input: the output starts inside it
    p = _fake_plan((16, 16))
    with pytest.raises(ValueError, match="overlap"):
        p.execute(4096 + 512, 4096, inverse=True)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_real_post_prototype_and_argument_errors():
    from pyfft_amd import _native as N
    assert "mifft_launch_real_post" in N.PROTOTYPES
    assert N.lib.mifft_launch_real_post(None, None) == N.E_INVALID
    assert "null descriptor" in N.last_error()

    def desc(**kw):
        d = N.MifftRealPost()
        d.precision, d.inverse, d.nx, d.ny, d.nz, d.outer = N.F32, 0, 16, 1, 1, 1
        d.stride_in, d.stride_out = 8, 9
        d.in_, d.out, d.tw, d.scale = 4096, 1 << 20, 1 << 21, 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for bad, why in (({"nx": 12}, "powers of two"), ({"nx": 1}, "powers of two"), ({"ny": 3}, "powers of two"),
                     ({"precision": 7}, "precision"), ({"inverse": 2}, "inverse"), ({"outer": -1}, "negative"),
                     ({"stride_out": 8}, "pitch"), ({"in_": None}, "null"), ({"tw": None}, "null"), ({"reserved": 1}, "reserved"),
                     ({"out": 4096 + 16}, "overlap"), ({"in_": 4100}, "aligned")):
        rc = N.lib.mifft_launch_real_post(ctypes.byref(desc(**bad)), None)
        assert rc == N.E_INVALID, (bad, rc)
        assert why in N.last_error(), (bad, N.last_error())
    # zero items: nothing to do, nothing launched
    assert N.lib.mifft_launch_real_post(ctypes.byref(desc(outer=0)), None) == 0


def test_real_row_prototypes_and_argument_errors():
    from pyfft_amd import _native as N
    for name in ("mifft_real_row_supported", "mifft_launch_real_row"):
        assert name in N.PROTOTYPES
    assert N.lib.mifft_real_row_supported(N.F32, 65536) == 0 and N.lib.mifft_real_row_supported(N.F32, 131072) == N.E_UNSUPPORTED
    assert N.lib.mifft_real_row_supported(N.F64, 32768) == 0 and N.lib.mifft_real_row_supported(N.F64, 65536) == N.E_UNSUPPORTED
    assert N.lib.mifft_real_row_supported(N.F32, 2) == N.E_UNSUPPORTED and N.lib.mifft_real_row_supported(N.F32, 12) == N.E_UNSUPPORTED
    assert N.lib.mifft_real_row_supported(5, 64) == N.E_UNSUPPORTED

    def launch(prec=N.F32, n=64, inverse=0, rows=1, src=4096, dst=1 << 20, twh=1 << 21, tws=1 << 22):
        return N.lib.mifft_launch_real_row(prec, n, inverse, rows, src, dst, twh, tws, 1.0, None)

    for kw, code, why in (({"n": 12}, N.E_INVALID, "power of two"), ({"n": 1 << 17}, N.E_UNSUPPORTED, "no kernel"),
                          ({"prec": 9}, N.E_INVALID, "precision"), ({"inverse": 3}, N.E_INVALID, "inverse"),
                          ({"rows": -1}, N.E_INVALID, "negative"), ({"src": None}, N.E_INVALID, "null"),
                          ({"twh": None}, N.E_INVALID, "null"), ({"dst": 4096 + 64}, N.E_INVALID, "overlap"),
                          ({"src": 4100}, N.E_INVALID, "aligned")):
        assert launch(**kw) == code, kw
        assert why in N.last_error(), (kw, N.last_error())
    assert launch(rows=0) == 0
