"""Half-precision (complex32) transforms without a device: argument handling of Plan(shape, dtype="complex32"), the shape set against
its definition (the one-launch shapes of interleaved fp32 data) and the C ABI's argument errors (docs/extensions.md, "Half-precision
transforms")."""
import numpy
import pytest

from pyfft_amd import _native as N
from pyfft_amd import passes as P

# numpy-order shapes with a one-launch complex32 kernel, unit axes included
ACCEPTED = [(2,), (64,), (255 + 1,), (32768,), (1, 64), (64, 1), (128, 128), (16, 1024), (128, 256), (256, 128), (1024, 32),
            (32, 32, 32), (16, 16, 64), (2, 2, 2), (1, 32768), (32768, 1, 1), (1024, 1, 32)]
REFUSED = [65536, (65536,), (1024, 1024), (256, 256), (64, 64, 64), (1, 65536), (3,), (48, 64)]


def _plan(*args, **kwds):
    import pyfft_amd.hip as hip
    return hip.Plan(*args, **kwds)


@pytest.mark.parametrize("shape", ACCEPTED, ids=str)
def test_complex32_accepts_the_shape_set(shape):
    from pyfft_amd.half import HalfFFTPlan, half_dims, half_kernel
    HalfFFTPlan.validate(shape, "complex32")
    dims = half_dims(shape)
    assert int(numpy.prod(dims)) == int(numpy.prod(shape)) and N.lib.mifft_half_supported(*dims) == 0
    assert half_kernel(dims).split(":")[0] in ("tile", "row", "nd2", "nd")


@pytest.mark.parametrize("shape", REFUSED, ids=str)
def test_complex32_refuses_other_shapes(shape):
    with pytest.raises(ValueError) as e:
        _plan(shape, dtype="complex32")
    msg = str(e.value)
    assert "32768" in msg or "16384" in msg or "powers of two" in msg, msg


def test_complex32_messages_name_the_limit():
    with pytest.raises(ValueError, match="2 ... 32768 points"):
        _plan((65536,), dtype="complex32")
    with pytest.raises(ValueError, match="16384 points"):
        _plan((1024, 1024), dtype="complex32")


def test_float16_planes_refused_with_message():
    for dt in (numpy.float16, "float16", numpy.dtype(numpy.float16)):
        with pytest.raises(ValueError, match="only interleaved complex32"):
            _plan((64,), dtype=dt)
    with pytest.raises(ValueError, match="only interleaved complex32"):
        _plan((16, 16), numpy.float16)


def test_complex32_refuses_extensions():
    for kw in ({"real": True}, {"any_size": True}, {"parent_shape": (128,)}):
        with pytest.raises(ValueError, match="complex32 cannot be combined"):
            _plan((64,), dtype="complex32", **kw)


def test_torch_complex32_is_the_same_dtype():
    torch = pytest.importorskip("torch")
    from pyfft_amd.half import HalfFFTPlan, is_complex32
    assert is_complex32(torch.complex32) and is_complex32("complex32")
    assert not is_complex32(torch.complex64) and not is_complex32(numpy.complex64)
    HalfFFTPlan.validate((64,), torch.complex32)
    with pytest.raises(ValueError):
        _plan((65536,), dtype=torch.complex32)


def _pow2_shapes(max_points):
    for lx in range(17):
        for ly in range(17 - lx):
            for lz in range(17 - lx - ly):
                if (1 << (lx + ly + lz)) <= max_points:
                    yield 1 << lx, 1 << ly, 1 << lz


def test_half_supported_matches_the_shape_set_definition():
    """mifft_half_supported: 1-D rows of 2 ... row_max(F32, interleaved) points, and every shape with y or z > 1 that
    mifft_nd_shape_supported(F32, ..., VARIANT_INTERLEAVED_ONLY) accepts -- every power-of-two shape up to 2^16 points."""
    row_max = P.row_max(N.F32, interleaved=True)
    assert row_max == 32768
    count = 0
    for x, y, z in _pow2_shapes(1 << 16):
        if y == 1 and z == 1:
            want = 2 <= x <= row_max
        else:
            want = N.lib.mifft_nd_shape_supported(N.F32, x, y, z, N.VARIANT_INTERLEAVED_ONLY) == 0
        got = N.lib.mifft_half_supported(x, y, z)
        assert got in (0, N.E_UNSUPPORTED)
        assert (got == 0) == want, (x, y, z, got)
        kind = N.lib.mifft_half_kernel(x, y, z, 0)
        assert (kind > 0) == want and (not want or kind in (N.HALF_KERNEL_TILE, N.HALF_KERNEL_ROW, N.HALF_KERNEL_ND2,
                                                              N.HALF_KERNEL_ND)), (x, y, z, kind)
        count += want
    assert count > 300
    assert N.lib.mifft_half_supported(0, 1, 1) == N.E_UNSUPPORTED and N.lib.mifft_half_supported(48, 1, 1) == N.E_UNSUPPORTED
    K = N.lib.mifft_half_kernel
    assert K(64, 1, 1, 0) == N.HALF_KERNEL_TILE and K(256, 1, 1, 0) == N.HALF_KERNEL_ROW and K(256, 1, 1, 1) == N.HALF_KERNEL_ROW
    assert K(32, 32, 32, 0) == N.HALF_KERNEL_ND2 and K(2, 2, 128, 0) == N.HALF_KERNEL_ND
    # variant 1: the run-time-shaped kernel wherever it takes the shape (up to 16384 points), as for an fp32 ND pass
    assert K(4, 4, 1, 1) == N.HALF_KERNEL_ND and K(128, 128, 1, 1) == N.HALF_KERNEL_ND and K(32, 32, 32, 1) == N.HALF_KERNEL_ND2
    assert K(4, 4, 1, 2) == N.E_UNSUPPORTED


def test_half_plan_follows_the_nd_generic_rule():
    """The complex32 plan runs the kernel an in-place complex64 plan of the same transforms runs: the tuning table's "nd_generic"
    shapes on the run-time-shaped kernel (always, or in launches beyond write_through_max complex64 bytes per side)."""
    from helpers import FakeContext
    from kernel_coverage import full_machine
    from pyfft_amd.half import HalfFFTPlan
    mach = full_machine()
    ctx = FakeContext(mach)
    always, big = mach.tuning.nd_generic["f32"]
    assert (4, 4, 1) in always and (8, 2, 1) in big
    small = HalfFFTPlan(ctx, (4, 4), "complex32")
    assert small.kernel == "nd:4096" and small.variant(1 << 20) == 1
    p = HalfFFTPlan(ctx, (2, 8), "complex32")                            # (x, y) = (8, 2): "big" only
    huge_batch = mach.write_through_max_bytes // (16 * 8) + 1
    assert p.kernel == "nd2:8x2x1" and p.kernel_for(huge_batch) == "nd:4096"
    assert HalfFFTPlan(ctx, (128, 128), "complex32").kernel_for(huge_batch) == "nd2:128x128x1"
    assert HalfFFTPlan(ctx, (64,), "complex32").kernel_for(huge_batch) == "tile:64"


def test_half_prototypes_and_argument_errors():
    for name in ("mifft_half_supported", "mifft_half_kernel", "mifft_launch_half"):
        assert name in N.PROTOTYPES

    def launch(x=64, y=1, z=1, variant=0, inverse=0, count=1, src=1 << 20, dst=1 << 21, twx=1 << 22, twy=None, twz=None):
        return N.lib.mifft_launch_half(x, y, z, variant, inverse, count, src, dst, twx, twy, twz, 1.0, None)

    for kw, code, why in (({"x": 48}, N.E_INVALID, "powers of two"), ({"x": 65536}, N.E_UNSUPPORTED, "no one-launch kernel"),
                          ({"x": 1024, "y": 1024, "twy": 1 << 23}, N.E_UNSUPPORTED, "no one-launch kernel"),
                          ({"inverse": 2}, N.E_INVALID, "inverse"), ({"variant": 2}, N.E_INVALID, "variant"), ({"count": -1}, N.E_INVALID, "negative"),
                          ({"src": None}, N.E_INVALID, "null"), ({"dst": None}, N.E_INVALID, "null"),
                          ({"twx": None}, N.E_INVALID, "null twiddle"), ({"x": 16, "y": 16}, N.E_INVALID, "null twiddle"),
                          ({"src": (1 << 20) + 8}, N.E_INVALID, "16-byte"), ({"dst": (1 << 21) + 4}, N.E_INVALID, "16-byte"),
                          ({"twx": (1 << 22) + 4}, N.E_INVALID, "8-byte"),
                          ({"dst": (1 << 20) + 16}, N.E_INVALID, "overlap"), ({"src": (1 << 21) - 64, "count": 2}, N.E_INVALID, "overlap")):
        assert launch(**kw) == code, kw
        assert why in N.last_error(), (kw, N.last_error())
    # nothing to do: no launch, no device
    assert launch(count=0) == 0
    assert launch(count=0, dst=1 << 20) == 0
    assert launch(x=1, y=64, twx=None, twy=1 << 22, count=0) == 0
    assert launch(x=16, y=16, twy=1 << 23, variant=1, count=0) == 0


def test_half_plan_refuses_buffers_of_another_dtype():
    from pyfft_amd.half import _check_dtype
    for ok in (numpy.zeros(4, numpy.float16), 1 << 20):
        _check_dtype(ok, "input")
    for bad in (numpy.zeros(4, numpy.complex64), numpy.zeros(4, numpy.float32)):
        with pytest.raises(ValueError, match="dtype"):
            _check_dtype(bad, "input")
    torch = pytest.importorskip("torch")
    _check_dtype(torch.zeros(2, 2, dtype=torch.float16), "output")
    with pytest.raises(ValueError, match="dtype"):
        _check_dtype(torch.zeros(2, 2, dtype=torch.float32), "output")
    with pytest.raises(ValueError, match="dtype"):
        _check_dtype(torch.zeros(2, dtype=torch.complex64), "output")
