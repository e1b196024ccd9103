"""HalfFFTPlan: half-precision complex transforms, Plan(shape, dtype="complex32") (docs/extensions.md, "Half-precision transforms").
`torch.complex32` names the same dtype.

Data is interleaved complex32: one fp16 real and one fp16 imaginary part per point, 4 bytes.  A buffer is a DeviceArray of float16 with
2 x points elements, a raw pointer, or a torch tensor of complex32 (or float16 with a trailing axis of 2).  Split half planes do not
exist: numpy.float16 (the reference's "float dtype means planes") is a ValueError.

Numerics: loads widen fp16 to fp32 exactly; every stage runs in fp32 on the complex64 plan's twiddle tables (evaluated in float64);
the plan's scale and normalisation are applied in fp32; the result is rounded to fp16 once, at the store, to nearest even.  A result
beyond +-65504 becomes +-inf (NaN stays NaN), so scale= is how a long forward transform stays in range.

Every shape runs in ONE launch (mifft_launch_half): the shapes one interleaved fp32 launch takes -- 1-D rows of 2 ... 32768 points,
and the 2-D / 3-D shapes of mifft_nd_shape_supported(F32, ..., VARIANT_INTERLEAVED_ONLY).  Each kernel is the complex32-storage twin
of the fp32 kernel an in-place complex64 plan runs for the same transforms: the tuning table's "nd_generic" rule picks the
run-time-shaped N-D kernel where it does for complex64 (judged on the complex64 bytes of the launch).  There is no twin of the
several-work-groups-per-transform kernels that complex64 runs out of place for some N-D shapes, nor of the wave kernel of short
complex64 rows in small launches.  Other shapes, any_size=, parent_shape= and real=True are ValueErrors.

    execute(a)       in place            execute(a, b)   out of place (a and b equal or not overlapping)
    forward  == fftn(x) * scale          inverse == ifftn(X) * (1 if normalize else size) / scale  (rounded to fp16)
Every execute is one launch on the caller's stream (a capture records one kernel node).
"""

import numpy

from . import _debug as D
from . import _native as N
from .extplan import ExtPlan, buffer_nbytes
from .plan import normalize_shape, on_plan_device, _twiddle_table

_COMPLEX64 = numpy.dtype(numpy.complex64)
_KIND_NAMES = {N.HALF_KERNEL_TILE: "tile", N.HALF_KERNEL_ROW: "row", N.HALF_KERNEL_ND2: "nd2", N.HALF_KERNEL_ND: "nd"}
ROW_MAX = 32768            # longest 1-D complex32 row (passes.row_max(F32, interleaved=True))


def is_complex32(dtype):
    """True for the names of the complex32 dtype: "complex32" and torch.complex32 (torch is not imported for it)."""
    if isinstance(dtype, str):
        return dtype.lower() in ("complex32", "torch.complex32", "chalf")
    return type(dtype).__module__ == "torch" and str(dtype) == "torch.complex32"


def is_float16(dtype):
    if isinstance(dtype, str) or type(dtype).__module__ == "torch":
        return str(dtype).lower() in ("float16", "torch.float16", "half", "torch.half")
    try:
        return numpy.dtype(dtype) == numpy.float16
    except TypeError:
        return False


def half_dims(shape):
    """(x, y, z) of a complex32 shape with its unit axes dropped (x fastest), or ValueError naming the limit."""
    _, xyz = normalize_shape(shape)
    for v in xyz:
        if not isinstance(v, (int, numpy.integer)) or isinstance(v, bool) or v < 1:
            raise ValueError("Wrong shape")
    xyz = tuple(int(v) for v in xyz)
    if not all(v & (v - 1) == 0 for v in xyz):
        raise ValueError("Array dimensions must be powers of two (complex32 has no any_size form)")
    size = xyz[0] * xyz[1] * xyz[2]
    if size < 2:
        raise ValueError("Array must have at least two elements")
    d = [v for v in xyz if v > 1]
    dims = tuple(d + [1] * (3 - len(d)))
    if N.lib.mifft_half_supported(*dims) != 0:
        if len(d) == 1:
            raise ValueError("complex32: 1-D transforms take 2 ... %d points, not %d (one launch per transform; longer rows are a "
                             "follow-up)" % (ROW_MAX, size))
        raise ValueError("complex32: no one-launch kernel for the %s shape %s: 2-D / 3-D shapes take up to %d points, or the fixed "
                         "shapes of up to %d points that one interleaved fp32 launch takes (mifft_half_supported)"
                         % ("2-D" if len(d) == 2 else "3-D", tuple(reversed(d)), N.lib.mifft_nd_max_points_for(N.F32),
                            2 * N.lib.mifft_nd_max_points_for(N.F32)))
    return dims


def half_kernel(dims, variant=0):
    """Name of the kernel instance a complex32 shape (half_dims) runs with `variant` (mifft_half_kernel): "tile:L" / "row:L" (1-D
    rows), "nd2:XxYxZ" (fixed-shape N-D) or "nd:P" (run-time-shaped N-D kernel on its tile of P points)."""
    kind = N.lib.mifft_half_kernel(dims[0], dims[1], dims[2], variant)
    if kind < 0:
        raise ValueError("complex32: unsupported shape %s" % (dims,))
    x, y, z = dims
    if kind in (N.HALF_KERNEL_TILE, N.HALF_KERNEL_ROW):
        return "%s:%d" % (_KIND_NAMES[kind], x)
    if kind == N.HALF_KERNEL_ND2:
        return "nd2:%dx%dx%d" % (x, y, z)
    n = x * y * z
    return "nd:%d" % (4096 if n <= 4096 else 8192 if n <= 8192 else 16384)


def _check_dtype(obj, what):
    """A buffer that knows its element type must hold complex32 data: a DeviceArray of float16, a torch tensor of complex32 or float16."""
    dt = getattr(obj, "dtype", None)
    if dt is None or isinstance(obj, (int, numpy.integer)):
        return
    if type(dt).__module__ == "torch":
        ok = str(dt) in ("torch.complex32", "torch.float16")
    else:
        try:
            ok = numpy.dtype(dt) == numpy.float16
        except TypeError:
            ok = False
    if not ok:
        raise ValueError("pyfft_amd: complex32 plan %s buffer has dtype %s: complex32 data is float16 pairs (numpy / DeviceArray "
                         "float16, torch complex32 or float16)" % (what, dt))


class HalfFFTPlan(ExtPlan):
    """complex32 plan: see the module docstring.  Of ExtPlan's state it uses the capture flag only: no inner plan and no batch-sized
    scratch, so _capture_keepalive stays empty and close() only finishes."""

    @staticmethod
    def validate(shape, dtype="complex32", normalize=True, wait_for_finish=None, fast_math=True, scale=1.0):
        if not is_complex32(dtype):
            raise ValueError("Data type " + str(dtype) + " is not supported")
        half_dims(shape)

    def __init__(self, context, shape, dtype="complex32", normalize=True, wait_for_finish=None, fast_math=True, scale=1.0):
        HalfFFTPlan.validate(shape, dtype)
        self._dims = half_dims(shape)
        self._size = self._dims[0] * self._dims[1] * self._dims[2]
        ExtPlan.__init__(self, context, wait_for_finish)
        self._normalize = normalize
        self._scale = float(scale)
        self._tables = []
        on_plan_device(HalfFFTPlan._build)(self)

    def _build(self):
        self._tw = []
        for n in self._dims:
            if n > 1:
                mem = self._upload(_twiddle_table(n, n, 1, _COMPLEX64))
                self._tables.append(mem)
                self._tw.append(self._context.pointer_of(mem))
            else:
                self._tw.append(None)

    def variant(self, batch=1):
        """mifft_half_kernel's variant for an execute of `batch` transforms: 1 where the complex64 plan of the shape runs its ND pass as
        variant 1 (the tuning table's "nd_generic" list, with the launch size in complex64 bytes), else 0."""
        mach = getattr(self._context, "machine", None)
        if mach is None or D.no_nd_generic() or self._dims[1] == 1:
            return 0
        big = int(batch) * self._size * _COMPLEX64.itemsize > mach.write_through_max_bytes
        return 1 if mach.tuning.nd_runs_generic(False, self._dims, big) else 0

    def kernel_for(self, batch):
        """The kernel instance an execute of `batch` transforms runs (half_kernel)."""
        return half_kernel(self._dims, self.variant(batch))

    @property
    def kernel(self):
        """The kernel instance this plan runs for one transform (kernel_for(1))."""
        return self.kernel_for(1)

    @property
    def dims(self):
        """(x, y, z) with the unit axes dropped, x contiguous."""
        return self._dims

    def _factor(self, inverse):
        if not inverse:
            return self._scale
        return 1.0 / ((self._size if self._normalize else 1.0) * self._scale)

    @on_plan_device
    def _execute(self, wait_for_finish, inverse, batch, data_in, data_out):
        ctx = self._context
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be positive")
        need = batch * self._size * 4
        for what, obj in (("input", data_in), ("output", data_out)):
            _check_dtype(obj, what)
            nb = buffer_nbytes(obj)
            if nb is not None and nb < need:
                raise ValueError("pyfft_amd: complex32 plan %s buffer holds %d bytes, batch %d needs %d" % (what, nb, batch, need))
        src, dst = ctx.pointer_of(data_in), ctx.pointer_of(data_out)
        if src != dst and src < dst + need and dst < src + need:
            raise ValueError("pyfft_amd: partially overlapping buffers (in place is the same buffer on both sides)")
        wait, capturing = self._open((data_in, data_out), wait_for_finish)
        self._stream_step(capturing)
        x, y, z = self._dims
        N.check(N.lib.mifft_launch_half(x, y, z, self.variant(batch), 1 if inverse else 0, batch, src, dst, self._tw[0], self._tw[1], self._tw[2],
                                        self._factor(inverse), ctx.stream_handle()), "mifft_launch_half")
        return self._epilogue(wait)

    def execute(self, data_in, data_out=None, inverse=False, batch=1, wait_for_finish=None):
        """execute(a) in place, execute(a, b) out of place; batch transforms one after the other."""
        if data_out is None:
            data_out = data_in
        return self._execute(wait_for_finish, bool(inverse), batch, data_in, data_out)

    def check(self):
        """(Nothing asynchronous to report: one launch, no dependency counters.)"""
