"""RealFFTPlan: transforms of real input, Plan(shape, dtype=numpy.float32 | numpy.float64, real=True) (docs/extensions.md,
"Real-input transforms").  An opt-in extension like any_size=: without real=True a float dtype keeps its reference meaning (split
complex planes).

A real array of shape (..., nx) read as interleaved complex numbers is the packed array z[..., m] = x[..., 2m] + i x[..., 2m + 1] of
shape (..., nx / 2), on the SAME bytes.  So

    forward   user real buffer --(complex plan of the packed shape, out of place)--> scratch Z --(separation)--> half spectrum
    inverse   half spectrum --(packing)--> scratch Z' --(inverse complex plan, out of place)--> user real buffer

1-D rows whose n / 2 has a ROW kernel (4 <= n <= 65536 fp32, 32768 fp64) take the one-launch form instead (plan._real_form ==
"fused_row", csrc/fft_real_row.hpp): the row transform and the separation / packing in one work-group, one HBM crossing, no scratch.

The complex plan is an ordinary FFTPlan (its own strategy selection: chain, pipelined, persistent) run with scale 1 and no
normalisation; the real plan's scale and normalisation are applied by the separation / packing launch (csrc/fft_real.hip,
mifft_launch_real_post), so no pass is added.  A packed shape of a single point (nx = 2 and no other axis longer than 1) has the
identity as its complex transform: the launch of the separation / packing step is all there is.

The spectrum is interleaved complex numbers of shape shape[:-1] + (nx // 2 + 1,) per item: numpy's rfftn layout.
    forward   execute(real_in, spec_out, batch=k)                  == numpy.fft.rfftn(x) * scale
    inverse   execute(spec_in, real_out, inverse=True, batch=k)    == numpy.fft.irfftn(X, s=shape) * (1 if normalize else prod(shape)) / scale
Executes are out of place only and leave their input untouched.  Every execute is a linear sequence of launches on the caller's
stream (a capture records a linear graph).
"""

import numpy

from . import _native as N
from .extplan import ExtPlan, buffer_nbytes, pow2_shape
from .plan import FFTPlan, on_plan_device, _twiddle_table


def real_params(shape, dtype):
    """(numpy-order shape, precision, real dtype, complex dtype) of a real plan, or ValueError."""
    shape = pow2_shape(shape, "Wrong shape", "Array dimensions must be powers of two (real=True has no any_size form)")
    if shape[-1] < 2:
        raise ValueError("real=True: the contiguous axis (the last numpy axis) must have at least two points")
    try:
        dt = numpy.dtype(dtype)
    except TypeError:
        raise ValueError("Data type " + str(dtype) + " is not supported")
    if dt in (numpy.dtype(numpy.float32), numpy.dtype(numpy.complex64)):
        return shape, N.F32, numpy.dtype(numpy.float32), numpy.dtype(numpy.complex64)
    if dt in (numpy.dtype(numpy.float64), numpy.dtype(numpy.complex128)):
        return shape, N.F64, numpy.dtype(numpy.float64), numpy.dtype(numpy.complex128)
    raise ValueError("Data type " + str(dtype) + " is not supported")


def spectrum_shape(shape):
    """Per-item shape of the half spectrum of a real transform of `shape` (numpy order)."""
    return tuple(shape[:-1]) + (shape[-1] // 2 + 1,)


class RealFFTPlan(ExtPlan):
    """Real-input plan: see the module docstring."""

    @staticmethod
    def validate(shape, dtype=numpy.float32, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0):
        real_params(shape, dtype)

    def __init__(self, context, shape, dtype=numpy.float32, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0):
        self._shape, self._precision, self._rdtype, self._cdtype = real_params(shape, dtype)
        ExtPlan.__init__(self, context, wait_for_finish)
        self._normalize = normalize
        self._scale = float(scale)
        self._size = int(numpy.prod(self._shape))
        nx = self._shape[-1]
        self._nx = nx
        lead = self._shape[:-1]
        self._ny = lead[-1] if len(lead) >= 1 else 1
        self._nz = lead[-2] if len(lead) >= 2 else 1
        self._packed = tuple(lead) + (nx // 2,)
        self._packed_points = self._size // 2
        self._spec_points = self._size // nx * (nx // 2 + 1)
        # 1-D rows whose n / 2 has a ROW kernel: one launch (mifft_launch_real_row); everything else: inner complex plan + separation
        self._real_form = "fused_row" if len(self._shape) == 1 and N.lib.mifft_real_row_supported(self._precision, nx) == 0 else "composed"
        on_plan_device(RealFFTPlan._build)(self)

    def _build(self):
        # the complex transform of the packed data: scale 1, no normalisation (the separation / packing launch applies the real plan's)
        self._tw_half = None
        if self._real_form == "fused_row":
            L = self._nx // 2
            self._tw_half = self._upload(_twiddle_table(L, L, 1, self._cdtype))
        elif self._packed_points > 1:
            packed = self._packed if len(self._packed) > 1 else self._packed[0]
            self._inner = FFTPlan(self._sub, packed, dtype=self._cdtype, normalize=False, wait_for_finish=False, scale=1.0)
        self._tw = self._upload(_twiddle_table(self._nx, self._nx // 2 + 1, 1, self._cdtype))

    # ------------------------------------------------------------------------------------
    def _prepare(self, batch):
        """Scratch of the packed spectrum, where an inner plan runs on it (with the batch unchanged it then always exists)."""
        self._size_scratch(batch, batch * self._packed_points * self._cdtype.itemsize if self._inner is not None else None)

    def _post(self, inverse, batch, src, dst, scale):
        d = N.MifftRealPost()
        d.precision = self._precision
        d.inverse = 1 if inverse else 0
        d.nx, d.ny, d.nz = self._nx, self._ny, self._nz
        d.reserved = 0
        d.outer = batch
        d.stride_in = self._spec_points if inverse else self._packed_points
        d.stride_out = self._packed_points if inverse else self._spec_points
        d.in_ = src
        d.out = dst
        d.tw = self._context.pointer_of(self._tw)
        d.scale = scale
        N.check(N.lib.mifft_launch_real_post(d, self._context.stream_handle()), "mifft_launch_real_post")

    def _check_buffers(self, inverse, batch, data_in, data_out):
        rs = self._rdtype.itemsize
        cs = self._cdtype.itemsize
        need_in = batch * (self._spec_points * cs if inverse else self._size * rs)
        need_out = batch * (self._size * rs if inverse else self._spec_points * cs)
        for what, obj, need in (("input", data_in, need_in), ("output", data_out, need_out)):
            nb = buffer_nbytes(obj)
            if nb is not None and nb < need:
                raise ValueError("pyfft_amd: real plan %s buffer holds %d bytes, batch %d needs %d" % (what, nb, batch, need))

    @on_plan_device
    def _execute(self, wait_for_finish, inverse, batch, data_in, data_out):
        ctx = self._context
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be positive")
        self.check()
        ptr = ctx.pointer_of
        src, dst = ptr(data_in), ptr(data_out)
        self._check_buffers(inverse, batch, data_in, data_out)
        rs, cs = self._rdtype.itemsize, self._cdtype.itemsize
        n_in = batch * (self._spec_points * cs if inverse else self._size * rs)
        n_out = batch * (self._size * rs if inverse else self._spec_points * cs)
        if src < dst + n_out and dst < src + n_in:
            raise ValueError("pyfft_amd: real plans are out of place only (input and output must not overlap)")
        # bases, refused here before anything is enqueued (an inverse used to enqueue its packing launch before the inner plan refused
        # the real side): the real side as real_side_alignment says, the spectrum one complex number
        real_ptr, spec_ptr = (dst, src) if inverse else (src, dst)
        need = self.real_side_alignment
        if real_ptr % need or spec_ptr % cs:
            raise ValueError("pyfft_amd: real plan bases must be aligned: the real side to %d bytes, the spectrum to %d (one complex "
                             "number)" % (need, cs))
        wait, capturing = self._open((data_in, data_out), wait_for_finish)
        self._prepare(batch)
        self._stream_step(capturing)
        if self._real_form == "fused_row":
            factor = self._scale if not inverse else 1.0 / ((self._size if self._normalize else 1.0) * self._scale)
            N.check(N.lib.mifft_launch_real_row(self._precision, self._nx, 1 if inverse else 0, batch, src, dst, ptr(self._tw_half), ptr(self._tw),
                                                factor, ctx.stream_handle()), "mifft_launch_real_row")
        elif not inverse:
            if self._inner is None:
                self._post(False, batch, src, dst, self._scale)
            else:
                z = ptr(self._scratch)
                self._inner.execute(src, z, batch=batch, wait_for_finish=False)
                self._post(False, batch, z, dst, self._scale)
        else:
            factor = 1.0 / ((self._size if self._normalize else 1.0) * self._scale)
            if self._inner is None:
                self._post(True, batch, src, dst, factor)
            else:
                z = ptr(self._scratch)
                self._post(True, batch, src, z, factor)
                self._inner.execute(z, dst, inverse=True, batch=batch, wait_for_finish=False)
        return self._epilogue(wait)

    def execute(self, data_in, data_out=None, *more, inverse=False, batch=1, wait_for_finish=None):
        """execute(real_in, spec_out) forward, execute(spec_in, real_out, inverse=True) inverse; batch items one after the other."""
        if more:
            # (a float dtype means split-complex planes without real=True; a real plan has no planes)
            if len(more) >= 2 and not isinstance(more[0], (bool, numpy.bool_)):
                raise ValueError("pyfft_amd: real plans take one interleaved buffer per side, not split planes")
            inverse = more[0]
            if len(more) >= 2:
                batch = more[1]
            if len(more) >= 3:
                wait_for_finish = more[2]
        if data_out is None:
            raise ValueError("pyfft_amd: real plans are out of place only: execute(data_in, data_out)")
        return self._execute(wait_for_finish, bool(inverse), batch, data_in, data_out)

    # introspection (tests, tools/real_bench.py; inner_plan: ExtPlan)
    @property
    def real_side_alignment(self):
        """Bytes the base of the real side must be aligned to: 16 where the inner complex plan reads or writes it, one complex number
        where the one-launch row or the packing launch alone does (the spectrum side always takes one complex number)."""
        return 16 if self._inner is not None else self._cdtype.itemsize

    def spectrum_shape(self):
        return spectrum_shape(self._shape)
