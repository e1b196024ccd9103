"""ConvPlan: FFT convolution, Plan(shape, dtype, convolve=True) (docs/extensions.md, "Convolution plans").

    y = scale * IFFTN(FFTN(x) * S)   per item,   S = H, or conj(H) with correlate=True

IFFTN divides by the item's point count only when normalize=True; `scale` multiplies the result once (a convolution has no forward /
inverse pair for it to cancel across).  Real plans (real=True): y == numpy.fft.irfftn(numpy.fft.rfftn(x) * S, s=shape) * scale, H in
numpy's rfftn half-spectrum layout, the edge planes kx = 0 and kx = nx / 2 of the product read through their Hermitian parts (numpy's
irfftn rule, docs/extensions.md "The edge-plane rule").

    execute(x, y, spectrum=H, batch=k, correlate=False, spectrum_batch=1)    y may be x (in place) or a disjoint buffer
    filter_spectrum(h, H, batch=1)                                          H = fftn(h) (rfftn for real plans), scale 1

Forms (plan.conv_form):
    "fused_row"  1-D rows with mifft_conv_row_supported(precision, real, n) == 0: ONE launch (csrc/fft_conv_row.hpp), the row crosses
                 HBM once
    "composed"   everything else: the inner plan's forward (x -> y), one spectrum product in place (mifft_aux_mul_spectrum), the inner
                 plan's inverse in place on y.  Real plans: the real plan's forward into a half-spectrum scratch, the product there, the real
                 plan's inverse into y.  The inner plans keep their own strategy selection.
"""

import numpy

from . import _native as N
from .extplan import ExtPlan, buffer_nbytes, pow2_shape
from .plan import FFTPlan, on_plan_device, _twiddle_table
from .real import RealFFTPlan, real_params, spectrum_shape


def conv_params(shape, dtype, real):
    """(numpy-order shape, precision, data dtype, complex dtype) of a convolution plan, or ValueError naming convolve."""
    if real:
        try:
            shape, prec, rdt, cdt = real_params(shape, dtype)
        except ValueError as e:
            raise ValueError("pyfft_amd: convolve=True: %s" % e)
        return shape, prec, rdt, cdt
    shape = pow2_shape(shape, "pyfft_amd: convolve=True: wrong shape", "pyfft_amd: convolve=True: array dimensions must be powers of two")
    if isinstance(dtype, str) and dtype.lower() in ("complex32", "chalf"):
        raise ValueError("pyfft_amd: convolve=True has no complex32 form")
    if "complex32" in str(dtype):
        raise ValueError("pyfft_amd: convolve=True has no complex32 form")
    try:
        dt = numpy.dtype(dtype)
    except TypeError:
        raise ValueError("pyfft_amd: convolve=True: data type " + str(dtype) + " is not supported")
    if dt == numpy.dtype(numpy.complex64):
        return shape, N.F32, dt, dt
    if dt == numpy.dtype(numpy.complex128):
        return shape, N.F64, dt, dt
    if dt.kind == "f":
        raise ValueError("pyfft_amd: convolve=True with a float dtype needs real=True (split planes have no convolution form)")
    raise ValueError("pyfft_amd: convolve=True: data type " + str(dtype) + " is not supported")


class ConvPlan(ExtPlan):
    """Convolution plan: see the module docstring."""

    @staticmethod
    def validate(shape, dtype=numpy.complex64, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0, real=False):
        conv_params(shape, dtype, real)

    def __init__(self, context, shape, dtype=numpy.complex64, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0, real=False):
        self._real = bool(real)
        self._shape, self._precision, self._dtype, self._cdtype = conv_params(shape, dtype, self._real)
        ExtPlan.__init__(self, context, wait_for_finish)
        self._normalize = bool(normalize)
        self._scale = float(scale)
        self._size = int(numpy.prod(self._shape))
        self._spec_points = int(numpy.prod(spectrum_shape(self._shape))) if self._real else self._size
        n = self._shape[0]
        fused = len(self._shape) == 1 and N.lib.mifft_conv_row_supported(self._precision, 1 if self._real else 0, n) == 0
        self.conv_form = "fused_row" if fused else "composed"
        on_plan_device(ConvPlan._build)(self)

    def _build(self):
        self._tw = self._tw_sep = None
        # the plain plan of the shape: the composed form's two transforms and filter_spectrum's forward (scale 1, no normalisation)
        shp = self._shape if len(self._shape) > 1 else self._shape[0]
        if self._real:
            self._inner = RealFFTPlan(self._sub, shp, dtype=self._dtype, normalize=False, wait_for_finish=False, scale=1.0)
        else:
            self._inner = FFTPlan(self._sub, shp, dtype=self._cdtype, normalize=False, wait_for_finish=False, scale=1.0)
        if self.conv_form == "fused_row":
            n = self._shape[0]
            L = n // 2 if self._real else n
            self._tw = self._upload(_twiddle_table(L, L, 1, self._cdtype))
            if self._real:
                self._tw_sep = self._upload(_twiddle_table(n, L + 1, 1, self._cdtype))

    @property
    def kernel(self):
        """The one-launch kernel's name ("conv_row_kernel" / "conv_row_real_kernel"), or "composed"."""
        if self.conv_form != "fused_row":
            return "composed"
        return "conv_row_real_kernel" if self._real else "conv_row_kernel"

    # ------------------------------------------------------------------------------------
    def _prepare(self, batch):
        """Real composed form: plan-owned half-spectrum scratch, sized by batch (kept alive for a graph that recorded the previous one)."""
        need = self._real and self.conv_form == "composed"
        self._size_scratch(batch, batch * self._spec_points * self._cdtype.itemsize if need else None)

    def _check_buffers(self, batch, x, y, spectrum, spectrum_batch):
        data_bytes = batch * self._size * self._dtype.itemsize
        spec_bytes = spectrum_batch * self._spec_points * self._cdtype.itemsize
        for what, obj, need in (("input", x, data_bytes), ("output", y, data_bytes), ("spectrum", spectrum, spec_bytes)):
            nb = buffer_nbytes(obj)
            if nb is not None and nb < need:
                raise ValueError("pyfft_amd: convolve plan %s buffer holds %d bytes, batch %d needs %d" % (what, nb, batch, need))
        ptr = self._context.pointer_of
        xs, ys, ss = ptr(x), ptr(y), ptr(spectrum)
        if xs != ys and xs < ys + data_bytes and ys < xs + data_bytes:
            raise ValueError("pyfft_amd: convolve plan input and output overlap without being the same buffer")
        for d in (xs, ys):
            if ss < d + data_bytes and d < ss + spec_bytes:
                raise ValueError("pyfft_amd: convolve plan spectrum overlaps the data")
        # bases, refused here before anything is enqueued: the data as every launch that touches it takes it (the one-launch row: one
        # complex number; the inner complex plan: 16 bytes; the inner real plan: its real_side_alignment), the spectrum one complex number
        cs = self._cdtype.itemsize
        if self.conv_form == "fused_row":
            need = cs
        elif self._real:
            need = self._inner.real_side_alignment
        else:
            need = 16
        if xs % need or ys % need or ss % cs:
            raise ValueError("pyfft_amd: convolve plan bases must be aligned: the data to %d bytes, the spectrum to %d (one complex number)"
                             % (need, cs))
        return xs, ys, ss

    @on_plan_device
    def _execute(self, wait_for_finish, batch, x, y, spectrum, spectrum_batch, correlate):
        ctx = self._context
        xs, ys, ss = self._check_buffers(batch, x, y, spectrum, spectrum_batch)
        wait, capturing = self._open((x, y, spectrum), wait_for_finish)
        self._prepare(batch)
        self._stream_step(capturing)
        factor = self._scale / (self._size if self._normalize else 1.0)
        pitch = self._spec_points if spectrum_batch > 1 else 0
        cj = 1 if correlate else 0
        if self.conv_form == "fused_row":
            ptr = ctx.pointer_of
            N.check(N.lib.mifft_launch_conv_row(self._precision, 1 if self._real else 0, self._shape[0], batch, xs, ys, ss, pitch, cj,
                                                ptr(self._tw), ptr(self._tw_sep) if self._tw_sep is not None else None, factor,
                                                ctx.stream_handle()), "mifft_launch_conv_row")
        elif self._real:
            z = ctx.pointer_of(self._scratch)
            self._inner.execute(xs, z, batch=batch, wait_for_finish=False)
            N.check(N.lib.mifft_aux_mul_spectrum(self._precision, z, ss, batch, self._spec_points, pitch, cj, factor, ctx.stream_handle()),
                    "mifft_aux_mul_spectrum")
            self._inner.execute(z, ys, inverse=True, batch=batch, wait_for_finish=False)
        else:
            if xs == ys:
                self._inner.execute(xs, batch=batch, wait_for_finish=False)
            else:
                self._inner.execute(xs, ys, batch=batch, wait_for_finish=False)
            N.check(N.lib.mifft_aux_mul_spectrum(self._precision, ys, ss, batch, self._size, pitch, cj, factor, ctx.stream_handle()),
                    "mifft_aux_mul_spectrum")
            self._inner.execute(ys, inverse=True, batch=batch, wait_for_finish=False)
        return self._epilogue(wait)

    def execute(self, x, y=None, spectrum=None, batch=1, correlate=False, spectrum_batch=1, wait_for_finish=None):
        """y = scale * IFFTN(FFTN(x) * S) for `batch` items; y None: in place.  S = spectrum (conj(spectrum) with correlate=True),
        one shared by every item (spectrum_batch=1) or one per item (spectrum_batch=batch)."""
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be positive")
        if spectrum is None:
            raise ValueError("pyfft_amd: convolve plans need spectrum= (a device buffer of the filter's spectrum)")
        spectrum_batch = int(spectrum_batch)
        if spectrum_batch not in (1, batch):
            raise ValueError("pyfft_amd: convolve plan spectrum_batch must be 1 or batch (%d), not %d" % (batch, spectrum_batch))
        self.check()
        return self._execute(wait_for_finish, batch, x, x if y is None else y, spectrum, spectrum_batch, bool(correlate))

    @on_plan_device
    def filter_spectrum(self, h, out, batch=1):
        """out = fftn(h) (rfftn for real plans), scale 1, per item: a spatial kernel's spectrum H for execute(spectrum=out).  The plain
        plan of the shape runs it (bit-identical to Plan(shape).execute(h, out) / Plan(shape, real=True).execute(h, out))."""
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be positive")
        nb = buffer_nbytes(out)
        need = batch * self._spec_points * self._cdtype.itemsize
        if nb is not None and nb < need:
            raise ValueError("pyfft_amd: convolve plan filter_spectrum output holds %d bytes, batch %d needs %d" % (nb, batch, need))
        wait, capturing = self._open((h, out), call="filter_spectrum")
        self._stream_step(capturing)
        self._inner.execute(h, out, batch=batch, wait_for_finish=False)
        if wait:
            self.finish()
        return out

    def spectrum_shape(self):
        return spectrum_shape(self._shape) if self._real else tuple(self._shape)
