"""FirPlan: overlap-save FIR filtering, Plan(n, dtype, convolve=True, taps=m) (docs/extensions.md, "FIR filtering plans").

    y[i, t] = scale * sum_{j < m} h[j] * x[i, t - j],   0 <= t < length,   x[i, t < 0] = 0

for `batch` signals of any length, each `pitch` elements after the previous one: scipy.signal.lfilter(h, 1, x) per item.  n is the BLOCK
(transform) length, a power of two with a one-launch instance (mifft_fir_row_supported); m <= n / 2 the number of taps.  The signal is
cut into blocks of n points that repeat the last `overlap` points of the block before (overlap = m - 1; real plans: rounded up to even, so
that a block starts on a packed pair) and advance by hop = n - overlap; every block runs as a convolution row (transform, product with
the filter's spectrum, inverse) in ONE work-group and stores its hop valid samples (csrc/fft_fir_row.hpp).  An execute is ONE launch,
needs no scratch, and moves the signal across HBM once in and once out.

    execute(x, y, spectrum=H, length=Lx, batch=k, pitch=None, spectrum_batch=1)     out of place only
    filter_spectrum(h, H, batch=1)           H = fft(h zero-padded to n) (rfft for real plans), scale 1: m taps per filter

normalize=True (the default) gives the linear convolution times `scale`; normalize=False n times that.  A spectrum of the user's own
design is taken as it is: if its impulse response is longer than m taps, the time aliasing of the blocks is the user's business.
"""

import numpy

from . import _native as N
from .extplan import ExtPlan, buffer_nbytes
from .plan import FFTPlan, on_plan_device, _twiddle_table
from .real import RealFFTPlan


def supported_lengths(precision, real):
    """The block lengths with a one-launch FIR kernel (mifft_fir_row_supported)."""
    return [1 << e for e in range(2, 18) if N.lib.mifft_fir_row_supported(precision, 1 if real else 0, 1 << e) == 0]


def fir_params(shape, dtype, real, taps):
    """(n, precision, data dtype, complex dtype, taps, overlap) of a FIR plan, or ValueError naming taps."""
    if isinstance(shape, tuple) and len(shape) == 1:
        shape = shape[0]
    if isinstance(shape, (tuple, list)):
        raise ValueError("pyfft_amd: taps= plans are 1-D: the block length n (N-D overlap-save is out of scope)")
    if not isinstance(shape, (int, numpy.integer)) or isinstance(shape, bool) or shape < 1:
        raise ValueError("pyfft_amd: taps=: wrong block length")
    n = int(shape)
    if "complex32" in str(dtype) or (isinstance(dtype, str) and dtype.lower() == "chalf"):
        raise ValueError("pyfft_amd: taps= plans have no complex32 form")
    try:
        dt = numpy.dtype(dtype)
    except TypeError:
        raise ValueError("pyfft_amd: taps=: data type " + str(dtype) + " is not supported")
    f32 = (numpy.dtype(numpy.float32), numpy.dtype(numpy.complex64))
    f64 = (numpy.dtype(numpy.float64), numpy.dtype(numpy.complex128))
    if dt not in f32 + f64:
        raise ValueError("pyfft_amd: taps=: data type " + str(dtype) + " is not supported")
    if dt.kind == "f" and not real:
        raise ValueError("pyfft_amd: taps= with a float dtype needs real=True (split planes have no FIR form)")
    prec = N.F32 if dt in f32 else N.F64
    cdt = numpy.dtype(numpy.complex64 if prec == N.F32 else numpy.complex128)
    ddt = numpy.dtype(numpy.float32 if prec == N.F32 else numpy.float64) if real else cdt
    if n & (n - 1):
        raise ValueError("pyfft_amd: taps=: the block length must be a power of two")
    if not isinstance(taps, (int, numpy.integer)) or isinstance(taps, bool):
        raise ValueError("pyfft_amd: taps= must be an integer")
    m = int(taps)
    if N.lib.mifft_fir_row_supported(prec, 1 if real else 0, n) != 0:
        raise ValueError("pyfft_amd: taps=: no one-launch FIR kernel for block length %d; supported: %s"
                         % (n, ", ".join(str(v) for v in supported_lengths(prec, real))))
    if not 1 <= m <= n // 2:
        raise ValueError("pyfft_amd: taps=%d is not in 1 .. n / 2 = %d" % (m, n // 2))
    overlap = m - 1
    if real:
        overlap += overlap & 1
    return n, prec, ddt, cdt, m, overlap


class FirPlan(ExtPlan):
    """Overlap-save FIR plan: see the module docstring."""

    fir_form = "fused_row"

    @staticmethod
    def validate(shape, dtype=numpy.complex64, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0, real=False, taps=None):
        fir_params(shape, dtype, real, taps)

    def __init__(self, context, shape, dtype=numpy.complex64, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0, real=False,
                 taps=None):
        self._real = bool(real)
        self._n, self._precision, self._dtype, self._cdtype, self._taps, self.overlap = fir_params(shape, dtype, self._real, taps)
        self.hop = self._n - self.overlap
        ExtPlan.__init__(self, context, wait_for_finish)
        self._normalize = bool(normalize)
        self._scale = float(scale)
        self._spec_points = self._n // 2 + 1 if self._real else self._n
        on_plan_device(FirPlan._build)(self)

    def _build(self):
        n = self._n
        # the plain plan of the block length: filter_spectrum's forward (scale 1, no normalisation)
        if self._real:
            self._inner = RealFFTPlan(self._sub, n, dtype=self._dtype, normalize=False, wait_for_finish=False, scale=1.0)
        else:
            self._inner = FFTPlan(self._sub, n, dtype=self._cdtype, normalize=False, wait_for_finish=False, scale=1.0)
        L = n // 2 if self._real else n
        self._tw = self._upload(_twiddle_table(L, L, 1, self._cdtype))
        self._tw_sep = self._upload(_twiddle_table(n, L + 1, 1, self._cdtype)) if self._real else None

    @property
    def kernel(self):
        """The one-launch kernel's name."""
        return "fir_row_real_kernel" if self._real else "fir_row_kernel"

    @property
    def taps(self):
        return self._taps

    def blocks(self, length):
        """Blocks (rows of the launch) per item of `length` samples: ceil(length / hop)."""
        length = int(length)
        if length < 1:
            raise ValueError("pyfft_amd: taps= plan: length must be at least 1")
        return -(-length // self.hop)

    # ------------------------------------------------------------------------------------
    def _prepare(self, batch):
        """filter_spectrum's padded taps: scratch of n points per filter (execute needs none and never prepares)."""
        self._size_scratch(batch, batch * self._n * self._dtype.itemsize, call="filter_spectrum")

    def _check_buffers(self, batch, x, y, spectrum, spectrum_batch, length, pitch):
        isz, cs = self._dtype.itemsize, self._cdtype.itemsize
        data_bytes = ((batch - 1) * pitch + length) * isz
        spec_bytes = spectrum_batch * self._spec_points * cs
        for what, obj, need in (("input", x, data_bytes), ("output", y, data_bytes), ("spectrum", spectrum, spec_bytes)):
            nb = buffer_nbytes(obj)
            if nb is not None and nb < need:
                raise ValueError("pyfft_amd: taps= plan %s buffer holds %d bytes, batch %d of length %d needs %d" % (what, nb, batch, length, need))
        ptr = self._context.pointer_of
        xs, ys, ss = ptr(x), ptr(y), ptr(spectrum)
        if xs < ys + data_bytes and ys < xs + data_bytes:
            raise ValueError("pyfft_amd: taps= plan input and output overlap (out of place only)")
        for d in (xs, ys):
            if ss < d + data_bytes and d < ss + spec_bytes:
                raise ValueError("pyfft_amd: taps= plan spectrum overlaps the data")
        if xs % cs or ys % cs or ss % cs:
            raise ValueError("pyfft_amd: taps= plan bases must be aligned to %d bytes (one complex number%s)"
                             % (cs, "; real data: one pair of reals" if self._real else ""))
        return xs, ys, ss

    @on_plan_device
    def _execute(self, wait_for_finish, batch, x, y, spectrum, spectrum_batch, length, pitch):
        ctx = self._context
        xs, ys, ss = self._check_buffers(batch, x, y, spectrum, spectrum_batch, length, pitch)
        wait, capturing = self._open((x, y, spectrum), wait_for_finish)
        self._stream_step(capturing)
        factor = self._scale / (self._n if self._normalize else 1.0)
        ptr = ctx.pointer_of
        N.check(N.lib.mifft_launch_fir_row(self._precision, 1 if self._real else 0, self._n, self.overlap, length, pitch, batch, xs, ys, ss,
                                           self._spec_points if spectrum_batch > 1 else 0, ptr(self._tw),
                                           ptr(self._tw_sep) if self._tw_sep is not None else None, factor, ctx.stream_handle()),
                "mifft_launch_fir_row")
        return self._epilogue(wait)

    def execute(self, x, y=None, spectrum=None, length=None, batch=1, pitch=None, spectrum_batch=1, correlate=False, wait_for_finish=None):
        """y[i, t] = scale * sum_j h[j] x[i, t - j], 0 <= t < length, for `batch` items `pitch` elements apart on both sides (default:
        length; real plans: rounded up to even).  H = spectrum: one shared by every item, or one per item (spectrum_batch=batch).
        Elements length .. pitch - 1 of y are never written."""
        if correlate:
            raise ValueError("pyfft_amd: taps= plans have no correlate=True: reverse and conjugate the taps instead")
        if y is None:
            raise ValueError("pyfft_amd: taps= plans are out of place only: pass y")
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be positive")
        if spectrum is None:
            raise ValueError("pyfft_amd: taps= plans need spectrum= (a device buffer of the filter's spectrum, see filter_spectrum)")
        if length is None:
            raise ValueError("pyfft_amd: taps= plans need length= (samples per item)")
        length = int(length)
        if length < 1:
            raise ValueError("pyfft_amd: taps= plan: length must be at least 1")
        if pitch is None:
            pitch = length + (length & 1) if self._real else length
        pitch = int(pitch)
        if pitch < length:
            raise ValueError("pyfft_amd: taps= plan: pitch %d is below the length %d" % (pitch, length))
        if self._real and pitch & 1:
            raise ValueError("pyfft_amd: taps= plan: real plans need an even pitch (every item starts on a packed pair), not %d" % pitch)
        spectrum_batch = int(spectrum_batch)
        if spectrum_batch not in (1, batch):
            raise ValueError("pyfft_amd: taps= plan spectrum_batch must be 1 or batch (%d), not %d" % (batch, spectrum_batch))
        self.check()
        return self._execute(wait_for_finish, batch, x, y, spectrum, spectrum_batch, length, pitch)

    @on_plan_device
    def filter_spectrum(self, h, out, batch=1):
        """out = fft(h zero-padded to n) (rfft for real plans), scale 1, per filter of m taps (dense: filter f starts at element f * m
        of h): one launch pads the taps into plan-owned scratch, the plain plan of n points transforms it (bit-identical to that plan
        run on the zero-padded taps)."""
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be positive")
        cs = self._cdtype.itemsize
        for what, obj, need in (("taps", h, batch * self._taps * self._dtype.itemsize), ("output", out, batch * self._spec_points * cs)):
            nb = buffer_nbytes(obj)
            if nb is not None and nb < need:
                raise ValueError("pyfft_amd: taps= plan filter_spectrum %s buffer holds %d bytes, batch %d needs %d" % (what, nb, batch, need))
        ctx = self._context
        wait, capturing = self._open((h, out), call="filter_spectrum")
        self._prepare(batch)
        self._stream_step(capturing)
        z = ctx.pointer_of(self._scratch)
        N.check(N.lib.mifft_launch_fir_pad(self._precision, 1 if self._real else 0, self._n, self._taps, batch, ctx.pointer_of(h), z,
                                           ctx.stream_handle()), "mifft_launch_fir_pad")
        self._inner.execute(z, out, batch=batch, wait_for_finish=False)
        if wait:
            self.finish()
        return out

    def spectrum_shape(self):
        return (self._spec_points,)
