"""R2RPlan: cosine and sine transforms, Plan(shape, dtype=numpy.float32 | numpy.float64, r2r="dct" | "dst") (docs/extensions.md,
"Real-to-real transforms").

    forward   execute(x, y, batch=k)                  y == scipy.fft.dctn(x, type=2) * scale              (dstn for "dst")
    inverse   execute(y, x, inverse=True, batch=k)    x == scipy.fft.idctn(y, type=2) / scale              (normalize=True)
                                                      x == scipy.fft.dctn(y, type=3) / scale               (normalize=False)
    ortho=True: norm="ortho" in both directions.  execute(x) transforms in place.

Makhoul's algorithm (csrc/fft_r2r.hip, tests/dct_model.py): the per-axis permutation v = [x0, x2, ..., x3, x1] read as interleaved complex
numbers is the packed array z of shape shape[:-1] + (n / 2,); its complex transform plus one twiddle step per output gives the result.

    forward   x --(pre: permutation)--> scratch v --(inner FFTPlan, in place)--> Z --(post: separation + twiddles)--> y
    inverse   y --(pre: twiddles + packing)--> scratch Z' --(inner inverse FFTPlan, in place)--> v --(post: permutation)--> x

Unit axes are dropped: scipy multiplies by 2 along an axis of length 1 (by 1 with ortho), a factor folded into the tables with the scale
and the normalisation, so the twiddle steps add no multiply for it.  The inner plan is an ordinary FFTPlan of the packed shape (its own
strategy selection) with scale 1 and no normalisation.

plan.r2r_form: "fused_row" for shapes with one axis longer than 1 whose length has a one-launch row (mifft_r2r_row_supported, n = 4 ...
8192: csrc/fft_r2r_row.hpp, the row crosses HBM once), "composed" otherwise.  A fused plan runs the composed form for an execute whose
buffers are not 16-byte aligned (the row kernel's 16-byte loads and stores need it).
"""

import numpy

from . import _native as N
from .extplan import ExtPlan, buffer_nbytes, pow2_shape
from .plan import FFTPlan, on_plan_device

KINDS = {"dct": 0, "dst": 1}


def r2r_params(shape, dtype, r2r, ortho=False, normalize=True):
    """(numpy-order shape, precision, real dtype, kind) of an r2r plan, or a ValueError naming r2r."""
    if not isinstance(r2r, str) or r2r not in KINDS:
        raise ValueError("pyfft_amd: r2r must be \"dct\" or \"dst\", not %r" % (r2r,))
    shape = pow2_shape(shape, "pyfft_amd: r2r=: wrong shape", "pyfft_amd: r2r=: array dimensions must be powers of two")
    if "complex32" in str(dtype) or "float16" in str(dtype) or (isinstance(dtype, str) and dtype.lower() in ("chalf", "half")):
        raise ValueError("pyfft_amd: r2r= has no half-precision form (float32 or float64)")
    if ortho and not normalize:
        raise ValueError("pyfft_amd: r2r= with ortho=True is orthonormal in both directions: normalize=False does not apply")
    try:
        dt = numpy.dtype(dtype)
    except TypeError:
        raise ValueError("pyfft_amd: r2r=: data type " + str(dtype) + " is not supported (float32 or float64)")
    if dt == numpy.dtype(numpy.float32):
        return shape, N.F32, dt, KINDS[r2r]
    if dt == numpy.dtype(numpy.float64):
        return shape, N.F64, dt, KINDS[r2r]
    raise ValueError("pyfft_amd: r2r=: data type " + str(dtype) + " is not supported (real float32 or float64)")


def _weights(n, ortho):
    """the ortho weight c[k] of the DCT index k, in extended precision (1 without ortho)"""
    c = numpy.ones(n, numpy.longdouble)
    if ortho:
        c[:] = numpy.sqrt(numpy.longdouble(1) / (2 * n))
        c[0] = numpy.sqrt(numpy.longdouble(1) / (4 * n))
    return c


def _phase(k, m, sign):
    """exp(sign 2 pi i k / m) in extended precision (exact integer phase reduced mod m first)"""
    k = numpy.asarray(k, numpy.int64) % m
    ang = numpy.longdouble(sign) * 2 * numpy.pi * (k.astype(numpy.longdouble) / numpy.longdouble(m))
    return numpy.cos(ang), numpy.sin(ang)


def global_factor(shape, inverse, ortho, normalize, scale):
    """(kept axes, g): the axes of length > 1 and the factor the last kept axis's table carries (tests/dct_model.py)"""
    kept = tuple(n for n in shape if n > 1)
    units = len(shape) - len(kept)
    one = numpy.longdouble(1)
    if not inverse:
        return kept, one / 2 * numpy.longdouble(scale) * (one if ortho else numpy.longdouble(2) ** units)
    g = one / numpy.longdouble(int(numpy.prod(kept))) * (one if ortho else (one / 2) ** units)
    if not normalize:
        g *= numpy.longdouble(int(numpy.prod([2 * n for n in shape])))
    return kept, g / numpy.longdouble(scale)


def tables(kept, inverse, ortho, g, complex_dtype):
    """The twiddle step's table (include/mifft.h, mifft_r2r_step): per axis t[k] = c[k] w(4n)^k (forward) or u[k] = w(4n)^-k / 2c[k]
    (inverse), the last axis's times g, then w(n_last)^k for k = 0 .. n_last / 4.  Evaluated in extended precision, rounded once."""
    parts = []
    for a, n in enumerate(kept):
        k = numpy.arange(n)
        c, s = _phase(k, 4 * n, 1 if inverse else -1)
        f = (1 / (2 * _weights(n, ortho))) if inverse else _weights(n, ortho)
        if a == len(kept) - 1:
            f = f * g
        parts.append((c * f, s * f))
    nl = kept[-1]
    c, s = _phase(numpy.arange(nl // 4 + 1), nl, -1)
    parts.append((c, s))
    re = numpy.concatenate([p[0] for p in parts])
    im = numpy.concatenate([p[1] for p in parts])
    out = numpy.empty(re.size, complex_dtype)
    out.real = re                                # one rounding, extended -> working precision
    out.imag = im
    return out


def r2r_form_of(shape, precision):
    """"fused_row" or "composed": the form a plan of this (numpy-order) shape and precision runs"""
    kept = tuple(n for n in shape if n > 1)
    if len(kept) == 1 and N.lib.mifft_r2r_row_supported(precision, kept[0]) == 0:
        return "fused_row"
    return "composed"


def row_tables(n, inverse, ortho, g, complex_dtype):
    """The one-launch row's tables (include/mifft.h, mifft_launch_r2r_row): w(n/2)^k, w(n)^k (n/2 entries each), and forward
    2 g c[k] w(4n)^k (k <= n/2) or inverse u[k] = g w(4n)^-k / 2c[k] (k < n).  Extended precision, rounded once."""
    L = n // 2

    def cx(re, im):
        out = numpy.empty(numpy.shape(re), complex_dtype)
        out.real = re
        out.imag = im
        return out
    stage = cx(*_phase(numpy.arange(L), L, -1))
    sep = cx(*_phase(numpy.arange(L), n, -1))
    k = numpy.arange(L + 1 if not inverse else n)
    c, s = _phase(k, 4 * n, 1 if inverse else -1)
    w = _weights(n, ortho)[k]
    f = (g / (2 * w)) if inverse else (2 * g * w)
    return stage, sep, cx(c * f, s * f)


class R2RPlan(ExtPlan):
    """Cosine / sine transform plan: see the module docstring."""

    @staticmethod
    def validate(shape, dtype=numpy.float32, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0, r2r="dct", ortho=False):
        r2r_params(shape, dtype, r2r, ortho, normalize)

    def __init__(self, context, shape, dtype=numpy.float32, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0, r2r="dct",
                 ortho=False):
        self._shape, self._precision, self._dtype, self._kind = r2r_params(shape, dtype, r2r, ortho, normalize)
        self._cdtype = numpy.dtype(numpy.complex64 if self._precision == N.F32 else numpy.complex128)
        ExtPlan.__init__(self, context, wait_for_finish)
        self._normalize = bool(normalize)
        self._ortho = bool(ortho)
        self._scale = float(scale)
        self._size = int(numpy.prod(self._shape))
        self._kept = tuple(n for n in self._shape if n > 1)
        self.r2r = r2r
        self.r2r_form = r2r_form_of(self._shape, self._precision)
        on_plan_device(R2RPlan._build)(self)

    def _build(self):
        self._tw = {}
        self._single = {}
        if not self._kept:
            # every axis a unit axis: the transform is a multiple of x, one permutation launch
            for inv in (False, True):
                self._single[inv] = float(global_factor(self._shape, inv, self._ortho, self._normalize, self._scale)[1] * (1 if inv else 2))
            return
        packed = tuple(n for n in self._kept[:-1]) + ((self._kept[-1] // 2,) if self._kept[-1] > 2 else ())
        if packed:
            self._inner = FFTPlan(self._sub, packed if len(packed) > 1 else packed[0], dtype=self._cdtype, normalize=False,
                                  wait_for_finish=False, scale=1.0)
        for inv in (False, True):
            kept, g = global_factor(self._shape, inv, self._ortho, self._normalize, self._scale)
            self._tw[inv] = self._upload(tables(kept, inv, self._ortho, g, self._cdtype))
        self._row = {}
        if self.r2r_form == "fused_row":
            for inv in (False, True):
                g = global_factor(self._shape, inv, self._ortho, self._normalize, self._scale)[1]
                self._row[inv] = [self._upload(host) for host in row_tables(self._kept[0], inv, self._ortho, g, self._cdtype)]

    @property
    def kernel(self):
        """The instance: "r2r_row_kernel<n>" (L <= 32: "r2r_row_small_kernel<n>") for a fused row, "r2r_perm_kernel" for an item of one
        point, else the composed form's three launches."""
        if not self._kept:
            return "r2r_perm_kernel"
        if self.r2r_form == "fused_row":
            n = self._kept[0]
            return ("r2r_row_small_kernel<%d>" if n <= 64 else "r2r_row_kernel<%d>") % n
        packed = tuple(self._kept[:-1]) + ((self._kept[-1] // 2,) if self._kept[-1] > 2 else ())
        return "r2r_perm_kernel + FFTPlan%s + r2r_orbit_kernel<D=%d>" % (packed, len(self._kept) - 1)

    # ------------------------------------------------------------------------------------
    def _prepare(self, batch, composed=True):
        """Scratch of the packed array for the composed form.  The one-launch route (composed=False) and an item of one point leave
        the scratch state alone: a fused execute at another batch neither releases the composed scratch nor records its batch."""
        if composed and self._kept:
            self._size_scratch(batch, batch * self._size * self._dtype.itemsize)

    def _step(self, post, inverse, batch, src, dst, scale=1.0, single=False):
        d = N.MifftR2rStep()
        d.precision = self._precision
        d.inverse = 1 if inverse else 0
        d.kind = self._kind
        dims = (1,) if single else self._kept
        d.ndim = len(dims)
        for a in range(3):
            d.n[a] = dims[a] if a < len(dims) else 0
        d.reserved = 0
        d.outer = batch
        d.in_ = src
        d.out = dst
        d.tw = None if (post == inverse) else self._context.pointer_of(self._tw[inverse])
        d.scale = scale
        fn = N.lib.mifft_launch_r2r_post if post else N.lib.mifft_launch_r2r_pre
        N.check(fn(d, self._context.stream_handle()), "mifft_launch_r2r_post" if post else "mifft_launch_r2r_pre")

    def _check_buffers(self, batch, data_in, data_out):
        need = batch * self._size * self._dtype.itemsize
        for what, obj in (("input", data_in), ("output", data_out)):
            nb = buffer_nbytes(obj)
            if nb is not None and nb < need:
                raise ValueError("pyfft_amd: r2r plan %s buffer holds %d bytes, batch %d needs %d" % (what, nb, batch, need))
        ptr = self._context.pointer_of
        src, dst = ptr(data_in), ptr(data_out)
        if src != dst and src < dst + need and dst < src + need:
            raise ValueError("pyfft_amd: r2r plan input and output overlap without being the same buffer")
        return src, dst

    @on_plan_device
    def _execute(self, wait_for_finish, inverse, batch, data_in, data_out):
        ctx = self._context
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be positive")
        self.check()
        src, dst = self._check_buffers(batch, data_in, data_out)
        wait, capturing = self._open((data_in, data_out), wait_for_finish)
        fused = self.r2r_form == "fused_row" and (src | dst) % 16 == 0
        self._prepare(batch, composed=not fused)
        self._stream_step(capturing)
        if not self._kept:
            self._step(inverse, inverse, batch, src, dst, self._single[inverse], single=True)
        elif fused:
            stage, sep, tab = (ctx.pointer_of(b) for b in self._row[inverse])
            N.check(N.lib.mifft_launch_r2r_row(self._precision, self._kept[0], 1 if inverse else 0, self._kind, batch, src, dst, stage, sep,
                                               tab, ctx.stream_handle()), "mifft_launch_r2r_row")
        else:
            z = ctx.pointer_of(self._scratch)
            self._step(False, inverse, batch, src, z)
            if self._inner is not None:
                self._inner.execute(z, inverse=inverse, batch=batch, wait_for_finish=False)
            self._step(True, inverse, batch, z, dst)
        return self._epilogue(wait)

    def execute(self, data_in, data_out=None, *more, inverse=False, batch=1, wait_for_finish=None):
        """execute(x, y) forward (type II), execute(y, x, inverse=True) inverse (type III); data_out None: in place."""
        if more:
            if len(more) >= 2 and not isinstance(more[0], (bool, numpy.bool_)):
                raise ValueError("pyfft_amd: r2r plans take one real buffer per side, not split planes")
            inverse = more[0]
            if len(more) >= 2:
                batch = more[1]
            if len(more) >= 3:
                wait_for_finish = more[2]
        if data_out is None:
            data_out = data_in
        return self._execute(wait_for_finish, bool(inverse), batch, data_in, data_out)
