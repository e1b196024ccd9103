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
from .generic import _SubContext
from .plan import FFTPlan, on_plan_device
from .real import _buffer_nbytes

KINDS = {"dct": 0, "dst": 1}


def _is_pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def r2r_params(shape, dtype, r2r, ortho=False, normalize=True):
    """(numpy-order shape, precision, real dtype, kind) of an r2r plan, or a ValueError naming r2r."""
    if not isinstance(r2r, str) or r2r not in KINDS:
        raise ValueError("pyfft_amd: r2r must be \"dct\" or \"dst\", not %r" % (r2r,))
    if isinstance(shape, (int, numpy.integer)) and not isinstance(shape, bool):
        shape = (shape,)
    if not isinstance(shape, tuple) or not 1 <= len(shape) <= 3:
        raise ValueError("pyfft_amd: r2r=: wrong shape")
    for v in shape:
        if not isinstance(v, (int, numpy.integer)) or isinstance(v, bool) or v < 1:
            raise ValueError("pyfft_amd: r2r=: wrong shape")
    shape = tuple(int(v) for v in shape)
    if not all(_is_pow2(v) for v in shape):
        raise ValueError("pyfft_amd: r2r=: array dimensions must be powers of two")
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


class R2RPlan(object):
    """Cosine / sine transform plan: see the module docstring."""

    @staticmethod
    def validate(shape, dtype=numpy.float32, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0, r2r="dct", ortho=False):
        r2r_params(shape, dtype, r2r, ortho, normalize)

    def __init__(self, context, shape, dtype=numpy.float32, normalize=True, wait_for_finish=None, fast_math=True, scale=1.0, r2r="dct",
                 ortho=False):
        self._shape, self._precision, self._dtype, self._kind = r2r_params(shape, dtype, r2r, ortho, normalize)
        self._cdtype = numpy.dtype(numpy.complex64 if self._precision == N.F32 else numpy.complex128)
        self._context = context
        self._normalize = bool(normalize)
        self._ortho = bool(ortho)
        self._scale = float(scale)
        self._wait_for_finish = wait_for_finish
        self._size = int(numpy.prod(self._shape))
        self._kept = tuple(n for n in self._shape if n > 1)
        self.r2r = r2r
        self.r2r_form = r2r_form_of(self._shape, self._precision)
        self._sub = _SubContext(context)
        self._scratch = None
        self._last_batch = 0
        self._captured = False
        self._capture_keepalive = []
        on_plan_device(R2RPlan._build)(self)

    def _build(self):
        ctx = self._context
        self._inner = None
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
            host = numpy.ascontiguousarray(tables(kept, inv, self._ortho, g, self._cdtype))
            buf = ctx.allocate_raw(host.nbytes)
            ctx.upload(buf, host)
            self._tw[inv] = buf
        self._row = {}
        if self.r2r_form == "fused_row":
            for inv in (False, True):
                g = global_factor(self._shape, inv, self._ortho, self._normalize, self._scale)[1]
                bufs = []
                for host in row_tables(self._kept[0], inv, self._ortho, g, self._cdtype):
                    host = numpy.ascontiguousarray(host)
                    buf = ctx.allocate_raw(host.nbytes)
                    ctx.upload(buf, host)
                    bufs.append(buf)
                self._row[inv] = bufs

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
        """Plan-owned scratch of the packed array for the composed form, sized by batch (kept alive for a graph that recorded the
        previous one)."""
        if not composed or not self._kept or (batch == self._last_batch and self._scratch is not None):
            return
        if self._context.capturing():
            raise RuntimeError("pyfft_amd: execute() on a capturing stream needs one eager execute() of the same batch first")
        self._release_scratch()
        self._scratch = self._context.allocate(batch * self._size * self._dtype.itemsize)
        self._last_batch = batch         # (committed only now: after a failed allocation the plan is as close() leaves it)

    def _release_scratch(self):
        """Let go of the scratch: to the keep-alive list once a graph has recorded an execute (it replays on it); else, where it came
        from a mempool, only after the plan's own asynchronous executes have finished with it (hipFree does that waiting itself)."""
        if self._scratch is not None:
            if self._captured:
                self._capture_keepalive.append(self._scratch)
            else:
                self._context.wait_scratch()
        self._scratch = None
        self._last_batch = 0

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
            nb = _buffer_nbytes(obj)
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
        ctx.createQueue((data_in, data_out))
        wait = self._wait_for_finish if wait_for_finish is None else wait_for_finish
        capturing = ctx.capturing()
        if capturing and wait:
            raise RuntimeError("pyfft_amd: execute() on a capturing stream cannot wait for the result: build the plan with stream= "
                               "(or wait_for_finish=False), or pass wait_for_finish=False to this call")
        fused = self.r2r_form == "fused_row" and (src | dst) % 16 == 0
        self._prepare(batch, composed=not fused)
        ctx.order_scratch(capturing)
        if capturing:
            from .hip import Graph
            self._captured = True
            Graph.retain(self)
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
        if wait:
            self.finish()
            return None
        ctx.flush()
        return ctx.getQueue()

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

    # ------------------------------------------------------------------------------------
    @on_plan_device
    def finish(self):
        """Wait for the plan's stream, then raise if the inner plan reported invalid results."""
        self._context.wait()
        if self._inner is not None:
            self._inner.finish()

    @on_plan_device
    def check(self):
        """Non-blocking: raise if a completed asynchronous execute() of the inner plan reported invalid results."""
        if self._inner is not None:
            self._inner.check()

    def close(self):
        try:
            self.finish()
        finally:
            self._release_scratch()
            if self._inner is not None:
                self._inner.close()

    def release_captured(self):
        self.finish()
        self._capture_keepalive = []
        self._captured = False
        if self._inner is not None:
            self._inner.release_captured()

    # introspection (tests, tools/dct_bench.py)
    @property
    def inner_plan(self):
        return self._inner
