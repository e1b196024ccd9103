"""numpy model of the cosine and sine transforms (pyfft_amd/r2r.py, csrc/fft_r2r.hip): Makhoul's algorithm as the kernels run it, the
host tables, and the extended-precision references the GPU tests hold the r2r plans to.

Conventions (scipy.fft, type 2 forward, type 3 inverse, per axis of n points):
    DCT-II   y[k] = 2 sum_j x[j] cos(pi k (2j + 1) / 2n)
    DST-II   y[k] = 2 sum_j x[j] sin(pi (k + 1) (2j + 1) / 2n)  = DCT-II((-1)^j x)[n - 1 - k]
    ortho    y[k] *= sqrt(1 / 4n) at the DCT index 0 (DST: k = n - 1), sqrt(1 / 2n) elsewhere
and the exact inverses (scipy's idctn / idstn with type=2)."""
import numpy


# ---------------------------------------------------------------------------------------------------------------------------------
# the algorithm
def permutation(n):
    """perm[i] = the position of x[i] in v = [x0, x2, x4, ..., x5, x3, x1]"""
    i = numpy.arange(n)
    return numpy.where(i % 2 == 0, i // 2, n - 1 - i // 2)


def permute(x, kind):
    """v = the per-axis permutation of x over every axis (DST: x times (-1)^(sum of its indices) first)."""
    x = numpy.asarray(x)
    if kind == "dst":
        x = x * _signs(x.shape)
    v = numpy.empty_like(x)
    idx = numpy.ix_(*[permutation(n) for n in x.shape])
    v[idx] = x
    return v


def unpermute(v, kind):
    v = numpy.asarray(v)
    x = v[numpy.ix_(*[permutation(n) for n in v.shape])]
    if kind == "dst":
        x = x * _signs(v.shape)
    return x


def _signs(shape):
    s = numpy.ones(shape)
    for a, n in enumerate(shape):
        sh = [1] * len(shape)
        sh[a] = n
        s = s * ((-1.0) ** numpy.arange(n)).reshape(sh)
    return s


def weights(n, ortho):
    """c[k]: the ortho weight of the DCT index k (1 without ortho)"""
    if not ortho:
        return numpy.ones(n)
    c = numpy.full(n, numpy.sqrt(1.0 / (2 * n)))
    c[0] = numpy.sqrt(1.0 / (4 * n))
    return c


def fwd_table(n, ortho, g=1.0):
    """t[k] = g c[k] w(4n)^k: the forward post step's per-axis table (g, the plan's global factor, on the last axis only)"""
    k = numpy.arange(n)
    return g * weights(n, ortho) * numpy.exp(-2j * numpy.pi * k / (4 * n))


def inv_table(n, ortho, g=1.0):
    """u[k] = g w(4n)^-k / (2 c[k]): the inverse pre step's per-axis table"""
    k = numpy.arange(n)
    return g * numpy.exp(2j * numpy.pi * k / (4 * n)) / (2.0 * weights(n, ortho))


def _reflect(a, axis):
    """a[(n - k) mod n] along axis"""
    return numpy.roll(numpy.flip(a, axis=axis), 1, axis=axis)


def _along(t, axis, ndim):
    sh = [1] * ndim
    sh[axis] = t.size
    return t.reshape(sh)


def full_spectrum(Z, n_last):
    """V = fftn(v) over the whole (..., n_last) real shape from Z = fftn of the packed v (2 V from the separation without its 1/2: the
    forward table carries the 1/2)"""
    L = n_last // 2
    lead = range(Z.ndim - 1)
    Zx = numpy.concatenate([Z, Z[..., :1]], axis=-1)                  # kx = 0 .. L
    Zm = Zx
    for a in lead:
        Zm = _reflect(Zm, a)
    Zm = numpy.conj(Zm[..., ::-1])                                     # conj Z[-kp, L - kx]
    w = numpy.exp(-2j * numpy.pi * numpy.arange(L + 1) / n_last)
    half = (Zx + Zm) - 1j * w * (Zx - Zm)                              # 2 V[kp, kx], kx = 0 .. L
    rest = numpy.conj(half)
    for a in lead:
        rest = _reflect(rest, a)
    rest = rest[..., 1:L][..., ::-1]                                   # 2 V[kp, n - kx] = conj 2 V[-kp, kx]
    return numpy.concatenate([half, rest], axis=-1)


def post_forward(Z, shape, ortho, g):
    """The forward post step: Z -> Y, per axis Y[k] = t[k] V[k] + conj(t[k]) V[-k] (V from full_spectrum, which is 2 V: g holds the
    1/2)"""
    V = full_spectrum(Z, shape[-1])
    d = len(shape)
    for a, n in enumerate(shape):
        t = _along(fwd_table(n, ortho, g if a == d - 1 else 1.0), a, d)
        V = t * V + numpy.conj(t) * _reflect(V, a)
    return V.real


def pre_inverse(Y, ortho, g):
    """The inverse pre step: Y -> Z', per axis V[k] = u[k] (Y[k] - i Y[n - k]) with Y[n] = 0, then the real packing
    Z'[kx] = (V[kx] + V[L + kx]) + i w(n)^-kx (V[kx] - V[L + kx])"""
    V = numpy.asarray(Y, numpy.complex128) if Y.dtype != numpy.longdouble else Y.astype(numpy.clongdouble)
    d = V.ndim
    for a in range(d):
        n = V.shape[a]
        u = _along(inv_table(n, ortho, g if a == d - 1 else 1.0), a, d)
        partner = _reflect(V, a)
        zero = [slice(None)] * d
        zero[a] = 0
        partner[tuple(zero)] = 0                                       # Y[n] = 0
        V = u * (V - 1j * partner)
    n = V.shape[-1]
    L = n // 2
    w = numpy.exp(2j * numpy.pi * numpy.arange(L) / n)
    a, b = V[..., :L], V[..., L:]
    return (a + b) + 1j * w * (a - b)


def global_factor(shape, inverse, ortho, normalize, scale):
    """(kept axes, g): the axes of length > 1 and the factor the last kept axis's table carries.  A dropped unit axis multiplies by 2
    forward and by 1 / 2 inverse (1 with ortho; 2 x 1 / 2 = 1 for the unnormalised type III)."""
    kept = tuple(n for n in shape if n > 1)
    units = len(shape) - len(kept)
    if not inverse:
        return kept, 0.5 * scale * (1.0 if ortho else 2.0 ** units)
    g = 1.0 / float(numpy.prod(kept)) * (1.0 if ortho else 0.5 ** units)
    if not normalize:
        g *= float(numpy.prod([2 * n for n in shape]))
    return kept, g / scale


def model(x, kind, inverse=False, ortho=False, normalize=True, scale=1.0):
    """The whole composed form in float64: pre step, the packed complex transform, post step (unit axes dropped)."""
    shape = numpy.shape(x)
    kept, g = global_factor(shape, inverse, ortho, normalize, scale)
    a = numpy.asarray(x, numpy.float64).reshape(kept if kept else (1,))
    if not kept:
        return (a * (g if inverse else 2.0 * g)).reshape(shape)      # every axis a unit axis: a multiple of x
    if not inverse:
        v = permute(a, kind)
        Z = numpy.fft.fftn(v[..., 0::2] + 1j * v[..., 1::2])
        Y = post_forward(Z, kept, ortho, g)
        if kind == "dst":
            Y = Y[tuple(slice(None, None, -1) for _ in kept)]
        return Y.reshape(shape)
    if kind == "dst":
        a = a[tuple(slice(None, None, -1) for _ in kept)]
    Zp = pre_inverse(a, ortho, g)
    z = numpy.fft.ifftn(Zp) * Zp.size                                  # the inner plan's unnormalised inverse
    v = numpy.empty(kept, numpy.float64)
    v[..., 0::2] = z.real
    v[..., 1::2] = z.imag
    return unpermute(v, kind).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# references
def _move(a, axis):
    return numpy.moveaxis(a, axis, -1)


def _dct2_axis(x, axis, ct):
    """DCT-II along axis through the mirror extension to 2n: y[k] = Re(w(4n)^k FFT_2n([x, x reversed])[k])"""
    a = _move(x, axis).astype(ct)
    n = a.shape[-1]
    ext = numpy.concatenate([a, a[..., ::-1]], axis=-1)
    X = numpy.fft.fft(ext, axis=-1)[..., :n]
    k = numpy.arange(n, dtype=numpy.longdouble)
    w = numpy.exp(-1j * numpy.pi * k / (2 * n)).astype(ct)
    return numpy.moveaxis((w * X).real, -1, axis)


def _dct3_axis(y, axis, ct):
    """unnormalised DCT-III along axis: x[j] = y[0] + 2 sum_k>0 y[k] cos(pi k (2j + 1) / 2n) = Re(IFFT_2n(y' w(4n)^-k))[j] * 2n,
    y' = (y[0], 2 y[1], ...), zero-padded to 2n"""
    a = _move(y, axis).astype(ct)
    n = a.shape[-1]
    k = numpy.arange(n, dtype=numpy.longdouble)
    w = numpy.exp(1j * numpy.pi * k / (2 * n)).astype(ct)
    yp = a * w
    yp[..., 1:] *= 2
    pad = numpy.concatenate([yp, numpy.zeros_like(yp)], axis=-1)
    x = numpy.fft.ifft(pad, axis=-1)[..., :n] * (2 * n)
    return numpy.moveaxis(x.real, -1, axis)


def reference(x, kind, inverse=False, ortho=False, normalize=True, scale=1.0, double=True):
    """scipy.fft.dctn / dstn (type=2) * scale, or idctn / idstn (type=2) / scale (normalize=True; dctn / dstn type=3 / scale with
    normalize=False), over every axis, in extended precision (clongdouble for fp64, complex128 for fp32)."""
    ct = numpy.clongdouble if double else numpy.complex128
    rt = numpy.longdouble if double else numpy.float64
    a = numpy.asarray(x).astype(rt)
    shape = a.shape
    for ax, n in enumerate(shape):
        c = _along(weights(n, ortho).astype(rt), ax, a.ndim)
        if not inverse:
            if kind == "dst":
                a = a * _along(((-1.0) ** numpy.arange(n)).astype(rt), ax, a.ndim)
            a = _dct2_axis(a, ax, ct) * c
            if kind == "dst":
                a = numpy.flip(a, axis=ax)
        else:
            if kind == "dst":
                a = numpy.flip(a, axis=ax)
            a = _dct3_axis(a / c, ax, ct)
            if normalize:
                a = a / (2 * n)
            if kind == "dst":
                a = a * _along(((-1.0) ** numpy.arange(n)).astype(rt), ax, a.ndim)
    return a * scale if not inverse else a / scale


def matrix(n, kind, inverse=False, ortho=False, normalize=True):
    """the direct O(n^2) matrix of one axis"""
    j = numpy.arange(n)[None, :]
    k = numpy.arange(n)[:, None]
    if kind == "dct":
        M = 2 * numpy.cos(numpy.pi * k * (2 * j + 1) / (2 * n))
    else:
        M = 2 * numpy.sin(numpy.pi * (k + 1) * (2 * j + 1) / (2 * n))
    c = weights(n, ortho)
    if kind == "dst":
        c = c[::-1]
    M = c[:, None] * M
    if not inverse:
        return M
    Mi = numpy.linalg.inv(M)
    return Mi if normalize else Mi * (2 * n)


def direct(x, kind, inverse=False, ortho=False, normalize=True, scale=1.0):
    """the N-D transform by the per-axis matrices"""
    a = numpy.asarray(x, numpy.float64)
    for ax, n in enumerate(a.shape):
        M = matrix(n, kind, inverse, ortho, normalize)
        a = numpy.moveaxis(numpy.tensordot(M, numpy.moveaxis(a, ax, 0), axes=(1, 0)), 0, ax)
    return a * scale if not inverse else a / scale
