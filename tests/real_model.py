"""numpy model of the real-input transforms (pyfft_amd/real.py, csrc/fft_real.hip): the packing identity in float64 / extended
precision, and the extended-precision references the GPU tests hold the real plans to."""
import numpy


def _mirror(a, axes):
    """a[-k] over the given axes (index 0 stays, k -> n - k)."""
    for ax in axes:
        a = numpy.roll(numpy.flip(a, axis=ax), 1, axis=ax)
    return a


def separate(Z, nx):
    """Forward separation: Z = fftn of the packed array (shape (..., nx / 2)) -> half spectrum (..., nx / 2 + 1)."""
    L = nx // 2
    Zx = numpy.concatenate([Z, Z[..., :1]], axis=-1)                  # kx = 0 .. L, Z periodic in kx with period L
    Zm = numpy.conj(_mirror(Zx, range(Z.ndim - 1))[..., ::-1])       # conj Z[-k] over all axes: kp -> -kp, kx -> L - kx
    k = numpy.arange(L + 1)
    w = numpy.exp(-2j * numpy.pi * k / nx).astype(Z.dtype)
    return 0.5 * (Zx + Zm) - 0.5j * w * (Zx - Zm)


def hermitian_edges(X):
    """X with the kx = 0 and kx = nx / 2 planes replaced by their Hermitian parts over the leading axes."""
    X = numpy.array(X, copy=True)
    lead = range(X.ndim - 1)
    for e in (0, -1):
        p = X[..., e]
        X[..., e] = 0.5 * (p + numpy.conj(_mirror(p, lead)))
    return X


def pack(X, nx, hermitian=True):
    """Inverse packing: half spectrum -> Z' whose unnormalised ifftn (times 1/size for ifftn's own 1/n) is the packed real result."""
    L = nx // 2
    if hermitian:
        X = hermitian_edges(X)
    Xm = numpy.conj(_mirror(X, range(X.ndim - 1))[..., ::-1])        # conj X[-kp, L - kx], kx = 0 .. L
    k = numpy.arange(L)
    w = numpy.exp(2j * numpy.pi * k / nx).astype(X.dtype)
    a, b = X[..., :L], Xm[..., :L]
    return (a + b) + 1j * w * (a - b)


def rfftn_model(x):
    """rfftn through the packing identity (complex FFT of nx / 2 points + separation)."""
    x = numpy.asarray(x, numpy.float64)
    z = x[..., 0::2] + 1j * x[..., 1::2]
    return separate(numpy.fft.fftn(z), x.shape[-1])


def irfftn_model(X, shape, hermitian=True):
    """irfftn (numpy's normalisation) through the packing identity."""
    nx = shape[-1]
    Zp = pack(numpy.asarray(X, numpy.complex128), nx, hermitian)
    z = numpy.fft.ifftn(Zp) / 2.0                                     # ifftn divides by size / 2; the real transform by size
    out = numpy.empty(tuple(shape), numpy.float64)
    out[..., 0::2] = z.real
    out[..., 1::2] = z.imag
    return out


def rfftn_exact(x, double):
    """The half spectrum of a real item, to well below the working precision (clongdouble for fp64, complex128 for fp32)."""
    ct = numpy.clongdouble if double else numpy.complex128
    full = numpy.fft.fftn(numpy.asarray(x).astype(ct))
    return full[..., : x.shape[-1] // 2 + 1]


def irfftn_exact(X, shape, double):
    """numpy.fft.irfftn(X, s=shape) (edge planes through their Hermitian parts) in extended precision for fp64."""
    ct = numpy.clongdouble if double else numpy.complex128
    X = hermitian_edges(numpy.asarray(X).astype(ct))
    nx = shape[-1]
    L = nx // 2
    full = numpy.empty(tuple(shape[:-1]) + (nx,), ct)
    full[..., : L + 1] = X
    if L > 1:
        rest = numpy.conj(_mirror(X, range(X.ndim - 1)))               # conj X[-kp, kx]
        full[..., L + 1:] = rest[..., 1:L][..., ::-1]                 # kx = nx - j -> conj X[-kp, j]
    return numpy.fft.ifftn(full).real
