"""The power of the per-instance accuracy contract (helpers.accuracy_bound, tests/test_instances_gpu.py), shown on CPU with a model.

The model is a radix-2 autosort (Stockham) FFT in numpy in the working precision: twiddles correctly rounded from extended precision,
every complex product as separate rounded real multiplies and adds (no fused multiply-add).  The correct model meets the bound with at
least 2x headroom from 2 to 2^20 points in both precisions; two subtly wrong models fail it, although both meet the reference's
thresholds (L1-relative < 1.1e-6 / 1e-11, max|err| <= 1e-5 / 1e-10 * max|ref|) that the protocol tests apply.  A later loosening of the
bound's formula fails here."""
import numpy
import pytest

from helpers import accuracy_bound, item_error, reference_fft

LEGACY = {numpy.complex64: (1.1e-6, 1e-5), numpy.complex128: (1e-11, 1e-10)}


def _twiddles(h, fdt):
    """w(2h)^k, k < h, correctly rounded to `fdt` from extended precision"""
    ang = -numpy.pi * numpy.arange(h, dtype=numpy.longdouble) / numpy.longdouble(h)
    return numpy.cos(ang).astype(fdt), numpy.sin(ang).astype(fdt)


def stockham(x, cdt, twiddle_scale=None, shift_last=None):
    """radix-2 autosort FFT of x in the precision of `cdt`.  Mutants: twiddle_scale multiplies every twiddle (a table wrong in the
    12th digit); shift_last = (k0, count) takes w^(k+1) for w^k on `count` columns k0 .. of the last pass (an index off by one)."""
    fdt = numpy.float64 if cdt == numpy.complex128 else numpy.float32
    n = x.size
    re = numpy.ascontiguousarray(x.real, fdt).reshape(n, 1)
    im = numpy.ascontiguousarray(x.imag, fdt).reshape(n, 1)
    h = 1
    while h < n:
        wr, wi = _twiddles(h, fdt)
        if twiddle_scale is not None:
            wr, wi = wr * fdt(twiddle_scale), wi * fdt(twiddle_scale)
        if shift_last is not None and 2 * h == n:
            k0, cnt = shift_last
            ang = -numpy.pi * (numpy.arange(k0, k0 + cnt, dtype=numpy.longdouble) + 1) / numpy.longdouble(h)
            wr[k0:k0 + cnt], wi[k0:k0 + cnt] = numpy.cos(ang).astype(fdt), numpy.sin(ang).astype(fdt)
        m = re.shape[0] // 2
        er, ei, orr, oi = re[:m], im[:m], re[m:], im[m:]
        tr = orr * wr - oi * wi               # (fdt arrays: every operation rounds on its own)
        ti = orr * wi + oi * wr
        re = numpy.concatenate([er + tr, er - tr], axis=1)
        im = numpy.concatenate([ei + ti, ei - ti], axis=1)
        h *= 2
    out = numpy.empty(n, cdt)
    out.real, out.imag = re.reshape(-1), im.reshape(-1)
    return out


def _data(n, cdt, seed):
    rng = numpy.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(cdt)


def _errors(n, cdt, seed=7, **mutant):
    x = _data(n, cdt, seed)
    got = stockham(x, cdt, **mutant)
    ref = reference_fft(x, (n,), cdt)
    l1, mx_rms = item_error(got, ref)
    mag = numpy.abs(ref)
    mx_legacy = float(numpy.abs(got.astype(ref.dtype) - ref).max() / mag.max())
    return l1, mx_rms, mx_legacy


def test_stockham_model_is_an_fft():
    x = _data(64, numpy.complex128, 1)
    assert numpy.allclose(stockham(x, numpy.complex128), numpy.fft.fft(x), rtol=0, atol=1e-13)


@pytest.mark.parametrize("cdt", [numpy.complex64, numpy.complex128], ids=["fp32", "fp64"])
def test_correct_model_meets_the_bound_with_headroom(cdt):
    for log in range(1, 21):
        n = 1 << log
        l1_bound, max_bound = accuracy_bound(cdt, n)
        l1, mx, _ = _errors(n, cdt, seed=log)
        assert l1 <= 0.5 * l1_bound and mx <= 0.5 * max_bound, (n, l1 / l1_bound, mx / max_bound)


def test_fp64_twiddles_wrong_in_the_12th_digit_fail_the_bound_only():
    n = 1 << 19
    l1_bound, max_bound = accuracy_bound(numpy.complex128, n)
    l1, mx, mx_legacy = _errors(n, numpy.complex128, twiddle_scale=1 + 1e-12)
    eps, mxn = LEGACY[numpy.complex128]
    assert l1 < eps and mx_legacy <= mxn, "the reference's thresholds were expected to let this mutant through"
    assert l1 > l1_bound and mx > max_bound, (l1 / l1_bound, mx / max_bound)


def test_fp32_index_error_on_64_columns_fails_the_bound_only():
    n = 1 << 20
    l1_bound, max_bound = accuracy_bound(numpy.complex64, n)
    l1, mx, mx_legacy = _errors(n, numpy.complex64, shift_last=((n // 2) // 3, 64))
    eps, mxn = LEGACY[numpy.complex64]
    assert l1 < eps and mx_legacy <= mxn, "the reference's thresholds were expected to let this mutant through"
    assert l1 <= l1_bound                 # (the L1 average does not see it ...)
    assert mx > max_bound, mx / max_bound  # (... the max-norm against rms(ref) does)
