"""The power of the per-instance accuracy contract (helpers.accuracy_bound, tests/test_instances_gpu.py), shown on CPU with a model.

The model is a radix-2 autosort (Stockham) FFT in numpy in the working precision: twiddles correctly rounded from extended precision,
every complex product as separate rounded real multiplies and adds (no fused multiply-add).  The correct model meets the bound with at
least 2x headroom from 2 to 2^20 points in both precisions; two subtly wrong models fail it, although both meet the reference's
thresholds (L1-relative < 1.1e-6 / 1e-11, max|err| <= 1e-5 / 1e-10 * max|ref|) that the protocol tests apply.  A later loosening of the
bound's formula fails here.  The second half does the same for the lengths of the opt-in extensions (tests/test_extension_instances_gpu.py)
with a mixed-radix Stockham model and a Bluestein model, which set the L of those forms (helpers.any_size_levels)."""
import ctypes
import os
import re

import numpy
import pytest

from helpers import accuracy_bound, any_size_levels, bound_levels, item_error, reference_fft

PI_LD = numpy.longdouble("3.14159265358979323846264338327950288")       # (numpy.pi is the float64 pi)
LEGACY = {numpy.complex64: (1.1e-6, 1e-5), numpy.complex128: (1e-11, 1e-10)}


def _twiddles(h, fdt):
    """w(2h)^k, k < h, correctly rounded to `fdt` from extended precision"""
    ang = -PI_LD * numpy.arange(h, dtype=numpy.longdouble) / numpy.longdouble(h)
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
            ang = -PI_LD * (numpy.arange(k0, k0 + cnt, dtype=numpy.longdouble) + 1) / numpy.longdouble(h)
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


# ---- lengths that are not powers of two: the mixed-radix and Bluestein forms of pyfft_amd/generic.py -------------------------------
# A mixed-radix Stockham model (the stage algebra of csrc/fft_mixed.hip, the radix lists of factor_search through mifft_mixed_radices,
# dft3 / dft5 / dft7 with the literal constants of csrc/fft_mixed.hpp, the composites 6 / 9 / 10 / 12 / 14 / 15 as dft_comp builds
# them) and a Bluestein model on top of it (the chirp, padding and bhat / m scaling of generic.py).  Tables either correctly rounded from
# extended precision ("exact") or exactly as generic.py builds them ("library").
_HPP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyfft_amd", "csrc", "fft_mixed.hpp")
_consts = {}


def dft_constants(name):
    """the (T) literals of dftR in csrc/fft_mixed.hpp, in the order written (dft3: c, s; dft5: c1, c2, s1, s2; dft7: c1 c2 c3 s1 s2 s3)"""
    if not _consts:
        src = open(_HPP).read()
        for fn in ("dft3", "dft5", "dft7"):
            body = re.search(r"void %s\(cplx<T>\* v\) \{(.*?)\n\}" % fn, src, re.S).group(1)
            _consts[fn] = tuple(float(v) for v in re.findall(r"\(T\)(-?[0-9.]+)", body))
    return _consts[name]


def radices(n):
    from pyfft_amd import _native as N
    r = (ctypes.c_int32 * N.MIFFT_MIXED_MAX_STAGES)()
    k = N.lib.mifft_mixed_radices(N.F32, int(n), r)
    assert k > 0, (n, k)
    return list(r[:k])


def _fdt(cdt):
    return numpy.float64 if numpy.dtype(cdt) == numpy.complex128 else numpy.float32


def _root(num, den, cdt):
    """exp(-2 pi i num / den) correctly rounded to double (unit_root of fft_mixed.hpp), then to the working precision"""
    ang = -2 * PI_LD * numpy.longdouble(num % den) / numpy.longdouble(den)
    return numpy.complex128(complex(float(numpy.cos(ang)), float(numpy.sin(ang)))).astype(cdt)


def _mi(a):
    return -1j * a            # (exact: a swap and a sign)


def _dft(v, cdt, consts):
    R = len(v)
    f = _fdt(cdt)
    if R == 1:
        return v
    if R == 3:
        c, s = (f(x) for x in consts["dft3"])
        t, d = v[1] + v[2], v[1] - v[2]
        m = v[0] + c * t
        return [v[0] + t, m + _mi(s * d), m - _mi(s * d)]
    if R == 5:
        c1, c2, s1, s2 = (f(x) for x in consts["dft5"])
        a1, b1, a2, b2 = v[1] + v[4], v[1] - v[4], v[2] + v[3], v[2] - v[3]
        m1, m2 = v[0] + c1 * a1 + c2 * a2, v[0] + c2 * a1 + c1 * a2
        n1, n2 = s1 * b1 + s2 * b2, s2 * b1 - s1 * b2
        return [v[0] + a1 + a2, m1 + _mi(n1), m2 + _mi(n2), m2 - _mi(n2), m1 - _mi(n1)]
    if R == 7:
        c1, c2, c3, s1, s2, s3 = (f(x) for x in consts["dft7"])
        a1, b1, a2, b2, a3, b3 = v[1] + v[6], v[1] - v[6], v[2] + v[5], v[2] - v[5], v[3] + v[4], v[3] - v[4]

        def re_(x1, x2, x3):
            return v[0] + x1 * a1 + x2 * a2 + x3 * a3

        def im_(y1, y2, y3):
            return y1 * b1 + y2 * b2 + y3 * b3
        m1, m2, m3 = re_(c1, c2, c3), re_(c2, c3, c1), re_(c3, c1, c2)
        n1, n2, n3 = im_(s1, s2, s3), im_(s2, -s3, -s1), im_(s3, -s1, s2)
        return [v[0] + a1 + a2 + a3, m1 + _mi(n1), m2 + _mi(n2), m3 + _mi(n3), m3 - _mi(n3), m2 - _mi(n2), m1 - _mi(n1)]
    comp = {6: (2, 3), 9: (3, 3), 10: (2, 5), 12: (4, 3), 14: (2, 7), 15: (3, 5)}
    if R in comp:                                   # dft_comp<A, B>
        A, B = comp[R]
        y = [None] * R
        for i1 in range(A):
            u = _dft([v[i1 + A * i2] for i2 in range(B)], cdt, consts)
            for k2 in range(B):
                y[i1 * B + k2] = u[k2] if (i1 == 0 or k2 == 0) else u[k2] * _root(i1 * k2, R, cdt)
        out = [None] * R
        for k2 in range(B):
            u = _dft([y[i1 * B + k2] for i1 in range(A)], cdt, consts)
            for k1 in range(A):
                out[B * k1 + k2] = u[k1]
        return out
    assert R & (R - 1) == 0, R                      # power-of-two radices: radix-2 decimation in time, correctly rounded constants
    e, o = _dft(v[0::2], cdt, consts), _dft(v[1::2], cdt, consts)
    h = R // 2
    t = [o[k] if k == 0 else (_mi(o[k]) if 4 * k == R else o[k] * _root(k, R, cdt)) for k in range(h)]
    return [e[k] + t[k] for k in range(h)] + [e[k] - t[k] for k in range(h)]


def exact_roots(count, step, period):
    k = (numpy.arange(count, dtype=numpy.int64) * step) % period
    ang = -2 * PI_LD * k.astype(numpy.longdouble) / numpy.longdouble(period)
    return numpy.cos(ang).astype(numpy.float64) + 1j * numpy.sin(ang).astype(numpy.float64)


def library_roots(count, step, period):
    from pyfft_amd.generic import _unit_roots
    return _unit_roots(count, step, period)


def mixed_stockham(x, cdt, tables="exact", consts=None, shift_last=None):
    """rows x (items, n) through the stage loop of fft_mixed_kernel in the precision of `cdt`.  Mutants: consts overrides the
    literals of dft3 / dft5 / dft7; shift_last = (jb0, count) takes table entry k * step + 1 for k * step on butterflies jb0 .. of the
    last stage (an index off by one)."""
    cdt = numpy.dtype(cdt)
    x = numpy.atleast_2d(numpy.asarray(x)).astype(cdt)
    n = x.shape[1]
    c = {k: dft_constants(k) for k in ("dft3", "dft5", "dft7")}
    c.update(consts or {})
    tw = (exact_roots if tables == "exact" else library_roots)(n, 1, n).astype(cdt)
    rad = radices(n)
    Ns = 1
    for s, R in enumerate(rad):
        LR = n // R
        jb = numpy.arange(LR)
        jm = jb % Ns
        v = [x[:, k * LR:(k + 1) * LR] for k in range(R)]
        if Ns > 1:
            step = jm * (LR // Ns)
            for k in range(1, R):
                idx = k * step
                if shift_last is not None and s == len(rad) - 1:
                    j0, cnt = shift_last
                    idx = idx.copy()
                    idx[j0:j0 + cnt] += 1
                v[k] = v[k] * tw[idx % n]
        v = _dft(v, cdt, c)
        q0 = (jb - jm) * R + jm
        y = numpy.empty_like(x)
        for k in range(R):
            y[:, q0 + k * Ns] = v[k]
        x = y
        Ns *= R
    return x


def _pow2_fft(x, cdt):
    """the power-of-two row plans of the work-array path: a radix-2 autosort FFT with correctly rounded twiddles (the model above)"""
    return numpy.stack([stockham(r, cdt) for r in numpy.atleast_2d(x)])


def bluestein(x, cdt, form, tables="library", bhat_scale=None, float64_tables=False):
    """rows x (items, n) through Bluestein's algorithm in the precision of `cdt`: form "one" = the one-launch kernel (m from
    mifft_bluestein_padded, bhat / m folded into the table, the second transform conj -> forward -> conj), "work" = the work-array path
    (m = 2^ceil(log2(2 n - 1)), power-of-two row plans, bhat unscaled and the inverse plan normalised).  The chirp and bhat are
    generic.py's own tables; `tables` chooses the w(m) tables of the mixed-radix transforms; bhat_scale multiplies bhat (a mutant).
    float64_tables: the chirp by float64 cos / sin and bhat by a float64 transform, as generic.py built them before."""
    from pyfft_amd.generic import _bluestein_spectrum, _chirp
    cdt = numpy.dtype(cdt)
    x = numpy.atleast_2d(numpy.asarray(x)).astype(cdt)
    n = x.shape[1]
    m = blue_padded(cdt, n) if form == "one" else 1 << (2 * n - 2).bit_length()
    cc = _chirp(n).astype(cdt)
    bhat = _bluestein_spectrum(n, m)
    if float64_tables:
        j = numpy.arange(n, dtype=numpy.int64)
        ang = -numpy.pi * ((j * j) % (2 * n)).astype(numpy.float64) / float(n)
        c64 = numpy.cos(ang) + 1j * numpy.sin(ang)
        b = numpy.zeros(m, numpy.complex128)
        b[:n] = numpy.conj(c64)
        b[m - n + 1:] = numpy.conj(c64[1:][::-1])
        cc = c64.astype(cdt)
        bhat = (mixed_stockham(b, numpy.complex128, "exact") if m & (m - 1) else _pow2_fft(b, numpy.complex128))[0]
    if bhat_scale is not None:
        bhat = bhat * bhat_scale
    a = numpy.zeros((x.shape[0], m), cdt)
    a[:, :n] = x * cc

    def fft_m(v):
        return mixed_stockham(v, cdt, tables) if m & (m - 1) else _pow2_fft(v, cdt)
    if form == "one":
        A = numpy.conj(fft_m(a) * (bhat / m).astype(cdt))
        y = numpy.conj(fft_m(A))
    else:
        A = _pow2_fft(a, cdt) * bhat.astype(cdt)
        y = numpy.conj(_pow2_fft(numpy.conj(A), cdt)) * _fdt(cdt)(1.0 / m)
    return y[:, :n] * cc


def blue_padded(cdt, n):
    from pyfft_amd import _native as N
    mb = ctypes.c_int32(0)
    prec = N.F64 if numpy.dtype(cdt) == numpy.complex128 else N.F32
    assert N.lib.mifft_bluestein_padded(prec, int(n), ctypes.byref(mb)) == 0, n
    return mb.value


def smooth_lengths(cdt):
    """every smooth length of one tile that is not a power of two (mifft_mixed_supported)"""
    from pyfft_amd import _native as N
    prec = N.F64 if numpy.dtype(cdt) == numpy.complex128 else N.F32
    return [n for n in range(3, 4097) if n & (n - 1) and N.lib.mifft_mixed_supported(prec, n) == 0]


def _model_errors(got, x, cdt):
    """(worst L1, worst max / rms, worst legacy max / max|ref|) over the rows"""
    out = [0.0, 0.0, 0.0]
    for g, xi in zip(got, x):
        ref = reference_fft(xi, (xi.size,), cdt)
        l1, mx = item_error(g, ref)
        leg = float(numpy.abs(g.astype(ref.dtype) - ref).max() / numpy.abs(ref).max())
        out = [max(out[0], l1), max(out[1], mx), max(out[2], leg)]
    return out


def _rows(n, cdt, seed, items=2):
    return numpy.stack([_data(n, cdt, seed * 10 + i) for i in range(items)])


def test_radix_model_constants_are_the_kernels():
    assert dft_constants("dft3") == (-0.5, 0.86602540378443864676)
    assert len(dft_constants("dft5")) == 4 and len(dft_constants("dft7")) == 6
    for R in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16):       # every butterfly of the model is a DFT
        v = _data(R, numpy.complex128, R)
        got = numpy.array(_dft(list(v.reshape(R, 1)), numpy.complex128, {k: dft_constants(k) for k in ("dft3", "dft5", "dft7")})).reshape(-1)
        assert numpy.allclose(got, numpy.fft.fft(v), rtol=0, atol=1e-13), R


@pytest.mark.parametrize("n", [6, 60, 1000, 2187, 3087, 4000])
def test_mixed_and_bluestein_models_are_ffts(n):
    x = _rows(n, numpy.complex128, 1, 1)
    assert numpy.allclose(mixed_stockham(x, numpy.complex128)[0], numpy.fft.fft(x[0]), rtol=0, atol=1e-9)
    assert numpy.array_equal(exact_roots(n, 1, n), library_roots(n, 1, n))
    for nb in (17, 1009):
        xb = _rows(nb, numpy.complex128, 2, 1)
        for form in ("one", "work"):
            assert numpy.allclose(bluestein(xb, numpy.complex128, form)[0], numpy.fft.fft(xb[0]), rtol=0, atol=1e-9), (nb, form)


def test_bound_for_powers_of_two_is_unchanged():
    for cdt in (numpy.complex64, numpy.complex128):
        u = 2.0 ** -53 if cdt == numpy.complex128 else 2.0 ** -24
        for log in range(1, 27):
            c = u * (log + 2)
            want = (c if cdt == numpy.complex128 else min(c, 1.1e-6), 4 * c)
            assert accuracy_bound(cdt, 1 << log) == want
            assert accuracy_bound(cdt, 1 << log, bound_levels(1 << log)) == want
            assert any_size_levels((1 << log,), cdt) == log


@pytest.mark.parametrize("tables", ["exact", "library"])
@pytest.mark.parametrize("cdt", [numpy.complex64, numpy.complex128], ids=["fp32", "fp64"])
def test_mixed_radix_model_meets_the_bound_with_headroom(cdt, tables):
    """every smooth length of one tile that is no power of two (so every radix list the row kernel runs), with the tables correctly
    rounded and exactly as generic.py builds them"""
    lengths = smooth_lengths(cdt)
    assert len(lengths) == (235 if cdt == numpy.complex64 else 178)
    for n in lengths:
        x = _rows(n, cdt, n)
        l1, mx, _ = _model_errors(mixed_stockham(x, cdt, tables), x, cdt)
        l1_bound, max_bound = accuracy_bound(cdt, n, bound_levels(n))
        assert l1 <= 0.5 * l1_bound and mx <= 0.5 * max_bound, (n, radices(n), l1 / l1_bound, mx / max_bound)


BLUE_N = [11, 13, 17, 19, 23, 29, 31, 61, 97, 127, 251, 509, 1009, 1021, 1531, 2039, 2053, 2503, 3001, 4099, 4999, 5000]   # (5000: split planes)


@pytest.mark.parametrize("tables", ["exact", "library"])
@pytest.mark.parametrize("cdt", [numpy.complex64, numpy.complex128], ids=["fp32", "fp64"])
def test_bluestein_model_meets_the_bound_with_headroom(cdt, tables):
    """both forms (one launch where mifft_bluestein_padded takes n; the work array for every n), L = log2 of the padded length"""
    from pyfft_amd import _native as N
    prec = N.F64 if cdt == numpy.complex128 else N.F32
    for n in BLUE_N:
        x = _rows(n, cdt, n)
        mb = ctypes.c_int32(0)
        forms = ["work"] + (["one"] if N.lib.mifft_bluestein_padded(prec, n, ctypes.byref(mb)) == 0 else [])
        for form in forms:
            m = mb.value if form == "one" else 1 << (2 * n - 2).bit_length()
            l1, mx, _ = _model_errors(bluestein(x, cdt, form, tables), x, cdt)
            l1_bound, max_bound = accuracy_bound(cdt, n, bound_levels(m))
            assert l1 <= 0.5 * l1_bound and mx <= 0.5 * max_bound, (n, form, m, l1 / l1_bound, mx / max_bound)


def test_fp64_radix5_constant_wrong_in_the_12th_digit_fails_the_bound_only():
    cdt = numpy.complex128
    c1, c2, s1, s2 = dft_constants("dft5")
    for n, seed in ((1000, 3), (3125, 4)):
        x = _rows(n, cdt, seed)
        l1, mx, leg = _model_errors(mixed_stockham(x, cdt, consts={"dft5": (c1 * (1 + 1e-12), c2, s1, s2)}), x, cdt)
        l1_bound, max_bound = accuracy_bound(cdt, n, bound_levels(n))
        eps, mxn = LEGACY[numpy.complex128]
        assert l1 < eps and leg <= mxn, "the reference's thresholds were expected to let this mutant through"
        assert l1 > l1_bound and mx > max_bound, (n, l1 / l1_bound, mx / max_bound)


def test_fp64_radix7_constant_wrong_in_the_12th_digit_fails_the_bound_only():
    cdt = numpy.complex128
    cs = list(dft_constants("dft7"))
    cs[4] *= 1 + 1e-12                    # s2
    n = 2401
    x = _rows(n, cdt, 5)
    l1, mx, leg = _model_errors(mixed_stockham(x, cdt, consts={"dft7": tuple(cs)}), x, cdt)
    l1_bound, max_bound = accuracy_bound(cdt, n, bound_levels(n))
    eps, mxn = LEGACY[numpy.complex128]
    assert l1 < eps and leg <= mxn, "the reference's thresholds were expected to let this mutant through"
    assert l1 > l1_bound and mx > max_bound, (l1 / l1_bound, mx / max_bound)


def test_fp32_index_error_on_a_few_radix5_columns_fails_the_bound_only():
    """5^8 points: eight radix-5 stages; table entry k * step + 1 on 8 butterflies of the last stage (32 outputs off by 2 pi / n)"""
    cdt = numpy.complex64
    n = 5 ** 8
    assert radices(n)[-1] == 5
    x = _rows(n, cdt, 6, 1)
    l1, mx, leg = _model_errors(mixed_stockham(x, cdt, shift_last=(n // 15, 8)), x, cdt)
    l1_bound, max_bound = accuracy_bound(cdt, n, bound_levels(n))
    eps, mxn = LEGACY[numpy.complex64]
    assert l1 < eps and leg <= mxn, "the reference's thresholds were expected to let this mutant through"
    assert l1 <= l1_bound                 # (the L1 average does not see it ...)
    assert mx > max_bound, mx / max_bound  # (... the max-norm against rms(ref) does)
    l1c, mxc, _ = _model_errors(mixed_stockham(x, cdt), x, cdt)
    assert mxc <= 0.5 * max_bound, mxc / max_bound


def test_fp64_bhat_scaled_by_1_plus_1e_12_fails_the_bound_only():
    cdt = numpy.complex128
    for n, form in ((1009, "one"), (2053, "one"), (4099, "work")):
        x = _rows(n, cdt, 8)
        m = blue_padded(cdt, n) if form == "one" else 1 << (2 * n - 2).bit_length()
        l1, mx, leg = _model_errors(bluestein(x, cdt, form, bhat_scale=1 + 1e-12), x, cdt)
        l1_bound, max_bound = accuracy_bound(cdt, n, bound_levels(m))
        eps, mxn = LEGACY[numpy.complex128]
        assert l1 < eps and leg <= mxn, "the reference's thresholds were expected to let this mutant through"
        assert l1 > l1_bound and mx > max_bound, (n, form, l1 / l1_bound, mx / max_bound)


def test_fp64_bluestein_tables_are_rounded_once():
    """the chirp and bhat evaluated in float64 (generic.py before: float64 cos / sin, a float64 device transform of the chirp) put a few
    units of float64 rounding into every fp64 Bluestein result: the correct model then loses the bound's 2x headroom; rounded once from
    extended precision it keeps it"""
    cdt = numpy.complex128
    worst_old, worst_new = 0.0, 0.0
    for n in (11, 13, 23, 97):
        x = _rows(n, cdt, n)
        for form in ("one", "work"):
            m = blue_padded(cdt, n) if form == "one" else 1 << (2 * n - 2).bit_length()
            l1_bound, _ = accuracy_bound(cdt, n, bound_levels(m))
            worst_old = max(worst_old, _model_errors(bluestein(x, cdt, form, float64_tables=True), x, cdt)[0] / l1_bound)
            worst_new = max(worst_new, _model_errors(bluestein(x, cdt, form), x, cdt)[0] / l1_bound)
    assert worst_old > 0.5 and worst_new <= 0.5, (worst_old, worst_new)
