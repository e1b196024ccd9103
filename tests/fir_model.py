"""numpy model of the overlap-save FIR rows (csrc/fft_fir_row.hpp; docs/extensions.md "FIR filtering plans") and the cases the CPU and
GPU tests share.

The index algebra as the issue states it: block r of an item, local element p (0 <= p < n), is sample g = r * hop - overlap + p of the
item, read if 0 <= g < length, else 0; local element p >= overlap of the block's circular convolution is output sample
t = r * hop + p - overlap, stored iff t < length.  The kernel does not test every element against the item: it derives per block a
window of POINTS (complex numbers; real plans: packed pairs) [plo, phi) for the loads and [ov, phi) for the stores, plus the one pair
that straddles an odd real item's end.  windows() restates that derivation; load_map() / store_map() expand it to element indices, and
tests/test_fir_cpu.py holds them to the statement above."""
import numpy

F32, F64 = numpy.float32, numpy.float64
CDT = {numpy.dtype(F32): numpy.complex64, numpy.dtype(F64): numpy.complex128,
       numpy.dtype(numpy.complex64): numpy.complex64, numpy.dtype(numpy.complex128): numpy.complex128}

# (precision, real, n): every length with a convolution-row instance on the register-edged stages (L >= 64 complex or packed points)
INSTANCES = ([(F32, False, 1 << e) for e in range(6, 16)] + [(F64, False, 1 << e) for e in range(6, 14)] +
             [(F32, True, 1 << e) for e in range(7, 15)] + [(F64, True, 1 << e) for e in range(7, 14)])


def plan_dtype(prec, real):
    return numpy.dtype(prec) if real else numpy.dtype(CDT[numpy.dtype(prec)])


def case_id(c):
    prec, real, n = c[:3]
    return "%s-%s-%d" % (numpy.dtype(prec).name, "real" if real else "complex", n) + "".join("-%s" % v for v in c[3:])


def overlap_of(m, real):
    ov = m - 1
    return ov + (ov & 1) if real else ov


def instance_case(n, real):
    """(m, length, batch, pitch) of the per-instance GPU case: three blocks, the last one partial (real: an odd length); 9 rows, no
    multiple of any W > 1; a gap of 2 or 3 elements behind every item"""
    m = n // 4 + 1
    hop = n - overlap_of(m, real)
    length = 2 * hop + hop // 2 + 1
    return m, length, 3, length + (length & 1) + 2


FOCUS_N = 256
FOCUS_KINDS = ((F32, False), (F32, True), (F64, False))


def focus_cases():
    """(precision, real, n, m, length) on n = 256: m in {1, 2, 128}, length in {1, overlap - 1, hop, hop + 1}; overlap - 1 is left out
    where it is no length (below 1: m = 1, and m = 2 on complex plans, whose overlap is 1)"""
    out = []
    for prec, real in FOCUS_KINDS:
        for m in (1, 2, 128):
            ov = overlap_of(m, real)
            hop = FOCUS_N - ov
            for length in sorted(set(v for v in (1, ov - 1, hop, hop + 1) if v >= 1)):
                out.append((prec, real, FOCUS_N, m, length))
    return out


def blocks(n, overlap, length):
    hop = n - overlap
    return -(-length // hop)


def windows(n, overlap, length, r, real):
    """What fir_row_body derives for block r: (start, plo, phi, half) in points."""
    sc = 2 if real else 1
    L, ov = n // sc, overlap // sc
    start = r * (L - ov) - ov
    rest = length - sc * start
    lim = min(rest, sc * L)
    return start, (ov if r == 0 else 0), lim // sc, bool(real and (lim & 1))


def _expand(n, overlap, length, r, real, lo_of):
    sc = 2 if real else 1
    start, plo, phi, half = windows(n, overlap, length, r, real)
    lo = lo_of(plo, overlap // sc)
    local, item = [], []
    for p in range(lo, phi):
        for s in range(sc):
            local.append(sc * p + s)
            item.append(sc * (start + p) + s)
    if half:
        local.append(sc * phi)
        item.append(sc * (start + phi))
    return numpy.array(local, dtype=numpy.int64), numpy.array(item, dtype=numpy.int64)


def load_map(n, overlap, length, r, real):
    """(local element indices, item element indices) block r loads"""
    return _expand(n, overlap, length, r, real, lambda plo, ov: plo)


def store_map(n, overlap, length, r, real):
    """(local element indices, item element indices) block r stores"""
    return _expand(n, overlap, length, r, real, lambda plo, ov: ov)


def filter_spectrum(h, n, real, dtype):
    """fft of the taps zero-padded to n, rounded to the plan's precision"""
    cdt = CDT[numpy.dtype(dtype)]
    hp = numpy.zeros(n, dtype=plan_dtype(dtype, real))
    hp[:h.size] = h
    return (numpy.fft.rfft(hp) if real else numpy.fft.fft(hp)).astype(cdt)


def run(x, H, n, m, length, pitch, batch, real, dtype, scale=1.0, normalize=True, fill=0):
    """The plan's execute on a flat array x of (batch - 1) * pitch + length elements: every block gathered by load_map, the circular
    convolution with every intermediate rounded to the plan's precision, the valid part scattered by store_map.  H: one spectrum
    (shared) or `batch` of them.  Returns (y, writes): y starts as `fill`, writes counts the stores per element."""
    pdt, cdt = plan_dtype(dtype, real), CDT[numpy.dtype(dtype)]
    overlap = overlap_of(m, real)
    total = (batch - 1) * pitch + length
    y = numpy.full(total, fill, dtype=pdt)
    writes = numpy.zeros(total, dtype=numpy.int64)
    H = numpy.asarray(H).reshape(-1, n // 2 + 1 if real else n)
    factor = (numpy.float64 if cdt is numpy.complex128 else numpy.float32)(scale / (n if normalize else 1.0))
    for i in range(batch):
        Hi = H[i if H.shape[0] > 1 else 0]
        for r in range(blocks(n, overlap, length)):
            block = numpy.zeros(n, dtype=pdt)
            local, item = load_map(n, overlap, length, r, real)
            assert item.size == 0 or (item.min() >= 0 and item.max() < length)
            block[local] = x[i * pitch + item]
            if real:
                Y = (numpy.fft.rfft(block).astype(cdt) * Hi).astype(cdt)
                out = (numpy.fft.irfft(Y, n) * n).astype(pdt) * factor
            else:
                Y = (numpy.fft.fft(block).astype(cdt) * Hi).astype(cdt)
                out = (numpy.fft.ifft(Y) * n).astype(cdt) * factor
            local, item = store_map(n, overlap, length, r, real)
            assert item.size == 0 or (item.min() >= 0 and item.max() < length)
            y[i * pitch + item] = out[local]
            writes[i * pitch + item] += 1
    return y, writes


def signal(dtype, real, count, seed):
    r = numpy.random.default_rng(seed)
    if real:
        return r.standard_normal(count).astype(numpy.dtype(dtype))
    return (r.standard_normal(count) + 1j * r.standard_normal(count)).astype(CDT[numpy.dtype(dtype)])


def reference(x, h, length, dtype, scale=1.0):
    """numpy.convolve(x, h)[:length] * scale of one item: complex128 / float64 for fp32 plans, clongdouble / longdouble for fp64 plans"""
    double = numpy.dtype(dtype) in (numpy.dtype(F64), numpy.dtype(numpy.complex128))
    if double:
        assert numpy.finfo(numpy.longdouble).eps <= 2.0 ** -63, "this host has no extended precision"
    cplx = numpy.iscomplexobj(x) or numpy.iscomplexobj(h)
    ext = (numpy.clongdouble if cplx else numpy.longdouble) if double else (numpy.complex128 if cplx else numpy.float64)
    return numpy.convolve(numpy.asarray(x).astype(ext), numpy.asarray(h).astype(ext))[:length] * ext(scale)
