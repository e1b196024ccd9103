"""Test harness: counterpart of the reference's test/helpers.py for the HIP backend.

HipContext mirrors helpers.CudaContext (test/helpers.py:29-74): allocate / toGpu / fromGpu /
getPlan / timers / supportsDouble.  Data generation and the error metric come from the oracle
(oracle/pyfft_oracle.py), which only tests may import.
"""
import numpy

COMPLEX_DTYPES = [numpy.complex64, numpy.complex128]
DOUBLE_DTYPES = [numpy.float64, numpy.complex128]


class HipContext(object):

    def __init__(self):
        import pyfft_amd.hip as hip
        self.hip = hip
        if hip.device_count() < 1:
            raise RuntimeError("no HIP device")
        self.context = 0  # device index; what Plan(context=...) accepts

    def allocate(self, shape, dtype):
        return self.hip.DeviceArray(shape, dtype)

    def toGpu(self, data):
        return self.hip.to_gpu(data)

    def fromGpu(self, gpu_buf, target_shape, target_dtype):
        return gpu_buf.get().reshape(target_shape)

    def getMemoryPool(self):
        return CountingPool(self.hip)

    def getPlan(self, *args, **kwds):
        return self.hip.Plan(*args, **kwds)

    def startTimer(self):
        self._start = self.hip.Event().record()
        self._stop = self.hip.Event()

    def stopTimer(self):
        self._stop.record()
        self._stop.synchronize()
        return self._stop.time_since(self._start) / 1000.0

    def supportsDouble(self):
        return True

    def __str__(self):
        return "hip"


class CountingPool(object):
    """mempool stand-in (pycuda.tools.DeviceMemoryPool counterpart): allocate(nbytes)."""

    def __init__(self, hip):
        self.hip = hip
        self.calls = 0

    def allocate(self, nbytes):
        self.calls += 1
        return self.hip.DeviceAllocation(nbytes)


def getDimensions(shape):
    """(test/helpers.py:149-158)"""
    if isinstance(shape, int):
        return shape, 1, 1
    shape = tuple(shape) + (1, 1)
    return shape[0], shape[1], shape[2]


# ---- shared by the GPU test modules (moved here from the per-round files in round 6) ------------------------------------------------
def _noise(rng, count, dtype):
    """`count` N(0, 1) numbers: a seeded block of 2^22 + 17 draws, repeated (the period is no multiple of any transform size, so every
    transform of a batch sees different numbers; drawing 300 MiB afresh for every case took most of the suite's time)."""
    blk = rng.standard_normal(min(int(count), (1 << 22) + 17)).astype(dtype)
    return numpy.resize(blk, int(count))


def _test_data(shape, dtype, batch, seed):
    """Interleaved test data of `batch` transforms (the layout of oracle.get_test_data: the first axis times batch) from tiled noise."""
    rng = numpy.random.default_rng(seed)
    dtype = numpy.dtype(dtype)
    fdt = numpy.float32 if dtype == numpy.complex64 else numpy.float64
    full = [int(v) for v in (shape if isinstance(shape, tuple) else (shape,))]
    full[0] *= batch
    count = int(numpy.prod(full))
    out = numpy.empty(count, dtype)
    out.real = _noise(rng, count, fdt)
    out.imag = _noise(rng, count, fdt)
    return out.reshape(full)


def _execute(ctx, shape, dtype, batch, data, inplace=False, inverse=False, expect=None):
    plan = ctx.getPlan(shape, dtype=dtype)
    if expect is not None:
        assert plan.strategy(batch)[0] == expect, plan.strategy(batch)
    a = ctx.toGpu(data)
    if inplace:
        plan.execute(a, batch=batch, inverse=inverse)
        return a.get()
    b = ctx.allocate(data.shape, data.dtype)
    plan.execute(a, b, batch=batch, inverse=inverse)
    assert numpy.array_equal(a.get(), data), "an out-of-place execute touched its input"
    return b.get()


# ---- split-complex fp32 on the persistent 1-D kernel: sibling tiles per item ------------------------------------------------------
def _execute_split(ctx, shape, rdtype, batch, re, im, inplace=False, inverse=False, expect=None):
    plan = ctx.getPlan(shape, dtype=rdtype)
    if expect is not None:
        assert plan.strategy(batch)[0] == expect, plan.strategy(batch)
    a_re, a_im = ctx.toGpu(re), ctx.toGpu(im)
    if inplace:
        plan.execute(a_re, a_im, batch=batch, inverse=inverse)
        return a_re.get(), a_im.get()
    b_re, b_im = ctx.allocate(re.shape, re.dtype), ctx.allocate(im.shape, im.dtype)
    plan.execute(a_re, a_im, b_re, b_im, batch=batch, inverse=inverse)
    assert numpy.array_equal(a_re.get(), re) and numpy.array_equal(a_im.get(), im), "an out-of-place execute touched its input"
    return b_re.get(), b_im.get()


EPS_F, MAX_F = 1.1e-6, 1e-5


# ---- persistent executes under stream capture / hipGraph replay -----------------------------------------------------------------
def _tiled_noise(count, dtype, seed):
    rng = numpy.random.default_rng(seed)
    cdt = numpy.dtype(dtype)
    fdt = numpy.float32 if cdt == numpy.complex64 else numpy.float64
    out = numpy.empty(count, cdt)
    for part in ("real", "imag"):
        blk = rng.standard_normal(min(count, (1 << 22) + 17)).astype(fdt)
        setattr(out, part, numpy.resize(blk, count))
    return out


class FakeContext(object):
    """A context without a device: tables are "uploaded" nowhere.  What FFTPlan._select_strategy reads is `machine`."""
    _guard = False

    def __init__(self, machine):
        self.machine = machine
        self.compute_units = machine.compute_units

    def allocate_raw(self, nbytes):
        return 4096

    allocate = allocate_raw

    def upload(self, mem, host):
        pass

    @staticmethod
    def pointer_of(obj):
        return obj

    def capturing(self):
        return False


# ---- the per-instance accuracy contract (tests/test_instances_gpu.py; docs/parity.md) ------------------------------------------------
NOISE_PERIOD = (1 << 22) + 17          # the period of _noise: element i of a _test_data set is element i % NOISE_PERIOD of its first block
SAMPLE_ALL_POINTS = 1 << 22            # up to this many points per side every item is checked, beyond it the first, the middle and the last


def unit_roundoff(dtype):
    """u of the working precision of a plan of `dtype` (2^-24 for complex64 / float32 planes, 2^-53 for complex128 / float64)"""
    return 2.0 ** -53 if numpy.dtype(dtype) in (numpy.dtype(numpy.complex128), numpy.dtype(numpy.float64)) else 2.0 ** -24


def accuracy_bound(dtype, n_points):
    """(L1-relative, max|err| / rms(ref)) that ONE transform of `n_points` points (all axes together) must meet, per item:
    u (L + 2) and 4 u (L + 2) with L = log2(n_points); fp32 also keeps the reference's L1 threshold 1.1e-6 where it is the tighter.
    The constants come from a radix-2 model with correctly rounded twiddles (tests/test_accuracy_model.py, which also shows that the
    bound catches a twiddle table wrong in the 12th digit and a localised index error that the reference's thresholds let through)."""
    n_points = int(n_points)
    assert n_points >= 1 and n_points & (n_points - 1) == 0, n_points
    u = unit_roundoff(dtype)
    c = u * (n_points.bit_length() - 1 + 2)
    l1 = c if u < 2.0 ** -30 else min(c, EPS_F)
    return l1, 4.0 * c


def sampled_items(batch, n_points):
    """The items check_accuracy compares: all of them up to SAMPLE_ALL_POINTS points per side, else the first, the middle and the last
    (the last lies in the ragged tile of a launch whose tiles hold several transforms)."""
    batch = int(batch)
    if batch * int(n_points) <= SAMPLE_ALL_POINTS:
        return list(range(batch))
    return sorted(set((0, batch // 2, batch - 1)))


def reference_fft(x, shape, dtype, inverse=False, normalize=True, scale=1.0):
    """The exact transform of one item, to well below the working precision's rounding: numpy.fft on clongdouble (64-bit mantissa) for
    fp64 plans, on complex128 for fp32 plans; with the normalize / scale semantics of the reference (kernel.py:23-37)."""
    double = unit_roundoff(dtype) < 2.0 ** -30
    if double:
        assert numpy.finfo(numpy.longdouble).eps <= 2.0 ** -63, "this host has no extended precision: the fp64 reference would be no better than the path"
        x = numpy.asarray(x).astype(numpy.clongdouble)
    else:
        x = numpy.asarray(x).astype(numpy.complex128)
    x = x.reshape(shape)
    size = x.size
    if inverse:
        ref = numpy.fft.ifftn(x)
        if not normalize:
            ref = ref * size
        ref = ref / scale
    else:
        ref = numpy.fft.fftn(x) * scale
    assert ref.dtype == x.dtype, (ref.dtype, x.dtype)
    return ref.reshape(-1)


def item_error(got, ref):
    """(L1-relative, max|err| / rms(ref)) of one item"""
    ref = numpy.asarray(ref).reshape(-1)
    diff = numpy.abs(numpy.asarray(got).reshape(-1).astype(ref.dtype) - ref)
    mag = numpy.abs(ref)
    return float(diff.sum() / mag.sum()), float(diff.max() / numpy.sqrt(numpy.mean(mag * mag)))


def check_accuracy(shape, dtype, batch, input_of, output_of, inverse=False, normalize=True, scale=1.0, what=""):
    """Hold the sampled items (sampled_items) of a result to accuracy_bound.  input_of(j) / output_of(j): item j's exact input and the
    path's output (complex, any shape of the item's size).  Returns {"l1", "max", "l1_ratio", "max_ratio", "item_l1", "item_max"}: the
    WORST item's metrics, and the ratios metric / (u (L + 2)) that tests report."""
    from concurrent.futures import ThreadPoolExecutor
    shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = int(numpy.prod(shape))
    items = sampled_items(batch, n)

    def one(j):
        ref = reference_fft(input_of(j), shape, dtype, inverse, normalize, scale)
        return item_error(output_of(j), ref)

    if len(items) > 1 and n >= (1 << 16):
        with ThreadPoolExecutor(min(4, len(items))) as ex:        # (numpy's FFT releases the GIL: the big fp64 references overlap)
            errs = list(ex.map(one, items))
    else:
        errs = [one(j) for j in items]
    l1_bound, max_bound = accuracy_bound(dtype, n)
    unit = unit_roundoff(dtype) * (n.bit_length() - 1 + 2)
    i1 = max(range(len(items)), key=lambda i: errs[i][0])
    im = max(range(len(items)), key=lambda i: errs[i][1])
    rep = {"l1": errs[i1][0], "max": errs[im][1], "l1_ratio": errs[i1][0] / unit, "max_ratio": errs[im][1] / unit,
           "item_l1": items[i1], "item_max": items[im]}
    assert rep["l1"] <= l1_bound and rep["max"] <= max_bound, \
        "%s %s %s batch %d %s: worst item %d L1-relative %.3g (bound %.3g), worst item %d max|err|/rms %.3g (bound %.3g)" % (
            what, shape, numpy.dtype(dtype).name, batch, "inverse" if inverse else "forward", items[i1], rep["l1"], l1_bound,
            items[im], rep["max"], max_bound)
    return rep


class GuardedBuffer(object):
    """A user range of `nbytes` inside ONE device allocation: it starts `offset` bytes past a 64 KiB front guard (`offset` 16-byte
    aligned: the C ABI's requirement; not 64-byte aligned, unlike every hipMalloc base) and is followed by a back guard of at least
    1 MiB, larger than any tile.  Both guards hold a quiet NaN with a recognisable payload in either precision, so that a kernel writing
    or reading out of its range lands in memory the test owns: check_guards() copies back the guard bytes alone and asserts that they
    are bit-identical to what was written."""

    FRONT = 64 << 10
    BACK = 1 << 20
    WORD = 0x7FC1D1E5            # a quiet NaN as fp32, and as the high word of an fp64

    def __init__(self, nbytes, offset):
        import pyfft_amd.hip as hip
        from pyfft_amd import _native as N
        assert offset % 16 == 0 and 0 <= offset < 4096, offset
        self._N = N
        self.nbytes = int(nbytes)
        self.offset = int(offset)
        self.front = self.FRONT + self.offset
        self.back = self.BACK + (-(self.front + self.nbytes) % 4096)
        self.alloc = hip.DeviceAllocation(self.front + self.nbytes + self.back)
        self.ptr = self.alloc.ptr + self.front
        self._front_host = numpy.full(self.front // 4, self.WORD, numpy.uint32)
        self._back_host = numpy.full(self.back // 4, self.WORD, numpy.uint32) if self.back != self.front else self._front_host
        assert self.front % 4 == 0 and self.nbytes % 4 == 0
        N.check(N.lib.mifft_memcpy_h2d(self.alloc.ptr, self._front_host.ctypes.data, self.front, None), "mifft_memcpy_h2d")
        N.check(N.lib.mifft_memcpy_h2d(self.ptr + self.nbytes, self._back_host.ctypes.data, self.back, None), "mifft_memcpy_h2d")

    def check_guards(self, what=""):
        N = self._N
        for name, start, want in (("front", self.alloc.ptr, self._front_host), ("back", self.ptr + self.nbytes, self._back_host)):
            got = numpy.empty_like(want)
            N.check(N.lib.mifft_memcpy_d2h(got.ctypes.data, start, want.nbytes, None), "mifft_memcpy_d2h")
            bad = numpy.flatnonzero(got != want)
            if bad.size:
                rel = (start - self.ptr) + 4 * bad          # byte offsets relative to the user range's start
                raise AssertionError("%s: %s guard damaged: %d words, bytes %d .. %d relative to the user range of %d bytes (base offset %d)"
                                     % (what, name, bad.size, int(rel[0]), int(rel[-1]) + 3, self.nbytes, self.offset))

    def free(self):
        self.alloc.free()
