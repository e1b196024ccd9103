"""Test harness: counterpart of the reference's test/helpers.py for the HIP backend.

HipContext mirrors helpers.CudaContext (test/helpers.py:29-74): allocate / toGpu / fromGpu /
getPlan / timers / supportsDouble.  Data generation and the error metric come from the oracle
(oracle/pyfft_oracle.py), which only tests may import.
"""
import ctypes

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


class FailingPool(object):
    """A pool for plans on PooledFakeContext (tests/test_lifecycle_cpu.py): every allocate(nbytes) is logged in `requests`, the
    fail_at-th call (counted from 1 since the last arm()) raises MemoryError.  Blocks are objects, so a test sees which one a plan holds."""

    class Block(object):
        def __init__(self, nbytes):
            self.nbytes = int(nbytes)

    def __init__(self):
        self.arm(None)

    def arm(self, fail_at):
        self.fail_at = fail_at
        self.requests = []

    def allocate(self, nbytes):
        self.requests.append(int(nbytes))
        if self.fail_at is not None and len(self.requests) == self.fail_at:
            raise MemoryError("FailingPool: allocation %d (%d bytes) fails" % (self.fail_at, nbytes))
        return FailingPool.Block(nbytes)


class PooledFakeContext(FakeContext):
    """FakeContext whose allocate() and allocate_raw() go through a FailingPool, with the two calls of a real context that a plan makes
    when it lets go of scratch: wait_scratch() (counted) and capturing() (settable)."""

    def __init__(self, machine, pool=None, capturing=False):
        FakeContext.__init__(self, machine)
        self.pool = pool if pool is not None else FailingPool()
        self.allocate = self.allocate_raw = self.pool.allocate
        self.is_capturing = capturing
        self.waits = 0          # wait_scratch() calls
        self.syncs = 0          # wait() calls (finish())

    def capturing(self):
        return self.is_capturing

    def wait_scratch(self):
        self.waits += 1

    def wait(self):
        self.syncs += 1

    # what an execute() calls before its first launch; every launch takes stream_handle() as an argument, so a plan that goes on
    # to one stops here
    def createQueue(self, buffers=()):
        pass

    def order_scratch(self, capturing=None):
        pass

    def stream_handle(self):
        raise AssertionError("the plan went on to a launch")


# ---- the per-instance accuracy contract (tests/test_instances_gpu.py; docs/parity.md) ------------------------------------------------
NOISE_PERIOD = (1 << 22) + 17          # the period of _noise: element i of a _test_data set is element i % NOISE_PERIOD of its first block
SAMPLE_ALL_POINTS = 1 << 22            # up to this many points per side every item is checked, beyond it the first, the middle and the last


def unit_roundoff(dtype):
    """u of the working precision of a plan of `dtype` (2^-24 for complex64 / float32 planes, 2^-53 for complex128 / float64)"""
    return 2.0 ** -53 if numpy.dtype(dtype) in (numpy.dtype(numpy.complex128), numpy.dtype(numpy.float64)) else 2.0 ** -24


def bound_levels(n_points):
    """L = ceil(log2(n_points)): log2 for a power of two"""
    return (int(n_points) - 1).bit_length()


def accuracy_bound(dtype, n_points, levels=None):
    """(L1-relative, max|err| / rms(ref)) that ONE transform of `n_points` points (all axes together) must meet, per item:
    u (L + 2) and 4 u (L + 2); fp32 also keeps the reference's L1 threshold 1.1e-6 where it is the tighter.  L = log2(n_points) for a
    power of two; any other length must say which L its form earns (`levels`: any_size_levels).  The constants come from a radix-2
    model with correctly rounded twiddles, and hold for the mixed-radix and Bluestein models of the extensions with L = ceil(log2 n)
    and L = log2 of the padded length (tests/test_accuracy_model.py, which also shows that the bound catches a twiddle table wrong in
    the 12th digit and a localised index error that the reference's thresholds let through)."""
    n_points = int(n_points)
    if levels is None:
        assert n_points >= 1 and n_points & (n_points - 1) == 0, n_points
        levels = n_points.bit_length() - 1
    u = unit_roundoff(dtype)
    c = u * (int(levels) + 2)
    l1 = c if u < 2.0 ** -30 else min(c, EPS_F)
    return l1, 4.0 * c


def bluestein_padded_length(dtype, n):
    """the m an axis of n points that Plan(..., any_size=True) runs by Bluestein's algorithm pads to: mifft_bluestein_padded's where the
    one-launch kernel takes it, else the work array's 2^ceil(log2(2 n - 1))"""
    from pyfft_amd import _native as N
    prec = N.F64 if unit_roundoff(dtype) < 2.0 ** -30 else N.F32
    mb = ctypes.c_int32(0)
    if N.lib.mifft_bluestein_padded(prec, int(n), ctypes.byref(mb)) == 0:
        return mb.value
    return 1 << (2 * int(n) - 2).bit_length()


def any_size_levels(shape, dtype):
    """L of a Plan(shape, dtype, any_size=True) (the form selection of generic.GenericFFTPlan): ceil(log2) of the points of the axes
    that run as powers of two, mixed-radix or long smooth transforms, plus ceil(log2 m) for every axis Bluestein pads to m.  The
    power-of-two shapes keep L = log2(points)."""
    from pyfft_amd import _native as N
    shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    prec = N.F64 if unit_roundoff(dtype) < 2.0 ** -30 else N.F32
    split = numpy.dtype(dtype).kind == "f"
    direct, levels = 1, 0
    for n in shape:
        if n & (n - 1) == 0 or N.lib.mifft_mixed_supported(prec, n) == 0:
            direct *= n
            continue
        n1, n2 = ctypes.c_int32(0), ctypes.c_int32(0)
        if all(v == 1 for v in shape[:-1]) and not split and \
                N.lib.mifft_mixed_long_split(prec, n, ctypes.byref(n1), ctypes.byref(n2)) == 0:
            direct *= n
            continue
        levels += bound_levels(bluestein_padded_length(dtype, n))
    return levels + bound_levels(direct)


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


def check_accuracy(shape, dtype, batch, input_of, output_of, inverse=False, normalize=True, scale=1.0, what="", levels=None):
    """Hold the sampled items (sampled_items) of a result to accuracy_bound.  input_of(j) / output_of(j): item j's exact input and the
    path's output (complex, any shape of the item's size); `levels`: the L of accuracy_bound for a length that is no power of two.  Returns {"l1", "max", "l1_ratio", "max_ratio", "item_l1", "item_max"}: the
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
    l1_bound, max_bound = accuracy_bound(dtype, n, levels)
    unit = unit_roundoff(dtype) * ((n.bit_length() - 1 if levels is None else int(levels)) + 2)
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
    """A user range of `nbytes` inside ONE device allocation: it starts `offset` bytes past a 64 KiB front guard (`offset` a multiple
    of `align`: 16 by default, the C ABI's requirement for most entry points; an element-aligned run passes the element's size; not
    64-byte aligned, unlike every hipMalloc base) and is followed by a back guard of at least
    1 MiB, larger than any tile.  Both guards hold a quiet NaN with a recognisable payload in either precision, so that a kernel writing
    or reading out of its range lands in memory the test owns: check_guards() copies back the guard bytes alone and asserts that they
    are bit-identical to what was written."""

    FRONT = 64 << 10
    BACK = 1 << 20
    WORD = 0x7FC1D1E5            # a quiet NaN as fp32, and as the high word of an fp64

    def __init__(self, nbytes, offset, align=16):
        import pyfft_amd.hip as hip
        from pyfft_amd import _native as N
        assert align in (4, 8, 16) and offset % align == 0 and 0 <= offset < 4096, (offset, align)
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


# ---- the steps of the per-instance contract, shared by tests/test_instances_gpu.py and tests/test_extension_instances_gpu.py --------
OFFSETS = (16, 48, 208, 80, 144, 272)          # user-range offsets past the front guard: 16-byte aligned, none 64-byte aligned

_blocks = {}
_poison = {}


def _block(cdt, count, seed):
    """the first min(count, NOISE_PERIOD) elements of _test_data of `count` points: the data set repeats them (helpers._noise)"""
    m = min(int(count), NOISE_PERIOD)
    key = (numpy.dtype(cdt).name, m, seed)
    if key not in _blocks:
        if len(_blocks) > 8:
            _blocks.clear()
        _blocks[key] = _test_data((m,), cdt, 1, seed).reshape(-1)
    return _blocks[key]


class _Case(object):
    """The guarded user buffers of one contract case: `batch` items of shape `shape` (tiles=(tile shape, counts (cz, cy, cx)): each
    item a parent array, the accuracy checked per tile), in dtype `dtname`; levels = the L of accuracy_bound (None: a power of two)."""

    def __init__(self, hip, N, case, index, tiles=None, levels=None):
        shape, dtname, batch = case[:3]
        self.hip, self.N = hip, N
        self.shape, self.batch = tuple(shape), int(batch)
        self.tiles, self.levels = tiles, levels
        self.dtype = numpy.dtype(dtname)
        self.split = self.dtype.kind == "f"
        self.cdt = numpy.dtype(numpy.complex128 if self.dtype in (numpy.dtype(numpy.float64), numpy.dtype(numpy.complex128)) else numpy.complex64)
        self.n = int(numpy.prod(self.shape))
        self.count = self.n * self.batch
        self.esize = self.cdt.itemsize // 2 if self.split else self.cdt.itemsize       # bytes per element of one plane
        self.item_bytes = self.n * self.esize
        self.plane_bytes = self.count * self.esize
        planes = 2 if self.split else 1
        o_in, o_out = OFFSETS[index % len(OFFSETS)], OFFSETS[(index + 1) % len(OFFSETS)]
        self.ins, self.outs, self.x0, self.ref, self._word = [], [], [], [], None
        try:
            for _ in range(planes):
                self.ins.append(GuardedBuffer(self.plane_bytes, o_in))
                self.outs.append(GuardedBuffer(self.plane_bytes, o_out))
                self.x0.append(hip.DeviceAllocation(self.plane_bytes))      # the input of step 1
                self.ref.append(hip.DeviceAllocation(self.plane_bytes))     # the clean forward result the poisoned runs are compared with
            w = ctypes.c_void_p()
            N.check(N.lib.mifft_host_alloc(ctypes.byref(w), 64), "mifft_host_alloc")
            self._word = w.value
            self._count = ctypes.c_uint64.from_address(w.value)
        except BaseException:
            self.close()
            raise

    def close(self):
        for b in self.ins + self.outs:
            b.free()
        for a in self.x0 + self.ref:
            a.free()
        if self._word is not None:
            self.N.lib.mifft_host_free(self._word)
            self._word = None

    # -- device data
    def _sync(self):
        self.N.check(self.N.lib.mifft_device_sync(), "mifft_device_sync")

    def _d2d(self, dst, src, nbytes):
        self.N.check(self.N.lib.mifft_memcpy_d2d(dst, src, nbytes, None), "mifft_memcpy_d2d")

    def _repeat(self, ptr, host, nbytes):
        """ptr[0 .. nbytes) = `host` (bytes) repeated: one upload, then copies of what is already there"""
        done = min(host.nbytes, nbytes)
        self.N.check(self.N.lib.mifft_memcpy_h2d(ptr, host.ctypes.data, done, None), "mifft_memcpy_h2d")
        while done < nbytes:
            step = min(done - done % host.nbytes, nbytes - done)
            self._d2d(ptr + done, ptr, step)
            done += step

    def fill(self, bufs, seed):
        """the data set of _test_data(shape, dtype, batch, seed) into the planes `bufs`; returns the block it repeats"""
        blk = _block(self.cdt, self.count, seed)
        hosts = [numpy.ascontiguousarray(blk.real), numpy.ascontiguousarray(blk.imag)] if self.split else [blk]
        for b, h in zip(bufs, hosts):
            self._repeat(b.ptr, h.view(numpy.uint8), self.plane_bytes)
        self._sync()
        return blk

    def item_input(self, blk, j):
        return blk[(j * self.n + numpy.arange(self.n, dtype=numpy.int64)) % blk.size]

    def item_planes(self, ptrs, j):
        """item j of the planes at `ptrs`, as host arrays of the plane dtype"""
        parts = []
        for p in ptrs:
            h = numpy.empty(self.n, self.cdt.type(0).real.dtype if self.split else self.cdt)
            self.N.check(self.N.lib.mifft_memcpy_d2h(h.ctypes.data, p + j * self.item_bytes, self.item_bytes, None), "mifft_memcpy_d2h")
            parts.append(h)
        return parts

    def item_output(self, bufs, j):
        parts = self.item_planes([b.ptr for b in bufs], j)
        return parts[0].astype(self.cdt) + 1j * parts[1] if self.split else parts[0]

    def poison(self, ptr, j, value):
        """item j of the plane at `ptr` all `value` (not synchronised)"""
        fdt = numpy.float64 if self.cdt == numpy.complex128 else numpy.float32
        key = (value, fdt)
        if key not in _poison:
            _poison[key] = numpy.full(1 << 17, value, fdt).view(numpy.uint8)
        host = _poison[key][:min(self.item_bytes, _poison[key].nbytes)]
        self._repeat(ptr + j * self.item_bytes, host, self.item_bytes)

    def mismatches(self, a, b, nbytes):
        """how much of device ranges a[0 .. nbytes) and b[0 .. nbytes) differs: 16-byte words on the device, bytes on the host (small or odd
        ranges); 0 when they are bit-identical"""
        if nbytes <= 0:
            return 0
        if nbytes % 16 or (a | b) % 16 or nbytes < 4096:
            ha, hb = numpy.empty(nbytes, numpy.uint8), numpy.empty(nbytes, numpy.uint8)
            self.N.check(self.N.lib.mifft_memcpy_d2h(ha.ctypes.data, a, nbytes, None), "mifft_memcpy_d2h")
            self.N.check(self.N.lib.mifft_memcpy_d2h(hb.ctypes.data, b, nbytes, None), "mifft_memcpy_d2h")
            return int(numpy.count_nonzero(ha != hb))
        self._count.value = 0
        self.N.check(self.N.lib.mifft_aux_count_mismatch(a, b, nbytes, self._word, None), "mifft_aux_count_mismatch")
        self._sync()
        return int(self._count.value)

    def guards(self, bufs, what):
        for i, b in enumerate(bufs):
            b.check_guards("%s, plane %d" % (what, i))

    # -- the accuracy of a result: per item, or per tile of every parent array
    def tile_of(self, item, t):
        """tile t (in the order [cz][cy][cx]) of one parent array `item` (flat)"""
        tile, counts = self.tiles
        full = tuple(a * b for a, b in zip(tile, counts[-len(tile):]))
        idx = numpy.unravel_index(t, counts[-len(tile):])
        sl = tuple(slice(i * a, (i + 1) * a) for i, a in zip(idx, tile))
        return numpy.asarray(item).reshape(full)[sl]

    def accuracy(self, bufs, blk, inverse=False, normalize=True, scale=1.0, what=""):
        if self.tiles is None:
            return check_accuracy(self.shape, self.dtype, self.batch, lambda j: self.item_input(blk, j), lambda j: self.item_output(bufs, j),
                                  inverse=inverse, normalize=normalize, scale=scale, what=what, levels=self.levels)
        tile, counts = self.tiles
        nt = int(numpy.prod(counts))
        last = {}

        def out_item(p):
            if p not in last:
                last.clear()
                last[p] = self.item_output(bufs, p)
            return last[p]
        return check_accuracy(tile, self.dtype, self.batch * nt, lambda j: self.tile_of(self.item_input(blk, j // nt), j % nt),
                              lambda j: self.tile_of(out_item(j // nt), j % nt), inverse=inverse, normalize=normalize, scale=scale,
                              what=what, levels=self.levels)


def _poison_layouts(batch):
    """{item: (plane, value)} of the poisoned runs: the middle item NaN and the last (ragged tile) +Inf; then every even item, NaN and +Inf
    in turn, so that every odd item lies between two poisoned ones (with batch 3 the first layout checks item 0, the second item 1)"""
    yield {batch // 2: (0, numpy.nan), batch - 1: (-1, numpy.inf)}
    yield {j: ((0, numpy.nan) if j % 4 == 0 else (-1, numpy.inf)) for j in range(0, batch, 2)}


def run_contract(plan, c, inplace_too, record_property):
    """Steps 1-4 of the per-instance contract (tests/test_instances_gpu.py) on the buffers of `c` (a _Case) through `plan`.  Leaves the
    clean forward result in c.ref; returns the reports [(step name, check_accuracy report)], which it also records.  inplace_too: the
    in-place executes are what the case is about (they run another instance than the out-of-place ones, or give the case's launch its
    buffer sides): step 2 is held to the bound itself, and steps 3 and 4 run in place as well."""
    N = c.N
    batch = c.batch
    ins, outs = c.ins, c.outs

    def run(src, dst=None, inverse=False):
        args = [b.ptr for b in src] + ([b.ptr for b in dst] if dst is not None else [])
        plan.execute(*args, batch=batch, inverse=inverse)

    def clear_outputs():
        for b in outs:
            N.check(N.lib.mifft_memset(b.ptr, 0xFF, b.nbytes, None), "mifft_memset")      # (all-ones: a NaN in both precisions)

    def inverse(inplace, blk3):
        """3. inverse (normalize on) on fresh data"""
        what = "in-place inverse" if inplace else "out-of-place inverse"
        c.fill(outs if inplace else ins, 202)
        if inplace:
            run(outs, inverse=True)
        else:
            clear_outputs()
            run(ins, outs, inverse=True)
        c._sync()
        if not inplace:
            c.guards(ins, what + ", input")
        c.guards(outs, what + ", output")
        return c.accuracy(outs, blk3, inverse=True, what=what)

    def isolation(inplace):
        """4. poisoned items: every other item bit-identical to the clean forward result in c.ref"""
        what = "in-place" if inplace else "out-of-place"
        src = outs if inplace else ins
        ib = c.item_bytes
        for layout in _poison_layouts(batch):
            for b, x in zip(src, c.x0):
                c._d2d(b.ptr, x.ptr, c.plane_bytes)
            for j, (plane, value) in layout.items():
                c.poison(src[plane].ptr, j, value)
            if inplace:
                run(outs)
            else:
                clear_outputs()
                run(ins, outs)
            c._sync()
            if not inplace:
                c.guards(ins, "poisoned %s forward, input" % what)
            c.guards(outs, "poisoned %s forward, output" % what)
            for j in layout:                                 # (the poisoned items' own results are not compared)
                for b, r in zip(outs, c.ref):
                    c._d2d(b.ptr + j * ib, r.ptr + j * ib, ib)
            c._sync()
            for b, r in zip(outs, c.ref):
                if c.mismatches(b.ptr, r.ptr, c.plane_bytes):
                    changed = [j for j in range(min(batch, 4096)) if c.mismatches(b.ptr + j * ib, r.ptr + j * ib, ib)]
                    raise AssertionError("%s forward: items %r changed when items %r were poisoned" % (what, changed[:20], sorted(layout)[:20]))

    # 1. out of place, forward
    blk = c.fill(ins, 101)
    for b, x in zip(ins, c.x0):
        c._d2d(x.ptr, b.ptr, c.plane_bytes)
    clear_outputs()
    run(ins, outs)
    c._sync()
    for b, x in zip(ins, c.x0):
        assert c.mismatches(b.ptr, x.ptr, c.plane_bytes) == 0, "an out-of-place execute touched its input"
    c.guards(ins, "out-of-place forward, input")
    c.guards(outs, "out-of-place forward, output")
    fw = c.accuracy(outs, blk, what="out of place")
    for b, r in zip(outs, c.ref):
        c._d2d(r.ptr, b.ptr, c.plane_bytes)

    # 2. in place, forward
    for b, x in zip(outs, c.x0):
        c._d2d(b.ptr, x.ptr, c.plane_bytes)
    run(outs)
    c._sync()
    c.guards(outs, "in-place forward")
    if inplace_too:
        c.accuracy(outs, blk, what="in place")
    else:
        for b, r in zip(outs, c.ref):
            assert c.mismatches(b.ptr, r.ptr, c.plane_bytes) == 0, "in place differs from out of place"

    # 3. + 4. out of place; and in place where the case is about those executes (c.ref then holds the in-place result)
    blk3 = _block(c.cdt, c.count, 202)
    inv = inverse(False, blk3)
    isolation(False)
    reps = [("forward", fw), ("inverse", inv)]
    if inplace_too:
        for b, x in zip(outs, c.x0):
            c._d2d(b.ptr, x.ptr, c.plane_bytes)
        run(outs)
        c._sync()
        for b, r in zip(outs, c.ref):
            c._d2d(r.ptr, b.ptr, c.plane_bytes)
        reps.append(("inplace_inverse", inverse(True, blk3)))
        isolation(True)

    for name, rep in reps:
        record_property(name + "_l1_ratio", "%.4g" % rep["l1_ratio"])
        record_property(name + "_max_ratio", "%.4g" % rep["max_ratio"])
    return reps


# ---- the contract for forms whose sides differ (tests/test_form_instances_gpu.py) -----------------------------------------------------
def _h2d(ptr, host):
    from pyfft_amd import _native as N
    host = numpy.ascontiguousarray(host)
    N.check(N.lib.mifft_memcpy_h2d(ptr, host.ctypes.data, host.nbytes, None), "mifft_memcpy_h2d")


def _d2h_bytes(ptr, nbytes):
    from pyfft_amd import _native as N
    host = numpy.empty(int(nbytes), numpy.uint8)
    N.check(N.lib.mifft_memcpy_d2h(host.ctypes.data, ptr, host.nbytes, None), "mifft_memcpy_d2h")
    return host


class SidedCase(object):
    """run_contract's sibling for the forms whose two sides differ in size and type (real <-> half spectrum; complex32 on fp16 storage)
    or that read a third buffer (a convolution's spectrum).  Items lie along axis 0 of the host arrays; the device buffers are guarded
    (GuardedBuffer), one per (role, size, base offset), kept for the case.  A subclass says how the plan executes
    (execute(plan, in_ptr, out_ptr or None for in place, inverse, **kw)) and how many bytes an output takes (out_bytes(inverse))."""

    def __init__(self, hip, shape, batch, index):
        from pyfft_amd import _native as N
        self.hip, self.N = hip, N
        self.shape, self.batch, self.index = tuple(shape), int(batch), int(index)
        self.n = int(numpy.prod(self.shape))
        self.off_in, self.off_out, self.off_spec = (OFFSETS[(self.index + k) % len(OFFSETS)] for k in range(3))
        self._bufs = {}

    def close(self):
        for b in self._bufs.values():
            b.free()
        self._bufs = {}

    def buf(self, role, nbytes, off):
        key = (role, int(nbytes), int(off))
        if key not in self._bufs:
            self._bufs[key] = GuardedBuffer(nbytes, off, align=min(16, off & -off))
        return self._bufs[key]

    def sync(self):
        self.N.check(self.N.lib.mifft_device_sync(), "mifft_device_sync")

    def run(self, plan, inverse, x, off_in=None, off_out=None, inplace=False, spec=None, refused=False, what="", **kw):
        """One execute of the host input x between guard bands: the input at off_in bytes past its front guard, the output at off_out
        pre-filled with all-ones bytes (a NaN in every float format), in place on the input's buffer; spec = (host array, offset): a
        third, read-only buffer passed as spectrum=.  Afterwards every guard is intact and the input (out of place) and the spectrum
        are bit-identical to what was uploaded.  Returns the output's bytes.  refused: the execute must raise ValueError, and the
        output must still hold its pre-filled bytes."""
        N = self.N
        off_in = self.off_in if off_in is None else off_in
        off_out = self.off_out if off_out is None else off_out
        xb = numpy.ascontiguousarray(x).view(numpy.uint8).reshape(-1)
        nout = self.out_bytes(inverse)
        assert not inplace or nout == xb.size
        a = self.buf("in", xb.size, off_in)
        b = a if inplace else self.buf("out", nout, off_out)
        bufs = [("input", a)] if inplace else [("input", a), ("output", b)]
        extra = []
        if spec is not None:
            sb = numpy.ascontiguousarray(spec[0]).view(numpy.uint8).reshape(-1)
            g = self.buf("spectrum", sb.size, spec[1])
            _h2d(g.ptr, sb)
            bufs.append(("spectrum", g))
            extra.append((g, sb))
            kw["spectrum"] = g.ptr
        _h2d(a.ptr, xb)
        if not inplace:
            N.check(N.lib.mifft_memset(b.ptr, 0xFF, nout, None), "mifft_memset")
        self.sync()
        if refused:
            try:
                self.execute(plan, a.ptr, None if inplace else b.ptr, inverse, **kw)
            except ValueError:
                pass
            else:
                raise AssertionError("%s: accepted, a ValueError was expected" % what)
        else:
            self.execute(plan, a.ptr, None if inplace else b.ptr, inverse, **kw)
        self.sync()
        for name, g in bufs:
            g.check_guards("%s, %s" % (what, name))
        if not inplace:
            assert numpy.array_equal(_d2h_bytes(a.ptr, xb.size), xb), "%s: an out-of-place execute touched its input" % what
        for g, sb in extra:
            assert numpy.array_equal(_d2h_bytes(g.ptr, sb.size), sb), "%s: the spectrum was written" % what
        out = _d2h_bytes(b.ptr, nout)
        if refused:
            assert (out == 0xFF).all(), "%s: a refused execute changed the output" % what
        return out

    def changed(self, got, ref, skip=()):
        """the items (equal byte ranges along the buffers) of got that differ from ref, those of `skip` left out"""
        g, r = got.reshape(self.batch, -1), ref.reshape(self.batch, -1)
        return [j for j in range(self.batch) if j not in skip and not numpy.array_equal(g[j], r[j])]

    @staticmethod
    def poisoned(x, layout):
        """a copy of the host batch x with every item of `layout` (_poison_layouts) all its value: both parts of a complex number,
        the fp16 value in complex32 data held as float16 pairs"""
        y = numpy.array(x, copy=True)
        for j, (_, value) in layout.items():
            y[j] = complex(value, value) if y.dtype.kind == "c" else value
        return y
