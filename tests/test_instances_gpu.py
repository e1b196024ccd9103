"""Every kernel instance a default plan can select, held to the per-instance contract (docs/parity.md): one case per instance key
(kernel_coverage.audit_cases(): the smallest shape / dtype / batch >= 3 that selects the key, on the model of the full part; the test
asserts that the device's own planner selects it too), on user buffers inside guarded allocations at bases that are 16- but not
64-byte aligned.

  1. out of place, forward: the input is untouched, both buffers' guards are intact, the sampled items meet accuracy_bound against an
     extended-precision reference (helpers.check_accuracy)
  2. in place, forward: guards intact, the result bit-identical to step 1 -- or, where an out-of-place execute of the plan may run
     another instance (a several-work-groups-per-transform kernel: keys nd_oop / nd2z / nd2zp), within the bound itself
  3. out of place, inverse (normalize on) on fresh data: within the bound, guards intact
  4. the input of step 1 poisoned, out of place: first the middle item all NaN and the last all +Inf (split planes: one in each plane),
     then every even item (NaN and +Inf in turn, so that each odd item has a poisoned item on both sides); every other item
     bit-identical to step 1 (compared on the device), guards intact -- no read across items, not even one multiplied by 0
  Where the out-of-place executes take another instance (step 2's second case), steps 3 and 4 also run IN PLACE on the guarded buffer,
  the poisoned runs compared with step 2's result: the case's own instance then gets the whole contract too.

Each case reports the worst item's error ratios (metric / (u (L + 2))) as junit properties (`record_property`): a `--junitxml` run
yields the per-key table."""
import ctypes

import numpy
import pytest

import kernel_coverage as KC
from helpers import NOISE_PERIOD, GuardedBuffer, check_accuracy, _test_data

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:record_property is incompatible with junit_family")]    # (the properties are written)

CASES = KC.audit_cases()
OFFSETS = (16, 48, 208, 80, 144, 272)          # user-range offsets past the front guard: 16-byte aligned, none 64-byte aligned
OOP_OWN_INSTANCE = ("nd_oop", "nd2z", "nd2zp")   # keys of instances only out-of-place executes run


def _case_id(case):
    keys = case[3]
    return "-".join(str(v).replace(" ", "_") for v in keys[0]) + ("+%d" % (len(keys) - 1) if len(keys) > 1 else "")


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
    def __init__(self, hip, N, case, index):
        shape, dtname, batch, keys = case
        self.hip, self.N = hip, N
        self.shape, self.batch, self.keys = tuple(shape), int(batch), keys
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

    def item_output(self, bufs, j):
        parts = []
        for b in bufs:
            h = numpy.empty(self.n, self.cdt.type(0).real.dtype if self.split else self.cdt)
            self.N.check(self.N.lib.mifft_memcpy_d2h(h.ctypes.data, b.ptr + j * self.item_bytes, self.item_bytes, None), "mifft_memcpy_d2h")
            parts.append(h)
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


def _poison_layouts(batch):
    """{item: (plane, value)} of the poisoned runs: the middle item NaN and the last (ragged tile) +Inf; then every even item, NaN and +Inf
    in turn, so that every odd item lies between two poisoned ones (with batch 3 the first layout checks item 0, the second item 1)"""
    yield {batch // 2: (0, numpy.nan), batch - 1: (-1, numpy.inf)}
    yield {j: ((0, numpy.nan) if j % 4 == 0 else (-1, numpy.inf)) for j in range(0, batch, 2)}


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_instance(ctx, case, record_property):
    from pyfft_amd import _native as N
    hip = ctx.hip
    shape, dtname, batch, keys = case
    plan, c = None, None
    try:
        plan = hip.Plan(tuple(shape), dtype=numpy.dtype(dtname))
        have = KC.keys_of_plan(plan, batch)
        lost = [k for k in keys if k not in have]
        assert not lost, "the device's planner does not select %r at batch %d (device %r, model %r): it selects %r" % (
            lost, batch, plan._context.machine, KC.full_machine(), sorted(have, key=str))
        c = _Case(hip, N, case, CASES.index(case))
        record_property("keys", repr(list(keys)))
        record_property("base_offsets", "%d/%d" % (c.ins[0].offset, c.outs[0].offset))
        ins, outs = c.ins, c.outs
        # an out-of-place execute of this plan may run another instance (a several-work-groups-per-transform kernel) than an in-place one:
        # then the in-place executes get the whole contract too
        oop_differs = any(k[0] in OOP_OWN_INSTANCE for k in have)

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
            return check_accuracy(shape, c.dtype, batch, lambda j: c.item_input(blk3, j), lambda j: c.item_output(outs, j), inverse=True,
                                  what=what)

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
        fw = check_accuracy(shape, c.dtype, batch, lambda j: c.item_input(blk, j), lambda j: c.item_output(outs, j), what="out of place")
        for b, r in zip(outs, c.ref):
            c._d2d(r.ptr, b.ptr, c.plane_bytes)

        # 2. in place, forward
        for b, x in zip(outs, c.x0):
            c._d2d(b.ptr, x.ptr, c.plane_bytes)
        run(outs)
        c._sync()
        c.guards(outs, "in-place forward")
        if oop_differs:
            check_accuracy(shape, c.dtype, batch, lambda j: c.item_input(blk, j), lambda j: c.item_output(outs, j), what="in place")
        else:
            for b, r in zip(outs, c.ref):
                assert c.mismatches(b.ptr, r.ptr, c.plane_bytes) == 0, "in place differs from out of place"

        # 3. + 4. out of place; and in place where that runs another instance (c.ref then holds the in-place result)
        blk3 = _block(c.cdt, c.count, 202)
        inv = inverse(False, blk3)
        isolation(False)
        reps = [("forward", fw), ("inverse", inv)]
        if oop_differs:
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
    finally:
        if c is not None:
            c.close()
        if plan is not None:
            plan.close()
