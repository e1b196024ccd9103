"""One lifecycle contract for every plan kind across re-plans (docs/parity.md, "Plan lifecycle").

THE RULE.  Every execute of a long-lived plan writes exactly the bits that a FRESH plan of the same arguments writes when it runs that
one execute alone and synchronously -- whatever batches, directions, in-place / out-of-place calls, close() and refused calls came
before it.  The fresh plan's first result per direction (per spectrum mode for a convolution) is held to the extended-precision
reference at the levels of the instance suites (test_instances_gpu / test_extension_instances_gpu / test_form_instances_gpu), which ties
the bit identity to that reference and not to the code under test.

One scripted sequence per case (_steps): 14 executes with wait_for_finish=False on one hip.Stream, synchronised once at the end; every
step has its own output buffer (an in-place step first copies its input there on the same stream); batches b1 < b2, neither a
multiple of 4; close() after the seventh step; three calls that must be refused on the way; finish() at the end.  Comparisons count
mismatching words over the WHOLE buffer (on the device beyond 4 MiB, on the host below).

Then, per case the property covers: graphs across re-plans (the extension and form classes; FFTPlan has
test_interop_gpu.test_captured_execute_replays_bit_identically), a failed allocation recovered, and no early return of pooled scratch.
"""
import ctypes

import numpy
import pytest

import dct_model as DM
import helpers as H
import real_model as RM
from dct_cases import levels as dct_levels
from test_conv_gpu import reference as conv_reference
from test_half_gpu import _c64_rounded, _check_item

pytestmark = pytest.mark.gpu

DEVICE_COMPARE_BYTES = 4 << 20
MAX_BUFFER_BYTES = 64 << 20
BATCHES = (3, 3, 5, 3, 5, 5, 3, 5, 3, 3, 5, 5, 3, 5)          # b1, b1, b2, b1, b2, b2, ... as indices below: 3 -> b1, 5 -> b2
CLOSE_BEFORE = 7
REFUSE_BEFORE = (2, 6, 11)


# ---- the device side -------------------------------------------------------------------------------------------------------------------
class _Dev(object):
    def __init__(self, hip):
        from pyfft_amd import _native as N
        self.hip, self.N = hip, N
        w = ctypes.c_void_p()
        N.check(N.lib.mifft_host_alloc(ctypes.byref(w), 64), "mifft_host_alloc")
        self._word = w.value
        self._count = ctypes.c_uint64.from_address(w.value)
        self._keep = {}

    def close(self):
        self.sync()
        for a in self._keep.values():
            a.free()
        self._keep = {}
        if self._word is not None:
            self.N.lib.mifft_host_free(self._word)
            self._word = None

    def sync(self):
        self.N.check(self.N.lib.mifft_device_sync(), "mifft_device_sync")

    limit = MAX_BUFFER_BYTES

    def allow(self, nbytes):
        """this test's buffers may take `nbytes` (a case that states why it cannot keep to MAX_BUFFER_BYTES)"""
        self.limit = int(nbytes)

    def free(self, ptrs):
        """give back ranges of alloc() / upload() before the test ends (the big cases)"""
        self.sync()
        for p in ptrs:
            self._keep.pop(p).free()

    def alloc(self, nbytes, off=0, fill=None):
        """a device range of nbytes, `off` bytes past a 256-byte-aligned base; fill: a byte value"""
        assert nbytes <= self.limit, "a buffer of %d bytes: the cases keep to %d" % (nbytes, self.limit)
        a = self.hip.DeviceAllocation(nbytes + off + 16)
        self._keep[a.ptr + off] = a
        if fill is not None:
            self.N.check(self.N.lib.mifft_memset(a.ptr, fill, nbytes + off + 16, None), "mifft_memset")
        return a.ptr + off

    def upload(self, host, off=0):
        host = numpy.ascontiguousarray(host).view(numpy.uint8).reshape(-1)
        p = self.alloc(host.nbytes, off)
        H._h2d(p, host)
        return p

    def copy(self, dst, src, nbytes, stream=None):
        self.N.check(self.N.lib.mifft_memcpy_d2d(dst, src, nbytes, stream), "mifft_memcpy_d2d")

    def mismatches(self, a, b, nbytes):
        """words (device, 16 bytes) or bytes (host) in which a[0 .. nbytes) and b[0 .. nbytes) differ"""
        if nbytes > DEVICE_COMPARE_BYTES and nbytes % 16 == 0 and (a | b) % 16 == 0:
            self._count.value = 0
            self.N.check(self.N.lib.mifft_aux_count_mismatch(a, b, nbytes, self._word, None), "mifft_aux_count_mismatch")
            self.sync()
            return int(self._count.value)
        return int(numpy.count_nonzero(H._d2h_bytes(a, nbytes) != H._d2h_bytes(b, nbytes)))


@pytest.fixture
def dev(ctx):
    d = _Dev(ctx.hip)
    yield d
    d.close()


def _hold(got_of, ref_of, dtname, n, batch, levels, what):
    """the sampled items within helpers.accuracy_bound at `levels` of the extended-precision reference"""
    l1b, mxb = H.accuracy_bound(dtname, n, levels)
    for j in H.sampled_items(batch, n):
        l1, mx = H.item_error(got_of(j), ref_of(j))
        assert l1 <= l1b and mx <= mxb, "%s item %d: L1-relative %.3g (bound %.3g), max|err|/rms %.3g (bound %.3g)" % (what, j, l1, l1b, mx, mxb)


# ---- the plan kinds ----------------------------------------------------------------------------------------------------------------------
class _Kind(object):
    """One case: how its plan is built and called, what a step's buffers hold, how a result is held to the reference, which calls it
    refuses.  A step is (inverse, mode): mode is the spectrum mode of a convolution (per item or shared), False elsewhere."""
    in_place = True
    directions = (False, True)
    modes = (False,)
    env = {}
    b1, b2 = 3, 5
    pattern, close_before, refuse_before = BATCHES, CLOSE_BEFORE, REFUSE_BEFORE
    max_buffer_bytes = MAX_BUFFER_BYTES
    lazy = False            # out of place the plan takes a route without scratch: in place allocates it lazily (_Complex)

    def __init__(self, name):
        self.name = name

    def setup(self, monkeypatch):
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)

    def offset(self, i):
        return 0

    def extra(self, dev):
        return {}

    def route(self, hip):
        """assert that the device's own plan takes the strategy or form the case is about"""


class _Complex(_Kind):
    """FFTPlan / GenericFFTPlan on interleaved complex numbers or split planes"""

    def __init__(self, name, shape, dtype, expect, env=None, batches=(3, 5), parent=None, any_size=False, oop=None, short=None,
                 lazy=False):
        _Kind.__init__(self, name)
        self.lazy = lazy
        if short is not None:       # a case too big for 14 steps: (pattern, close_before, refuse_before, the size its buffers may take)
            self.pattern, self.close_before, self.refuse_before, self.max_buffer_bytes = short
        self.shape, self.dtype, self.expect, self.env, self.parent, self.any_size, self.oop = shape, numpy.dtype(dtype), expect, env or {}, \
            parent, any_size, oop
        self.b1, self.b2 = batches
        self.split = self.dtype.kind == "f"
        self.cdt = numpy.dtype(numpy.complex128 if self.dtype.itemsize * (2 if self.split else 1) == 16 else numpy.complex64)
        self.n = int(numpy.prod(shape))
        self.points = int(numpy.prod(parent)) if parent is not None else self.n
        self.planes = 2 if self.split else 1

    def kw(self):
        kw = {"dtype": self.dtype}
        if self.parent is not None:
            kw["parent_shape"] = self.parent
        if self.any_size:
            kw["any_size"] = True
        return kw

    def plan(self, hip, **more):
        return hip.Plan(self.shape, **dict(self.kw(), **more))

    def route(self, hip):
        plan = self.plan(hip)
        for b in (self.b1, self.b2):
            if self.parent is not None or self.any_size:
                import kernel_coverage as KC
                assert KC.form_of(plan) == self.expect, (self.name, KC.form_of(plan))
            else:
                assert plan.strategy(b)[0] == self.expect, (self.name, b, plan.strategy(b))
                if self.oop is not None:
                    assert plan.strategy(b, inplace=False)[0] == self.oop, (self.name, b, plan.strategy(b, inplace=False))
                    assert plan._temp_buffer_needed == self.lazy, "%s: in place %s a temp buffer" % (
                        self.name, "takes" if plan._temp_buffer_needed else "takes no")
                elif self.expect == "chain":
                    assert plan._temp_buffer_needed, "%s: the chain of this shape needs no temp buffer" % self.name
        plan.close()

    def nbytes(self, inverse, b, side):
        return b * self.points * self.cdt.itemsize // self.planes

    def host_input(self, inverse, mode, b, seed):
        z = H._tiled_noise(b * self.points, self.cdt, seed)
        return [numpy.ascontiguousarray(z.real), numpy.ascontiguousarray(z.imag)] if self.split else [z]

    def execute(self, plan, ins, outs, inverse, mode, b, **kw):
        args = list(ins) + (list(outs) if outs is not None else [])
        return plan.execute(*args, inverse=inverse, batch=b, **kw)

    def _complex(self, planes, b):
        fdt = numpy.float64 if self.cdt == numpy.complex128 else numpy.float32
        if self.split:
            return (planes[0].view(fdt) + 1j * planes[1].view(fdt)).astype(self.cdt)
        return planes[0].view(self.cdt)

    def accuracy(self, hip, inverse, mode, b, ins, outs, extra):
        x, y = self._complex(ins, b), self._complex(outs, b)
        what = "%s, fresh plan" % self.name
        if self.parent is None:
            levels = H.any_size_levels(self.shape, self.dtype) if self.any_size else None
            H.check_accuracy(self.shape, self.cdt, b, lambda j: x[j * self.n:(j + 1) * self.n], lambda j: y[j * self.n:(j + 1) * self.n],
                             inverse=inverse, what=what, levels=levels)
            return
        # tiles of a parent array: every tile of the first and the last parent array
        ty, tx = self.shape
        py, px = self.parent
        l1b, mxb = H.accuracy_bound(self.cdt, self.n)
        for j in sorted({0, b - 1}):
            X, Y = (a[j * self.points:(j + 1) * self.points].reshape(py, px) for a in (x, y))
            for r in range(0, py, ty):
                for c in range(0, px, tx):
                    ref = H.reference_fft(X[r:r + ty, c:c + tx], self.shape, self.cdt, inverse)
                    l1, mx = H.item_error(Y[r:r + ty, c:c + tx], ref)
                    assert l1 <= l1b and mx <= mxb, "%s, parent %d tile (%d, %d): %.3g (%.3g), %.3g (%.3g)" % (what, j, r, c, l1, l1b, mx, mxb)

    def refusals(self, plan, dev, out, stream):
        """complex plans take raw addresses and check no sizes: what they refuse is a batch below one; FFTPlan also one plane of a pair
        aliased (refused when the pointer triples are built, after the batch was prepared) and, interleaved, an execute that would wait
        on a recording stream (refused after the stream of the call was chosen; at a batch between b1 and b2)"""
        hip = dev.hip
        a = [dev.alloc(self.nbytes(False, self.b2, 0), fill=0) for _ in range(self.planes)]
        calls = [(lambda: plan.execute(*(a + out), batch=0), ValueError), (lambda: plan.execute(*(a + out), batch=-self.b1), ValueError)]
        generic = self.parent is not None or self.any_size
        if self.split and not generic:
            calls.append((lambda: plan.execute(a[0], a[1], a[0], out[1], batch=self.b1), ValueError))       # one plane aliased, the other not
        elif self.split:
            calls.append((lambda: plan.execute(a[0], a[1], out[0], batch=self.b1), ValueError))             # one output plane without the other
        elif not generic:
            def waits_while_recording():
                with hip.Graph(stream):
                    plan.execute(a[0], out[0], batch=self.b1 + 1, wait_for_finish=True)
            calls.append((waits_while_recording, RuntimeError))
        else:
            calls.append((lambda: plan.execute(*(a + out), batch=0, inverse=True), ValueError))
        return calls


class _Real(_Kind):
    in_place = False

    def __init__(self, name, shape, dtname):
        _Kind.__init__(self, name)
        self.shape, self.dtname = shape, dtname
        self.double = dtname == "float64"
        self.cdt = numpy.dtype(numpy.complex128 if self.double else numpy.complex64)
        self.n = int(numpy.prod(shape))
        self.sshape = shape[:-1] + (shape[-1] // 2 + 1,)
        self.spec = int(numpy.prod(self.sshape))

    def plan(self, hip, **more):
        return hip.Plan(self.shape, dtype=numpy.dtype(self.dtname), real=True, **more)

    def route(self, hip):
        plan = self.plan(hip)
        assert plan._real_form == "composed" and plan.inner_plan is not None, self.name
        plan.close()

    def nbytes(self, inverse, b, side):
        real = (side == 0) != inverse
        return b * (self.n * self.cdt.itemsize // 2 if real else self.spec * self.cdt.itemsize)

    def host_input(self, inverse, mode, b, seed):
        if inverse:
            return [H._tiled_noise(b * self.spec, self.cdt, seed)]
        return [numpy.ascontiguousarray(H._tiled_noise(b * self.n, self.cdt, seed).real)]

    def execute(self, plan, ins, outs, inverse, mode, b, **kw):
        return plan.execute(ins[0], outs[0], inverse=inverse, batch=b, **kw)

    def accuracy(self, hip, inverse, mode, b, ins, outs, extra):
        levels = self.n.bit_length() - 1
        if inverse:
            X, y = ins[0].view(self.cdt).reshape((b,) + self.sshape), outs[0].view(self.dtname).reshape((b,) + self.shape)
            _hold(lambda j: y[j], lambda j: RM.irfftn_exact(X[j], self.shape, self.double), self.dtname, self.n, b, levels, self.name + " inverse")
        else:
            x, Y = ins[0].view(self.dtname).reshape((b,) + self.shape), outs[0].view(self.cdt).reshape((b,) + self.sshape)
            _hold(lambda j: Y[j], lambda j: RM.rfftn_exact(x[j], self.double), self.dtname, self.n, b, levels, self.name + " forward")

    def refusals(self, plan, dev, out, stream):
        hip = dev.hip
        a = dev.alloc(self.nbytes(False, self.b2, 0), fill=0)
        short = hip.DeviceArray((self.nbytes(False, self.b1, 1) // 32,), numpy.complex128, allocation=_Borrowed(out[0]))     # half of what it needs
        return [(lambda: plan.execute(a, short, batch=self.b1), ValueError),                    # a short output buffer
                (lambda: plan.execute(a, batch=self.b1), ValueError),                           # a real plan in place
                (lambda: plan.execute(a, a + 16, batch=self.b1), ValueError),                   # an overlapping pair
                (lambda: plan.execute(a + 4, out[0], batch=self.b1), ValueError)]               # a base the form refuses


class _Borrowed(object):
    """DeviceArray's allocation argument for a range some other allocation owns"""

    def __init__(self, ptr):
        self.ptr = ptr


class _Conv(_Kind):
    directions = (False,)
    modes = (False, True)           # shared spectrum, one spectrum per item

    def __init__(self, name, shape, dtname):
        _Kind.__init__(self, name)
        self.shape, self.dtname = shape, dtname
        self.real = dtname.startswith("float")
        self.double = dtname in ("float64", "complex128")
        self.cdt = numpy.dtype(numpy.complex128 if self.double else numpy.complex64)
        self.n = int(numpy.prod(shape))
        self.sshape = shape[:-1] + (shape[-1] // 2 + 1,) if self.real else shape
        self.spec = int(numpy.prod(self.sshape))
        r = numpy.random.default_rng(4242)
        self.S = numpy.exp(2j * numpy.pi * r.random((self.b2 + 1,) + self.sshape)).astype(self.cdt)

    def plan(self, hip, **more):
        return hip.Plan(self.shape, dtype=numpy.dtype(self.dtname), convolve=True, real=self.real, **more)

    def route(self, hip):
        plan = self.plan(hip)
        assert plan.conv_form == "composed", self.name
        plan.close()

    def extra(self, dev):
        return {"spectrum": dev.upload(self.S)}

    def nbytes(self, inverse, b, side):
        return b * self.n * numpy.dtype(self.dtname).itemsize

    def host_input(self, inverse, mode, b, seed):
        z = H._tiled_noise(b * self.n, self.cdt, seed)
        return [numpy.ascontiguousarray(z.real) if self.real else z]

    def execute(self, plan, ins, outs, inverse, mode, b, spectrum=None, **kw):
        args = [ins[0]] + ([outs[0]] if outs is not None else [])
        return plan.execute(*args, spectrum=spectrum, batch=b, spectrum_batch=b if mode else 1, **kw)

    def accuracy(self, hip, inverse, mode, b, ins, outs, extra):
        pdt = numpy.dtype(self.dtname)
        x, y = ins[0].view(pdt).reshape((b,) + self.shape), outs[0].view(pdt).reshape((b,) + self.shape)
        _hold(lambda j: y[j], lambda j: conv_reference(x[j], self.S[j if mode else 0], self.shape, pdt, self.real), self.dtname, self.n, b,
              2 * (self.n.bit_length() - 1) + 1, "%s, %s spectrum" % (self.name, "per-item" if mode else "shared"))

    def refusals(self, plan, dev, out, stream):
        hip = dev.hip
        nb = self.nbytes(False, self.b1, 0)
        a = dev.alloc(self.nbytes(False, self.b2, 0), fill=0)
        S = dev.upload(self.S)
        short = hip.DeviceArray((nb // 2,), numpy.uint8, allocation=_Borrowed(out[0]))
        return [(lambda: plan.execute(a, short, spectrum=S, batch=self.b1), ValueError),        # a short output buffer
                (lambda: plan.execute(a, a + 16, spectrum=S, batch=self.b1), ValueError),       # an overlapping pair
                (lambda: plan.execute(a, out[0], spectrum=a, batch=self.b1), ValueError),       # the spectrum overlaps the data
                (lambda: plan.execute(a, out[0], spectrum=S, batch=self.b1, spectrum_batch=2), ValueError)]


class _R2R(_Kind):
    def __init__(self, name, shape, dtname, form, misalign=False):
        _Kind.__init__(self, name)
        self.shape, self.dtname, self.form, self.misalign = shape, dtname, form, misalign
        self.double = dtname == "float64"
        self.cdt = numpy.dtype(numpy.complex128 if self.double else numpy.complex64)
        self.n = int(numpy.prod(shape))

    def plan(self, hip, **more):
        return hip.Plan(self.shape, dtype=numpy.dtype(self.dtname), r2r="dct", **more)

    def route(self, hip):
        plan = self.plan(hip)
        assert plan.r2r_form == self.form, (self.name, plan.r2r_form)
        plan.close()

    def offset(self, i):
        """a fused row: steps 1, 2, 5, 6, 9, 10, 13 on bases 8 bytes off a 16-byte boundary -- the composed fallback and its scratch,
        allocated by the first of them and again after close()"""
        return 8 if self.misalign and ((i + 1) // 2) % 2 else 0

    def nbytes(self, inverse, b, side):
        return b * self.n * numpy.dtype(self.dtname).itemsize

    def host_input(self, inverse, mode, b, seed):
        return [numpy.ascontiguousarray(H._tiled_noise(b * self.n, self.cdt, seed).real)]

    def execute(self, plan, ins, outs, inverse, mode, b, **kw):
        args = [ins[0]] + ([outs[0]] if outs is not None else [])
        return plan.execute(*args, inverse=inverse, batch=b, **kw)

    def accuracy(self, hip, inverse, mode, b, ins, outs, extra):
        x, y = (a[0].view(self.dtname).reshape((b,) + self.shape) for a in (ins, outs))
        _hold(lambda j: y[j], lambda j: DM.reference(x[j], "dct", inverse, False, True, 1.0, double=self.double), self.dtname, self.n, b,
              dct_levels(self.shape), "%s %s" % (self.name, "inverse" if inverse else "forward"))

    def refusals(self, plan, dev, out, stream):
        hip = dev.hip
        nb = self.nbytes(False, self.b1, 0)
        a = dev.alloc(self.nbytes(False, self.b2, 0), fill=0)
        short = hip.DeviceArray((nb // 2,), numpy.uint8, allocation=_Borrowed(out[0]))
        short_in = hip.DeviceArray((nb // 2,), numpy.uint8, allocation=_Borrowed(a))
        return [(lambda: plan.execute(a, short, batch=self.b1), ValueError),                    # a short output buffer
                (lambda: plan.execute(a, a + 16, batch=self.b1), ValueError),                   # an overlapping pair
                (lambda: plan.execute(short_in, out[0], batch=self.b1), ValueError)]            # a short input buffer


class _Half(_Kind):
    def __init__(self, name, shape):
        _Kind.__init__(self, name)
        self.shape = shape
        self.n = int(numpy.prod(shape))

    def plan(self, hip, **more):
        return hip.Plan(self.shape, dtype="complex32", **more)

    def nbytes(self, inverse, b, side):
        return b * self.n * 4

    def host_input(self, inverse, mode, b, seed):
        z = H._tiled_noise(b * self.n, numpy.complex64, seed)
        return [numpy.stack([z.real, z.imag], axis=-1).astype(numpy.float16)]

    def execute(self, plan, ins, outs, inverse, mode, b, **kw):
        args = [ins[0]] + ([outs[0]] if outs is not None else [])
        return plan.execute(*args, inverse=inverse, batch=b, **kw)

    def accuracy(self, hip, inverse, mode, b, ins, outs, extra):
        x, y = (a[0].view(numpy.float16).reshape((b,) + self.shape + (2,)) for a in (ins, outs))
        want = _c64_rounded(hip, self.shape, x, b, inverse)
        for j in H.sampled_items(b, self.n):
            _check_item(self.shape, y[j], x[j], want[j], inverse, what="%s item %d" % (self.name, j))

    def refusals(self, plan, dev, out, stream):
        hip = dev.hip
        nb = self.nbytes(False, self.b1, 0)
        a = dev.alloc(self.nbytes(False, self.b2, 0), fill=0)
        short = hip.DeviceArray((nb // 4,), numpy.float16, allocation=_Borrowed(out[0]))
        wrong = hip.DeviceArray((nb // 4,), numpy.float32, allocation=_Borrowed(out[0]))
        return [(lambda: plan.execute(a, short, batch=self.b1), ValueError),                    # a short output buffer
                (lambda: plan.execute(a, a + 16, batch=self.b1), ValueError),                   # an overlapping pair
                (lambda: plan.execute(a, wrong, batch=self.b1), ValueError)]                    # a buffer of another element type


def _smallest_long():
    """the smallest length mifft_mixed_long_split takes (the library says which)"""
    from pyfft_amd import _native as N
    a, b = ctypes.c_int32(0), ctypes.c_int32(0)
    n = 4097
    while True:
        m = n
        for c in (2, 3, 5, 7):
            while m % c == 0:
                m //= c
        if m == 1 and N.lib.mifft_mixed_long_split(N.F32, n, ctypes.byref(a), ctypes.byref(b)) == 0:
            return n
        n += 1
        assert n < 1 << 20


FUSED = {"PYFFT_AMD_STRATEGY": "fused"}
C64, F32 = numpy.complex64, numpy.float32
CASES = [
    _Complex("fft-chain-temp-2^17-c64", (1 << 17,), C64, "chain"),
    _Complex("fft-chain-temp-2^17-f32-planes", (1 << 17,), F32, "chain"),
    _Complex("fft-pipelined-2^16-c64", (1 << 16,), C64, "pipelined", env={"PYFFT_AMD_STRATEGY": "pipelined", "PYFFT_AMD_PIPE_MB": "1"},
             batches=(9, 13)),
    _Complex("fft-fused2-2^16-c64", (1 << 16,), C64, "fused2", env=FUSED, batches=(9, 13)),
    _Complex("fft-fused2-2^16-f32-planes", (1 << 16,), F32, "fused2", env=FUSED, batches=(9, 13)),
    _Complex("fft-fusedp-64^3-c64", (64, 64, 64), C64, "fusedp", env=dict(FUSED, PYFFT_AMD_FUSED_RING="4,8"), batches=(17, 19)),
    # (256, 256) takes the one-launch out-of-place route only beyond half the last-level cache per side (128 MiB), and its chain needs
    # no temp buffer in place: at these batches both calls run the chain.  (16, 2048) is a smallest shape that takes the route at
    # every size.  As complex64 its chain needs no temp buffer either: the alternation switches between two routes without scratch.
    # As float32 planes the chain detours through a temp buffer (FFTPlan._via_temp): in place needs scratch, out of place does not,
    # so an out-of-place execute of a new batch commits the batch without scratch and the next in-place one allocates it lazily.
    _Complex("fft-256x256-c64", (256, 256), C64, "chain", oop="chain"),
    _Complex("fft-nd_oop-16x2048-c64", (16, 2048), C64, "chain", oop="nd_oop"),
    _Complex("fft-nd_oop-16x2048-f32-planes", (16, 2048), F32, "chain", oop="nd_oop", lazy=True),
    # the smallest shape the fused2z rule takes is 256 MiB per transform (more than half the last-level cache), from batch 2: four steps
    # on buffers of 512 and 768 MiB
    _Complex("fft-fused2z-128x512x512-c64", (128, 512, 512), C64, "fused2z", batches=(2, 3), short=((3, 5, 3, 5), 2, (1, 3), 768 << 20)),
    _Complex("generic-work-17x4-f32-planes", (17, 4), F32, "_uses_work", any_size=True),
    _Complex("generic-work-16411-c64", (16411,), C64, "_uses_work", any_size=True),
    _Complex("generic-blue-4099-c64", (4099,), C64, "_direct_blue", any_size=True),
    _Complex("generic-tiles-16x4-in-64x64-c64", (16, 4), C64, "_uses_work", parent=(64, 64)),
    _Complex("generic-long-c64", (_smallest_long(),), C64, "_direct_long", any_size=True),
    _Real("real-composed-8x16-f32", (8, 16), "float32"),
    _Real("real-composed-2^17-f64", (1 << 17,), "float64"),
    _Conv("conv-composed-16x16-c64", (16, 16), "complex64"),
    _Conv("conv-composed-8x16-f32-real", (8, 16), "float32"),
    _R2R("r2r-composed-8x8-f64", (8, 8), "float64", "composed"),
    _R2R("r2r-fused-row-256-f32-bases", (256,), "float32", "fused_row", misalign=True),
    _Half("half-128x128", (128, 128)),
]
# (the other properties: the cases whose plan owns batch-sized scratch, at sizes that keep to MAX_BUFFER_BYTES)
OWNS_SCRATCH = [c for c in CASES if not isinstance(c, _Half) and
                c.name not in ("generic-blue-4099-c64", "conv-composed-16x16-c64", "fft-256x256-c64", "fft-nd_oop-16x2048-c64", "fft-fused2z-128x512x512-c64")]
EXTENSION_CASES = [c for c in CASES if not c.name.startswith("fft-")]


def _ids(cases):
    return [c.name for c in cases]


def _steps(case):
    """(batch, inverse, mode, in place, base offset) of the 14 steps: directions (spectrum modes) alternate every step, in place and out
    of place every second step.  A lazy case the other way round: out of place, in place, out of place ..., so that the first execute of
    a batch is out of place (no scratch) and an in-place one of the same batch follows (steps 0-1, 4-5, 8-9, 10-11)."""
    out = []
    for i, b in enumerate(case.pattern):
        fast, slow = i, i // 2
        turn, place = (slow, fast + 1) if case.lazy else (fast, slow)
        out.append((case.b1 if b == 3 else case.b2, case.directions[turn % len(case.directions)], case.modes[turn % len(case.modes)],
                    case.in_place and place % 2 == 1, case.offset(i)))
    return out


def _run_fresh(dev, case, extra, step, src, ref, sides, **plan_kw):
    """the step alone and synchronously on a fresh plan, into `ref`"""
    b, inverse, mode, inplace, off = step
    fresh = case.plan(dev.hip, **plan_kw)
    try:
        if inplace:
            for r, s, nb in zip(ref, src, sides):
                dev.copy(r, s, nb)
            dev.sync()
            case.execute(fresh, ref, None, inverse, mode, b, **extra)
        else:
            case.execute(fresh, src, ref, inverse, mode, b, **extra)
        fresh.finish()
    finally:
        fresh.close()


def _planes(case):
    return getattr(case, "planes", 1)


# ---- the sequence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_every_execute_of_a_long_lived_plan_equals_a_fresh_plan(ctx, dev, monkeypatch, case):
    hip = ctx.hip
    case.setup(monkeypatch)
    case.route(hip)
    dev.allow(case.max_buffer_bytes)
    steps = _steps(case)
    extra = case.extra(dev)
    np_ = _planes(case)
    # every input and every output buffer exists before the first execute: nothing between the steps waits for the device
    hosts, srcs, outs = [], [], []
    for i, (b, inverse, mode, inplace, off) in enumerate(steps):
        host = case.host_input(inverse, mode, b, 7000 + i)
        hosts.append(host)
        srcs.append([dev.upload(h, off) for h in host])
        outs.append([dev.alloc(case.nbytes(inverse, b, 1), off, fill=0xFF) for _ in range(np_)])
    refused_out = [[dev.alloc(case.nbytes(False, case.b2, 1), fill=0xFF) for _ in range(np_)] for _ in case.refuse_before]
    dev.sync()

    s = hip.Stream()
    plan = case.plan(hip, stream=s)
    refusals = {}
    for k, i in enumerate(case.refuse_before):
        calls = case.refusals(plan, dev, refused_out[k], s)
        refusals[i] = calls[k % len(calls)], calls[(k + 1) % len(calls)]
    dev.sync()
    for i, (b, inverse, mode, inplace, off) in enumerate(steps):
        if i == case.close_before:
            plan.close()
        for call, error in refusals.get(i, ()):
            with pytest.raises(error):
                call()
        if inplace:
            for o, a in zip(outs[i], srcs[i]):
                dev.copy(o, a, case.nbytes(inverse, b, 0), s.handle)
            case.execute(plan, outs[i], None, inverse, mode, b, wait_for_finish=False, **extra)
        else:
            case.execute(plan, srcs[i], outs[i], inverse, mode, b, wait_for_finish=False, **extra)
    plan.finish()                   # (raises if a persistent kernel reported invalid results)
    s.synchronize()

    assert not plan._context.capturing()
    ones = dev.alloc(case.nbytes(False, case.b2, 1), fill=0xFF)
    for k in range(len(case.refuse_before)):
        for p in refused_out[k]:
            bad = dev.mismatches(p, ones, case.nbytes(False, case.b2, 1))
            assert bad == 0, "%s: a refused call wrote its output (%d words or bytes)" % (case.name, bad)
    checked = set()
    for i, step in enumerate(steps):
        b, inverse, mode, inplace, off = step
        nout = case.nbytes(inverse, b, 1)
        ref = [dev.alloc(nout, off, fill=0xFF) for _ in range(np_)]
        _run_fresh(dev, case, extra, step, srcs[i], ref, [case.nbytes(inverse, b, 0)] * np_)
        bad = sum(dev.mismatches(o, r, nout) for o, r in zip(outs[i], ref))
        assert bad == 0, "%s, step %d (batch %d, %s, %s%s%s): %d words differ from the fresh plan's result" % (
            case.name, i, b, "inverse" if inverse else "forward", "in place" if inplace else "out of place",
            ", per-item spectrum" if mode else "", ", base +%d" % off if off else "", bad)
        if not inplace and nout <= MAX_BUFFER_BYTES:
            for a, h in zip(srcs[i], hosts[i]):
                hb = numpy.ascontiguousarray(h).view(numpy.uint8).reshape(-1)
                assert numpy.array_equal(H._d2h_bytes(a, hb.size), hb), "%s, step %d: an out-of-place execute touched its input" % (case.name, i)
        if (inverse, mode) not in checked:
            checked.add((inverse, mode))
            got = [H._d2h_bytes(r, nout) for r in ref]
            ins = [numpy.ascontiguousarray(h).view(numpy.uint8).reshape(-1) for h in hosts[i]]
            case.accuracy(hip, inverse, mode, b, ins, got, extra)
        dev.free(ref + outs[i] + srcs[i])           # (the big case: nothing of a checked step stays on the card)
        hosts[i] = None
    assert len(plan._capture_keepalive) == 0
    plan.close()


# ---- graphs across re-plans: the extension and form classes -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXTENSION_CASES, ids=_ids(EXTENSION_CASES))
def test_recorded_graph_survives_replans_and_close(ctx, dev, monkeypatch, case):
    hip = ctx.hip
    case.setup(monkeypatch)
    extra = case.extra(dev)
    np_ = _planes(case)
    b1, b2 = case.b1, case.b2
    inverse, mode = case.directions[0], case.modes[-1]
    inplace = case.name == "generic-long-c64"             # (in place is where the long smooth transform owns scratch)
    owns = case in OWNS_SCRATCH and not getattr(case, "misalign", False)
    host = case.host_input(inverse, mode, b2, 8100)
    nin, nout = case.nbytes(inverse, b1, 0), case.nbytes(inverse, b1, 1)
    src = [dev.upload(h) for h in host]
    rec = [dev.alloc(case.nbytes(inverse, b2, 1), fill=0xFF) for _ in range(np_)]       # what the graph writes (b1 items)
    eager = [dev.alloc(nout, fill=0xFF) for _ in range(np_)]
    other = [dev.alloc(case.nbytes(inverse, b2, 1), fill=0xFF) for _ in range(np_)]
    s = hip.Stream()
    plan = case.plan(hip, stream=s)

    def run(dst, b):
        if inplace:
            for o, a in zip(dst, src):
                dev.copy(o, a, case.nbytes(inverse, b, 0), s.handle)
            case.execute(plan, dst, None, inverse, mode, b, wait_for_finish=False, **extra)
        else:
            case.execute(plan, src, dst, inverse, mode, b, wait_for_finish=False, **extra)

    def replay_and_compare(what):
        for p in rec:
            dev.N.check(dev.N.lib.mifft_memset(p, 0xFF, nout, s.handle), "mifft_memset")
        if inplace:
            for o, a in zip(rec, src):
                dev.copy(o, a, nin, s.handle)
        graph.launch()
        s.synchronize()
        bad = sum(dev.mismatches(r, e, nout) for r, e in zip(rec, eager))
        assert bad == 0, "%s: the replay %s differs from the eager result in %d words" % (case.name, what, bad)

    run(eager, b1)                                          # 1. eager at b1, then record it
    s.synchronize()
    with hip.Graph(s) as graph:
        if inplace:
            case.execute(plan, rec, None, inverse, mode, b1, wait_for_finish=False, **extra)
        else:
            case.execute(plan, src, rec, inverse, mode, b1, wait_for_finish=False, **extra)
    assert len(plan._capture_keepalive) == 0
    replay_and_compare("after the recording")
    run(other, b2)                                          # 2. eager at b2 (re-prepare), then replay
    s.synchronize()
    assert len(plan._capture_keepalive) <= 1
    replay_and_compare("after a re-prepare for another batch")
    plan.close()                                            # 3. close(), then replay
    assert len(plan._capture_keepalive) <= 2
    replay_and_compare("after close()")
    run(other, b1)                                          # 4. eager at b1 again, then replay
    s.synchronize()
    replay_and_compare("after the batch was prepared again")
    kept = len(plan._capture_keepalive)
    assert kept <= 2, kept
    # a batch that was never run eagerly: refused where the plan would allocate, the capture ends cleanly, the first graph still replays
    b3 = b2 + 1
    src3 = [dev.alloc(case.nbytes(inverse, b3, 0), fill=0) for _ in range(np_)]
    dst3 = [dev.alloc(case.nbytes(inverse, b3, 1), fill=0xFF) for _ in range(np_)]
    if owns:
        with pytest.raises(RuntimeError, match="needs one eager execute"):
            with hip.Graph(s):
                case.execute(plan, dst3 if inplace else src3, None if inplace else dst3, inverse, mode, b3, wait_for_finish=False, **extra)
        assert not plan._context.capturing(), "the stream still records after the refused execute"
        assert len(plan._capture_keepalive) == kept
        s.synchronize()
        for p in dst3:
            raw = H._d2h_bytes(p, case.nbytes(inverse, b3, 1))
            assert (raw == 0xFF).all(), "%s: the refused recording wrote its output" % case.name
        replay_and_compare("after a refused recording")
    plan.release_captured()
    assert len(plan._capture_keepalive) == 0
    # uncaptured batch changes keep nothing alive
    for k in range(20):
        run(other, b1 if k % 2 else b2)
    plan.finish()
    assert len(plan._capture_keepalive) == 0
    plan.close()


# ---- a failed allocation, recovered ----------------------------------------------------------------------------------------------------
class _Pool(object):
    """A mempool that counts, can be told to fail its next allocate(), and tracks its live blocks: each block calls back when the
    plan lets go of it (`on_release(block)`: the hook of the early-return test)."""

    class Block(object):
        def __init__(self, pool, hip, nbytes):
            self._pool, self._alloc = pool, hip.DeviceAllocation(nbytes)
            self.ptr, self.nbytes = self._alloc.ptr, int(nbytes)

        def __int__(self):
            return self.ptr

        def __del__(self):
            pool = self._pool
            pool.live -= 1
            if pool.on_release is not None:
                pool.on_release(self)

    def __init__(self, hip):
        self.hip, self.calls, self.live, self.fail_next, self.on_release = hip, 0, 0, False, None

    def allocate(self, nbytes):
        self.calls += 1
        if self.fail_next:
            self.fail_next = False
            raise MemoryError("the pool is out of memory (on request)")
        self.live += 1
        return _Pool.Block(self, self.hip, nbytes)


@pytest.mark.parametrize("case", OWNS_SCRATCH, ids=_ids(OWNS_SCRATCH))
def test_failed_allocation_is_recovered(ctx, dev, monkeypatch, case):
    """b_large first: stale scratch could only be too big, never too small, so even a regressed build writes nothing out of range here.
    The detector is the host-side call count: the plan must ask the pool again after the failure."""
    hip = ctx.hip
    case.setup(monkeypatch)
    extra = case.extra(dev)
    np_ = _planes(case)
    inverse, mode = case.directions[0], case.modes[-1]
    inplace = case.name == "generic-long-c64" or case.lazy
    off = 8 if getattr(case, "misalign", False) else 0
    small, large = case.b1, case.b2
    scrap = [dev.alloc(case.nbytes(inverse, large, 1), off, fill=0xFF) for _ in range(np_)] if case.lazy else None
    src = [dev.upload(h, off) for h in case.host_input(inverse, mode, large, 8200)]
    nin, nout = case.nbytes(inverse, small, 0), case.nbytes(inverse, small, 1)
    dst = [dev.alloc(case.nbytes(inverse, large, 1), off, fill=0xFF) for _ in range(np_)]
    pool = _Pool(hip)
    plan = case.plan(hip, mempool=pool)

    def run(b):
        if case.lazy:
            # out of place first: the one-launch route commits the batch (and lets go of the other batch's temp buffer) without asking
            # for scratch; the in-place execute below then allocates it with the batch already current
            asked = pool.calls
            case.execute(plan, src, scrap, inverse, mode, b, **extra)
            assert pool.calls == asked and plan._last_batch_size == b and plan._tempmemobj is None and not plan._scratch_ready
        if inplace:
            for o, a in zip(dst, src):
                dev.copy(o, a, case.nbytes(inverse, b, 0))
            dev.sync()
            case.execute(plan, dst, None, inverse, mode, b, **extra)
        else:
            case.execute(plan, src, dst, inverse, mode, b, **extra)

    run(large)
    assert pool.calls >= 1, "%s: the case owns no pooled scratch" % case.name
    before = pool.calls
    pool.fail_next = True
    with pytest.raises(MemoryError):
        run(small)
    assert pool.calls == before + 1
    run(small)
    plan.finish()
    # a fresh plan's one execute of that batch says how many blocks the batch takes: the retry must have asked for every one of them
    ref = [dev.alloc(nout, off, fill=0xFF) for _ in range(np_)]
    fresh_pool = _Pool(hip)
    _run_fresh(dev, case, extra, (small, inverse, mode, inplace, off), src, ref, [nin] * np_, mempool=fresh_pool)
    assert fresh_pool.calls >= 1
    assert pool.calls - (before + 1) == fresh_pool.calls, "%s: after the failed allocation the plan asked for %d blocks at batch %d, a fresh " \
        "plan asks for %d: it ran on scratch of another batch" % (case.name, pool.calls - (before + 1), small, fresh_pool.calls)
    bad = sum(dev.mismatches(o, r, nout) for o, r in zip(dst, ref))
    assert bad == 0, "%s: %d words differ from the fresh plan's result after the recovered failure" % (case.name, bad)
    plan.close()
    assert pool.live == 0, "%s: %d pooled blocks alive after close()" % (case.name, pool.live)


# ---- no early return of pooled scratch ---------------------------------------------------------------------------------------------------
_cycles_per_second = []


def _sleep_cycles(seconds):
    """the argument of torch.cuda._sleep for `seconds` of device time: the counter it spins on is measured once (its rate differs
    between devices)"""
    import torch
    if not _cycles_per_second:
        probe = 2000000
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        e1.synchronize()
        _cycles_per_second.append(probe / max(e0.elapsed_time(e1) * 1e-3, 1e-6))
    return int(seconds * _cycles_per_second[0])


@pytest.mark.parametrize("how", ["batch-change", "close"])
@pytest.mark.parametrize("case", OWNS_SCRATCH, ids=_ids(OWNS_SCRATCH))
def test_pooled_scratch_is_not_returned_while_an_execute_is_pending(ctx, dev, monkeypatch, case, how):
    """The plan's stream first waits for an event behind a long sleep on another stream, so the execute is certainly pending when the
    host changes the batch (or closes the plan).  Every block the pool gets back is checked against an event recorded right after the
    execute: a release while that event is incomplete is the defect.  The check reads the event, never the data."""
    import torch
    hip, N = ctx.hip, dev.N
    case.setup(monkeypatch)
    extra = case.extra(dev)
    np_ = _planes(case)
    inverse, mode = case.directions[0], case.modes[-1]
    inplace = case.name == "generic-long-c64" or case.lazy
    off = 8 if getattr(case, "misalign", False) else 0
    b1, b2 = case.b1, case.b2
    scrap = [dev.alloc(case.nbytes(inverse, b2, 1), off, fill=0xFF) for _ in range(np_)] if case.lazy else None
    src = [dev.upload(h, off) for h in case.host_input(inverse, mode, b2, 8300)]
    dst = [dev.alloc(case.nbytes(inverse, b2, 1), off, fill=0xFF) for _ in range(np_)]
    if inplace:
        for o, a in zip(dst, src):
            dev.copy(o, a, case.nbytes(inverse, b2, 0))
    dev.sync()
    pool = _Pool(hip)
    s = hip.Stream()
    plan = case.plan(hip, stream=s, mempool=pool)

    def run(b, oop_first=case.lazy):
        if oop_first:             # (a lazy case: the batch is committed by an out-of-place execute, the scratch allocated by the in-place one)
            case.execute(plan, src, scrap, inverse, mode, b, wait_for_finish=False, **extra)
        case.execute(plan, dst if inplace else src, None if inplace else dst, inverse, mode, b, wait_for_finish=False, **extra)

    run(b1)                       # scratch of b1 exists
    plan.finish()
    assert pool.live >= 1, "%s: the case owns no pooled scratch" % case.name
    early = []
    done = hip.Event()

    def on_release(block):
        if N.lib.mifft_event_query(done.handle) != 0:
            early.append(block.nbytes)

    side = torch.cuda.Stream()
    gate = hip.Event()
    with torch.cuda.stream(side):
        torch.cuda._sleep(_sleep_cycles(0.2))             # two tenths of a second of device time on the side stream
    gate.record(side)
    N.check(N.lib.mifft_stream_wait_event(s.handle, gate.handle), "mifft_stream_wait_event")
    run(b1, oop_first=False)      # pending behind the gate, on the scratch of b1
    done.record(s)
    pending = N.lib.mifft_event_query(done.handle) != 0
    pool.on_release = on_release
    if how == "close":
        plan.close()
        assert pool.live == 0, "%s: %d pooled blocks alive after close()" % (case.name, pool.live)
    else:
        run(b2)                   # the batch changes: the scratch of b1 goes back to the pool
    pool.on_release = None
    plan.finish()
    side.synchronize()
    assert pending, "the blocker did not hold the execute back: the test saw nothing"
    assert not early, "%s: %s returned pooled scratch (%s bytes) while an execute on it was still pending" % (case.name, how, early)
    plan.close()
    assert pool.live == 0
