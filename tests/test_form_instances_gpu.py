"""The four forms added after the per-instance contract -- Plan(real=True), Plan(dtype="complex32"), Plan(convolve=True) and
Plan(r2r="dct" | "dst") -- held to it (docs/parity.md), as tests/test_instances_gpu.py and tests/test_extension_instances_gpu.py hold the
complex kernels: one case per form key (kernel_coverage.form_audit_cases(): every one-launch real, convolution and cosine / sine row, the
real separation / packing launch by lanes and rank, the spectrum product's vector and scalar paths with shared and per-item spectra and
correlation, the r2r permutation and twiddle steps by rank and path, every complex32 instance), the smallest shape that reaches the key,
at a batch that leaves the last work-group of a launch partly filled.  Each case runs through the plan itself, with its own tables, and
asserts that the device's plan takes the case's keys.  Per direction (real, r2r, complex32: forward, then inverse on fresh data; a
convolution has one):

  1. out of place, into an output pre-filled with all-ones bytes: every guard intact (the spectrum's too), the input and the spectrum
     bit-identical afterwards, every sampled item within helpers.accuracy_bound of the form's extended-precision reference at the form's
     levels -- real log2 n, convolution 2 log2 n + 1 (test_conv_gpu.bound), r2r dct_cases.levels; complex32 test_half_gpu._check_item (the
     fp16 bound and one fp16 ulp of the complex64 plan).  A convolution runs all four spectrum variants (shared / per item, correlating
     or not) through this step; the per-item correlation carries the other steps
  2. the same execute again: bit-identical
  3. in place: bit-identical to step 1 (a composed convolution whose inner plan takes another instance out of place: within the bound);
     real plans refuse aliasing with a ValueError
  4. poisoned items (helpers._poison_layouts: NaN and +Inf, the middle and the last item, then every even one): every other item
     bit-identical to step 1; a per-item spectrum with one item poisoned: only that item's output changes
  5. bases that are whole elements but not 16-byte aligned: the output, then the input, 8 bytes past the case's base (fp32 real input 4
     bytes too), with the outcome BASES gives -- accepted and bit-identical to step 1, accepted through the composed form within the
     bound (fused r2r rows), or a ValueError before anything is enqueued with the output still holding its pre-filled bytes
Then an inverse with normalize=False, scale=3.0 through a second plan (a convolution: its one transform), and r2r both ways with
ortho=True.  Each case reports its worst error ratios per step (metric / (u (L + 2)); complex32: metric / (2^-11 + u (L + 2))) and the
outcome of every base as junit properties."""
import numpy
import pytest

import dct_model as DM
import kernel_coverage as KC
import real_model as RM
from dct_cases import levels as dct_levels
from helpers import SidedCase, _poison_layouts, accuracy_bound, item_error, reference_fft, sampled_items, unit_roundoff
from test_conv_gpu import _unit_spectrum, reference as conv_reference
from test_half_gpu import F16_UNIT, _as_complex, _c64_rounded, _check_item, _half_data

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:record_property is incompatible with junit_family")]    # (the properties are written)

CASES = KC.form_audit_cases()
OOP_OWN_INSTANCE = ("nd_oop", "nd2z", "nd2zp")   # keys of instances only out-of-place executes of a complex plan run

# The bases each form variant accepts, per side (docs/extensions.md, "Element-aligned bases"): "complex" = one complex number of the
# precision, "real" = one real number, 16 = 16 bytes, "fallback" = any whole element (a fused r2r row runs the composed form there).  A
# base a variant does not accept is a ValueError raised before anything is enqueued.
#   (form, variant)                              (data side, spectrum side)
BASES = {
    ("real", "fused_row"):                      ("complex", "complex"),     # the one-launch real row
    ("real", "composed"):                       (16, "complex"),            # the inner complex plan reads / writes the real side
    ("real", "composed, no inner plan"):        ("complex", "complex"),     # nx = 2: the packing launch alone
    ("conv", "fused_row"):                      ("complex", "complex"),     # the one-launch convolution row
    ("conv", "composed"):                       (16, "complex"),            # the inner complex plan on x and y, then the product
    ("conv", "composed real, fused inner"):     ("complex", "complex"),     # the inner real plan: its row / packing launch on x and y
    ("conv", "composed real, composed inner"):  (16, "complex"),
    ("r2r", "fused_row"):                       ("fallback", None),
    ("r2r", "composed"):                        ("real", None),             # the pre / post steps; the inner plan runs on scratch
    ("half", "one launch"):                     (16, None),
}


def variant_of(form, plan):
    if form == "real":
        return "composed, no inner plan" if plan._real_form == "composed" and plan.inner_plan is None else plan._real_form
    if form == "conv":
        if plan.conv_form == "fused_row" or not plan._real:
            return plan.conv_form
        inner = plan.inner_plan
        return "composed real, %s inner" % ("fused" if inner.real_side_alignment != 16 else "composed")
    if form == "r2r":
        return plan.r2r_form
    return "one launch"


def outcome(need, off, csize, rsize):
    """"same" (accepted, the kernels of the aligned run), "bound" (accepted through another form) or "refused", for a base `off` bytes
    past a 16-byte boundary"""
    if need == "fallback":
        return "bound"
    align = {"complex": csize, "real": rsize}.get(need, need)
    return "same" if off % align == 0 else "refused"


def _case_id(case):
    form, shape, dtname, batch, kind, keys = case
    return "-".join(str(v).replace(" ", "") for v in keys[0]) + ("+%d" % (len(keys) - 1) if len(keys) > 1 else "") + \
        "-%s-%s%s" % ("x".join(map(str, shape)), dtname, "-" + kind if kind else "")


class _Form(SidedCase):
    """A case of a form with two directions (real, r2r, complex32)"""
    DIRECTIONS = (False, True)

    def __init__(self, hip, case, index):
        form, shape, dtname, batch, kind, keys = case
        SidedCase.__init__(self, hip, shape, batch, index)
        self.form, self.dtname, self.kind, self.keys = form, dtname, kind, keys
        self.double = dtname in ("float64", "complex128")
        self.rsize = 8 if self.double else 4
        self.csize = 2 * self.rsize
        self.cdt = numpy.dtype(numpy.complex128 if self.double else numpy.complex64)
        self.plans, self.ratios, self.base_log = [], [], []
        self.plan = self.make_plan()
        have = KC.form_keys_of_plan(form, self.plan, dtname, batch, kind)
        lost = [k for k in keys if k not in have]
        assert not lost, "the device's plan does not take %r at batch %d: it takes %r" % (lost, batch, sorted(have, key=str))
        self.variant = variant_of(form, self.plan)

    def make_plan(self, **kw):
        args = dict(self.plan_kw())
        args.update(kw)
        p = self.hip.Plan(self.shape, **args)
        self.plans.append(p)
        return p

    def close(self):
        SidedCase.close(self)
        for p in self.plans:
            p.close()

    def execute(self, plan, src, dst, inverse, **kw):
        if dst is None:
            plan.execute(src, inverse=inverse, batch=self.batch)
        else:
            plan.execute(src, dst, inverse=inverse, batch=self.batch)

    def items(self, got, ref_of, levels, what):
        """every sampled item of got within accuracy_bound (the form's levels) of ref_of(j); returns the worst ratios"""
        l1b, mxb = accuracy_bound(self.dtname, self.n, levels)
        unit = unit_roundoff(self.dtname) * (levels + 2)
        w1 = wm = 0.0
        for j in sampled_items(self.batch, self.n):
            l1, mx = item_error(got[j], ref_of(j))
            assert l1 <= l1b and mx <= mxb, "%s item %d: L1-relative %.3g (bound %.3g), max|err|/rms %.3g (bound %.3g)" % (
                what, j, l1, l1b, mx, mxb)
            w1, wm = max(w1, l1 / unit), max(wm, mx / unit)
        return w1, wm

    # -- the steps
    def contract(self):
        for inverse in self.DIRECTIONS:
            d = "inverse" if inverse else "forward"
            x = self.data(inverse, 101 + inverse)
            ref = self.run(self.plan, inverse, x, what=d + ", out of place")                                  # 1.
            self.ratios.append((d,) + self.check(inverse, x, self.decode(inverse, ref), what=d + ", out of place"))
            again = self.run(self.plan, inverse, x, what=d + ", again")                                      # 2.
            assert numpy.array_equal(again, ref), "%s: a repeated execute is not bit-identical" % d
            self.in_place(inverse, x, ref, d)                                                                 # 3.
            for layout in _poison_layouts(self.batch):                                                        # 4.
                got = self.run(self.plan, inverse, self.poisoned(x, layout), what=d + ", poisoned")
                changed = self.changed(got, ref, layout)
                assert not changed, "%s: items %r changed when items %r were poisoned" % (d, changed[:20], sorted(layout)[:20])
            self.bases(inverse, x, ref, d)                                                                    # 5.
        p3 = self.make_plan(normalize=False, scale=3.0)
        x = self.data(True, 303)
        got = self.run(p3, True, x, what="inverse, normalize off, scale 3")
        self.ratios.append(("scaled_inverse",) + self.check(True, x, self.decode(True, got), normalize=False, scale=3.0,
                                                              what="inverse, normalize off, scale 3"))

    def in_place(self, inverse, x, ref, d):
        got = self.run(self.plan, inverse, x, inplace=True, what=d + ", in place")
        assert numpy.array_equal(got, ref), "%s: in place is not bit-identical to out of place" % d

    def bases(self, inverse, x, ref, d, **kw):
        sides = self.sides(inverse)
        runs = []
        if self.elem(sides[1]) <= 8:
            runs.append(("output", 8))
        if self.elem(sides[0]) <= 8:
            runs.append(("input", 8))
        if self.elem(sides[0]) == 4 and self.real_input(inverse):
            runs.append(("input", 4))
        need = BASES[(self.form, self.variant)]
        for which, off in runs:
            side = sides[0 if which == "input" else 1]
            res = outcome(need[0 if side == "data" else 1], off, self.csize, self.rsize)
            what = "%s, %s base %d bytes off (%s)" % (d, which, off, res)
            got = self.run(self.plan, inverse, x, off_in=self.off_in + (off if which == "input" else 0),
                           off_out=self.off_out + (off if which == "output" else 0), refused=res == "refused", what=what, **kw)
            self.base_log.append("%s:%s+%d:%s" % (d, which, off, res))
            if res == "same":
                assert numpy.array_equal(got, ref), "%s: not bit-identical to the aligned run" % what
            elif res == "bound":
                self.ratios.append((d + "_fallback",) + self.check(inverse, x, self.decode(inverse, got), what=what))


class _Real(_Form):
    def plan_kw(self):
        return {"dtype": numpy.dtype(self.dtname), "real": True}

    def sshape(self):
        return self.shape[:-1] + (self.shape[-1] // 2 + 1,)

    def sides(self, inverse):
        return ("spectrum", "data") if inverse else ("data", "spectrum")

    def elem(self, side):
        return self.rsize if side == "data" else self.csize

    def real_input(self, inverse):
        return not inverse

    def data(self, inverse, seed):
        r = numpy.random.default_rng(seed)
        if not inverse:
            return r.standard_normal((self.batch,) + self.shape).astype(self.dtname)
        s = (self.batch,) + self.sshape()
        return (r.standard_normal(s) + 1j * r.standard_normal(s)).astype(self.cdt)

    def out_bytes(self, inverse):
        return self.batch * (self.n * self.rsize if inverse else int(numpy.prod(self.sshape())) * self.csize)

    def decode(self, inverse, raw):
        if inverse:
            return raw.view(self.dtname).reshape((self.batch,) + self.shape)
        return raw.view(self.cdt).reshape((self.batch,) + self.sshape())

    def check(self, inverse, x, got, normalize=True, scale=1.0, what=""):
        levels = self.n.bit_length() - 1
        if inverse:
            f = numpy.longdouble(1 if normalize else self.n) / numpy.longdouble(scale)
            return self.items(got, lambda j: RM.irfftn_exact(x[j], self.shape, self.double) * f, levels, what)
        return self.items(got, lambda j: RM.rfftn_exact(x[j], self.double) * scale, levels, what)

    def in_place(self, inverse, x, ref, d):
        a = self.buf("in", x.nbytes, self.off_in)
        for args in ((a.ptr, a.ptr), (a.ptr,)):
            with pytest.raises(ValueError):
                self.plan.execute(*args, inverse=inverse, batch=self.batch)


class _R2R(_Form):
    def plan_kw(self):
        return {"dtype": numpy.dtype(self.dtname), "r2r": self.kind}

    def sides(self, inverse):
        return ("data", "data")

    def elem(self, side):
        return self.rsize

    def real_input(self, inverse):
        return True

    def data(self, inverse, seed):
        return numpy.random.default_rng(seed).standard_normal((self.batch,) + self.shape).astype(self.dtname)

    def out_bytes(self, inverse):
        return self.batch * self.n * self.rsize

    def decode(self, inverse, raw):
        return raw.view(self.dtname).reshape((self.batch,) + self.shape)

    def check(self, inverse, x, got, normalize=True, scale=1.0, ortho=False, what=""):
        return self.items(got, lambda j: DM.reference(x[j], self.kind, inverse, ortho, normalize, scale, double=self.double),
                          dct_levels(self.shape), what)

    def contract(self):
        _Form.contract(self)
        po = self.make_plan(ortho=True)
        for inverse in (False, True):
            d = "ortho_" + ("inverse" if inverse else "forward")
            x = self.data(inverse, 404 + inverse)
            got = self.run(po, inverse, x, what=d)
            self.ratios.append((d,) + self.check(inverse, x, self.decode(inverse, got), ortho=True, what=d))


class _Half(_Form):
    def plan_kw(self):
        return {"dtype": "complex32"}

    def sides(self, inverse):
        return ("data", "data")

    def elem(self, side):
        return 4

    def real_input(self, inverse):
        return False

    def data(self, inverse, seed):
        return _half_data(self.shape, self.batch, seed)

    def out_bytes(self, inverse):
        return self.batch * self.n * 4

    def decode(self, inverse, raw):
        return raw.view(numpy.float16).reshape((self.batch,) + self.shape + (2,))

    def check(self, inverse, x, got, normalize=True, scale=1.0, what=""):
        want = _c64_rounded(self.hip, self.shape, x, self.batch, inverse, normalize, scale)
        unit = F16_UNIT + unit_roundoff(numpy.complex64) * (self.n.bit_length() - 1 + 2)
        w1 = wm = 0.0
        for j in sampled_items(self.batch, self.n):
            _check_item(self.shape, got[j], x[j], want[j], inverse, normalize, scale, what="%s item %d" % (what, j))
            ref = reference_fft(_as_complex(x[j]), self.shape, numpy.complex64, inverse, normalize, scale)
            l1, mx = item_error(_as_complex(got[j]), ref)
            w1, wm = max(w1, l1 / unit), max(wm, mx / unit)
        return w1, wm


CONV_VARIANTS = ((True, True), (False, False), (False, True), (True, False))    # (per-item spectrum, correlate); the first carries the steps


class _Conv(_Form):
    DIRECTIONS = (False,)

    def __init__(self, hip, case, index):
        self.real = case[2].startswith("float")
        _Form.__init__(self, hip, case, index)
        self.sshape = self.shape[:-1] + (self.shape[-1] // 2 + 1,) if self.real else self.shape

    def plan_kw(self):
        return {"dtype": numpy.dtype(self.dtname), "convolve": True, "real": self.real}

    def sides(self, inverse):
        return ("data", "data")

    def elem(self, side):
        return self.rsize if self.real else self.csize

    def real_input(self, inverse):
        return self.real

    def data(self, inverse, seed):
        r = numpy.random.default_rng(seed)
        s = (self.batch,) + self.shape
        if self.real:
            return r.standard_normal(s).astype(self.dtname)
        return (r.standard_normal(s) + 1j * r.standard_normal(s)).astype(self.dtname)

    def out_bytes(self, inverse):
        return self.batch * self.n * numpy.dtype(self.dtname).itemsize

    def decode(self, inverse, raw):
        return raw.view(self.dtname).reshape((self.batch,) + self.shape)

    def execute(self, plan, src, dst, inverse, spectrum=None, per_item=True, correlate=True):
        kw = dict(spectrum=spectrum, batch=self.batch, correlate=correlate, spectrum_batch=self.batch if per_item else 1)
        if dst is None:
            plan.execute(src, **kw)
        else:
            plan.execute(src, dst, **kw)

    def check(self, inverse, x, got, normalize=True, scale=1.0, per_item=True, correlate=True, S=None, what=""):
        S = self.S[per_item] if S is None else S
        pdt = numpy.dtype(self.dtname)

        def ref(j):
            s = S[j if per_item else 0]
            return conv_reference(x[j], numpy.conj(s) if correlate else s, self.shape, pdt, self.real, normalize, scale)
        return self.items(got, ref, 2 * (self.n.bit_length() - 1) + 1, what)

    def oop_differs(self):
        """a composed complex convolution whose inner plan runs an instance of its own out of place: in place is held to the bound"""
        if self.plan.conv_form != "composed" or self.real:
            return False
        return any(k[0] in OOP_OWN_INSTANCE for k in KC.keys_of_plan(self.plan.inner_plan, self.batch))

    def contract(self):
        x = self.data(False, 101)
        self.S = dict((p, _unit_spectrum(self.sshape, numpy.dtype(self.dtname).type, self.batch if p else 1, 7)) for p in (False, True))
        ref = None
        for per_item, correlate in CONV_VARIANTS:                                                             # 1.
            name = ("per_item" if per_item else "shared") + ("_correlate" if correlate else "")
            got = self.run(self.plan, False, x, spec=(self.S[per_item], self.off_spec), per_item=per_item, correlate=correlate,
                           what="out of place, " + name)
            self.ratios.append(("forward_" + name,) + self.check(False, x, self.decode(False, got), per_item=per_item,
                                                                  correlate=correlate, what="out of place, " + name))
            if ref is None:
                ref = got
        spec = (self.S[True], self.off_spec)
        assert numpy.array_equal(self.run(self.plan, False, x, spec=spec, what="again"), ref), "a repeated execute is not bit-identical"
        got = self.run(self.plan, False, x, inplace=True, spec=spec, what="in place")                          # 3.
        if self.oop_differs():
            self.ratios.append(("in_place",) + self.check(False, x, self.decode(False, got), what="in place"))
        else:
            assert numpy.array_equal(got, ref), "in place is not bit-identical to out of place"
        for layout in _poison_layouts(self.batch):                                                            # 4.
            got = self.run(self.plan, False, self.poisoned(x, layout), spec=spec, what="poisoned")
            changed = self.changed(got, ref, layout)
            assert not changed, "items %r changed when items %r were poisoned" % (changed[:20], sorted(layout)[:20])
        j = self.batch // 2
        Sp = self.poisoned(self.S[True], {j: (0, numpy.nan)})
        got = self.run(self.plan, False, x, spec=(Sp, self.off_spec), what="one spectrum item poisoned")
        changed = self.changed(got, ref, (j,))
        assert not changed, "items %r changed when the spectrum of item %d was poisoned" % (changed[:20], j)
        self.bases(False, x, ref, "forward", spec=spec)                                                       # 5.
        p3 = self.make_plan(normalize=False, scale=3.0)
        x3 = self.data(False, 303)
        got = self.run(p3, False, x3, spec=spec, what="normalize off, scale 3")
        self.ratios.append(("scaled",) + self.check(False, x3, self.decode(False, got), normalize=False, scale=3.0,
                                                      what="normalize off, scale 3"))


FORM_CLASSES = {"real": _Real, "conv": _Conv, "r2r": _R2R, "half": _Half}


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_form_instance(ctx, case, record_property):
    c = None
    try:
        c = FORM_CLASSES[case[0]](ctx.hip, case, CASES.index(case))
        record_property("keys", repr(list(case[5])))
        record_property("variant", c.variant)
        record_property("base_offsets", "%d/%d" % (c.off_in, c.off_out))
        c.contract()
        record_property("bases", " ".join(c.base_log))
        for step, l1, mx in c.ratios:
            record_property(step + "_l1_ratio", "%.4g" % l1)
            record_property(step + "_max_ratio", "%.4g" % mx)
    finally:
        if c is not None:
            c.close()
