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

test_instance_sides holds the same kernels to the same contract on each buffer SIDE a plan's schedule can give them.  A key does not
say which side of a launch holds split planes and which the interleaved temp buffer, nor whether the launch reads and writes one buffer;
the dispatcher and the kernels branch on both (kernel_coverage.launch_sides_of_plan).  One case per (key, sides) that no case of
test_instance launches in either placement (kernel_coverage.sides_audit_cases(): the smallest, out of place or in place as the pair
needs); a pair that arises in place runs steps 2-4 in place on the guarded buffer, held to the bound itself.

Each case reports the worst item's error ratios (metric / (u (L + 2))) as junit properties (`record_property`): a `--junitxml` run
yields the per-key table."""
import numpy
import pytest

import kernel_coverage as KC
from helpers import _Case, run_contract

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:record_property is incompatible with junit_family")]    # (the properties are written)

CASES = KC.audit_cases()
OOP_OWN_INSTANCE = ("nd_oop", "nd2z", "nd2zp")   # keys of instances only out-of-place executes run


def _case_id(case):
    keys = case[3]
    return "-".join(str(v).replace(" ", "_") for v in keys[0]) + ("+%d" % (len(keys) - 1) if len(keys) > 1 else "")


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
        # an out-of-place execute of this plan may run another instance (a several-work-groups-per-transform kernel) than an in-place one:
        # then the in-place executes get the whole contract too
        inplace_too = any(k[0] in OOP_OWN_INSTANCE for k in have)
        run_contract(plan, c, inplace_too, record_property)
    finally:
        if c is not None:
            c.close()
        if plan is not None:
            plan.close()


SIDES_CASES = KC.sides_audit_cases()


def _sides_id(case):
    inplace, pairs = case[3], case[4]
    key, sides = pairs[0]
    names = ("planes" if sides[0] else "il") + "_" + ("planes" if sides[1] else "il") + ("_aliased" if sides[2] else "")
    return "-".join(str(v).replace(" ", "_") for v in key) + "-" + names + ("+%d" % (len(pairs) - 1) if len(pairs) > 1 else "") + \
        ("-ip" if inplace else "-oop")


@pytest.mark.parametrize("case", SIDES_CASES, ids=_sides_id)
def test_instance_sides(ctx, case, record_property):
    from pyfft_amd import _native as N
    hip = ctx.hip
    shape, dtname, batch, inplace, pairs = case
    plan, c = None, None
    try:
        plan = hip.Plan(tuple(shape), dtype=numpy.dtype(dtname))
        have = KC.launch_sides_of_plan(plan, batch, inplace)
        lost = [p for p in pairs if p not in have]
        assert not lost, "the device's planner does not launch %r at batch %d %s (device %r, model %r): it launches %r" % (
            lost, batch, "in place" if inplace else "out of place", plan._context.machine, KC.full_machine(), sorted(have, key=str))
        c = _Case(hip, N, case, SIDES_CASES.index(case))
        record_property("pairs", repr(list(pairs)))
        record_property("placement", "ip" if inplace else "oop")
        record_property("base_offsets", "%d/%d" % (c.ins[0].offset, c.outs[0].offset))
        # a pair that arises in place: the in-place executes get the whole contract (as where out of place runs another instance)
        inplace_too = inplace or any(k[0] in OOP_OWN_INSTANCE for k in KC.keys_of_plan(plan, batch))
        run_contract(plan, c, inplace_too, record_property)
    finally:
        if c is not None:
            c.close()
        if plan is not None:
            plan.close()
