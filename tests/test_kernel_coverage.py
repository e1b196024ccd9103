"""CPU test of the rule "every kernel instance a default plan can select runs in the default GPU suite" (tests/kernel_coverage.py).

The planner itself (passes.build_chain, FFTPlan._select_strategy on the model of the full MI355X) enumerates what default plans launch
for every power-of-two shape of up to 2^24 points in the four dtypes -- rows, strided passes, one-launch N-D shapes, pass pairs, persistent
launches by tuning rule, the several-work-groups-per-transform kernels of out-of-place executes -- and the same planner says what each
default-collected GPU test case launches.  The reference covers its kernels by shape sweeps too: test/test_errors.py:125-145."""
import numpy

import kernel_coverage as KC
from pyfft_amd import _native as N


def test_every_kernel_instance_a_default_plan_selects_has_a_default_gpu_test():
    uni = KC.universe()
    cov = KC.covered_keys()
    kinds = {}
    for k in uni:
        kinds[k[0]] = kinds.get(k[0], 0) + 1
    # the enumeration reaches every family (a planner change that silently drops one would make the rule vacuous)
    assert kinds["pairXY"] >= 15 and kinds["pairYZ"] >= 25 and kinds["persistent"] >= 60 and kinds["nd_oop"] >= 20 and kinds["nd_fixed"] >= 350 and kinds["nd2z"] >= 30 and kinds["nd_generic"] >= 20
    assert kinds["row"] >= 40 and kinds["col"] >= 80
    for prec in ("f32", "f64"):            # every instance of the several-work-groups tables is somebody's default choice (or dead code)
        for xyz in KC.nd_instances(N.ND_KERNEL_ND2Z, prec):
            assert ("nd2z", prec) + xyz in uni or ("nd_oop", prec) + xyz in uni, (prec, xyz)
    missing = sorted(((k, ex) for k, ex in uni.items() if k not in cov), key=str)
    assert not missing, "kernel instances no default-collected GPU test runs (key, an example plan): %r" % (missing[:40],)


REGISTER_ONLY_LENGTHS = (4, 8, 16, 32)      # the lengths of the register-only strided kernel (mifft_colr_eligible)


def _sides_run_by(test, case_of):
    """{(key, sides)} the cases of a function of tests/test_instances_gpu.py launch, read off its parametrize mark; case_of(case) ->
    (shape, dtype name, batch, the placements the test runs the contract in)"""
    import test_instances_gpu as T
    out = set()
    for p in KC.params_of(getattr(T, test)):
        shape, dtname, batch, placements = case_of(p["case"])
        out |= KC.sides_of_cases([(shape, dtname, batch)], placements)
    return out


def test_every_kernel_runs_on_every_buffer_side_a_plan_gives_it():
    """Every (key, sides) a default plan can launch -- which side holds split planes, whether the launch is aliased
    (kernel_coverage.launch_sides_of_plan) -- runs under the per-instance contract: test_instance runs each of its cases out of place and
    in place, test_instance_sides each case in the placement that produces its pairs."""
    import test_instances_gpu as T
    uni = KC.sides_universe()
    run = _sides_run_by("test_instance", lambda c: (c[0], c[1], c[2], KC.PLACEMENTS))
    if hasattr(T, "test_instance_sides"):         # (without it the rule fails below and names what nothing runs)
        run |= _sides_run_by("test_instance_sides", lambda c: (c[0], c[1], c[2], (c[3],)))
    # every key of universe() on at least one side (and the keys only a batch of 3 reaches: the chains of shapes whose big batches run
    # persistent, fixed-shape plane kernels of small launches)
    assert set(k for k, _ in uni) >= set(KC.universe())
    # floors, about 5 % below the measured values: a planner or schedule change must not make the rule vacuous
    one_side = [(k, s) for k, s in uni if s[0] != s[1]]
    aliased = set(k for k, s in uni if s[2])
    split_cols = {}
    for k, s in uni:
        if k[0] == "col" and k[2] == "split" and k[3] in REGISTER_ONLY_LENGTHS:
            split_cols.setdefault((k[1], k[3]), set()).add(s[:2])
    both_forms = sorted(pl for pl, forms in split_cols.items() if (False, False) in forms and any(planes_out for _, planes_out in forms))
    assert len(uni) >= 1590, len(uni)                       # measured: 1676 pairs
    assert len(one_side) >= 134, len(one_side)              # measured: 141 pairs with planes on exactly one side
    assert len(aliased) >= 674, len(aliased)                # measured: 710 keys with an aliased launch
    # measured: 4, the fp32 lengths (fp64 split plans take no detour through the interleaved temp buffer: their passes have planes on both sides)
    assert set(both_forms) >= set(("f32", L) for L in REGISTER_ONLY_LENGTHS), both_forms
    missing = sorted(((pair, ex) for pair, ex in uni.items() if pair not in run), key=str)
    assert not missing, "%d (key, (planes in, planes out, aliased)) pairs no case of tests/test_instances_gpu.py launches (pair, an example " \
        "(shape, dtype, batch, in place)): %r" % (len(missing), missing[:40])


def test_no_pass_pair_is_scheduled_on_planes_it_cannot_take():
    """The side between the two launches of a pair chain is interleaved (classify_pair, csrc/mifft_runtime.cpp): the library refuses a
    (COL y, COL z) pair that reads split planes and a (ROW x, COL y) pair that writes them, so no default plan may schedule one (the
    fp64 split plan of (256, 4, 16384): its row pass goes through the temp buffer, passes.yz_pair_chain)."""
    bad = sorted(((k, s, ex) for (k, s), ex in KC.sides_universe().items() if (k[0] == "pairYZ" and s[0]) or (k[0] == "pairXY" and s[1])), key=str)
    assert not bad, "pass pairs scheduled with split planes on their inner side (key, sides, an example): %r" % (bad,)


def test_sides_cases_produce_their_pairs_and_nothing_the_key_cases_run():
    run = KC.sides_of_cases(KC.audit_cases())
    for shape, dtname, batch, inplace, pairs in KC.sides_audit_cases():
        assert batch >= KC.AUDIT_MIN_BATCH
        assert set(pairs) <= KC.launch_sides_of(shape, numpy.dtype(dtname), batch, inplace), (shape, dtname, batch, inplace)
        assert not set(pairs) & run, (shape, dtname, batch, inplace)
    # both placements of an execute together launch exactly the keys of keys_of(): a side is a property of a key's launch, no key of its own
    for shape, dtname, batch, _ in KC.audit_cases():
        dt = numpy.dtype(dtname)
        keys = set(k for inplace in KC.PLACEMENTS for k, _ in KC.launch_sides_of(shape, dt, batch, inplace))
        assert keys == set(k for k in KC.keys_of(shape, dt, batch) if k is not None), (shape, dtname, batch)


def test_pair_kernel_table_and_reachable_pair_keys_agree():
    """mifft_pair_kernel_supported over its key space (include/mifft.h): every pair key a plan reaches has a kernel, and every kernel of
    the table is reached by some default plan -- no dead instance, no plan that would ask for a missing one."""
    have = set()
    pows = [1 << k for k in range(1, 15)]
    for prec, pname in ((N.F32, "f32"), (N.F64, "f64")):
        for lay, lname in ((N.INTERLEAVED, "interleaved"), (N.SPLIT, "split")):
            for kind, kname in ((0, "pairXY"), (1, "pairYZ")):
                for k0 in pows + [1 << 15, 1 << 16, 1 << 17, 1 << 18]:
                    for k1 in pows[:12]:
                        for k2 in pows[:12]:
                            if N.lib.mifft_pair_kernel_supported(prec, lay, kind, k0, k1, k2) == 0:
                                have.add((kname, pname, lname, k0, k1, k2))
    reached = set(k for k in KC.universe() if k[0] in ("pairXY", "pairYZ"))
    assert reached <= have, sorted(reached - have)
    # (instances only the persistent two-pair launch uses -- the {64, 128}^3 shapes whose chain is a plane pass + a z pass -- are reached
    # through their 'persistent' keys; what is left over here would be a kernel no plan selects)
    from pyfft_amd.plan import FFTPlan     # noqa: F401
    fusedp_only = set()
    for k, (shape, dtname, batch) in KC.universe().items():
        if k[0] == "persistent" and len(shape) == 3:
            plan = KC.plan_for(shape, numpy.dtype(dtname))
            chain = plan._pair_alt or plan._kernels
            fusedp_only |= KC._chain_keys(plan, chain)
    dead = sorted(k for k in have - reached - fusedp_only - KC.SWITCH_ONLY_PAIR_KEYS)
    assert not dead, "pair kernels no default plan reaches: %r" % (dead,)


def test_registry_names_every_gpu_test_function():
    """A GPU test added without saying what it covers fails here, not silently."""
    cases = KC.collected_cases()                 # raises on a missing / stale entry
    assert len(cases) > 1800
    mods = set(m for m, _, _ in cases)
    assert {"test_errors_gpu", "test_persistent_gpu", "test_pairs_gpu", "test_nd_gpu", "test_strided_gpu", "test_interop_gpu"} <= mods


def test_every_extension_kernel_instance_has_a_contract_case():
    """The opt-in extensions' kernels (kernel_coverage.extension_universe(): mixed-radix rows, lines, long transforms, the N-D and both
    Bluestein kernels, Bluestein axes on the work array, the tiled kernels, split planes) each run in tests/test_extension_instances_gpu.py."""
    uni = KC.extension_universe()
    kinds = {}
    for k in uni:
        kinds[k[0]] = kinds.get(k[0], 0) + 1
    assert kinds["mixed_row"] == 235 + 178
    assert kinds["mixed_stage"] >= 200 and kinds["tiled"] >= 2 * 2 * 13 and kinds["blue1"] == 4 and kinds["blue_work"] >= 10
    assert kinds["long"] == 6 and kinds["split"] >= 4
    stages = set(k[1] for k in uni if k[0] == "mixed_stage")
    assert stages == {"lines", "long_first", "nd", "blue", "blue_big"}, stages
    for prec in ("f32", "f64"):
        assert ("blue_work", prec, "interleaved", "nd", "one_launch") in uni and ("long", prec, "beyond") in uni
        for inst in ("lines", "nd", "blue"):
            for R in (3, 5, 7):
                assert ("mixed_stage", inst, prec, R, "first") in uni, (inst, prec, R)
    cov = KC.extension_covered_keys()
    missing = sorted(set(uni) - set(cov), key=str)
    assert not missing, "extension kernel instances without a contract case: %r" % (missing[:40],)


def test_every_form_kernel_instance_has_a_contract_case():
    """The kernels of Plan(real=True), Plan(convolve=True), Plan(r2r=...) and Plan(dtype="complex32") (kernel_coverage.form_universe():
    the one-launch rows, the real separation / packing launch, the spectrum product, the r2r steps and fallback, every complex32
    instance) each run in tests/test_form_instances_gpu.py."""
    import conv_cases
    import dct_cases
    uni = KC.form_universe()
    kinds = {}
    for k in uni:
        kinds[k[0]] = kinds.get(k[0], 0) + 1
    assert kinds["real_row"] == 2 * 29 and kinds["conv_row"] == len(conv_cases.FUSED) and kinds["r2r_row"] == 4 * len(dct_cases.FUSED)
    assert kinds["r2r_fallback"] == len(dct_cases.FUSED) and kinds["mul_spectrum"] == 12
    # floors for the step families: a planner change that drops a branch must not make the rule vacuous
    assert kinds["real_post"] >= 80 and kinds["r2r_perm"] >= 24 and kinds["r2r_orbit"] >= 34 and kinds["half"] >= 200
    prec = {numpy.float32: "f32", numpy.float64: "f64", numpy.complex64: "f32", numpy.complex128: "f64"}
    assert set(k for k in uni if k[0] == "conv_row") == set(("conv_row", prec[dt], real, n) for dt, real, n in conv_cases.FUSED)
    for p in ("f32", "f64"):
        for d in ("forward", "inverse"):
            for rank in (2, 3):
                for e in range(9):
                    assert ("real_post", p, d, 1 << e, rank) in uni, (p, d, 1 << e, rank)
            for rank in (1, 2, 3):
                assert ("r2r_orbit", p, rank, "fold", d) in uni and ("r2r_orbit", p, rank, "one_lane", d) in uni
                assert ("r2r_perm", p, rank, "vec", d) in uni and ("r2r_perm", p, rank, "scalar", d) in uni
        for s in ("shared", "per_item"):
            for c in (False, True):
                assert ("mul_spectrum", p, "scalar", s, c) in uni
    cov = KC.form_covered_keys()
    missing = sorted(set(uni) - set(cov), key=str)
    assert not missing, "form kernel instances without a contract case: %r" % (missing[:40],)


def test_form_cases_take_ragged_batches():
    for form, shape, dtname, batch, kind, keys in KC.form_audit_cases():
        n = int(numpy.prod(shape))
        assert batch == (67 if n <= 2048 else 3), (form, shape, batch)
        assert set(keys) <= KC.form_keys(form, shape, dtname, batch, kind)


def test_extension_cases_take_their_forms_and_ragged_batches():
    top32, beyond32 = KC.long_limits(numpy.complex64)
    top64, beyond64 = KC.long_limits(numpy.complex128)
    assert top32 < beyond32 < (1 << 18) + (1 << 16) and top64 < beyond64
    cases = KC.extension_audit_cases()
    forms = set(c[4] for c in cases)
    assert forms >= {"_direct_mixed", "_direct_nd", "_direct_nd1", "_direct_nd_planes", "_direct_long", "_direct_blue", "_tiled", "_uses_work"}
    for shape, dtname, batch, parent, form, keys in cases:
        assert batch >= 3
        if form == "_direct_mixed" and batch > 3:
            assert batch % ((4096 if dtname == "complex64" else 2048) // 2 // shape[0]) != 0
    for dt in ("float32", "float64"):
        assert any(c[1] == dt and c[3] is None and c[4] == "_uses_work" for c in cases), dt
