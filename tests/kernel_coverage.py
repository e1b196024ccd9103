"""Which kernel instances do default plans select, and which GPU test runs each of them?  (Round 6; test infrastructure, CPU only.)

The library holds several hundred ahead-of-time kernel instances; a plan reaches one through `passes.build_chain` (the chain's
launches: rows, strided passes, one-launch N-D shapes, pass pairs) and through `FFTPlan._select_strategy` (a persistent launch by a
rule of the tuning table, the several-work-groups-per-transform kernel of out-of-place executes).  The rule this module makes
mechanical: EVERY instance some default plan can select must be exercised by a GPU test that the default `pytest -m gpu` run
collects (about half of the pass-pair instances had their only parity test behind a soak switch).

  keys_of(shape, dtype, batch, mode)   the instance keys one test case exercises, computed with the planner itself on the model
                                       of the full part (256 CUs, 8 XCDs, 256 MiB last-level cache) -- no device needed
  keys_of_plan(plan, batch, mode)      the same for a given plan (a device plan: what the device's planner selects)
  universe()                           every key reachable by SOME power-of-two shape of up to 2^24 points in the four dtypes
  collected_cases()                    the (shape, dtype, batch, mode) cases of the default-collected GPU tests, read off the
                                       tests' own parametrize marks through REGISTRY (one adapter per test function)
  audit_cases()                        for every key of universe(), the smallest case (shape, dtype, batch >= 3) that selects it: the
                                       cases of tests/test_instances_gpu.py, which holds each instance to the accuracy contract
  launch_sides_of_plan(plan, batch, inplace)   {(key, (planes in, planes out, aliased))} of one execute: the buffer sides the plan's schedule
                                       gives each launch, read off the plan's descriptors
  sides_universe()                     every (key, sides) reachable by those shapes at batch 3 and universe()'s batches, in either placement
  sides_audit_cases()                  the smallest case (shape, dtype, batch >= 3, placement) for every (key, sides) audit_cases() launches
                                       in neither placement: the cases of test_instances_gpu.py::test_instance_sides

The reference sweeps its kernels the same way, by shape lists: test/test_errors.py:125-145.
"""
import importlib
import itertools

import numpy

from helpers import FakeContext

GPU_MODULES = ["test_errors_gpu", "test_full_size_gpu", "test_functionality_gpu", "test_random_sweep_gpu", "test_rows_gpu",
               "test_strided_gpu", "test_persistent_gpu", "test_pairs_gpu", "test_nd_gpu", "test_generic_gpu", "test_interop_gpu",
               "test_instances_gpu", "test_extension_instances_gpu", "test_form_instances_gpu"]

C64, C128, F32, F64 = numpy.complex64, numpy.complex128, numpy.float32, numpy.float64
ALL_DTYPES = [C64, F32, C128, F64]
_machine = None


def full_machine():
    global _machine
    if _machine is None:
        from pyfft_amd.machine import Machine
        _machine = Machine(256, 8, 4 << 20, 256 << 20)
    return _machine


_plans = {}


def plan_for(shape, dtype):
    """A plan on the model of the full part (no device: tables are uploaded nowhere), cached per (shape, dtype)."""
    from pyfft_amd.plan import FFTPlan
    shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    key = (shape, numpy.dtype(dtype).name)
    if key not in _plans:
        _plans[key] = FFTPlan(FakeContext(full_machine()), shape, dtype=dtype)
    return _plans[key]


_tables = {}


def fixed_nd_shapes(prec):
    """(x, y, z) of the generated fixed-shape N-D tables csrc/fft_nd2_<prec>_*.hip (tools/gen_nd2_tables.py is their single source)"""
    if "fixed" not in _tables:
        import importlib.util
        import os
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_nd2_tables.py")
        spec = importlib.util.spec_from_file_location("gen_nd2_tables", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _tables["fixed"] = {"f32": frozenset(tuple(t) for t in mod.shapes("f32")), "f64": frozenset(tuple(t) for t in mod.shapes("f64"))}
    return _tables["fixed"][prec]


def nd_kernel(d, aliased, small_launch=None, variant=None):
    """The kernel form (N.ND_KERNEL_*) the library runs for the ND pass descriptor `d`: mifft_nd_kernel, the selector mifft_launch_pass
    itself goes through.  aliased: bit 0 in0 == out0, bit 1 in1 == out1.  small_launch: override the descriptor's write-through mark (what
    the plan sets for launches of up to write_through_max per side); variant: override its variant (0: the shape's own instance, not the
    plan's per-batch choice of the run-time-shaped kernel in its place).  A negative code: the launch would be refused."""
    import ctypes
    from pyfft_amd import _native as N
    d = type(d).from_buffer_copy(d)
    if small_launch is not None:
        d.flags = (d.flags | N.FLAG_WRITE_THROUGH) if small_launch else (d.flags & ~N.FLAG_WRITE_THROUGH)
    if variant is not None:
        d.variant = variant
    return N.lib.mifft_nd_kernel(ctypes.byref(d), aliased)


def nd_pass(prec, x, y, z, planes=False):
    """a dense ND pass descriptor of the shape, interleaved or planes on both sides (tables: any non-null address; nothing is launched)"""
    from pyfft_amd import _native as N
    d = N.MifftPass()
    d.kind, d.precision, d.layout = N.PASS_ND, (N.F64 if prec == "f64" else N.F32), (N.SPLIT if planes else N.INTERLEAVED)
    d.L, d.M, d.S, d.outer, d.scale = x, y, z, 4, 1.0
    d.outer_stride_in = d.outer_stride_out = x * y * z
    d.tw_L = d.tw_lo = d.tw_hi = 4096
    return d


def nd_instances(form, prec):
    """every (x, y, z) of up to 2^MAX_LOG2_POINTS points that runs the several-work-groups form N.ND_KERNEL_ND2Z (interleaved) /
    N.ND_KERNEL_ND2ZP (planes) in a small out-of-place launch: the whole instance table of that form, asked of the library"""
    from pyfft_amd import _native as N
    out = set()
    for lx in range(MAX_LOG2_POINTS + 1):
        for ly in range(MAX_LOG2_POINTS + 1 - lx):
            for lz in range(MAX_LOG2_POINTS + 1 - lx - ly):
                xyz = (1 << lx, 1 << ly, 1 << lz)
                if nd_kernel(nd_pass(prec, *xyz, planes=form == N.ND_KERNEL_ND2ZP), 0, small_launch=True) == form:
                    out.add(xyz)
    return frozenset(out)


def _nd_key(d):
    """The instance an N-D pass of the plan runs in place: the shape's own fixed instance (interleaved: the generated tables; planes: the
    dense 16-byte kernel, or the tiled fixed-shape kernel where it takes dense planes), else the ONE run-time-shaped kernel, whose instances
    differ by the tile's size class.  A shape whose only kernel runs out of place is keyed by its shape too.  The answer is the library's
    (mifft_nd_kernel) for variant 0 of the pass: the key names the shape's instance, not the plan's per-batch choice of the run-time-shaped
    kernel in its place (variant 1, the tuning table's "nd_generic" lists)."""
    from pyfft_amd import _native as N
    prec = "f64" if d.precision == N.F64 else "f32"
    lay = "split" if d.layout == N.SPLIT else "interleaved"
    x, y, z = int(d.L), int(d.M), int(d.S)
    form = nd_kernel(d, 3, variant=0)
    if form == N.ND_KERNEL_ND2P:
        return ("nd_planes16", prec, x, y, z)
    if form != N.ND_KERNEL_ND:
        assert form in (N.ND_KERNEL_ND2, N.ND_KERNEL_ND2T, N.E_UNSUPPORTED), (form, N.last_error())
        return ("nd_fixed", prec, lay, x, y, z)
    n = x * y * z
    return ("nd_generic", prec, lay, "dims%d" % ((x > 1) + (y > 1) + (z > 1)), "log2n=%d" % (n.bit_length() - 1))


def _chain_launches(plan, chain, batch=1, first=0):
    """[(key, index of the launch's first descriptor, of its last)] per LAUNCH of a chain: plan._kernels[first:], or a pass list without
    ND passes.  The indices count from the start of plan._kernels (a pass pair: two descriptors, one launch)."""
    from pyfft_amd import _native as N
    p = plan._params
    prec = "f64" if p.precision == N.F64 else "f32"
    lay = "split" if p.split else "interleaved"
    out, i = [], 0
    while i < len(chain):
        k = chain[i]
        if k.pair_with_next:
            k2 = chain[i + 1]
            if k.kind == N.PASS_ROW:
                key = ("pairXY", prec, lay, int(k.L), int(k2.L), int(k2.M))        # (nx, R0, R1): mifft_pair_kernel_supported kind 0
            else:
                key = ("pairYZ", prec, lay, int(k.S), int(k.L), int(k2.L))         # (S0, R1, nz): kind 1
            out.append((key, first + i, first + i + 1))
            i += 2
            continue
        if k.kind == N.PASS_ND:
            key = _nd_key(plan._descriptors(int(batch), True, False)[first + i])
        elif k.kind == N.PASS_ROW:
            key = ("row", prec, lay, int(k.L))
        else:
            # a strided pass: its length, whether it carries the inter-pass twiddle (M > 1), and the class of its stride (S == 1: the
            # transposing first pass of a long contiguous axis; S < 16: columns narrower than a tile; else whole 16-column tiles)
            # (fp32 interleaved 256 / 512 points with rows >= 2^16 points apart: the 32-column plain tiles of csrc/fft_col2_f32.hip)
            far = prec == "f32" and lay == "interleaved" and k.L in (256, 512) and k.M == 1 and k.S >= 65536
            key = ("col", prec, lay, int(k.L), "twiddled" if k.M > 1 else "plain",
                   "S1" if k.S == 1 else ("S<16" if k.S < 16 else ("S>=65536" if far else "S>=16")))
        out.append((key, first + i, first + i))
        i += 1
    return out


def _chain_keys(plan, chain, batch=1, first=0):
    """one key per LAUNCH of a chain (_chain_launches)"""
    return set(key for key, _, _ in _chain_launches(plan, chain, batch, first))


def _persistent_key(plan):
    from pyfft_amd import _native as N
    p = plan._params
    rule = plan._persistent_rule()
    if rule is None:
        return None
    # (the planes of a big 3-D transform run the 2-D plan's instance: strategy "fused2z")
    return ("persistent", rule["name"], "f64" if p.precision == N.F64 else "f32", "split" if p.split else "interleaved",
            int(p.x), int(p.y), 1 if plan._plane_fused() else int(p.z))


def keys_of(shape, dtype, batch, mode="auto"):
    """Instance keys the test case (shape, dtype, batch) exercises.  mode: "auto" = the plan's own strategy at this batch, in place and
    out of place (what the tests' protocols run); "chain" / "pipelined" = the chain's launches; "fused" = the plan's persistent launch
    whatever the batch (PYFFT_AMD_STRATEGY=fused, or a forced ring)."""
    return keys_of_plan(plan_for(shape, dtype), batch, mode)


def keys_of_plan(plan, batch, mode="auto"):
    """keys_of for a given plan: one on the model of the full part (plan_for), or a device plan (what that device's planner selects)"""
    keys = set()
    if mode in ("chain", "pipelined"):
        return _chain_keys(plan, plan._kernels, batch)
    if mode == "fused":
        k = _persistent_key(plan)
        return {k} if k is not None else set()
    strat = plan._select_strategy(int(batch))
    if strat[0] == "fused2z":
        # one persistent 2-D launch over the (y, x) planes -- the 2-D plan's instance; what is new is the planner's route -- then the
        # chain's z launches
        pk = _persistent_key(plan)
        keys.add(pk)
        keys.add(("plane_fused",) + pk[1:4])
        keys |= _chain_keys(plan, plan._kernels[2:], batch, 2)
    elif strat[0] in plan.PERSISTENT:
        keys.add(_persistent_key(plan))
    else:
        keys |= _chain_keys(plan, plan._kernels, batch)
    from pyfft_amd import _native as N
    p = plan._params
    prec = "f64" if p.precision == N.F64 else "f32"
    if plan._runs_oop_nd(int(batch)):
        keys.add(("nd_oop", prec + ("_planes" if p.split else ""), int(p.x), int(p.y), int(p.z)))
    # a one-launch plan of a shape with a several-work-groups-per-transform instance (csrc/fft_nd2z.hip; split-complex planes:
    # csrc/fft_nd2zp.hip): its OUT-OF-PLACE executes take that instance inside the library (mifft_nd_kernel, the selector of
    # mifft_launch_pass; for some interleaved shapes in small launches only -- the tests assert which -- so the key is asked for those)
    if len(plan._kernels) == 1 and plan._kernels[0].kind == N.PASS_ND:
        form = nd_kernel(plan._descriptors(int(batch), False, False)[0], 0, small_launch=True, variant=0)     # (variant 0: as _nd_key)
        if form in (N.ND_KERNEL_ND2Z, N.ND_KERNEL_ND2ZP):
            keys.add(("nd2zp" if form == N.ND_KERNEL_ND2ZP else "nd2z", prec, int(p.x), int(p.y), int(p.z)))
    return keys


# ---- the buffer sides of a launch ----------------------------------------------------------------------------------------------------
# A key says which kernel family, length and stride class a launch is; the plan's buffer schedule adds three run-time facts per launch
# that the dispatcher and the kernels branch on (mifft_colr_eligible, mifft_col2x_f32_eligible, the a.split / a.split_out paths of
# csrc/fft_tile.hpp, select_nd's alias bits): which side holds split planes, and whether the launch reads and writes one buffer.
def _unit_sides(plan, d_first, d_last, inplace):
    """(planes in, planes out, aliased) of a launch whose first / last descriptors are given (a pass pair: two; else the same one)"""
    from pyfft_amd import _native as N
    split = bool(plan._params.split)
    src, dst = int(d_first.src), int(d_last.dst)
    # (an in-place execute passes the user's buffer as both 0 and 1)
    aliased = src == dst or (bool(inplace) and src in (0, 1) and dst in (0, 1))
    return (split and not (d_first.flags & N.FLAG_SRC_INTERLEAVED), split and not (d_last.flags & N.FLAG_DST_INTERLEAVED), aliased)


def launch_sides_of_plan(plan, batch, inplace):
    """{(key, (planes in, planes out, aliased))} over the launches of ONE execute of `batch` items, in place or out of place: the keys
    of keys_of_plan(plan, batch) that this placement launches, each with the sides read off the plan's own descriptors.  Persistent
    launches and the one-launch out-of-place route (nd_oop, nd2z, nd2zp) work on the user's buffers: (layout, layout, in place)."""
    from pyfft_amd import _native as N
    batch, inplace = int(batch), bool(inplace)
    p = plan._params
    split = bool(p.split)
    prec = "f64" if p.precision == N.F64 else "f32"
    user = (split, split, inplace)
    if not inplace and plan._runs_oop_nd(batch):
        return {(("nd_oop", prec + ("_planes" if split else ""), int(p.x), int(p.y), int(p.z)), user)}
    out = set()
    descs = plan._descriptors(batch, inplace, False)
    strat = plan._select_strategy(batch)
    first = 0
    if strat[0] == "fused2z":
        pk = _persistent_key(plan)
        out |= {(pk, user), (("plane_fused",) + pk[1:4], user)}
        first = 2
    elif strat[0] in plan.PERSISTENT:
        return {(_persistent_key(plan), user)}
    for key, i0, i1 in _chain_launches(plan, plan._kernels[first:], batch, first):
        out.add((key, _unit_sides(plan, descs[i0], descs[i1], inplace)))
    # (the several-work-groups instance of a one-launch plan's out-of-place executes: as keys_of_plan)
    if not inplace and len(plan._kernels) == 1 and plan._kernels[0].kind == N.PASS_ND:
        form = nd_kernel(descs[0], 0, small_launch=True, variant=0)
        if form in (N.ND_KERNEL_ND2Z, N.ND_KERNEL_ND2ZP):
            out.add((("nd2zp" if form == N.ND_KERNEL_ND2ZP else "nd2z", prec, int(p.x), int(p.y), int(p.z)), user))
    return out


def launch_sides_of(shape, dtype, batch, inplace):
    """launch_sides_of_plan on the model of the full part"""
    return launch_sides_of_plan(plan_for(shape, dtype), batch, inplace)


PLACEMENTS = (False, True)        # in place?  (out of place first: where both produce a pair, the case runs the shorter contract)


# pair kernels of the library that no default plan selects, only a development switch (MIFFT_DEBUG_PAIR = 2: the other y split of 256^3,
# interleaved fp64); tests/test_pairs_gpu.py::test_pass_pairs_256_cubed_alternative_split runs it
SWITCH_ONLY_PAIR_KEYS = {("pairXY", "f64", "interleaved", 256, 64, 4), ("pairYZ", "f64", "interleaved", 16384, 4, 256)}

MAX_LOG2_POINTS = 24          # shapes of up to 2^24 points: 4096 x 4096, 256^3, 2^24 (128 MiB fp32 / 256 MiB fp64 per transform)


UNIVERSE_SIDES = (512 << 20, 2 << 30, 8 << 30)


def _shapes(max_log):
    """every power-of-two shape of up to 2^max_log points (x contiguous; numpy shapes (z, y, x))"""
    for lx in range(0, max_log + 1):
        for ly in range(0, max_log + 1 - lx):
            for lz in range(0, max_log + 1 - lx - ly):
                if lx + ly + lz < 1:
                    continue
                if (ly == 0 and lz > 0) or (lx == 0 and (ly > 0 or lz > 0)):
                    continue            # (unit axes in front of longer ones are the same plans as the lower-rank shape: tests cover them by name)
                yield (1 << lx,) if ly == 0 else ((1 << ly, 1 << lx) if lz == 0 else (1 << lz, 1 << ly, 1 << lx))


def _item_bytes(shape, dtype):
    return _prod(shape) * (8 if dtype in (C64, F32) else 16)


_universe = {}


def universe(max_log=MAX_LOG2_POINTS):
    """{key: an example (shape, dtype, batch)} over every power-of-two shape of up to 2^max_log points (x contiguous; numpy shapes
    (z, y, x)), the four dtypes, and batches of 512 MiB, 2 GiB and 8 GiB per side -- where the planner's default choices live."""
    if max_log in _universe:
        return dict(_universe[max_log])
    out = {}
    for shape in _shapes(max_log):
        for dtype in ALL_DTYPES:
            item = _item_bytes(shape, dtype)
            for side in UNIVERSE_SIDES:
                batch = max(1, side // item)
                for k in keys_of(shape, dtype, batch):
                    if k is not None and k not in out:
                        out[k] = (shape, numpy.dtype(dtype).name, batch)
    _universe[max_log] = out
    return dict(out)


# ---- one audit case per instance key (tests/test_instances_gpu.py) -------------------------------------------------------------------
AUDIT_MIN_BATCH = 3
_audit = {}


def _smallest_cases(want, things_of, max_log, placements=(None,)):
    """{thing: (bytes per side, order, shape, dtype name, batch, placement)}: for every member of `want` the smallest case (bytes per
    side, then enumeration order) with batch >= 3 whose things_of(shape, dtype, batch, placement) holds it, in a batch that is no multiple
    of 4 where the thing allows one (tiles that hold several transforms then end partially filled).  Per (shape, dtype, placement) the
    planner is asked at batch 3 and at universe()'s batches; a thing that only appears at a larger batch is bisected down to the batch
    where it appears."""
    best = {}
    order = 0
    for shape in _shapes(max_log):
        for dtype in ALL_DTYPES:
            item = _item_bytes(shape, dtype)
            probes = sorted(set([AUDIT_MIN_BATCH] + [max(AUDIT_MIN_BATCH, side // item) for side in UNIVERSE_SIDES]))
            for placement in placements:
                memo = {}

                def at(b):
                    if b not in memo:
                        memo[b] = set(k for k in things_of(shape, dtype, b, placement) if k in want)
                    return memo[b]

                prev = None
                for b in probes:
                    for k in at(b):
                        if (prev is not None and k in at(prev)) or (k in best and best[k][0] <= AUDIT_MIN_BATCH * item):
                            continue        # (recorded at the previous probe; or no batch of this shape beats the case found)
                        lo, hi = prev, b
                        while lo is not None and hi - lo > 1:
                            mid = (lo + hi) // 2
                            if k in at(mid):
                                hi = mid
                            else:
                                lo = mid
                        if hi % 4 == 0 and k in at(hi + 1):
                            hi += 1
                        order += 1
                        cand = (hi * item, order, shape, numpy.dtype(dtype).name, hi, placement)
                        if k not in best or cand[0] < best[k][0]:
                            best[k] = cand
                    prev = b
    return best


def audit_cases(max_log=MAX_LOG2_POINTS):
    """[(shape, dtype name, batch, keys)]: for every key of universe() but SWITCH_ONLY_PAIR_KEYS, the smallest case that selects it
    (_smallest_cases); a case that is the smallest for several keys appears once, `keys` sorted.  A key without such a case raises (the
    audit must not silently lose an instance)."""
    if max_log in _audit:
        return list(_audit[max_log])
    uni = universe(max_log)
    want = set(uni) - SWITCH_ONLY_PAIR_KEYS
    best = _smallest_cases(want, lambda shape, dtype, b, _: keys_of(shape, dtype, b), max_log)
    missing = sorted(want - set(best), key=str)
    if missing:
        raise AssertionError("tests/kernel_coverage.py audit_cases: no case with batch >= %d selects %r" % (AUDIT_MIN_BATCH, missing[:40]))
    cases = {}
    for k, (_, _, shape, dtname, batch, _) in best.items():
        cases.setdefault((shape, dtname, batch), []).append(k)
    out = sorted(((shape, dtname, batch, tuple(sorted(ks, key=str))) for (shape, dtname, batch), ks in cases.items()), key=lambda c: str(c[3][0]))
    _audit[max_log] = out
    return list(out)


# ---- one audit case per (key, sides) that audit_cases() leaves out (tests/test_instances_gpu.py::test_instance_sides) -----------------
_sides_universe = {}
_sides_audit = {}


def sides_universe(max_log=MAX_LOG2_POINTS):
    """{(key, sides): an example (shape, dtype name, batch, in place)} over universe()'s shapes and dtypes, at batch 3 and universe()'s
    batches, in place and out of place"""
    if max_log in _sides_universe:
        return dict(_sides_universe[max_log])
    out = {}
    for shape in _shapes(max_log):
        for dtype in ALL_DTYPES:
            item = _item_bytes(shape, dtype)
            for batch in sorted(set([AUDIT_MIN_BATCH] + [max(1, side // item) for side in UNIVERSE_SIDES])):
                for inplace in PLACEMENTS:
                    for pair in launch_sides_of(shape, dtype, batch, inplace):
                        if pair not in out:
                            out[pair] = (shape, numpy.dtype(dtype).name, batch, inplace)
    _sides_universe[max_log] = out
    return dict(out)


def sides_of_cases(cases, placements=PLACEMENTS):
    """{(key, sides)} the cases (shape, dtype name, batch, ...) launch on the model of the full part in the given placements"""
    out = set()
    for case in cases:
        for inplace in placements:
            out |= launch_sides_of(case[0], numpy.dtype(case[1]), case[2], inplace)
    return out


def sides_audit_cases(max_log=MAX_LOG2_POINTS):
    """[(shape, dtype name, batch, in place, pairs)]: for every (key, sides) of sides_universe() that audit_cases() launches in neither
    placement, the smallest case that launches it (_smallest_cases: out of place before in place); a case that is the smallest for
    several pairs appears once, `pairs` sorted.  A pair without such a case raises."""
    if max_log in _sides_audit:
        return list(_sides_audit[max_log])
    want = set(sides_universe(max_log)) - sides_of_cases(audit_cases(max_log))
    best = _smallest_cases(want, launch_sides_of, max_log, PLACEMENTS)
    missing = sorted(want - set(best), key=str)
    if missing:
        raise AssertionError("tests/kernel_coverage.py sides_audit_cases: no case with batch >= %d launches %r" % (AUDIT_MIN_BATCH, missing[:40]))
    cases = {}
    for pair, (_, _, shape, dtname, batch, inplace) in best.items():
        cases.setdefault((shape, dtname, batch, inplace), []).append(pair)
    out = sorted(((shape, dtname, batch, inplace, tuple(sorted(ps, key=str))) for (shape, dtname, batch, inplace), ps in cases.items()),
                 key=lambda c: str(c[4][0]))
    _sides_audit[max_log] = out
    return list(out)


# ---- the default-collected GPU cases, read off the tests' parametrize marks ----------------------------------------------------------
def params_of(fn):
    """[{argname: value}] of a test function's (stacked) parametrize marks"""
    combos = [{}]
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [n.strip() for n in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        new = []
        for c in combos:
            for v in m.args[1]:
                vals = v.values if type(v).__name__ == "ParameterSet" else v
                if len(names) == 1:
                    vals = (vals,)
                d = dict(c)
                d.update(zip(names, vals))
                new.append(d)
        combos = new
    return combos


def _prod(shape):
    return int(numpy.prod(shape))


def _c(shape, dtype, batch, mode="auto"):
    return (tuple(shape), dtype, int(batch), mode)


def _fixed_nd(p):
    x, y, z = p["xyz"]
    shape = (y, x) if z == 1 else (z, y, x)
    n = x * y * z
    tile = 4096 if p["dtype"] == C64 else 2048
    return [_c(shape, p["dtype"], 3 if n >= tile else (tile // n) * 2 + 1)]


def _is_double(dt):
    return numpy.dtype(dt) in (numpy.dtype(C128), numpy.dtype(F64))


def _split(dt):
    return numpy.dtype(dt).kind == "f"


# adapter(params) -> [(shape, dtype, batch, mode)]; None = the test builds no default power-of-two plan worth counting (API checks,
# direct C-ABI launches, opt-in extensions)
REGISTRY = {
    "test_errors_gpu": {
        "test_errors_batch_1_and_3": lambda p: [_c(p["shape"], p["dtype"], b) for b in (1, 3) if _prod(p["shape"]) * b <= (1 << 19)],
        "test_errors_batched": lambda p: [_c(p["shape"], p["dtype"], p["batch"]), _c(p["shape"], p["dtype"], p["batch"] - 1 if p["batch"] > 1 else 5)],
        "test_register_edged_rows": lambda p: [_c((p["n"],), p["dtype"], 37)] + ([_c((128, p["n"]), p["dtype"], 3)] if p["n"] <= 4096 else []),
        "test_fixed_shape_nd_kernels": _fixed_nd,
        "test_fixed_shape_nd_planes": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_fp64_two_phase_col_512": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_unit_axes": lambda p: [_c(p["shape"], p["dtype"], 3)],
        "test_errors_large_1d": lambda p: [_c((1 << 20,), p["dtype"], 2)],
        "test_errors_config3_shape": lambda p: [_c((1024, 1024), C64, 2)],
        "test_errors_config4_shape_reduced": lambda p: [_c((64, 64, 64), p["dtype"], 1), _c((256, 16, 16), p["dtype"], 2)],
        "test_fused_two_pass_kernel": lambda p: [_c((p["n"],), C64, p["batch"], "fused"), _c((p["n"],), C64, p["batch"], "chain")],
        "test_fused_2d_1024": lambda p: [_c((1024, 1024), p["dtype"], 29 if _is_double(p["dtype"]) else 57, "fused"),
                                         _c((1024, 1024), p["dtype"], 29 if _is_double(p["dtype"]) else 57, "chain")],
        "test_fused_2d_other_squares": lambda p: [_c((p["side"], p["side"]), C64, p["batch"])],
        "test_fused_two_pass_kernel_fp64": lambda p: [_c((1 << 20,), C128, 31, "fused"), _c((1 << 20,), C128, 31, "chain"), _c((1 << 20,), F64, 31, "fused")],
        "test_pipelined_chunks": lambda p: [_c(p["shape"], C64, p["batch"], "pipelined")],
        "test_split_plane_strategies": lambda p: [_c((p["n"],), F32, p["batch"], p["strat"]), _c((p["n"],), F32, p["batch"], "chain")],
        "test_golden_fixture_through_hip": lambda p: [_c(p["entry"]["shape"], numpy.dtype(p["entry"]["dtype"]).type, p["entry"]["batch"])],
        "test_reference_error_grid": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_fused2_refuses_a_shape_without_a_kernel_before_it_touches_the_counters": None,      # (a refusal: no kernel runs)
    },
    "test_full_size_gpu": {
        "test_config2_full": lambda p: [_c((1 << 20,), C64, 4096)],
        "test_config3_full": lambda p: [_c((1024, 1024), C64, 512)],
        "test_config4_full": lambda p: [_c((256, 256, 256), p["dtype"], 64)],
        "test_config5_per_gpu_chunk": lambda p: [_c((1 << 22,), C64, 256)],
        "test_linearity_large": lambda p: [_c((1 << 20,), C64, 4)],
    },
    "test_functionality_gpu": None,      # the reference's API checks (test/test_functionality.py) on tiny shapes
    "test_random_sweep_gpu": {
        "test_random_case": lambda p: [_c(p["case"][0], p["case"][2], p["case"][1])],
    },
    "test_rows_gpu": {
        "test_small_n_wave_path_parity": lambda p: [_c((p["n"],), p["dtype"], b) for b in (1, 3, 63, 64, 65, 1000)],
        "test_wave_kernel_matches_lds_kernel": None,
        "test_16x16_wave_plane_kernel": None,
        "test_small_launch_write_through_is_bit_identical": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_write_through_rule_stops_at_128_mib": None,
    },
    "test_strided_gpu": {
        "test_l2048_strided_pass": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_l1024_fp64_strided_pass": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_l2048_fp64_strided_pass": lambda p: [_c(p["shape"], C128, p["batch"])],
        "test_l2048_fp64_fallback_kernel": None,
        "test_register_only_short_strided_pass": None,
        "test_long_strided_axes": lambda p: [_c(p["shape"], p["dtype"], 1 if _prod(p["shape"]) * numpy.dtype(p["dtype"]).itemsize * (2 if _split(p["dtype"]) else 1) >= (64 << 20) else 2)],
    },
    "test_persistent_gpu": {
        "test_async_error_mailbox": lambda p: [_c((1 << 20,), C64, 64)],
        "test_error_mailbox_keeps_the_oldest_word_when_the_ring_is_full": None,
        "test_fused_pair_cube_128": lambda p: [_c((128, 128, 128), p["dtype"], p["batch"], "fused"), _c((128, 128, 128), p["dtype"], p["batch"], "chain")],
        "test_fused_ring_rule_2_19": lambda p: [_c((1 << 19,), C64, 130), _c((1 << 19,), C64, 130, "chain")],
        "test_alternating_counter_sets_and_memset_form_agree": lambda p: [_c((1 << 20,), C64, 70)],
        "test_fused_2d_rectangles": lambda p: [_c(p["shape"], C64, p["batch"], "fused" if tuple(p["shape"]) == (512, 2048) else "auto"),
                                               _c(p["shape"], C64, p["batch"], "chain")],
        "test_fused_long_fp64": lambda p: [_c((p["n"],), C128, p["batch"], "fused"), _c((p["n"],), C128, p["batch"], "chain")],
        "test_fused_mid_sizes_fp64": lambda p: [_c((p["n"],), C128, p["batch"], "fused"), _c((p["n"],), C128, p["batch"], "chain")],
        "test_fused_2d_fp64_512_sides": lambda p: [_c(p["shape"], C128, p["batch"], "fused"), _c(p["shape"], C128, p["batch"], "chain")],
        "test_wide_tiles_fp32_mid_sizes_against_the_chain": lambda p: [_c((p["n"],), C64, p["batch"]), _c((p["n"],), C64, p["batch"], "chain")],
        "test_fused_2d_256_sides": lambda p: ([] if (_is_double(p["dtype"]) and max(p["shape"]) > 512) else
                                              [_c(p["shape"], p["dtype"], p["batch"] // 2 + 1 if _is_double(p["dtype"]) else p["batch"]),
                                               _c(p["shape"], p["dtype"], p["batch"], "chain")]),
        "test_split_planes_on_sibling_tiles": lambda p: [_c((p["n"],), F32, p["batch"]), _c((p["n"],), F32, p["batch"], "chain")],
        "test_fused_pair_small_axes": lambda p: [_c(p["shape"], p["dtype"], p["batch"] // 2 + 1 if _is_double(p["dtype"]) else p["batch"]),
                                                 _c(p["shape"], p["dtype"], p["batch"], "chain")],
        "test_fused_pair_split_planes": lambda p: [_c(p["shape"], p["rdtype"], p["batch"]), _c(p["shape"], p["rdtype"], p["batch"], "chain")],
        "test_plane_fused_3d": lambda p: [_c(p["shape"], p["dtype"], p["batch"]), _c(p["shape"], p["dtype"], p["batch"], "chain")],
        "test_fused_2d_split_row_first": lambda p: [_c(p["shape"], F32, p["batch"], "fused" if tuple(p["shape"]) == (256, 256) else "auto"),
                                                    _c(p["shape"], F32, p["batch"], "chain")],
        "test_fused_split_planes_fp64": lambda p: [_c(p["shape"], F64, p["batch"]), _c(p["shape"], F64, p["batch"], "chain")],
        "test_config5_per_gpu_share": lambda p: [_c((1 << 22,), C64, 256)],
        "test_config5_share_as_one_execute": lambda p: [_c((1 << 22,), C64, 8192)],
        "test_config5_share_every_output_bit_identical_to_its_period_mate": lambda p: [_c((1 << 22,), C64, 8192)],
        "test_direct_abi_two_set_launch_refuses_capture_and_null_error_word": lambda p: [_c((1 << 18,), C64, 160)],
    },
    "test_pairs_gpu": {
        "test_pass_pairs_256_cubed": lambda p: [_c((256, 256, 256), p["dtype"], 1)],
        "test_pass_pairs_256_cubed_alternative_split": None,         # (an A/B instance behind a development switch: SWITCH_ONLY_PAIR_KEYS above)
        "test_pair_chains_two_launches": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_pair_chains_pipelined_chunks": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_pass_pairs_for_256_point_rows": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
    },
    "test_nd_gpu": {
        "test_two_work_groups_per_transform_nd": "nd2z",        # (the shapes are a list inside the module: see collected_cases)
        "test_four_work_groups_per_transform_out_of_place": lambda p: [
            _c(p["shape"], p["dtype"], (261 * 65536 * 8) // (_prod(p["shape"]) * numpy.dtype(p["dtype"]).itemsize))],
        "test_two_work_groups_per_transform_split_planes": lambda p: [_c(p["shape"], F32, 13 if p["small"] else (261 * 65536 * 8) // (_prod(p["shape"]) * 8))],
        "test_tiny_nd_shapes_small_launches": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_tiny_nd_shapes_big_launches": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_run_time_shaped_nd_kernel_size_classes": lambda p: [_c(p["shape"], p["dtype"], 5 if _prod(p["shape"]) >= 4096 else 4099 // _prod(p["shape"]))],
        "test_dense_split_planes_on_the_tiled_fixed_kernels": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_dense_split_planes_16_byte_accesses": lambda p: [_c(p["shape"], p["dtype"], 1)],
    },
    "test_generic_gpu": None,            # opt-in extensions (any_size / parent_shape): their kernels are extension keys (extension_universe)
    "test_interop_gpu": {
        "test_reference_quick_start_literally": lambda p: [_c((1 << 22,), C64, 1)],
        "test_default_plan_orders_against_torch_producer": lambda p: [_c((1 << 20,), C64, 64)],
        "test_context_device_must_be_current": None,
        "test_bench_nccl_path_at_world_size_one": lambda p: [_c((1 << 20,), C64, 128)],
        "test_plan_close_releases_and_plan_stays_usable": lambda p: [_c((1 << 16,), C64, 64)],
        "test_two_ranks_share_one_gpu_sharded_path": None,
        "test_hipfft_and_libmifft_agree_on_the_comparator_shapes": None,
        "test_perf_table_quick_uses_the_reference_formula": None,
        "test_plan_following_two_torch_streams_without_host_sync": lambda p: [_c((1 << 18,), C64, 160)],
        "test_plan_for_a_device_given_by_index": lambda p: [_c((4096,), C64, 4)],
        "test_device_props_carry_cus_xcds_and_caches": None,
        "test_plan_with_stream_and_context_index": lambda p: [_c((8192,), C64, 3)],
        "test_four_ranks_share_one_gpu": lambda p: [_c((1 << 20,), C64, 40)],
        "test_captured_execute_replays_bit_identically": lambda p: [_c(p["shape"], p["dtype"], p["batch"])],
        "test_plans_of_four_host_threads_run_side_by_side": "threads",
        "test_torch_cuda_graph_around_execute": lambda p: [_c((1 << 18,), C64, 160)],
        "test_sharded_plan_two_shards_on_one_device": lambda p: [_c(p["shape"], p["dtype"], p["batch"] // 2)],
        "test_bench_single_process_four_shards_share_one_gpu": lambda p: [_c((1 << 20,), C64, 40)],
    },
    "test_instances_gpu": {
        "test_instance": lambda p: [_c(p["case"][0], numpy.dtype(p["case"][1]).type, p["case"][2])],
        "test_instance_sides": lambda p: [_c(p["case"][0], numpy.dtype(p["case"][1]).type, p["case"][2])],
    },
    "test_extension_instances_gpu": {
        "test_extension_instance": None,     # (extension keys: extension_covered_keys)
    },
    "test_form_instances_gpu": {
        "test_form_instance": None,          # (form keys: form_covered_keys)
    },
}


def test_functions(modname):
    mod = importlib.import_module(modname)
    return mod, sorted(n for n in dir(mod) if n.startswith("test_") and callable(getattr(mod, n)))


def collected_cases():
    """[(module, test, (shape, dtype, batch, mode))] of every default-collected GPU test; raises if a test function of a GPU module
    has no entry in REGISTRY (a new test must say what it covers)."""
    import os
    assert not os.environ.get("PYFFT_AMD_SWEEP"), "the coverage rule is about the DEFAULT collection: unset PYFFT_AMD_SWEEP"
    out = []
    for modname in GPU_MODULES:
        mod, fns = test_functions(modname)
        reg = REGISTRY[modname]
        if reg is None:
            continue
        missing = [f for f in fns if f not in reg]
        stale = [f for f in reg if f not in fns]
        if missing or stale:
            raise AssertionError("tests/kernel_coverage.py REGISTRY[%r]: no entry for %r, stale entries %r" % (modname, missing, stale))
        for f in fns:
            ad = reg[f]
            if ad is None:
                continue
            if ad == "nd2z":
                cases = [_c(sh, dt, 11) for dt in (C64, C128) for sh in mod.ND2Z_SHAPES[dt]]
            elif ad == "threads":
                cases = [_c(sh, dt, b) for sh, b, dt, _ in mod.THREAD_CASES]
            else:
                cases = list(itertools.chain.from_iterable(ad(p) for p in params_of(getattr(mod, f))))
            out += [(modname, f, c) for c in cases]
    return out


def covered_keys(cases=None):
    """{key: (module, test)} over the collected cases"""
    out = {}
    for modname, f, (shape, dtype, batch, mode) in (collected_cases() if cases is None else cases):
        for k in keys_of(shape, dtype, batch, mode):
            if k is not None:
                out.setdefault(k, (modname, f))
    return out


# ---- the opt-in extensions (pyfft_amd/generic.py: Plan(..., any_size=True), Plan(tile, parent_shape=...)) ----------------------------
# Their kernels (csrc/fft_mixed.hip, fft_mixed_nd.hip, fft_nd2t*.hip) are instances no power-of-two plan selects.  The form a plan takes
# is GenericFFTPlan's own selection, run here on the model of the full part (a plan on FakeContext: tables are uploaded nowhere); the
# launch geometry comes from the library's host queries (mifft_mixed_radices, mifft_mixed_long_split, mifft_bluestein_padded,
# mifft_mixed_nd_supported, mifft_nd_tiled_supported).
#   mixed_row   (prec, n)                       every smooth length of one tile that is no power of two: every radix list of the rows
#   mixed_stage (instance, prec, R, position)   the stage loops of the lines kernel (MODE 1), the long transform's first pass (MODE 2),
#                                               the N-D kernel, both Bluestein kernels: every radix first / middle / last in the list
#   blue1       (prec, tile | big)              the one-launch Bluestein kernel on a 1-D length
#   blue_work   (prec, layout, 1d | nd, pow2 | one_launch)   Bluestein axes on the work array
#   tiled       (prec, layout, tile shape)      one launch straight on the parent array
#   long        (prec, largest | beyond)        the largest N mifft_mixed_long_split takes; the next smooth N, which takes Bluestein
#   split       (prec, form)                    split planes through the work array (gather / scatter)
_ext_plans = {}


def ext_plan(shape, dtype, parent=None):
    """a GenericFFTPlan on FakeContext, cached: its tables go nowhere, so they are not evaluated either (zeros of the right length)"""
    from pyfft_amd import generic
    key = (tuple(shape), numpy.dtype(dtype).name, parent)
    if key not in _ext_plans:
        kw = {"parent_shape": parent} if parent is not None else {"any_size": True}
        saved = generic._unit_roots, generic._chirp, generic._bluestein_spectrum
        generic._unit_roots = lambda count, step, period: numpy.zeros(count, numpy.complex128)
        generic._chirp = lambda n, *a: numpy.zeros(n, numpy.complex128)
        generic._bluestein_spectrum = lambda n, m: numpy.zeros(m, numpy.complex128)
        try:
            _ext_plans[key] = generic.GenericFFTPlan(FakeContext(full_machine()), tuple(shape), dtype=dtype, **kw)
        finally:
            generic._unit_roots, generic._chirp, generic._bluestein_spectrum = saved
    return _ext_plans[key]


def _prec_name(dtype):
    return "f64" if _is_double(dtype) else "f32"


def mixed_radices(n):
    import ctypes
    from pyfft_amd import _native as N
    r = (ctypes.c_int32 * N.MIFFT_MIXED_MAX_STAGES)()
    k = N.lib.mifft_mixed_radices(N.F32, int(n), r)
    assert k > 0, n
    return list(r[:k])


def _stage_keys(instance, prec, lengths):
    """(mixed_stage, instance, prec, R, position) of a launch whose stage list is the radix lists of `lengths`, one after the other"""
    rad = list(itertools.chain.from_iterable(mixed_radices(n) for n in lengths if n > 1))
    out = set()
    for i, R in enumerate(rad):
        if i == 0:
            out.add(("mixed_stage", instance, prec, R, "first"))
        if i == len(rad) - 1:
            out.add(("mixed_stage", instance, prec, R, "last"))
        if 0 < i < len(rad) - 1:
            out.add(("mixed_stage", instance, prec, R, "middle"))
    return out


def form_of(plan):
    """the attribute of the form a GenericFFTPlan takes"""
    for f in ("_tiled", "_direct_nd1", "_direct_nd_planes", "_direct_long", "_direct_blue", "_direct_mixed"):
        if getattr(plan, f):
            return f
    if plan._direct_nd is not None:
        return "_direct_nd"
    return "_uses_work"


def extension_keys(shape, dtype, parent=None):
    """the extension keys one plan exercises (any batch: every form runs the same kernels at every batch)"""
    from pyfft_amd.generic import _is_pow2
    plan = ext_plan(shape, dtype, parent)
    prec = _prec_name(dtype)
    lay = "split" if _split(dtype) else "interleaved"
    x, y, z = plan._xyz
    form = form_of(plan)
    keys = set()
    if form == "_tiled":
        keys.add(("tiled", prec, lay, (x, y, z)))
    elif form == "_direct_mixed":
        keys.add(("mixed_row", prec, x))
    elif form == "_direct_nd1":
        keys |= _stage_keys("nd", prec, (x, y, z))
    elif form == "_direct_nd_planes":
        keys |= _stage_keys("nd", prec, (x, y)) | _stage_keys("lines", prec, (z,))
    elif form == "_direct_nd":
        for a, n in enumerate((x, y, z)):
            if n > 1 and a > 0 and (x, y, z)[:a] != (1,) * a:
                keys |= _stage_keys("lines", prec, (n,))
    elif form == "_direct_long":
        n1, n2 = plan._direct_long[:2]
        keys |= _stage_keys("long_first", prec, (n1,)) | _stage_keys("lines", prec, (n2,))
        keys.add(("long", prec))
        if x == long_limits(dtype)[0]:
            keys.add(("long", prec, "largest"))
    elif form == "_direct_blue":
        m = plan._axes[0].blue[0]
        big = m > (2048 if prec == "f64" else 4096)
        keys.add(("blue1", prec, "big" if big else "tile"))
        keys |= _stage_keys("blue_big" if big else "blue", prec, (m,))
    else:
        dims = "1d" if (y, z) == (1, 1) else "nd"
        if dims == "1d" and not _split(dtype) and x == long_limits(dtype)[1]:
            keys.add(("long", prec, "beyond"))
        for ax in plan._axes:
            if ax.blue is not None:
                keys.add(("blue_work", prec, lay, dims, "one_launch"))
            elif not ax.pow2 and ax.mixed_tw is None:
                keys.add(("blue_work", prec, lay, dims, "pow2"))
        if lay == "split":
            keys.add(("split", prec, "tiles" if parent is not None else ("pow2" if all(_is_pow2(v) for v in (x, y, z)) else "any_size")))
    return keys


def _smooth_upto(limit):
    out = []
    for n in range(2, limit + 1):
        m = n
        for c in (2, 3, 5, 7):
            while m % c == 0:
                m //= c
        if m == 1:
            out.append(n)
    return out


def long_limits(dtype):
    """(the largest N mifft_mixed_long_split takes, the smallest smooth N beyond it) for the precision of `dtype`"""
    prec = _prec_name(dtype)
    if prec not in _long_limits:
        _long_limits[prec] = _long_limits_of(dtype)
    return _long_limits[prec]


_long_limits = {}


def _long_limits_of(dtype):
    import ctypes
    from pyfft_amd import _native as N
    prec = N.F64 if _is_double(dtype) else N.F32
    a, b = ctypes.c_int32(0), ctypes.c_int32(0)
    ok = [n for n in _smooth_upto(1 << 20) if n > 4096 and N.lib.mifft_mixed_long_split(prec, n, ctypes.byref(a), ctypes.byref(b)) == 0]
    top = max(ok)
    beyond = min(n for n in _smooth_upto(1 << 21) if n > top)
    return top, beyond


def tiled_tile_shapes(dtype):
    """numpy tile shapes (2-D and 3-D, power-of-two axes up to 256) with a one-launch tiled kernel (mifft_nd_tiled_supported)"""
    from pyfft_amd import _native as N
    prec = N.F64 if _is_double(dtype) else N.F32
    pows = [1 << k for k in range(0, 9)]
    out = []
    for z in pows[:7]:
        for y in pows:
            for x in pows:
                if (x > 1) + (y > 1) + (z > 1) < 2 or x * y * z > (1 << 16):
                    continue
                if N.lib.mifft_nd_shape_supported(prec, x, y, z, N.VARIANT_INTERLEAVED_ONLY) == 0 and N.lib.mifft_nd_tiled_supported(prec, x, y, z) == 0:
                    out.append((y, x) if z == 1 else (z, y, x))
    return out


def _ext_candidates():
    """(shape, dtype, parent) of the candidate plans: every 1-D length up to 5000 (the one-launch Bluestein limit), the long limits,
    2-D / 3-D shapes of smooth and prime axes, the tiled tile shapes, in the four dtypes"""
    small = _smooth_upto(64)
    for dtype in ALL_DTYPES:
        for n in (range(3, 5001) if not _split(dtype) else (12, 17, 1009, 4099, 5000)):
            if n & (n - 1):
                yield (n,), dtype, None
        top, beyond = long_limits(dtype)
        yield (top,), dtype, None
        yield (beyond,), dtype, None
        for yv in small + [100, 128, 210, 256, 512, 1000]:
            for xv in (3, 5, 7, 12, 15, 16, 60, 64, 100, 210, 1000):
                if (xv & (xv - 1)) or (yv & (yv - 1)):
                    yield (yv, xv), dtype, None
        for sh in ((12, 10, 14), (60, 60, 60), (5, 6, 7), (9, 8, 15), (6, 64, 64), (3, 128, 128)):
            yield sh, dtype, None
        for sh in ((17, 4), (4, 17), (5000, 4), (4099, 4), (3, 17, 4), (4, 1009)):
            yield sh, dtype, None
        for t in tiled_tile_shapes(dtype):
            yield t, dtype, tuple(v * f for v, f in zip(t, (2, 3, 2)))
        yield (16, 4), dtype, (64, 64)


_ext_table = []


def _ext_candidate_keys():
    """[(order, shape, dtype, parent, bytes per item, keys)] of every candidate (computed once)"""
    if not _ext_table:
        for order, (shape, dtype, parent) in enumerate(_ext_candidates()):
            size = _prod(parent if parent is not None else shape) * (16 if _is_double(dtype) else 8)
            _ext_table.append((order, shape, dtype, parent, size, extension_keys(shape, dtype, parent)))
    return _ext_table


def extension_universe():
    """{key: the first candidate (shape, dtype name, parent) that selects it}"""
    out = {}
    for order, shape, dtype, parent, size, keys in _ext_candidate_keys():
        for k in keys:
            out.setdefault(k, (shape, numpy.dtype(dtype).name, parent))
    return out


def _ragged_batch(shape, dtype, parent):
    """at least 3 items, and a last work-group that is partly filled: rows (items times the lines of an axis) no multiple of the
    work-group's count where a work-group holds several"""
    n = _prod(shape)
    full = 2048 if _is_double(dtype) else 4096
    if parent is not None or len(shape) > 1 or n > full // 2:
        return 3
    W = (full // 2) // n
    return 2 * W + 1 if W > 1 else 3


def extension_audit_cases():
    """[(shape, dtype name, batch, parent, form, keys)]: for every key of extension_universe(), the smallest candidate that selects it
    (bytes per item, then the candidate order); a candidate that is the smallest for several keys appears once"""
    best = {}
    for order, shape, dtype, parent, size, keys in _ext_candidate_keys():
        for k in keys:
            if k not in best or (size, order) < best[k][:2]:
                best[k] = (size, order, shape, dtype, parent)
    cases = {}
    for k, (_, order, shape, dtype, parent) in best.items():
        cases.setdefault((order, shape, dtype, parent), []).append(k)
    out = []
    for (order, shape, dtype, parent), ks in sorted(cases.items(), key=lambda kv: kv[0][0]):
        form = form_of(ext_plan(shape, dtype, parent))
        out.append((shape, numpy.dtype(dtype).name, _ragged_batch(shape, dtype, parent), parent, form, tuple(sorted(ks, key=str))))
    return out


def extension_covered_keys():
    """{key: case} over the cases of tests/test_extension_instances_gpu.py, read off its parametrize mark"""
    mod = importlib.import_module("test_extension_instances_gpu")
    out = {}
    for p in params_of(mod.test_extension_instance):
        shape, dtname, batch, parent, form, keys = p["case"]
        for k in extension_keys(shape, numpy.dtype(dtname), parent):
            out.setdefault(k, p["case"])
    return out


# ---- the four forms (pyfft_amd/real.py, conv.py, r2r.py, half.py) -------------------------------------------------------------------
# Plan(real=True), Plan(convolve=True), Plan(r2r=...) and Plan(dtype="complex32") run kernels of their own around (or instead of) an
# inner power-of-two plan, whose instances universe() holds already.  The form a plan takes is the plan's own selection, made in its
# __init__ on the model of the full part (a plan on FakeContext whose _build is skipped: no tables, no inner plans); the launch
# geometry comes from the library's host queries and the launchers' own rules.  Keys of an execute on 16-byte-aligned bases, both
# directions:
#   real_row      (prec, n, direction)                       the one-launch real row (mifft_real_row_supported)
#   real_post     (prec, direction, lanes, rank)             the separation / packing launch of composed real plans (lanes: real_post_lanes)
#   conv_row      (prec, real, n)                            the one-launch convolution row (mifft_conv_row_supported)
#   mul_spectrum  (prec, vector | scalar, shared | per_item, correlate)   the spectrum product of composed convolutions (vector: the
#                                                            fp32 16-byte path of csrc/fft_aux.hip: an even point count on 16-byte bases)
#   r2r_row       (prec, n, kind, direction)                 the one-launch cosine / sine row (mifft_r2r_row_supported)
#   r2r_perm      (prec, rank, vec | scalar, direction)      the permutation step of the composed r2r form (launch_perm: vec = nl % 4 == 0)
#   r2r_orbit     (prec, rank, fold | no_fold | one_lane, direction)   its twiddle step (launch_orbit: fold = L / 2 >= 64; nl = 2: one lane)
#   r2r_fallback  (prec, n)                                  a fused r2r row run on a base that is not 16-byte aligned: the composed form
#   half          (kernel, variant)                          the complex32 instance, half_kernel(dims, plan.variant(batch))
FORMS = ("real", "conv", "r2r", "half")
FORM_DTYPES = {"real": ("float32", "float64"), "conv": ("complex64", "float32", "complex128", "float64"), "r2r": ("float32", "float64"),
               "half": ("complex32",)}
FORM_ITEM_BYTES = {"float32": 4, "float64": 8, "complex64": 8, "complex128": 16, "complex32": 4}     # per point of the input
R2R_KINDS = ("dct", "dst")
_form_plans = {}


def form_plan(form, shape, dtname, kind=None):
    """the plan of a form on FakeContext(full_machine()), its _build skipped (the form is selected in __init__), cached; ValueError for a
    shape the form has no plan of"""
    key = (form, tuple(shape), dtname, kind)
    if key not in _form_plans:
        ctx = FakeContext(full_machine())
        shape = tuple(int(v) for v in shape)
        if form == "real":
            from pyfft_amd.real import RealFFTPlan as cls
            kw = {"dtype": dtname}
        elif form == "conv":
            from pyfft_amd.conv import ConvPlan as cls
            kw = {"dtype": dtname, "real": dtname.startswith("float")}
        elif form == "r2r":
            from pyfft_amd.r2r import R2RPlan as cls
            kw = {"dtype": dtname, "r2r": kind}
        else:
            from pyfft_amd.half import HalfFFTPlan as cls
            kw = {"dtype": "complex32"}
        saved = cls._build
        cls._build = lambda self: None
        try:
            _form_plans[key] = cls(ctx, shape, **kw)
        finally:
            cls._build = saved
    return _form_plans[key]


def real_post_lanes(nx):
    """threads per row segment of mifft_real_post_launch (csrc/fft_real.hip): the power of two >= nx / 2, at most 256"""
    lanes = 1
    while lanes < nx // 2 and lanes < 256:
        lanes *= 2
    return lanes


def form_keys_of_plan(form, plan, dtname, batch, kind=None):
    """the form keys an execute of `batch` items takes in both directions on 16-byte-aligned bases (a model plan of form_plan, or a
    device plan: what its own selection takes); a convolution: its four spectrum variants"""
    prec = "f64" if dtname in ("float64", "complex128") else "f32"
    dirs = ("forward", "inverse")
    keys = set()
    if form == "real":
        nx = plan._shape[-1]
        if plan._real_form == "fused_row":
            keys |= set(("real_row", prec, nx, d) for d in dirs)
        else:
            keys |= set(("real_post", prec, d, real_post_lanes(nx), len(plan._shape)) for d in dirs)
    elif form == "conv":
        if plan.conv_form == "fused_row":
            keys.add(("conv_row", prec, bool(plan._real), int(plan._shape[0])))
        else:
            vec = prec == "f32" and plan._spec_points % 2 == 0          # (the per-item pitch is the point count: even with it)
            for spectrum in ("shared", "per_item"):
                for correlate in (False, True):
                    keys.add(("mul_spectrum", prec, "vector" if vec else "scalar", spectrum, correlate))
    elif form == "r2r":
        kept = plan._kept
        if plan.r2r_form == "fused_row":
            keys |= set(("r2r_row", prec, kept[0], kind, d) for d in dirs)
            keys.add(("r2r_fallback", prec, kept[0]))
        elif kept:
            nl = kept[-1]
            perm = "vec" if nl % 4 == 0 else "scalar"
            orbit = "one_lane" if nl == 2 else ("fold" if nl // 4 >= 64 else "no_fold")
            for d in dirs:
                keys.add(("r2r_perm", prec, len(kept), perm, d))
                keys.add(("r2r_orbit", prec, len(kept), orbit, d))
    else:
        from pyfft_amd.half import half_kernel
        v = plan.variant(batch)
        keys.add(("half", half_kernel(plan.dims, v), v))
    return keys


def form_keys(form, shape, dtname, batch, kind=None):
    return form_keys_of_plan(form, form_plan(form, shape, dtname, kind), dtname, batch, kind)


def form_batch(shape):
    """items of a form case: 67 for items of up to 2048 points (a prime above every row count of a work-group of such rows except the
    shortest, whose one work-group 67 rows leave partly filled), else 3 (a prime above the one or two rows a work-group of longer rows
    holds)"""
    return 67 if _prod(shape) <= 2048 else 3


_form_table = []


def _form_candidate_keys():
    """[(order, form, shape, dtype name, kind, bytes per item, batch, keys, big)] of every plan of the four forms over the power-of-two
    shapes of up to 2^24 points; `big`: keys only a batch of universe()'s sides per side reaches (complex32's variant rule)"""
    if not _form_table:
        order = 0
        for shape in _shapes(MAX_LOG2_POINTS):
            for form in FORMS:
                for dtname in FORM_DTYPES[form]:
                    for kind in (R2R_KINDS if form == "r2r" else (None,)):
                        try:
                            plan = form_plan(form, shape, dtname, kind)
                        except ValueError:
                            continue            # (complex32: a shape without a one-launch kernel)
                        item = _prod(shape) * FORM_ITEM_BYTES[dtname]
                        batch = form_batch(shape)
                        keys = form_keys_of_plan(form, plan, dtname, batch, kind)
                        big = set()
                        if form == "half":
                            for side in UNIVERSE_SIDES:
                                big |= form_keys_of_plan(form, plan, dtname, max(1, side // item), kind)
                        _form_table.append((order, form, shape, dtname, kind, item, batch, keys, big - keys))
                        order += 1
    return _form_table


def form_universe():
    """{key: the first candidate (form, shape, dtype name, kind) that reaches it}"""
    out = {}
    for order, form, shape, dtname, kind, item, batch, keys, big in _form_candidate_keys():
        for k in keys | big:
            out.setdefault(k, (form, shape, dtname, kind))
    return out


def form_audit_cases():
    """[(form, shape, dtype name, batch, kind, keys)]: for every key of form_universe(), the smallest candidate that reaches it at its
    batch (bytes per side, then the candidate order); a candidate that is the smallest for several keys appears once.  A key that only
    a bigger batch reaches raises (the audit must not silently lose an instance)."""
    best = {}
    for order, form, shape, dtname, kind, item, batch, keys, big in _form_candidate_keys():
        for k in keys:
            if k not in best or (item * batch, order) < best[k][:2]:
                best[k] = (item * batch, order)
    missing = sorted(set(form_universe()) - set(best), key=str)
    if missing:
        raise AssertionError("tests/kernel_coverage.py form_audit_cases: no case at a ragged batch reaches %r" % (missing[:40],))
    table = dict((c[0], c) for c in _form_candidate_keys())
    cases = {}
    for k, (_, order) in best.items():
        cases.setdefault(order, []).append(k)
    out = []
    for order in sorted(cases):
        _, form, shape, dtname, kind, item, batch, keys, big = table[order]
        out.append((form, shape, dtname, batch, kind, tuple(sorted(cases[order], key=str))))
    return out


def form_covered_keys():
    """{key: case} over the cases of tests/test_form_instances_gpu.py, read off its parametrize mark"""
    mod = importlib.import_module("test_form_instances_gpu")
    out = {}
    for p in params_of(mod.test_form_instance):
        form, shape, dtname, batch, kind, keys = p["case"]
        for k in form_keys(form, shape, dtname, batch, kind):
            out.setdefault(k, p["case"])
    return out
