"""The opt-in extensions' kernels held to the per-instance contract (docs/parity.md), like tests/test_instances_gpu.py holds the
power-of-two ones: one case per extension key (kernel_coverage.extension_audit_cases(): every smooth row length of a tile, every radix at
every stage position of the lines / long / N-D / Bluestein kernels, the one-launch Bluestein kernels, Bluestein axes on the work array,
every tiled tile shape, the long transform's largest length and the first one beyond it, split planes through the gather / scatter).
Each case runs through Plan(shape, any_size=True) or Plan(tile, parent_shape=parent), with the plan's own tables, and asserts the form
the plan takes.  Batches leave the last work-group of a launch partly filled.

  1.-4. the steps of helpers.run_contract, against the bound of helpers.accuracy_bound with L = helpers.any_size_levels(shape): guards,
        bases 16- but not 64-byte aligned, input untouched, in place bit-identical to out of place, inverse, poisoned items
  5.    inverse with normalize=False, scale=3.0 (a second plan): the scale and the conjugation these kernels fold into their last stage
  6.    tiled plans: one tile inside a parent array poisoned; every other tile, of that parent and of the others, bit-identical

Each case reports the worst item's error ratios (metric / (u (L + 2))) as junit properties (`record_property`)."""
import numpy
import pytest

import kernel_coverage as KC
from helpers import _Case, any_size_levels, run_contract

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("ignore:record_property is incompatible with junit_family")]    # (the properties are written)

CASES = KC.extension_audit_cases()


def _case_id(case):
    shape, dtname, batch, parent, form, keys = case
    return "-".join(str(v).replace(" ", "") for v in keys[0]) + ("+%d" % (len(keys) - 1) if len(keys) > 1 else "") + \
        "-%s-%s" % ("x".join(map(str, shape)), dtname)


def _tiles(shape, parent):
    """(tile shape, counts) of a tiled case, both as numpy shapes padded to three axes"""
    pad = (1,) * (3 - len(shape))
    tile = pad + tuple(shape)
    counts = pad + tuple(p // t for p, t in zip(parent, shape))
    return tile, counts


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_extension_instance(ctx, case, record_property):
    from pyfft_amd import _native as N
    hip = ctx.hip
    shape, dtname, batch, parent, form, keys = case
    dtype = numpy.dtype(dtname)
    kw = {"parent_shape": parent} if parent is not None else {"any_size": True}
    plan, plan3, c = None, None, None
    try:
        plan = hip.Plan(tuple(shape), dtype=dtype, **kw)
        assert KC.form_of(plan) == form, (KC.form_of(plan), form)
        have = KC.extension_keys(shape, dtype, parent)
        assert set(keys) <= have, sorted(set(keys) - have, key=str)
        item_shape = tuple(parent) if parent is not None else tuple(shape)
        tiles = _tiles(shape, parent) if parent is not None else None
        levels = any_size_levels(shape, dtype) if parent is None else None
        c = _Case(hip, N, (item_shape, dtname, batch), CASES.index(case), tiles=tiles, levels=levels)
        record_property("keys", repr(list(keys)))
        record_property("form", form)
        record_property("levels", str(levels if levels is not None else int(numpy.prod(shape)).bit_length() - 1))
        record_property("base_offsets", "%d/%d" % (c.ins[0].offset, c.outs[0].offset))
        run_contract(plan, c, False, record_property)

        # 5. inverse, normalize off, scale 3 (out of place, fresh data)
        plan3 = hip.Plan(tuple(shape), dtype=dtype, normalize=False, scale=3.0, **kw)
        assert KC.form_of(plan3) == form
        blk = c.fill(c.ins, 303)
        for b in c.outs:
            N.check(N.lib.mifft_memset(b.ptr, 0xFF, b.nbytes, None), "mifft_memset")
        plan3.execute(*([b.ptr for b in c.ins] + [b.ptr for b in c.outs]), batch=batch, inverse=True)
        c._sync()
        c.guards(c.ins, "scaled inverse, input")
        c.guards(c.outs, "scaled inverse, output")
        rep = c.accuracy(c.outs, blk, inverse=True, normalize=False, scale=3.0, what="inverse, normalize off, scale 3")
        record_property("scaled_inverse_l1_ratio", "%.4g" % rep["l1_ratio"])
        record_property("scaled_inverse_max_ratio", "%.4g" % rep["max_ratio"])

        # 6. one tile inside a parent poisoned: every other tile bit-identical to the clean result (c.ref, from run_contract)
        if tiles is not None:
            p = batch // 2
            ntiles = int(numpy.prod(tiles[1]))
            t = ntiles // 2
            for b, x in zip(c.ins, c.x0):
                c._d2d(b.ptr, x.ptr, c.plane_bytes)
            planes = c.item_planes([x.ptr for x in c.x0], p)
            c.tile_of(planes[0], t)[...] = numpy.nan                      # (a view: the tile inside the parent array)
            for b, h in zip(c.ins, planes):
                N.check(N.lib.mifft_memcpy_h2d(b.ptr + p * c.item_bytes, h.ctypes.data, c.item_bytes, None), "mifft_memcpy_h2d")
            for b in c.outs:
                N.check(N.lib.mifft_memset(b.ptr, 0xFF, b.nbytes, None), "mifft_memset")
            plan.execute(*([b.ptr for b in c.ins] + [b.ptr for b in c.outs]), batch=batch)
            c._sync()
            c.guards(c.ins, "one poisoned tile, input")
            c.guards(c.outs, "one poisoned tile, output")
            ib = c.item_bytes
            for b, r in zip(c.outs, c.ref):
                others = [j for j in range(batch) if j != p and c.mismatches(b.ptr + j * ib, r.ptr + j * ib, ib)]
                assert not others, "parents %r changed when tile %d of parent %d was poisoned" % (others, t, p)
            got, want = c.item_planes([b.ptr for b in c.outs], p), c.item_planes([r.ptr for r in c.ref], p)
            for g, w in zip(got, want):
                changed = [k for k in range(ntiles) if k != t and
                           not numpy.array_equal(numpy.ascontiguousarray(c.tile_of(g, k)).view(numpy.uint8),
                                                 numpy.ascontiguousarray(c.tile_of(w, k)).view(numpy.uint8))]
                assert not changed, "tiles %r of parent %d changed when its tile %d was poisoned" % (changed[:20], p, t)
    finally:
        if c is not None:
            c.close()
        for pl in (plan, plan3):
            if pl is not None and hasattr(pl, "close"):
                pl.close()
