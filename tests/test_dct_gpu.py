"""Cosine and sine transforms on the device: Plan(shape, dtype=float32 | float64, r2r="dct" | "dst") against an extended-precision
reference of scipy's dctn / dstn (type 2) and their inverses (tests/dct_model.py), held to the project's per-item accuracy bound with the
levels tests/test_dct_cpu.py justifies; guard bands, a poisoned neighbour item, in place vs out of place, and stream / graph interop.
No scipy here: the reference is numpy's FFT of the mirror extension."""
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dct_model as M                                                # noqa: E402
from dct_cases import COMPOSED, FUSED, ROWS, levels                         # noqa: E402
from helpers import GuardedBuffer, accuracy_bound, item_error, sampled_items   # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = numpy.float32, numpy.float64


def _hip():
    import pyfft_amd.hip as hip
    if hip.device_count() < 1:
        pytest.fail("no HIP device")
    return hip


def _data(shape, dtype, batch, seed):
    return numpy.random.default_rng(seed).standard_normal((batch,) + tuple(shape)).astype(dtype)


def _check(shape, dtype, kind, inp, got, inverse, ortho=False, normalize=True, scale=1.0, items=None, what=""):
    n = int(numpy.prod(shape))
    l1b, mxb = accuracy_bound(dtype, n, levels=levels(shape))
    items = range(len(inp)) if items is None else items
    for j in items:
        ref = M.reference(inp[j], kind, inverse, ortho, normalize, scale, double=dtype == F64)
        l1, mx = item_error(got[j], ref)
        assert l1 <= l1b and mx <= mxb, "%s %s %s %s item %d %s: L1 %.3g (bound %.3g) max %.3g (bound %.3g)" % (
            what, kind, shape, numpy.dtype(dtype).name, j, "inverse" if inverse else "forward", l1, l1b, mx, mxb)


def _run_guarded(hip, plan, shape, dtype, batch, inverse, seed, poison=None):
    """One out-of-place execute between guard bands (the input must come back untouched), then the same in place, which must be
    bit-identical; item `poison` of the input holds a NaN, which must not reach its neighbours."""
    from pyfft_amd import _native as N
    inp = _data(shape, dtype, batch, seed)
    if poison is not None:
        inp[poison].reshape(-1)[0] = numpy.nan
    gi = GuardedBuffer(inp.nbytes, 16)
    go = GuardedBuffer(inp.nbytes, 48)
    N.check(N.lib.mifft_memcpy_h2d(gi.ptr, inp.ctypes.data, inp.nbytes, None), "h2d")
    plan.execute(gi.ptr, go.ptr, inverse=inverse, batch=batch)
    got = numpy.empty_like(inp)
    N.check(N.lib.mifft_memcpy_d2h(got.ctypes.data, go.ptr, inp.nbytes, None), "d2h")
    back = numpy.empty_like(inp)
    N.check(N.lib.mifft_memcpy_d2h(back.ctypes.data, gi.ptr, inp.nbytes, None), "d2h")
    assert numpy.array_equal(back, inp, equal_nan=True), "the out-of-place input was modified"
    plan.execute(gi.ptr, inverse=inverse, batch=batch)
    inplace = numpy.empty_like(inp)
    N.check(N.lib.mifft_memcpy_d2h(inplace.ctypes.data, gi.ptr, inp.nbytes, None), "d2h")
    gi.check_guards("input")
    go.check_guards("output")
    gi.free()
    go.free()
    assert numpy.array_equal(inplace, got, equal_nan=True), "in place differs from out of place"
    return inp, got


def _batch(shape, dtype):
    n = int(numpy.prod(shape)) * numpy.dtype(dtype).itemsize
    return 67 if n <= (16 << 10) else (3 if n <= (64 << 20) else 1)


def _case(shape, dtype, kind, inverse, form=None, **kw):
    hip = _hip()
    plan = hip.Plan(shape, dtype=dtype, r2r=kind, **kw)
    if form is not None:
        assert plan.r2r_form == form, (plan.r2r_form, plan.kernel)
    batch = _batch(shape, dtype)
    poison = 1 if batch >= 3 else None
    inp, got = _run_guarded(hip, plan, shape, dtype, batch, inverse, seed=int(numpy.prod(shape)) + batch, poison=poison)
    keep = [j for j in range(batch) if j != poison]
    assert numpy.isfinite(got[keep]).all(), "a poisoned item leaked into its neighbours"
    n = int(numpy.prod(shape))
    items = [j for j in sampled_items(batch, n) if j != poison] or keep[:1]
    _check(shape, dtype, kind, inp, got, inverse, items=items, what="composed", **{k: v for k, v in kw.items() if k != "dtype"})


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("kind", ["dct", "dst"])
@pytest.mark.parametrize("dtype,n", FUSED, ids=["%s-%d" % (numpy.dtype(d).name, n) for d, n in FUSED])
def test_r2r_fused_row_instance(dtype, n, kind, inverse):
    """One case per one-launch row instance: guard bands, a ragged last work-group, a poisoned item, in place == out of place."""
    _case((n,), dtype, kind, inverse, form="fused_row")


@pytest.mark.parametrize("dtype,n", [(F32, 1024), (F64, 64), (F32, 4096), (F32, 16)], ids=str)
def test_r2r_misaligned_rows(dtype, n):
    """Buffers offset by one real number: the composed form's one-point permutation path (and, for a fused plan, the composed form
    instead of the 16-byte row kernel)."""
    hip = _hip()
    from pyfft_amd import _native as N
    s = numpy.dtype(dtype).itemsize
    for kind in ("dct", "dst"):
        for inverse in (False, True):
            plan = hip.Plan((n,), dtype=dtype, r2r=kind)
            x = _data((n,), dtype, 5, n)
            gi = GuardedBuffer(x.nbytes + 16, 16)
            go = GuardedBuffer(x.nbytes + 16, 48)
            N.check(N.lib.mifft_memcpy_h2d(gi.ptr + s, x.ctypes.data, x.nbytes, None), "h2d")
            plan.execute(gi.ptr + s, go.ptr + s, inverse=inverse, batch=5)
            got = numpy.empty_like(x)
            N.check(N.lib.mifft_memcpy_d2h(got.ctypes.data, go.ptr + s, x.nbytes, None), "d2h")
            gi.check_guards("input")
            go.check_guards("output")
            gi.free()
            go.free()
            _check((n,), dtype, kind, x, got, inverse, what="misaligned")


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("kind", ["dct", "dst"])
@pytest.mark.parametrize("dtype,n", ROWS, ids=["%s-%d" % (numpy.dtype(d).name, n) for d, n in ROWS])
def test_r2r_row(dtype, n, kind, inverse):
    """Every row length a real-row kernel exists for, and n = 1, 2: guard bands, a ragged batch (67 rows of the short ones), a poisoned
    item, in place == out of place."""
    _case((n,), dtype, kind, inverse)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("kind", ["dct", "dst"])
@pytest.mark.parametrize("dtype,shape", COMPOSED, ids=["%s-%s" % (numpy.dtype(d).name, s) for d, s in COMPOSED])
def test_r2r_composed(dtype, shape, kind, inverse):
    _case(shape, dtype, kind, inverse)


# the inner plan each composed shape is chosen to reach (plan.inner_plan.strategy(batch, inplace=True)[0])
INNER = [((8, 8), 4096), ((64, 64), 64), ((1024, 1024), 2), ((64, 64, 64), 2), ((1 << 21,), 2)]


@pytest.mark.parametrize("shape,batch", INNER, ids=str)
def test_r2r_composed_inner_strategy(shape, batch):
    """The composed shapes reach the inner plan's strategies: the packed shape's own selection, recorded here so that a change of it
    shows; every one is checked against the reference."""
    hip = _hip()
    plan = hip.Plan(shape, dtype=F32, r2r="dct")
    assert plan.r2r_form == "composed" and plan.inner_plan is not None
    x = _data(shape, F32, batch, 2)
    g = hip.to_gpu(x)
    y = hip.DeviceArray(x.shape, F32)
    plan.execute(g, y, batch=batch)
    strat = plan.inner_plan.strategy(batch, inplace=True)
    assert isinstance(strat, tuple) and strat, strat
    print("inner strategy", shape, batch, strat)
    got = y.get()
    items = sampled_items(batch, int(numpy.prod(shape)))
    _check(shape, F32, "dct", x, got, False, items=items, what="inner %s" % (strat[0],))


SAMPLE = [(F32, (256,)), (F64, (4096,)), (F32, (8, 8)), (F64, (4, 1, 16)), (F32, (1,)), (F32, (16, 64))]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("kind", ["dct", "dst"])
@pytest.mark.parametrize("dtype,shape", SAMPLE, ids=["%s-%s" % (numpy.dtype(d).name, s) for d, s in SAMPLE])
def test_r2r_ortho_and_unnormalised(dtype, shape, kind, inverse):
    _case(shape, dtype, kind, inverse, ortho=True)
    _case(shape, dtype, kind, inverse, normalize=False, scale=3.0)


@pytest.mark.parametrize("dtype,shape", [(F32, (1024,)), (F64, (64, 64)), (F32, (8, 4, 16)), (F32, (1, 8)), (F64, (2,))], ids=str)
def test_r2r_round_trip(dtype, shape):
    hip = _hip()
    for kind in ("dct", "dst"):
        for ortho in (False, True):
            plan = hip.Plan(shape, dtype=dtype, r2r=kind, ortho=ortho)
            x = _data(shape, dtype, 2, 3)
            g = hip.to_gpu(x)
            plan.execute(g, batch=2)
            plan.execute(g, inverse=True, batch=2)
            y = g.get()
            l1b, mxb = accuracy_bound(dtype, int(numpy.prod(shape)), levels=2 * levels(shape))
            for j in range(2):
                l1, mx = item_error(y[j], x[j].astype(numpy.float64))
                assert l1 <= l1b and mx <= mxb, (kind, ortho, l1, mx)


def test_r2r_torch_stream_and_graphs():
    hip = _hip()
    import torch
    shape = (32, 64)
    dev = torch.device("cuda:0")
    x = torch.randn((3,) + shape, device=dev, dtype=torch.float32)
    y = torch.empty_like(x)
    plan = hip.Plan(shape, dtype=F32, r2r="dct")
    plan.execute(x, y, batch=3)
    _check(shape, F32, "dct", x.cpu().numpy(), y.cpu().numpy(), False, what="torch")
    # asynchronous on a side torch stream
    s = torch.cuda.Stream(device=dev)
    aplan = hip.Plan(shape, dtype=F32, r2r="dct", stream=s)
    out = torch.empty_like(x)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        ret = aplan.execute(x, out, batch=3)
    assert ret is not None
    s.synchronize()
    assert torch.equal(out, y)
    # torch.cuda.graph capture of forward + inverse, replayed twice: bit-identical to the eager execute
    gplan = hip.Plan(shape, dtype=F32, r2r="dst", stream=s)
    xs = x.clone()
    o1 = torch.empty_like(x)
    y1 = torch.empty_like(x)
    with torch.cuda.stream(s):
        gplan.execute(xs, o1, batch=3)
        gplan.execute(o1, y1, inverse=True, batch=3)
    s.synchronize()
    eager_o, eager_y = o1.clone(), y1.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        gplan.execute(xs, o1, batch=3, wait_for_finish=False)
        gplan.execute(o1, y1, inverse=True, batch=3, wait_for_finish=False)
    for _ in range(2):
        o1.zero_()
        y1.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o1, eager_o) and torch.equal(y1, eager_y)
    assert (y1 - x).abs().max().item() <= 1e-4 * x.abs().max().item()


def test_r2r_hip_graph_capture():
    hip = _hip()
    s = hip.Stream()
    shape = (1 << 14,)
    plan = hip.Plan(shape, dtype=F64, r2r="dct", ortho=True, stream=s)
    x = _data(shape, F64, 2, 11)
    gx = hip.to_gpu(x)
    gy = hip.DeviceArray((2,) + shape, F64)
    plan.execute(gx, gy, batch=2)
    s.synchronize()
    eager = gy.get()
    gy.set(numpy.zeros_like(eager))
    with hip.Graph(s) as g:
        plan.execute(gx, gy, batch=2)
    g.launch()
    g.launch()
    s.synchronize()
    assert numpy.array_equal(gy.get(), eager)
    _check(shape, F64, "dct", x, eager, False, ortho=True, what="graph")


def test_r2r_short_buffer_and_overlap():
    hip = _hip()
    plan = hip.Plan((64,), dtype=F32, r2r="dct")
    a = hip.DeviceArray((4, 64), F32)
    b = hip.DeviceArray((3, 64), F32)
    with pytest.raises(ValueError, match="r2r"):
        plan.execute(a, b, batch=4)
    with pytest.raises(ValueError, match="r2r"):
        plan.execute(a.ptr, a.ptr + 64, batch=2)
