"""Overlap-save FIR plans on the device (docs/extensions.md, "FIR filtering plans"): one case per one-launch instance (three blocks, the
last one partial, nine rows so that a work-group holds blocks of two items, guard bands of NaN around x and y, untouched gaps between
the items, a poisoned item), focused cases on the window edges, filter_spectrum, graph capture, torch interop, refusals and lifecycle,
each against numpy.convolve in extended precision within helpers.accuracy_bound with L = 2 log2 n + 1 (two transforms and a product)."""
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fir_model as M                                                    # noqa: E402
from helpers import GuardedBuffer, accuracy_bound, item_error            # noqa: E402

pytestmark = pytest.mark.gpu

PATTERN = 0x5A                # every byte of y before an execute: 0x5A5A5A5A is a finite number in either precision


def _hip():
    import pyfft_amd.hip as hip
    if hip.device_count() < 1:
        pytest.fail("no HIP device")
    return hip


def _N():
    from pyfft_amd import _native as N
    return N


def _h2d(ptr, host):
    _N().check(_N().lib.mifft_memcpy_h2d(ptr, host.ctypes.data, host.nbytes, None), "h2d")


def _d2h(host, ptr):
    _N().check(_N().lib.mifft_memcpy_d2h(host.ctypes.data, ptr, host.nbytes, None), "d2h")
    return host


def bound(dtype, n):
    return accuracy_bound(dtype, n, levels=2 * (int(n).bit_length() - 1) + 1)


def _plan(hip, prec, real, n, m, **kw):
    return hip.Plan(n, dtype=M.plan_dtype(prec, real), convolve=True, real=real, taps=m, **kw)


def _taps(prec, real, m, count, seed):
    return numpy.stack([M.signal(prec, real, m, seed=seed + 31 * j) for j in range(count)])


def _spectrum(hip, plan, h):
    """H of the filters h (count, m) through filter_spectrum, in a guarded buffer"""
    count = h.shape[0]
    cdt = numpy.dtype(M.CDT[h.dtype])
    hd = hip.to_gpu(numpy.ascontiguousarray(h))
    gs = GuardedBuffer(count * plan.spectrum_shape()[0] * cdt.itemsize, 80)
    plan.filter_spectrum(hd, gs.ptr, batch=count)
    plan.finish()
    return gs


def run_guarded(hip, plan, prec, real, n, m, length, batch, pitch, per_item, seed, poison=None, scale=1.0, normalize=True, default_pitch=False):
    """One execute between guard bands; checks the guards, the gaps, the spectrum and the input, and every item but `poison` against
    numpy.convolve.  Returns the worst (L1, max) over the bound."""
    pdt = M.plan_dtype(prec, real)
    total = (batch - 1) * pitch + length
    x = M.signal(prec, real, total, seed)
    if poison is not None:
        x[poison * pitch:poison * pitch + length] = numpy.nan
    h = _taps(prec, real, m, batch if per_item else 1, seed + 1)
    gs = _spectrum(hip, plan, h)
    S = _d2h(numpy.empty(h.shape[0] * plan.spectrum_shape()[0], M.CDT[h.dtype]), gs.ptr)
    gx = GuardedBuffer(x.nbytes, 16)
    gy = GuardedBuffer(x.nbytes, 48)
    before = numpy.full(x.nbytes, PATTERN, numpy.uint8)
    _h2d(gx.ptr, x)
    _h2d(gy.ptr, before)
    kw = {} if default_pitch else dict(pitch=pitch)
    plan.execute(gx.ptr, gy.ptr, spectrum=gs.ptr, length=length, batch=batch, spectrum_batch=batch if per_item else 1, **kw)
    got = _d2h(numpy.empty_like(x), gy.ptr)
    assert numpy.array_equal(_d2h(numpy.empty_like(S), gs.ptr), S), "the spectrum was written"
    assert numpy.array_equal(_d2h(numpy.empty_like(x), gx.ptr).view(numpy.uint8), x.view(numpy.uint8)), "the input was modified"
    for g, w in ((gx, "x"), (gy, "y"), (gs, "spectrum")):
        g.check_guards(w)
    for g in (gx, gy, gs):
        g.free()
    raw, isz = got.view(numpy.uint8), pdt.itemsize
    for i in range(batch - 1):
        gap = raw[(i * pitch + length) * isz:(i + 1) * pitch * isz]
        assert (gap == PATTERN).all(), "the gap behind item %d was written" % i
    l1b, mxb = bound(prec, n)
    worst = [0.0, 0.0]
    f = scale * (1 if normalize else n)
    for i in range(batch):
        if i == poison:
            continue
        item = got[i * pitch:i * pitch + length]
        assert numpy.isfinite(item).all(), "item %d is not finite: a read outside the item, or a poisoned neighbour" % i
        ref = M.reference(x[i * pitch:i * pitch + length], h[i if per_item else 0], length, prec, f)
        l1, mx = item_error(item, ref)
        print("n %d m %d length %d item %d: L1 %.3g (bound %.3g) max %.3g (bound %.3g)" % (n, m, length, i, l1, l1b, mx, mxb))
        assert l1 <= l1b and mx <= mxb, "n %d m %d length %d item %d: L1 %.3g (bound %.3g) max %.3g (bound %.3g)" % (n, m, length, i, l1, l1b, mx, mxb)
        worst = [max(worst[0], l1 / l1b), max(worst[1], mx / mxb)]
    return worst


@pytest.mark.parametrize("case", M.INSTANCES, ids=[M.case_id(c) for c in M.INSTANCES])
def test_fir_instance(case):
    prec, real, n = case
    hip = _hip()
    m, length, batch, pitch = M.instance_case(n, real)
    plan = _plan(hip, prec, real, n, m)
    assert plan.fir_form == "fused_row" and plan.kernel == ("fir_row_real_kernel" if real else "fir_row_kernel")
    assert plan.overlap == M.overlap_of(m, real) and plan.hop == n - plan.overlap
    assert plan.blocks(length) == 3 and (not real or length % 2 == 1) and pitch % 2 == 0 and pitch >= length + 2
    run_guarded(hip, plan, prec, real, n, m, length, batch, pitch, False, seed=n + real, poison=1)
    plan.close()


@pytest.mark.parametrize("case", M.focus_cases(), ids=[M.case_id(c) for c in M.focus_cases()])
def test_fir_window_edges(case):
    """n = 256: the shortest and the longest filter, lengths on both sides of the first block's end and below the overlap; a spectrum
    per item, scale 2.5 without normalisation, the default pitch"""
    prec, real, n, m, length = case
    hip = _hip()
    plan = _plan(hip, prec, real, n, m, normalize=False, scale=2.5)
    batch = 3
    pitch = length + (length & 1) if real else length           # what execute takes without pitch=
    run_guarded(hip, plan, prec, real, n, m, length, batch, pitch, True, seed=m + length, scale=2.5, normalize=False, default_pitch=True)
    plan.close()


@pytest.mark.parametrize("prec,real,n,m", [(M.F32, False, 1024, 257), (M.F64, False, 256, 1), (M.F32, True, 2048, 100), (M.F64, True, 128, 64)],
                         ids=str)
def test_filter_spectrum_is_the_plain_plan_on_padded_taps(prec, real, n, m):
    hip = _hip()
    pdt = M.plan_dtype(prec, real)
    plan = _plan(hip, prec, real, n, m)
    plain = hip.Plan(n, dtype=pdt, real=True) if real else hip.Plan(n, dtype=pdt)
    sp = plan.spectrum_shape()[0]
    for batch in (1, 3):
        h = _taps(prec, real, m, batch, seed=n + m)
        padded = numpy.zeros((batch, n), pdt)
        padded[:, :m] = h
        # the taps one element past a 16-byte boundary: a filter's first tap has no alignment beyond its element
        raw = hip.DeviceArray((h.size + 1,), pdt)
        raw.set(numpy.concatenate([numpy.zeros(1, pdt), h.reshape(-1)]))
        a = hip.DeviceArray((batch, sp), M.CDT[pdt])
        b = hip.DeviceArray((batch, sp), M.CDT[pdt])
        plan.filter_spectrum(raw.ptr + pdt.itemsize, a, batch=batch)
        plain.execute(hip.to_gpu(padded), b, batch=batch)
        assert numpy.array_equal(a.get().view(numpy.uint8), b.get().view(numpy.uint8))
    plan.close()


def _eager_case(prec, real, n, m, length, batch, seed):
    pitch = length + (length & 1)
    x = M.signal(prec, real, batch * pitch, seed)
    h = _taps(prec, real, m, 1, seed + 1)
    return pitch, x, h


@pytest.mark.parametrize("prec,real,n,m", [(M.F32, False, 4096, 1025), (M.F32, True, 1024, 200)], ids=str)
def test_fir_hip_graph_capture(prec, real, n, m):
    """One launch and no scratch: a captured execute needs no eager execute first, and replays on fresh input."""
    hip = _hip()
    s = hip.Stream()
    plan = _plan(hip, prec, real, n, m, stream=s)
    length, batch = 3 * plan.hop + 17, 4
    pitch, x, h = _eager_case(prec, real, n, m, length, batch, 3)
    Hd = hip.DeviceArray((plan.spectrum_shape()[0],), M.CDT[h.dtype])
    plan.filter_spectrum(hip.to_gpu(h), Hd)
    s.synchronize()
    xd = hip.to_gpu(x)
    yd = hip.DeviceArray(x.shape, x.dtype)
    yd.set(numpy.zeros_like(x))
    with hip.Graph(s) as g:
        plan.execute(xd, yd, spectrum=Hd, length=length, batch=batch, pitch=pitch)
    l1b, mxb = bound(prec, n)
    for replay in range(2):
        x = M.signal(prec, real, batch * pitch, 40 + replay)
        xd.set(x)
        g.launch()
        s.synchronize()
        got = yd.get()
        for i in range(batch):
            l1, mx = item_error(got[i * pitch:i * pitch + length], M.reference(x[i * pitch:i * pitch + length], h[0], length, prec))
            assert l1 <= l1b and mx <= mxb, (replay, i, l1, l1b, mx, mxb)
    plan.release_captured()
    plan.close()


def test_fir_torch_tensors_on_a_torch_stream():
    torch = pytest.importorskip("torch")
    hip = _hip()
    dev = torch.device("cuda:0")
    for prec, real, n, m in ((M.F32, False, 2048, 300), (M.F32, True, 4096, 1025)):
        plan = _plan(hip, prec, real, n, m)
        length, batch = 2 * plan.hop + 5, 2
        pitch, x, h = _eager_case(prec, real, n, m, length, batch, 9)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            xt = torch.from_numpy(x).to(dev)
            ht = torch.from_numpy(h[0]).to(dev)
            Ht = torch.empty(plan.spectrum_shape()[0], dtype=torch.complex64, device=dev)
            yt = torch.zeros_like(xt)
            plan.filter_spectrum(ht, Ht)
            plan.execute(xt, yt, spectrum=Ht, length=length, batch=batch, pitch=pitch)
            st.synchronize()
            got = yt.cpu().numpy()
        l1b, mxb = bound(prec, n)
        for i in range(batch):
            l1, mx = item_error(got[i * pitch:i * pitch + length], M.reference(x[i * pitch:i * pitch + length], h[0], length, prec))
            assert l1 <= l1b and mx <= mxb, (n, i, l1, l1b, mx, mxb)
        plan.close()


def test_fir_refusals_leave_the_output_untouched():
    hip = _hip()
    prec, real, n, m = M.F32, False, 256, 33
    plan = _plan(hip, prec, real, n, m)
    length, batch = 1000, 2
    x = M.signal(prec, real, batch * length, 5)
    xd = hip.to_gpu(x)
    yd = hip.DeviceArray(x.shape, x.dtype)
    before = numpy.full(x.shape, 7.0 - 3.0j, x.dtype)
    yd.set(before)
    Hd = hip.DeviceArray((n,), numpy.complex64)
    plan.filter_spectrum(hip.to_gpu(_taps(prec, real, m, 1, 6)), Hd)
    isz = x.dtype.itemsize
    with pytest.raises(ValueError, match="taps.*overlap"):
        plan.execute(xd, xd.ptr + (batch * length - 1) * isz, spectrum=Hd, length=length, batch=batch)
    with pytest.raises(ValueError, match="taps.*overlap"):
        plan.execute(xd, xd, spectrum=Hd, length=length, batch=batch)
    with pytest.raises(ValueError, match="taps.*holds"):
        plan.execute(xd, yd, spectrum=Hd, length=length + 1, batch=batch)
    with pytest.raises(ValueError, match="taps.*aligned"):
        plan.execute(xd, yd.ptr + 4, spectrum=Hd, length=length - 1, batch=batch)
    with pytest.raises(ValueError, match="taps.*aligned"):
        plan.execute(xd.ptr + 4, yd, spectrum=Hd, length=length - 1, batch=batch)
    plan.finish()
    assert numpy.array_equal(yd.get(), before) and numpy.array_equal(xd.get(), x)
    plan.close()


def test_fir_lifecycle():
    """close() means what it means for every plan here (ConvPlan, docs/extensions.md): it waits, lets go of filter_spectrum's scratch
    and leaves the plan usable -- check() has nothing to report, and the next filter_spectrum re-plans the scratch, for another batch too."""
    hip = _hip()
    prec, real, n, m = M.F32, True, 512, 65
    plan = _plan(hip, prec, real, n, m)
    length = plan.hop + 9
    for batch in (2, 5, 2):                 # filter_spectrum's scratch follows the batch
        run_guarded(hip, plan, prec, real, n, m, length, batch, length + 1, True, seed=batch)
        assert plan._last_batch == batch and plan._scratch is not None
    plan.close()
    assert plan._scratch is None and plan._last_batch == 0 and plan._capture_keepalive == []
    plan.check()
    run_guarded(hip, plan, prec, real, n, m, length, 3, length + 1, True, seed=8)
    assert plan._last_batch == 3
    plan.close()
    plan.close()
