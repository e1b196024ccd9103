"""Overlap-save FIR plans without a device (docs/extensions.md, "FIR filtering plans"): the numpy model of the kernel's index algebra
(tests/fir_model.py) against numpy.convolve on every case the GPU tests run, the coverage of its load and store index sets, the
planner's overlap / hop / blocks, the refusals of Plan(..., convolve=True, taps=m) and of execute, and the C ABI's argument checks."""
import ctypes
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fir_model as M                                           # noqa: E402
from helpers import FakeContext, accuracy_bound, item_error     # noqa: E402


def _native():
    from pyfft_amd import _native as N
    return N


def _prec(dt):
    N = _native()
    return N.F64 if numpy.dtype(dt) in (numpy.dtype(numpy.float64), numpy.dtype(numpy.complex128)) else N.F32


def bound(dtype, n):
    return accuracy_bound(dtype, n, levels=2 * (int(n).bit_length() - 1) + 1)


# ---- the model reproduces numpy.convolve on the GPU tests' cases ------------------------------------------------------------------
def _model_case(prec, real, n, m, length, batch, pitch, scale=1.0, normalize=True, per_item=False):
    total = (batch - 1) * pitch + length
    x = M.signal(prec, real, total, seed=n + m + length)
    h = [M.signal(prec, real, m, seed=7 * n + m + j) for j in range(batch if per_item else 1)]
    H = numpy.stack([M.filter_spectrum(hj, n, real, prec) for hj in h])
    y, writes = M.run(x, H, n, m, length, pitch, batch, real, prec, scale=scale, normalize=normalize)
    l1b, mxb = bound(prec, n)
    for i in range(batch):
        ref = M.reference(x[i * pitch:i * pitch + length], h[i if per_item else 0], length, prec, scale * (1 if normalize else n))
        l1, mx = item_error(y[i * pitch:i * pitch + length], ref)
        assert l1 <= l1b and mx <= mxb, (i, l1, l1b, mx, mxb)
        assert (writes[i * pitch:i * pitch + length] == 1).all()
    gaps = numpy.ones(total, bool)
    for i in range(batch):
        gaps[i * pitch:i * pitch + length] = False
    assert (writes[gaps] == 0).all()


@pytest.mark.parametrize("case", M.INSTANCES, ids=[M.case_id(c) for c in M.INSTANCES])
def test_model_reproduces_convolve_on_the_instance_cases(case):
    prec, real, n = case
    m, length, batch, pitch = M.instance_case(n, real)
    assert length % 2 == 1 or not real
    _model_case(prec, real, n, m, length, batch, pitch)


@pytest.mark.parametrize("case", M.focus_cases(), ids=[M.case_id(c) for c in M.focus_cases()])
def test_model_reproduces_convolve_on_the_focused_cases(case):
    prec, real, n, m, length = case
    _model_case(prec, real, n, m, length, 3, length + (length & 1) if real else length, scale=2.5, normalize=False, per_item=True)


def test_focus_cases_are_the_issues():
    cases = M.focus_cases()
    for prec, real in M.FOCUS_KINDS:
        for m in (1, 2, 128):
            ov = M.overlap_of(m, real)
            got = sorted(c[4] for c in cases if c[:4] == (prec, real, 256, m))
            assert got == sorted(set(v for v in (1, ov - 1, 256 - ov, 256 - ov + 1) if v >= 1)), (prec, real, m)


# ---- index coverage: the kernel's windows are the issue's element-wise statement --------------------------------------------------
@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("n", [128, 256])
def test_index_sets(n, real):
    for m in (1, 2, 3, n // 4 + 1, n // 2):
        overlap = M.overlap_of(m, real)
        assert overlap >= m - 1 and overlap <= n // 2 and (not real or overlap % 2 == 0)
        hop = n - overlap
        for length in (1, overlap - 1, hop - 1, hop, hop + 1, 2 * hop + hop // 2 + 1):
            if length < 1:
                continue
            stored = numpy.zeros(length, int)
            for r in range(M.blocks(n, overlap, length)):
                p = numpy.arange(n)
                g = r * hop - overlap + p
                want = (g >= 0) & (g < length)
                local, item = M.load_map(n, overlap, length, r, real)
                assert sorted(local) == sorted(p[want]) and (item == r * hop - overlap + local).all(), (m, length, r)
                assert item.size == 0 or (item.min() >= 0 and item.max() < length)
                t = r * hop + p - overlap
                want = (p >= overlap) & (t < length)
                local, item = M.store_map(n, overlap, length, r, real)
                assert sorted(local) == sorted(p[want]) and (item == r * hop + local - overlap).all(), (m, length, r)
                assert item.size and item.min() >= 0 and item.max() < length        # (every block of the launch stores something)
                stored[item] += 1
                if real:            # whole pairs, but for the one that straddles an odd length's end
                    odd = [v for v in local if v % 2 == 0 and v + 1 not in local]
                    assert len(odd) == (1 if (length % 2 and r * hop + n - overlap >= length) else 0)
            assert (stored == 1).all(), (m, length)


# ---- planner and refusals ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import pyfft_amd.hip as hip

    def touched(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(hip, "device_count", touched)
    monkeypatch.setattr(hip, "Context", touched)
    return hip


def test_taps_is_a_keyword_now(no_device):
    """Plan(256, convolve=True, taps=5) was a TypeError before FIR plans; now it gets as far as the device."""
    with pytest.raises(AssertionError, match="a device was touched"):
        no_device.Plan(256, convolve=True, taps=5)


@pytest.mark.parametrize("shape,kw", [
    (256, dict(taps=5)),                                                    # without convolve=True
    (256, dict(convolve=True, taps=0)), (256, dict(convolve=True, taps=129)), (256, dict(convolve=True, taps=-3)),
    (256, dict(convolve=True, taps=2.5)),
    ((64, 64), dict(convolve=True, taps=5)), ((4, 256), dict(convolve=True, taps=5)),
    (32, dict(convolve=True, taps=5)), (65536, dict(convolve=True, taps=5)), (64, dict(convolve=True, taps=5, real=True, dtype=numpy.float32)),
    (16384, dict(convolve=True, taps=5, dtype=numpy.complex128)), (32768, dict(convolve=True, taps=5, real=True, dtype=numpy.float32)),
    (16384, dict(convolve=True, taps=5, real=True, dtype=numpy.float64)), (96, dict(convolve=True, taps=5)),
    (256, dict(convolve=True, taps=5, correlate=True)),
    (256, dict(convolve=True, taps=5, any_size=True)), (256, dict(convolve=True, taps=5, parent_shape=(2048,))),
    (256, dict(taps=5, r2r="dct", dtype=numpy.float32)), (256, dict(convolve=True, taps=5, r2r="dct", dtype=numpy.float32)),
    (256, dict(convolve=True, taps=5, dtype="complex32")),
    (256, dict(convolve=True, taps=5, dtype=numpy.float32)), (256, dict(convolve=True, taps=5, dtype=numpy.float64)),
    (256, dict(convolve=True, taps=5, dtype=numpy.int32)),
], ids=str)
def test_refusals_before_the_device(no_device, shape, kw):
    with pytest.raises(ValueError, match="taps"):
        no_device.Plan(shape, **kw)


def test_torch_complex32_refused(no_device):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="taps"):
        no_device.Plan(256, dtype=torch.complex32, convolve=True, taps=5)


def test_no_instance_message_lists_the_lengths(no_device):
    with pytest.raises(ValueError, match=r"taps.*supported: 64, 128, .*32768$"):
        no_device.Plan(32, convolve=True, taps=5)
    with pytest.raises(ValueError, match=r"taps.*supported: 128, 256, .*8192$"):
        no_device.Plan(16384, dtype=numpy.float64, real=True, convolve=True, taps=5)


def test_convolve_refusals_without_taps_are_unchanged(no_device):
    for kw in (dict(dtype=numpy.float32), dict(dtype="complex32"), dict(dtype=numpy.complex64, any_size=True)):
        with pytest.raises(ValueError, match="convolve"):
            no_device.Plan((1024,), convolve=True, **kw)


def _fake(n, dtype=numpy.complex64, real=False, taps=5, **kw):
    from pyfft_amd.fir import FirPlan
    from kernel_coverage import full_machine
    return FirPlan(FakeContext(full_machine()), n, dtype=dtype, real=real, taps=taps, **kw)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_planner(real):
    dt = numpy.float32 if real else numpy.complex64
    for n in (128, 256, 4096):
        for m in (1, 2, 3, 4, n // 4 + 1, n // 2):
            p = _fake(n, dt, real, m)
            want = M.overlap_of(m, real)
            assert p.overlap == want and p.hop == n - want and p.taps == m
            assert p.overlap == (m - 1 if not real else (m - 1) + ((m - 1) & 1))
            assert p.fir_form == "fused_row" and p.kernel == ("fir_row_real_kernel" if real else "fir_row_kernel")
            for length in (1, p.hop - 1, p.hop, p.hop + 1, 10 * p.hop + 1):
                assert p.blocks(length) == -(-length // p.hop) == M.blocks(n, want, length)
            assert p.spectrum_shape() == ((n // 2 + 1,) if real else (n,))
    with pytest.raises(ValueError, match="length"):
        _fake(256).blocks(0)


class _Obj(int):
    """A device address that knows its size (FakeContext.pointer_of passes buffers through as they are)."""
    def __new__(cls, ptr, nbytes):
        o = int.__new__(cls, ptr)
        o.nbytes = nbytes
        return o


@pytest.mark.parametrize("dtype,real", [(numpy.complex64, False), (numpy.float32, True), (numpy.complex128, False), (numpy.float64, True)], ids=str)
def test_execute_refusals(dtype, real):
    """Every refusal comes before anything is enqueued: FakeContext has no createQueue, so a plan that went on would raise AttributeError."""
    n, length, batch = 256, 1001, 4
    p = _fake(n, dtype, real, 33)
    isz = numpy.dtype(dtype).itemsize
    pitch = length + 1
    need = ((batch - 1) * pitch + length) * isz
    sp = (n // 2 + 1 if real else n) * isz * (2 if real else 1)
    X, Y, S = 1 << 30, 1 << 31, 1 << 32
    x, y, s = _Obj(X, need), _Obj(Y, need), _Obj(S, sp)
    ok = dict(spectrum=s, length=length, batch=batch, pitch=pitch)

    def refused(match, *a, **k):
        with pytest.raises(ValueError, match=match):
            p.execute(*a, **k)
    refused("taps.*holds", _Obj(X, need - isz), y, **ok)                                        # short buffers
    refused("taps.*holds", x, _Obj(Y, need - isz), **ok)
    refused("taps.*spectrum", x, y, **dict(ok, spectrum=_Obj(S, sp - 8)))
    refused("taps.*spectrum", x, y, **dict(ok, spectrum=_Obj(S, 3 * sp), spectrum_batch=batch))
    refused("taps.*pitch", x, y, **dict(ok, pitch=length - 1))
    if real:
        refused("taps.*even", x, y, **dict(ok, pitch=length + 2))                                 # 1003: odd
    refused("taps.*aligned", _Obj(X + isz // (1 if real else 2), need), y, **ok)                 # half a complex number / one real off
    refused("taps.*aligned", x, _Obj(Y + isz // (1 if real else 2), need), **ok)
    refused("taps.*aligned", x, y, **dict(ok, spectrum=_Obj(S + 4, sp)))
    refused("taps.*spectrum_batch", x, y, **dict(ok, spectrum_batch=2))
    refused("taps.*overlap", x, _Obj(X, need), **ok)                                            # in place
    refused("taps.*overlap", x, _Obj(X + need - 2 * isz, need), **ok)                            # y starts in x's last element pair
    refused("taps.*overlap", _Obj(Y + 2 * isz, need), y, **ok)
    refused("taps.*spectrum overlaps", x, y, **dict(ok, spectrum=_Obj(Y + need - 2 * isz, sp)))
    refused("taps.*out of place", x, **ok)
    refused("taps.*spectrum=", x, y, length=length, batch=batch)
    refused("taps.*length", x, y, spectrum=s, batch=batch)
    refused("taps.*length", x, y, **dict(ok, length=0))
    refused("taps.*correlate", x, y, correlate=True, **ok)
    with pytest.raises(ValueError, match="batch"):
        p.execute(x, y, **dict(ok, batch=0))
    with pytest.raises(AttributeError):
        p.execute(x, y, **ok)                   # the one call that is fine goes on (to FakeContext's missing createQueue)


def test_sharded_plan_has_no_fir_form():
    from pyfft_amd.sharded import ShardedPlan
    import inspect
    assert "taps" not in inspect.signature(ShardedPlan.__init__).parameters


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_supported_agrees_with_the_instance_list():
    N = _native()
    want = set((_prec(p), 1 if real else 0, n) for p, real, n in M.INSTANCES)
    got = set()
    for prec in (N.F32, N.F64):
        for real in (0, 1):
            for e in range(0, 18):
                if N.lib.mifft_fir_row_supported(prec, real, 1 << e) == 0:
                    got.add((prec, real, 1 << e))
                    assert N.lib.mifft_conv_row_supported(prec, real, 1 << e) == 0          # the convolution row it follows
    assert got == want
    assert len(M.INSTANCES) == 10 + 8 + 8 + 7
    assert N.lib.mifft_fir_row_supported(N.F32, 0, 96) == N.E_UNSUPPORTED
    assert N.lib.mifft_fir_row_supported(7, 0, 256) == N.E_UNSUPPORTED
    assert N.lib.mifft_fir_row_supported(N.F32, 2, 256) == N.E_UNSUPPORTED


def test_prototypes():
    N = _native()
    for name in ("mifft_fir_row_supported", "mifft_launch_fir_row", "mifft_launch_fir_pad"):
        assert name in N.PROTOTYPES
        assert hasattr(N.lib, name)
    assert len(N.PROTOTYPES["mifft_launch_fir_row"][1]) == 15


def test_abi_argument_errors():
    N = _native()
    lib = N.lib
    a, b, s, t = (ctypes.c_void_p(v) for v in (1 << 20, 1 << 24, 1 << 28, 1 << 29))

    def row(prec=N.F32, real=0, n=256, ov=32, length=1000, pitch=1000, items=4, x=a, y=b, sp=s, spp=0, tw=t, tws=None, scale=1.0):
        return lib.mifft_launch_fir_row(prec, real, n, ov, length, pitch, items, x, y, sp, spp, tw, tws, scale, None)

    def err(rc, text, code=None):
        assert rc == (N.E_INVALID if code is None else code), rc
        assert text in N.last_error(), N.last_error()
    err(row(prec=7), "fir row: bad precision 7")
    err(row(real=2), "fir row: real must be 0 or 1")
    err(row(n=96), "fir row: n = 96 is not a power of two")
    err(row(n=32), "fir row: no kernel for n = 32", N.E_UNSUPPORTED)
    err(row(prec=N.F64, n=16384), "fir row: no kernel for n = 16384", N.E_UNSUPPORTED)
    err(row(ov=-1), "fir row: overlap -1")
    err(row(ov=129), "fir row: overlap 129")
    err(row(real=1, ov=33, tws=t), "fir row: overlap 33")
    err(row(length=0), "fir row: length must be at least 1")
    err(row(pitch=999), "fir row: pitch 999 is below the length")
    err(row(real=1, pitch=1001, tws=t), "fir row: pitch 1001")
    err(row(items=-1), "fir row: negative item count")
    err(row(x=None), "fir row: null buffer")
    err(row(y=None), "fir row: null buffer")
    err(row(sp=None), "fir row: null buffer")
    err(row(tw=None), "fir row: null buffer")
    err(row(real=1), "fir row: null buffer")                                                 # no tw_sep
    err(row(x=ctypes.c_void_p((1 << 20) + 4)), "fir row: buffers must be aligned")
    err(row(prec=N.F64, y=ctypes.c_void_p((1 << 24) + 8)), "fir row: buffers must be aligned")
    err(row(real=1, tws=t, x=ctypes.c_void_p((1 << 20) + 4)), "fir row: buffers must be aligned")     # one real: half a pair
    err(row(spp=255), "fir row: spectrum_pitch 255")
    err(row(real=1, tws=t, spp=128), "fir row: spectrum_pitch 128")
    err(row(items=1 << 61), "fir row: items * pitch overflows")
    err(row(y=a), "fir row: input and output overlap")
    err(row(y=ctypes.c_void_p((1 << 20) + 8 * 3999)), "fir row: input and output overlap")
    err(row(sp=ctypes.c_void_p((1 << 20) + 8 * 3999)), "fir row: the spectrum overlaps the data")
    err(row(sp=ctypes.c_void_p((1 << 24) - 8 * 255)), "fir row: the spectrum overlaps the data")
    # a grid beyond 2^31 - 1 work-groups: n = 4096 runs one block per work-group
    err(row(n=4096, ov=2048, length=1 << 43, pitch=1 << 43, items=2, x=ctypes.c_void_p(1 << 20), y=ctypes.c_void_p(1 << 50),
            sp=ctypes.c_void_p(1 << 60), tw=ctypes.c_void_p((1 << 60) + (1 << 20))), "grid too large")
    assert row(items=0) == 0

    def pad(prec=N.F32, real=0, n=256, taps=33, filters=2, h=a, out=b):
        return lib.mifft_launch_fir_pad(prec, real, n, taps, filters, h, out, None)
    err(pad(prec=5), "fir pad: bad precision 5")
    err(pad(real=3), "fir pad: real must be 0 or 1")
    err(pad(n=100), "fir pad: n = 100")
    err(pad(taps=0), "fir pad: taps = 0")
    err(pad(taps=257), "fir pad: taps = 257")
    err(pad(filters=-1), "fir pad: negative filter count")
    err(pad(h=None), "fir pad: null buffer")
    err(pad(out=None), "fir pad: null buffer")
    err(pad(h=ctypes.c_void_p((1 << 20) + 4)), "fir pad: the taps must be aligned")
    err(pad(out=ctypes.c_void_p((1 << 24) + 8)), "fir pad: the taps must be aligned")
    err(pad(filters=1 << 60), "fir pad: filters * n overflows")
    err(pad(out=ctypes.c_void_p((1 << 20) + 16)), "fir pad: input and output overlap")
    assert pad(real=1, h=ctypes.c_void_p((1 << 20) + 4), filters=0) == 0                      # one real is aligned enough
