"""Cosine and sine transforms without a device: the numpy model of the composed form (tests/dct_model.py) against the direct matrices
and scipy.fft, the host tables, argument errors raised before any device is touched, and the new C ABI symbols."""
import os
import sys

import numpy
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dct_model as M                                                # noqa: E402
from dct_cases import levels                                         # noqa: E402

SHAPES = [(1,), (2,), (4,), (8,), (16,), (1, 8), (8, 1), (1, 1), (2, 2), (4, 8), (8, 2), (2, 4, 8), (4, 1, 2), (8, 8, 8), (32,)]
VARIANTS = [(kind, inverse, ortho, normalize) for kind in ("dct", "dst") for inverse in (False, True) for ortho in (False, True)
            for normalize in ((True, False) if not ortho else (True,))]


def _vid(v):
    return "%s-%s-%s-%s" % (v[0], "inv" if v[1] else "fwd", "ortho" if v[2] else "plain", "norm" if v[3] else "raw")


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_model_matches_direct_matrices(shape, variant):
    kind, inverse, ortho, normalize = variant
    x = numpy.random.default_rng(len(shape) * 31 + sum(shape)).standard_normal(shape)
    want = M.direct(x, kind, inverse, ortho, normalize, scale=3.0)
    got = M.model(x, kind, inverse, ortho, normalize, scale=3.0)
    assert numpy.abs(got - want).max() <= 1e-12 * max(1.0, numpy.abs(want).max())
    ref = numpy.asarray(M.reference(x, kind, inverse, ortho, normalize, scale=3.0), numpy.float64)
    assert numpy.abs(ref - want).max() <= 1e-12 * max(1.0, numpy.abs(want).max())


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", SHAPES + [(64, 32), (16, 8, 4), (1024,)], ids=str)
def test_model_matches_scipy(shape, variant):
    sf = pytest.importorskip("scipy.fft")
    kind, inverse, ortho, normalize = variant
    x = numpy.random.default_rng(5).standard_normal(shape)
    norm = "ortho" if ortho else None
    if not inverse:
        want = (sf.dctn if kind == "dct" else sf.dstn)(x, type=2, norm=norm) * 2.5
    elif normalize:
        want = (sf.idctn if kind == "dct" else sf.idstn)(x, type=2, norm=norm) / 2.5
    else:
        want = (sf.dctn if kind == "dct" else sf.dstn)(x, type=3) / 2.5
    for got in (M.model(x, kind, inverse, ortho, normalize, 2.5), M.reference(x, kind, inverse, ortho, normalize, 2.5)):
        assert numpy.abs(numpy.asarray(got, numpy.float64) - want).max() <= 1e-11 * max(1.0, numpy.abs(want).max())


def test_levels_justified():
    """levels = log2(N) + ndim: the packed complex transform has log2(N / 2) radix-2 levels, the real separation / packing one, and
    every axis one twiddle butterfly (Y[k] = t V[k] + conj(t) V[-k]).  The model's float32 error stays inside that bound with margin."""
    from helpers import accuracy_bound
    for shape in ((256,), (64, 64), (16, 16, 16)):
        assert levels(shape) == (int(numpy.prod(shape)) // 2).bit_length() - 1 + 1 + len(shape)
        x = numpy.random.default_rng(1).standard_normal(shape)
        ref = numpy.asarray(M.reference(x, "dct"), numpy.float64)
        # the model run in float32 arithmetic end to end
        v = M.permute(x.astype(numpy.float32), "dct")
        Z = numpy.fft.fftn((v[..., 0::2] + 1j * v[..., 1::2]).astype(numpy.complex64)).astype(numpy.complex64)
        kept, g = M.global_factor(shape, False, False, True, 1.0)
        got = M.post_forward(Z, kept, False, g)
        l1 = numpy.abs(got - ref).sum() / numpy.abs(ref).sum()
        assert l1 <= accuracy_bound(numpy.float32, int(numpy.prod(shape)), levels=levels(shape))[0]


def test_host_tables_match_model():
    from pyfft_amd import r2r
    for kept, inverse, ortho in (((8,), False, False), ((4, 16), True, True), ((2, 2, 8), False, True), ((2,), True, False)):
        kept_, g = r2r.global_factor(kept, inverse, ortho, True, 1.5)
        tab = r2r.tables(kept_, inverse, ortho, g, numpy.complex128)
        want = []
        for a, n in enumerate(kept):
            f = float(g) if a == len(kept) - 1 else 1.0
            want.append(M.inv_table(n, ortho, f) if inverse else M.fwd_table(n, ortho, f))
        nl = kept[-1]
        want.append(numpy.exp(-2j * numpy.pi * numpy.arange(nl // 4 + 1) / nl))
        want = numpy.concatenate(want)
        assert tab.shape == want.shape and numpy.abs(tab - want).max() <= 1e-15 * max(1.0, numpy.abs(want).max())
        kept2, g2 = M.global_factor(kept, inverse, ortho, True, 1.5)
        assert kept2 == kept_ and abs(float(g) - g2) <= 1e-15 * abs(g2)


BAD = [
    dict(dtype=numpy.complex64), dict(dtype=numpy.complex128), dict(dtype="complex32"), dict(dtype=numpy.float16),
    dict(dtype=numpy.float32, real=True), dict(dtype=numpy.float32, convolve=True), dict(dtype=numpy.float32, any_size=True),
    dict(dtype=numpy.float32, parent_shape=(64,)), dict(dtype=numpy.float32, r2r_kind="dct4"),
    dict(dtype=numpy.float32, ortho=True, normalize=False), dict(dtype=numpy.int32),
]


@pytest.mark.parametrize("kw", BAD, ids=[str(sorted(k.items())) for k in BAD])
def test_value_errors_before_the_device(kw, monkeypatch):
    import pyfft_amd.hip as hip
    monkeypatch.setattr(hip, "device_count", lambda: pytest.fail("the device was touched"))
    kw = dict(kw)
    r2r = kw.pop("r2r_kind", "dct")
    with pytest.raises(ValueError, match="r2r"):
        hip.Plan((16,), r2r=r2r, **kw)


def test_bad_shapes_and_kind_values():
    import pyfft_amd.hip as hip
    for shape in ((12,), (4, 4, 4, 4), (0,)):
        with pytest.raises(ValueError, match="r2r"):
            hip.Plan(shape, numpy.float32, r2r="dct")
    for kind in ("DCT", "dct2", 2, ""):
        with pytest.raises(ValueError, match="r2r"):
            hip.Plan((16,), numpy.float32, r2r=kind)


def test_without_the_keyword_nothing_changes():
    """ortho= without r2r= is an unknown keyword, as before"""
    import pyfft_amd.hip as hip
    with pytest.raises(TypeError):
        hip.Plan((16,), numpy.complex64, ortho=True)


def test_coverage_rule():
    """the lengths the library runs in one launch are FUSED; every other real-row length is in LEFT_OUT, with its log line present"""
    from pyfft_amd import _native as N
    from dct_cases import FUSED, LEFT_OUT
    log = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07_dct_transforms.log")).read()
    for dt, prec, top in ((numpy.float32, N.F32, 65536), (numpy.float64, N.F64, 32768)):
        accepted = {(dt, 1 << e) for e in range(0, 20) if N.lib.mifft_r2r_row_supported(prec, 1 << e) == 0}
        assert accepted == {c for c in FUSED if c[0] is dt}
        for e in range(2, 20):
            n = 1 << e
            real_row = N.lib.mifft_real_row_supported(prec, n) == 0
            assert real_row == (n <= top)
            if real_row and (dt, n) not in accepted:
                assert (dt, n) in LEFT_OUT and LEFT_OUT[(dt, n)] in log, (dt, n)
    for key, line in LEFT_OUT.items():
        assert line in log


def test_form_follows_row_supported():
    from pyfft_amd import _native as N
    from pyfft_amd.r2r import r2r_form_of
    for prec in (N.F32, N.F64):
        for e in range(0, 17):
            n = 1 << e
            want = "fused_row" if N.lib.mifft_r2r_row_supported(prec, n) == 0 else "composed"
            assert r2r_form_of((n,), prec) == want
            assert r2r_form_of((1, n), prec) == want and r2r_form_of((n, 1), prec) == want
        assert r2r_form_of((8, 8), prec) == "composed" and r2r_form_of((4, 4, 4), prec) == "composed"


def test_row_tables_match_model():
    from pyfft_amd import r2r
    for n, inverse, ortho in ((16, False, False), (64, True, True), (4, False, True), (256, True, False)):
        g = r2r.global_factor((n,), inverse, ortho, True, 2.0)[1]
        stage, sep, tab = r2r.row_tables(n, inverse, ortho, g, numpy.complex128)
        L = n // 2
        assert numpy.allclose(stage, numpy.exp(-2j * numpy.pi * numpy.arange(L) / L), atol=1e-15)
        assert numpy.allclose(sep, numpy.exp(-2j * numpy.pi * numpy.arange(L) / n), atol=1e-15)
        want = M.inv_table(n, ortho, float(g)) if inverse else 2 * M.fwd_table(n, ortho, float(g))[: L + 1]
        assert numpy.allclose(tab, want, rtol=1e-14, atol=1e-17)


def test_new_symbols_and_abi():
    from pyfft_amd import _native as N
    assert N.lib.mifft_abi_version() == 6
    for name in ("mifft_launch_r2r_pre", "mifft_launch_r2r_post", "mifft_r2r_row_supported", "mifft_launch_r2r_row"):
        assert hasattr(N.lib, name)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mifft.h")).read()
    assert "mifft_r2r_step" in hdr and "mifft_launch_r2r_pre" in hdr and "mifft_launch_r2r_post" in hdr


def test_abi_argument_errors():
    from pyfft_amd import _native as N
    d = N.MifftR2rStep()
    d.precision, d.inverse, d.kind, d.ndim = N.F32, 0, 0, 1
    d.n[0] = 12
    d.outer = 1
    d.in_, d.out, d.tw = 4096, 1 << 20, 8192
    assert N.lib.mifft_launch_r2r_post(d, None) != 0            # 12 is not a power of two
    d.n[0] = 16
    d.kind = 2
    assert N.lib.mifft_launch_r2r_post(d, None) != 0            # unknown kind
    d.kind = 0
    d.out = 4096 + 16
    assert N.lib.mifft_launch_r2r_post(d, None) != 0            # overlap
    d.out = 1 << 20
    d.tw = None
    assert N.lib.mifft_launch_r2r_post(d, None) != 0            # the twiddle step needs its table
    d.reserved = 1
    assert N.lib.mifft_launch_r2r_pre(d, None) != 0


def test_sharded_plan_has_no_r2r():
    from pyfft_amd.sharded import ShardedPlan
    with pytest.raises(ValueError, match="r2r"):
        ShardedPlan((16,), numpy.float32, r2r="dct")
