"""Ring size of the persistent two-pass kernel for N < 2^20: PYFFT_AMD_FUSED_LAGF sweep (lag = LAGF * grid / (4 * gsize), ring = 2 lag).
python3 tools/fused_lag_probe.py"""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one child process per run: 512 MiB per side, sampled parity against numpy, best of three timings of five executes
CHILD = r'''
import sys, os, numpy
sys.path.insert(0, %r)
from pyfft_amd.hip import Plan, DeviceArray, Event
from pyfft_amd import _native as N
n = 1 << int(sys.argv[1]); batch = (1 << 29) // n
a = DeviceArray((n * batch,), numpy.complex64); b = DeviceArray((n * batch,), numpy.complex64)
rng = numpy.random.default_rng(5)
blk = (rng.standard_normal((8, n)) + 1j * rng.standard_normal((8, n))).astype(numpy.complex64)
for i in range(0, batch, 8):
    N.check(N.lib.mifft_memcpy_h2d(a.ptr + i * n * 8, blk.ctypes.data, blk.nbytes, None))
plan = Plan(n, dtype=numpy.complex64, wait_for_finish=True)
plan.execute(a, b, batch=batch)
out = numpy.empty(n, numpy.complex64); worst = 0.0
for item in (0, 1, 7, 8, 9, batch // 2 + 3, batch - 1):
    N.check(N.lib.mifft_memcpy_d2h(out.ctypes.data, b.ptr + item * n * 8, n * 8, None))
    ref = numpy.fft.fft(blk[item %% 8].astype(numpy.complex128))
    worst = max(worst, numpy.abs(out - ref).sum() / numpy.abs(ref).sum())
st = plan._context.getQueue(); best = 1e9
for _ in range(3):
    e0 = Event().record(st)
    for _ in range(5): plan.execute(a, b, batch=batch, wait_for_finish=False)
    e1 = Event().record(st); e1.synchronize(); best = min(best, e1.time_since(e0) / 5)
plan.finish()
print("2^%%s x %%-5d %%-34s %%8.3f ms  %%.3f of roofline  err %%.1e" %% (sys.argv[1], batch, str(plan.strategy(batch)[:5]), best, 16.0 * n * batch / (best * 1e-3) / 8e12, worst))
''' % ROOT
for log2n in (17, 18, 19, 20):
    for lagf in (0, 7, 14, 28, 56):
        e = dict(os.environ)
        if lagf:
            e.update({"PYFFT_AMD_STRATEGY": "fused", "PYFFT_AMD_FUSED_LAGF": str(lagf)})
        r = subprocess.run([sys.executable, "-c", CHILD, str(log2n)], env=e, capture_output=True, text=True)
        print(("LAGF=%d" % lagf if lagf else "auto").ljust(10), r.stdout.strip() or r.stderr.strip()[-300:], flush=True)
