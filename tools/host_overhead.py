"""Host cost of one asynchronous execute() (batch 1 of a tiny plan: the device work is negligible).  Development tool.
--shape: the plan's shape, default 16 (one ROW pass); 16,16 is one ND pass.  --real: a real-input plan of that shape (float32 in,
half spectrum out: the one-launch real row where the library has one)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
from pyfft_amd.hip import Plan, DeviceArray, Stream
shape = tuple(int(v) for v in sys.argv[sys.argv.index("--shape") + 1].split(",")) if "--shape" in sys.argv else (16,)
real = "--real" in sys.argv
s = Stream()
if real:
    a = DeviceArray(shape, numpy.float32); b = DeviceArray(shape[:-1] + (shape[-1] // 2 + 1,), numpy.complex64)
    plan = Plan(shape, dtype=numpy.float32, real=True, stream=s)
else:
    a = DeviceArray(shape, numpy.complex64); b = DeviceArray(shape, numpy.complex64)
    plan = Plan(shape, dtype=numpy.complex64, stream=s)
for n in (2000, 20000):
    plan.execute(a, b); s.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        plan.execute(a, b)
    t1 = time.perf_counter()
    s.synchronize()
    t2 = time.perf_counter()
    print("%s%s: %d executes: %.2f us per call on the host (%.2f us with the final sync)" % (shape, " real" if real else "", n, (t1 - t0) / n * 1e6, (t2 - t0) / n * 1e6))
