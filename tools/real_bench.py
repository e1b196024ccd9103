"""Real-input transforms (Plan(shape, real=True)) at 1 GiB of real input: one JSON line per shape.

Timing as bench.py times: HIP events around K back-to-back executes on the plan's stream, K grown until a block lasts >= 20 ms, the
best of three blocks.  Fields: transforms/s and nominal GFLOPS (2.5 N log2 N per real transform), the roofline fraction against the
algorithmic bytes (N s in + (N / 2 + 1) 2 s out per transform, over 8 TB/s), the same data widened to complex and transformed by the
complex plan (its time alone, widening not counted; its own roofline fraction over 2 N s in + 2 N s out), the speed-up of the real
transform over that route, and the plan's form.
    python tools/real_bench.py [--gib 1] [fwd|inv]
"""
import json
import math
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
SHAPES = [((1 << 10,), "float32"), ((1 << 12,), "float32"), ((1 << 14,), "float32"), ((1 << 16,), "float32"), ((1 << 21,), "float32"),
          ((1 << 15,), "float64"), ((2048, 2048), "float32"), ((256, 256, 256), "float32")]


def timed(hip, plan, args, kw, stream_plan=None):
    """Seconds per execute: blocks of back-to-back executes between two events, >= 20 ms each, best of three."""
    plan.execute(*args, **kw)
    plan.finish()
    reps, best = 1, None
    while True:
        e0, e1 = hip.Event(), hip.Event()
        q = plan._context.getQueue()
        e0.record(q)
        for _ in range(reps):
            plan.execute(*args, wait_for_finish=False, **kw)
        e1.record(q)
        e1.synchronize()
        ms = e1.time_since(e0)
        if ms >= 20.0:
            t = [ms / reps]
            for _ in range(2):
                e0.record(q)
                for _ in range(reps):
                    plan.execute(*args, wait_for_finish=False, **kw)
                e1.record(q)
                e1.synchronize()
                t.append(e1.time_since(e0) / reps)
            best = min(t)
            break
        reps *= 2 if ms < 5 else max(2, int(math.ceil(22.0 / max(ms, 1e-3))))
    plan.finish()
    return best / 1000.0


def main():
    import pyfft_amd.hip as hip
    gib = float(sys.argv[sys.argv.index("--gib") + 1]) if "--gib" in sys.argv else 1.0
    inverse = "inv" in sys.argv[1:]
    for shape, dt in SHAPES:
        rdt = numpy.dtype(dt)
        cdt = numpy.dtype(numpy.complex64 if rdt == numpy.float32 else numpy.complex128)
        s = rdt.itemsize
        n = int(numpy.prod(shape))
        batch = max(1, int(gib * (1 << 30)) // (n * s))
        spec_pts = n // shape[-1] * (shape[-1] // 2 + 1)
        stream = hip.Stream()
        plan = hip.Plan(shape, dtype=rdt, real=True, stream=stream)
        x = hip.DeviceArray((batch * n,), rdt)
        X = hip.DeviceArray((batch * spec_pts,), cdt)
        rng = numpy.random.default_rng(1)
        x.set(rng.standard_normal(batch * n).astype(rdt))
        args = (X, x) if inverse else (x, X)
        t_real = timed(hip, plan, args, {"batch": batch, "inverse": inverse})
        del plan
        # the widen-to-complex route: the complex transform of the same data as complex numbers
        cplan = hip.Plan(shape, dtype=cdt, stream=stream)
        del X
        zi = hip.DeviceArray((batch * n,), cdt)
        zo = hip.DeviceArray((batch * n,), cdt)
        N = __import__("pyfft_amd._native", fromlist=["lib"])
        N.lib.mifft_memset(zi.ptr, 0, zi.nbytes, None)
        t_cplx = timed(hip, cplan, (zi, zo), {"batch": batch, "inverse": inverse})
        del cplan, zi, zo, x
        bytes_real = n * s + spec_pts * 2 * s
        bytes_cplx = 4 * n * s
        rec = {
            "shape": list(shape), "dtype": dt, "direction": "inverse" if inverse else "forward", "batch": batch,
            "real_form": hip.Plan(shape, dtype=rdt, real=True)._real_form,
            "transforms_per_s": batch / t_real,
            "gflops_nominal": 2.5 * n * math.log2(n) * batch / t_real / 1e9,
            "roofline_fraction": bytes_real * batch / t_real / HBM,
            "ms_per_execute": t_real * 1e3,
            "complex_widened_ms_per_execute": t_cplx * 1e3,
            "complex_widened_roofline_fraction": bytes_cplx * batch / t_cplx / HBM,
            "speedup_vs_widened_complex": t_cplx / t_real,
        }
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
