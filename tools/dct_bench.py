"""Cosine transforms (Plan(shape, r2r="dct")) at about 1 GiB per side: one JSON line per shape.

Three routes on the same data, out of place, forward (and the r2r and real plans' inverse):
    the r2r plan (the composed form: permutation, the inner complex plan of the packed shape, separation + twiddles),
    Plan(shape, real=True) of the same shape (the real transform alone, a floor for the composed form),
    the widened route a user has today: a torch mirror extension to 2n on the last axis, Plan(2 shape, real=True), a torch twiddle and
    real part (1-D shapes; the mirror of every axis for N-D shapes).
Timing as tools/conv_bench.py: device events around back-to-back executes, blocks of >= 20 ms, the best of three.  roofline_fraction:
the algorithmic bytes 2 N s per item over 8 TB/s.
    python tools/dct_bench.py [--gib 1]
"""
import json
import math
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
SHAPES = [((256,), "float32"), ((1024,), "float32"), ((4096,), "float32"), ((16384,), "float32"), ((65536,), "float32"),
          ((1 << 21,), "float32"), ((4096,), "float64"), ((64, 64), "float32"), ((1024, 1024), "float32"), ((2048, 2048), "float32"),
          ((8, 8), "float32")]


def timed(run, sync, event):
    """Seconds per call of run(): blocks of back-to-back calls between two events, >= 20 ms each, best of three."""
    run()
    sync()
    reps = 1
    while True:
        ms = event(run, reps)
        if ms >= 20.0:
            return min([ms / reps] + [event(run, reps) / reps for _ in range(2)]) / 1000.0
        reps *= 2 if ms < 5 else max(2, int(math.ceil(22.0 / max(ms, 1e-3))))


def main():
    import torch
    import pyfft_amd.hip as hip
    gib = float(sys.argv[sys.argv.index("--gib") + 1]) if "--gib" in sys.argv else 1.0
    dev = torch.device("cuda:0")
    tdt = {"float32": torch.float32, "float64": torch.float64}
    stream = torch.cuda.Stream()

    def event(run, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            run()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with torch.cuda.stream(stream):
        for shape, dt in SHAPES:
            d = numpy.dtype(dt)
            n = int(numpy.prod(shape))
            s = d.itemsize
            batch = max(1, int(gib * (1 << 30)) // (n * s))
            x = torch.randn((batch,) + tuple(shape), dtype=tdt[dt], device=dev)
            y = torch.empty_like(x)
            plan = hip.Plan(shape, dtype=d, r2r="dct", wait_for_finish=False)
            t_plan = timed(lambda: plan.execute(x, y, batch=batch), stream.synchronize, event)
            t_inv = timed(lambda: plan.execute(y, x, inverse=True, batch=batch), stream.synchronize, event)
            form = plan.r2r_form
            del plan
            rp = hip.Plan(shape, dtype=d, real=True, wait_for_finish=False)
            spec = torch.empty((batch,) + tuple(shape[:-1]) + (shape[-1] // 2 + 1,), dtype=torch.complex64 if s == 4 else torch.complex128,
                               device=dev)
            t_real = timed(lambda: rp.execute(x, spec, batch=batch), stream.synchronize, event)
            t_real_inv = timed(lambda: rp.execute(spec, x, inverse=True, batch=batch), stream.synchronize, event)
            del rp, spec
            # the widened route: mirror every axis to 2n, a real transform of that, twiddle and real part per axis
            wshape = tuple(2 * v for v in shape)
            wp = hip.Plan(wshape, dtype=d, real=True, wait_for_finish=False)
            axes = list(range(1, len(shape) + 1))
            tw = []
            for a, v in enumerate(shape):
                k = torch.arange(v, device=dev, dtype=torch.float64)
                w = torch.exp(-1j * math.pi * k / (2 * v)).to(torch.complex64 if s == 4 else torch.complex128)
                sh = [1] * (len(shape) + 1)
                sh[a + 1] = v
                tw.append(w.reshape(sh))

            def widened():
                e = x
                for a in axes:
                    e = torch.cat([e, torch.flip(e, dims=[a])], dim=a)
                W = torch.empty((batch,) + wshape[:-1] + (wshape[-1] // 2 + 1,), dtype=tw[0].dtype, device=dev)
                wp.execute(e.contiguous(), W, batch=batch)
                # (N-D: the leading axes' halves combine through their conjugate partners as well; the last axis's twiddle and the
                # real part are the work a 1-D user does, and the N-D route is at least this much)
                Wt = W[(slice(None),) + tuple(slice(0, v) for v in shape)] * tw[-1]
                y.copy_(Wt.real)
            try:
                t_wide = timed(widened, stream.synchronize, event)
            except RuntimeError:          # the widened copies do not fit next to the data
                t_wide = float("nan")
            del wp
            item_bytes = 2 * n * s
            rec = {"shape": list(shape), "dtype": dt, "batch": batch, "form": form, "ms": t_plan * 1e3,
                   "roofline_fraction": item_bytes * batch / t_plan / HBM,
                   "real_plan_ms": t_real * 1e3, "time_vs_real_plan": t_plan / t_real,
                   "inverse_ms": t_inv * 1e3, "real_plan_inverse_ms": t_real_inv * 1e3, "inverse_time_vs_real_plan": t_inv / t_real_inv,
                   "widened_ms": t_wide * 1e3, "speedup_vs_widened": t_wide / t_plan}
            print(json.dumps(rec), flush=True)
            del x, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
