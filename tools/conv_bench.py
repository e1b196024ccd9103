"""Convolution plans (Plan(shape, convolve=True)) at about 1 GiB per side: one JSON line per shape.

Three routes on the same data, in place, one spectrum shared by every item (--per-item: one per item):
    the plan as it selects its form (fused_row where one exists),
    the composed form on the same shape (forward plan, mifft_aux_mul_spectrum, inverse plan),
    the three-step user route: a plain forward plan, a torch multiply, a plain inverse plan.
Timing as tools/real_bench.py: device events around back-to-back executes, blocks of >= 20 ms, the best of three.  roofline_fraction:
the algorithmic bytes 2 N s per item (plus N s for a per-item spectrum) over 8 TB/s.
    python tools/conv_bench.py [--gib 1] [--per-item]
"""
import json
import math
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
SHAPES = [((256,), "complex64", False), ((1024,), "complex64", False), ((4096,), "complex64", False), ((16384,), "complex64", False),
          ((32768,), "complex64", False), ((4096,), "complex128", False), ((8192,), "complex128", False),
          ((4096,), "float32", True), ((16384,), "float32", True), ((1024,), "float64", True), ((8192,), "float64", True),
          ((1 << 20,), "complex64", False), ((1024, 1024), "complex64", False), ((2048, 2048), "float32", True)]


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
    per_item = "--per-item" in sys.argv[1:]
    dev = torch.device("cuda:0")
    tdt = {"complex64": torch.complex64, "complex128": torch.complex128, "float32": torch.float32, "float64": torch.float64}
    ctd = {"float32": torch.complex64, "float64": torch.complex128, "complex64": torch.complex64, "complex128": torch.complex128}
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
        for shape, dt, real in SHAPES:
            d = numpy.dtype(dt)
            n = int(numpy.prod(shape))
            s = d.itemsize
            batch = max(1, int(gib * (1 << 30)) // (n * s))
            sshape = tuple(shape[:-1]) + (shape[-1] // 2 + 1,) if real else tuple(shape)
            sp = int(numpy.prod(sshape))
            x = torch.randn((batch,) + tuple(shape), dtype=tdt[dt], device=dev)
            H = torch.randn((batch if per_item else 1,) + sshape, dtype=ctd[dt], device=dev)
            sb = batch if per_item else 1
            plan = hip.Plan(shape, dtype=d, convolve=True, real=real, wait_for_finish=False)
            form = plan.conv_form
            t_plan = timed(lambda: plan.execute(x, spectrum=H, batch=batch, spectrum_batch=sb), stream.synchronize, event)
            t_comp = t_plan
            if form == "fused_row":
                plan.conv_form = "composed"          # the composed form on the same shape (its inner plans exist on every plan)
                t_comp = timed(lambda: plan.execute(x, spectrum=H, batch=batch, spectrum_batch=sb), stream.synchronize, event)
            del plan
            # the three-step user route: plain plans and a torch multiply
            if real:
                fw = hip.Plan(shape, dtype=d, real=True, wait_for_finish=False)
                X = torch.empty((batch,) + sshape, dtype=ctd[dt], device=dev)

                def three():
                    fw.execute(x, X, batch=batch)
                    X.mul_(H)
                    fw.execute(X, x, inverse=True, batch=batch)
            else:
                fw = hip.Plan(shape, dtype=d, wait_for_finish=False)

                def three():
                    fw.execute(x, batch=batch)
                    x.mul_(H)
                    fw.execute(x, inverse=True, batch=batch)
            t_three = timed(three, stream.synchronize, event)
            del fw
            item_bytes = 2 * n * s + (sp * ctd[dt].itemsize if per_item else 0)
            rec = {"shape": list(shape), "dtype": dt, "real": real, "batch": batch, "per_item_spectrum": per_item, "form": form,
                   "ms": t_plan * 1e3, "roofline_fraction": item_bytes * batch / t_plan / HBM,
                   "composed_ms": t_comp * 1e3, "composed_roofline_fraction": item_bytes * batch / t_comp / HBM,
                   "three_step_ms": t_three * 1e3, "three_step_roofline_fraction": item_bytes * batch / t_three / HBM,
                   "speedup_vs_composed": t_comp / t_plan, "speedup_vs_three_step": t_three / t_plan}
            print(json.dumps(rec), flush=True)
            del x, H
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
