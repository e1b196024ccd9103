"""Overlap-save FIR plans (Plan(n, convolve=True, taps=m)) at about 1 GiB per side: one JSON line per (dtype, n, m).

Three routes on the same signals (64 items, one spectrum shared by every item):
    the FIR plan: one launch, the signal crosses HBM once in and once out,
    the fused convolution row Plan(n, convolve=True) on as many dense rows as the FIR plan has blocks (the same transforms and products
        per row; time per ROW against the FIR plan's time per BLOCK),
    the three-step user route: a torch gather of the overlapping blocks into a padded array (unfold + copy), the fused convolution rows
        in place on it, a torch copy of every block's valid part into the output.
Timing as tools/conv_bench.py: device events around back-to-back executes, blocks of >= 20 ms, the best of three.  roofline_fraction:
the algorithmic bytes 2 length s per item over 8 TB/s.  expected_speedup: the three-step route's bytes over the plan's,
(2 + 3 n / hop) / 2.
    python tools/fir_bench.py [--gib 1]
"""
import json
import math
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
ITEMS = 64
CASES = [("complex64", False, 256), ("complex64", False, 1024), ("complex64", False, 4096), ("complex64", False, 16384),
         ("float32", True, 4096)]


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
    tdt = {"complex64": torch.complex64, "float32": torch.float32}
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
        for dt, real, n in CASES:
            d = numpy.dtype(dt)
            s = d.itemsize
            for m in (n // 4 + 1, n // 2):
                plan = hip.Plan(n, dtype=d, convolve=True, real=real, taps=m, wait_for_finish=False)
                ov, hop = plan.overlap, plan.hop
                length = int(gib * (1 << 30)) // (ITEMS * s) // hop * hop        # whole blocks: the three-step route needs no tail case
                blocks = plan.blocks(length)
                # the signals behind `ov` zeros each, so that the gather of the three-step route is one unfold
                xp = torch.zeros((ITEMS, ov + length), dtype=tdt[dt], device=dev)
                xp[:, ov:] = torch.randn((ITEMS, length), dtype=tdt[dt], device=dev)
                x = xp[:, ov:]
                pitch = ov + length
                y = torch.empty((ITEMS, pitch), dtype=tdt[dt], device=dev)
                h = torch.randn((m,), dtype=tdt[dt], device=dev)
                H = torch.empty(plan.spectrum_shape(), dtype=torch.complex64, device=dev)
                plan.filter_spectrum(h, H)
                stream.synchronize()
                if real and pitch & 1:
                    raise SystemExit("odd pitch")
                xptr, yptr = x.data_ptr(), y.data_ptr()
                t_fir = timed(lambda: plan.execute(xptr, yptr, spectrum=H, length=length, batch=ITEMS, pitch=pitch), stream.synchronize, event)
                kernel = plan.kernel
                del plan
                rows = ITEMS * blocks
                conv = hip.Plan(n, dtype=d, convolve=True, real=real, wait_for_finish=False)
                buf = torch.empty((ITEMS, blocks, n), dtype=tdt[dt], device=dev)
                buf.copy_(xp.unfold(1, n, hop))
                t_conv = timed(lambda: conv.execute(buf, spectrum=H, batch=rows), stream.synchronize, event)
                yv = y[:, :length].unflatten(1, (blocks, hop))

                def three():
                    buf.copy_(xp.unfold(1, n, hop))
                    conv.execute(buf, spectrum=H, batch=rows)
                    yv.copy_(buf[:, :, ov:])
                t_three = timed(three, stream.synchronize, event)
                del conv
                rec = {"dtype": dt, "real": real, "n": n, "taps": m, "overlap": ov, "hop": hop, "items": ITEMS, "length": length,
                       "blocks_per_item": blocks, "kernel": kernel, "ms": t_fir * 1e3,
                       "roofline_fraction": 2.0 * length * s * ITEMS / t_fir / HBM,
                       "ns_per_block": t_fir / rows * 1e9, "conv_row_ns_per_row": t_conv / rows * 1e9,
                       "block_over_conv_row": t_fir / t_conv,
                       "three_step_ms": t_three * 1e3, "speedup_vs_three_step": t_three / t_fir,
                       "expected_speedup": (2.0 + 3.0 * n / hop) / 2.0}
                print(json.dumps(rec), flush=True)
                del xp, x, y, buf, yv, H, h
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
