"""Half-precision transforms (Plan(shape, dtype="complex32")) against the complex64 plan on the same number of transforms: one JSON line
per shape, about 1 GiB of fp16 data per side.

Timing as tools/real_bench.py times: HIP events around K back-to-back executes on the plan's stream, K grown until a block lasts >= 20
ms, the best of three blocks.  The complex32 plan runs out of place.  complex64 runs twice: IN PLACE, where it takes the fp32 kernel the
complex32 kernel is the twin of ("c64_twin"), and OUT OF PLACE, where it may take a kernel with several work-groups per transform that
has no complex32 twin ("c64_oop"; its kernel family in "c64_oop_nd2z").  Fields: transforms/s and ratios, each run's fraction of the
8 TB/s roofline against its algorithmic bytes (complex32: 4 read + 4 written per point; complex64: 8 + 8), the complex32 kernel instance.
    python tools/half_bench.py [--gib 1] [fwd|inv] [--shape 128x256 ...]
    python tools/half_bench.py --once K [--shape ...]     K untimed executes of each run (for a counter collection), no output
"""
import json
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from real_bench import HBM, timed      # noqa: E402

SHAPES = [(64,), (1024,), (4096,), (16384,), (32768,), (128, 128), (128, 256), (32, 32, 32)]


def _shapes(argv):
    picked = [tuple(int(v) for v in argv[i + 1].split("x")) for i, a in enumerate(argv) if a == "--shape"]
    return picked or SHAPES


def _oop_runs_nd2z(N, shape):
    """The complex64 plan's out-of-place N-D pass at this size runs several work-groups per transform (fft_nd2z.hpp): the one-tile-per-CU
    shapes beyond the run-time-shaped kernel's 16384 points where that kernel is preferred at every buffer size (select_nd, csrc/mifft_runtime.cpp)."""
    x, y, z = tuple(reversed(shape)) + (1,) * (3 - len(shape))
    return len(shape) > 1 and x * y * z > N.lib.mifft_nd_max_points_for(N.F32) and \
        N.lib.mifft_nd_shape_supported(N.F32, x, y, z, N.VARIANT_OUT_OF_PLACE_ANY_SIZE) == 0


def main():
    import pyfft_amd.hip as hip
    import pyfft_amd._native as N
    argv = sys.argv[1:]
    gib = float(argv[argv.index("--gib") + 1]) if "--gib" in argv else 1.0
    once = int(argv[argv.index("--once") + 1]) if "--once" in argv else 0
    inverse = "inv" in argv

    def run(plan, args, kw):
        if not once:
            return timed(hip, plan, args, kw)
        for _ in range(once):
            plan.execute(*args, **kw)
        plan.finish()
        return None

    for shape in _shapes(argv):
        n = int(numpy.prod(shape))
        batch = max(1, int(gib * (1 << 30)) // (n * 4))
        stream = hip.Stream()
        plan = hip.Plan(shape, dtype="complex32", stream=stream)
        hi = hip.DeviceArray((batch * n * 2,), numpy.float16)
        ho = hip.DeviceArray((batch * n * 2,), numpy.float16)
        rng = numpy.random.default_rng(1)
        chunk = 1 << 24                    # (float32 draws in chunks: the host never holds more than 64 MiB of them)
        host = numpy.empty(batch * n * 2, numpy.float16)
        for i in range(0, host.size, chunk):
            host[i:i + chunk] = rng.standard_normal(min(chunk, host.size - i), dtype=numpy.float32)
        hi.set(host)
        del host
        kw = {"batch": batch, "inverse": inverse}
        t_half = run(plan, (hi, ho), kw)
        kernel = plan.kernel_for(batch)
        del plan, hi, ho
        cplan = hip.Plan(shape, dtype=numpy.complex64, stream=stream)
        zi = hip.DeviceArray((batch * n,), numpy.complex64)
        zo = hip.DeviceArray((batch * n,), numpy.complex64)
        N.lib.mifft_memset(zi.ptr, 0, zi.nbytes, None)
        t_twin = run(cplan, (zi,), kw)
        t_oop = run(cplan, (zi, zo), kw)
        del cplan, zi, zo
        if once:
            continue
        rec = {
            "shape": list(shape), "direction": "inverse" if inverse else "forward", "batch": batch, "kernel": kernel,
            "half_transforms_per_s": batch / t_half,
            "c64_twin_transforms_per_s": batch / t_twin,
            "c64_oop_transforms_per_s": batch / t_oop,
            "half_over_c64_twin": t_twin / t_half,
            "half_over_c64_oop": t_oop / t_half,
            "c64_oop_nd2z": _oop_runs_nd2z(N, shape),
            "half_roofline_fraction": 8.0 * n * batch / t_half / HBM,
            "c64_twin_roofline_fraction": 16.0 * n * batch / t_twin / HBM,
            "c64_oop_roofline_fraction": 16.0 * n * batch / t_oop / HBM,
        }
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
