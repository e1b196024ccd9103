"""Generator of tests/golden/fused2_kernel_snapshot.json: which kernel form (MIFFT_FUSED2_KERNEL_*) a persistent two-pass launch
(mifft_launch_fused2) runs and how many work-list tiles per transform its two passes have, for both precisions, both layouts, the 1-D
descriptor pair (COL L = a, M = b, S = 1, then COL L = b, M = 1, S = a) and the 2-D one (ROW L = nx = a over batch * ny rows, then COL
L = ny = b, S = nx, M = 1) of every (a, b) in {128 ... 4096}^2 -- under the default development switches and under each setting of the
four switches a persistent launch reads, one at a time.  A point is [a, b, form, tiles0, tiles1] or [a, b, negative code].  The grid's
pairs are all well formed, so "malformed" adds the pairs the launch refuses before it looks at a shape.

The committed file was written from the rule of the commit BEFORE the selection moved into one selector (mifft_launch_fused2 of
csrc/mifft_runtime.cpp and the host code of the seven unit launchers, copied into a stand-alone program with every launch replaced by
"return this form"), so it holds the library to what that code launched.  This script regenerates it from mifft_fused2_kernel and must
reproduce it byte for byte.  Runs without a GPU (the query touches no device):

    python tests/golden/make_fused2_kernel_snapshot.py            # rewrites the json
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fused2_kernel_snapshot.json")
SIDES = (128, 256, 512, 1024, 2048, 4096)
FORMS = ("fused2", "fused2s", "fused2w", "fused2m", "fused2d", "fused2dw", "fused3", "fused3d", "fused2r", "fusedx64")   # MIFFT_FUSED2_KERNEL_* 1 ... 10
# (name, MIFFT_DEBUG_* key, value)
SETTINGS = (("default", None, 0), ("narrow_tiles", 9, 1), ("no_rowfirst", 10, 1), ("store_1", 7, 1), ("store_2", 7, 2), ("store_3", 7, 3),
            ("pair_lanes_1", 12, 1), ("pair_lanes_2", 12, 2), ("pair_lanes_3", 12, 3), ("pair_lanes_4", 12, 4))
# settings that leave every point as it is: they act inside the chosen kernel (non-temporal stores; the paired-lane sub-form of the
# 1024 x 1024 kernel, which the launch settles from the pointers' alignment), never on the choice
SAME_AS_DEFAULT = ("store_1", "pair_lanes_1", "pair_lanes_4")
BATCH = 4


def pair(N, prec, layout, twod, a, b):
    """the two descriptors of the grid point (tables: never read, the query touches no device)"""
    d = (N.MifftPass * 2)()
    for p in d:
        p.precision, p.layout, p.scale, p.tw_shift = prec, layout, 1.0, 10
        p.tw_L = p.tw_lo = p.tw_hi = 4096
        p.outer_stride_in = p.outer_stride_out = a * b
    if twod:
        d[0].kind, d[0].L, d[0].M, d[0].S, d[0].outer = N.PASS_ROW, a, 1, 1, BATCH * b
        d[0].outer_stride_in = d[0].outer_stride_out = a
    else:
        d[0].kind, d[0].L, d[0].M, d[0].S, d[0].outer = N.PASS_COL, a, b, 1, BATCH
    d[1].kind, d[1].L, d[1].M, d[1].S, d[1].outer = N.PASS_COL, b, 1, a, BATCH
    return d


def ask(N, d):
    """[form name, tiles0, tiles1] or [negative code] of a descriptor pair"""
    t0, t1 = ctypes.c_uint32(0), ctypes.c_uint32(0)
    code = N.lib.mifft_fused2_kernel(ctypes.byref(d[0]), ctypes.byref(d[1]), ctypes.byref(t0), ctypes.byref(t1))
    return [FORMS[code - 1], t0.value, t1.value] if code > 0 else [code]


def malformed(N):
    """pairs the launch refuses whatever their lengths: [[what, code], ...]"""
    out = []
    d = pair(N, N.F32, N.INTERLEAVED, False, 1024, 1024)
    d[1].precision = N.F64
    out.append(["1-D, passes of two precisions"] + ask(N, d))
    d = pair(N, N.F32, N.INTERLEAVED, False, 1024, 1024)
    d[0].M = 512
    out.append(["1-D, p0.M != p1.L"] + ask(N, d))
    d = pair(N, N.F32, N.INTERLEAVED, False, 1024, 1024)
    d[1].layout = N.SPLIT
    out.append(["1-D, passes of two layouts"] + ask(N, d))
    d = pair(N, N.F32, N.INTERLEAVED, True, 1024, 1024)
    d[1].S = 512
    out.append(["2-D, p1.S != nx"] + ask(N, d))
    d = pair(N, N.F64, N.SPLIT, True, 1024, 1024)
    d[0].L = 1000
    out.append(["2-D, nx = 1000"] + ask(N, d))
    return out


def enumerate_library():
    """{"setting/precision/layout/1d|2d": [point, ...]} and the malformed pairs, asked of mifft_fused2_kernel"""
    from pyfft_amd import _native as N
    points = {}
    for name, key, value in SETTINGS:
        saved = N.lib.mifft_debug_get(key) if key is not None else 0
        if key is not None:
            N.check(N.lib.mifft_debug_set(key, value))
        try:
            for prec in (N.F32, N.F64):
                for layout in (N.INTERLEAVED, N.SPLIT):
                    for twod in (False, True):
                        group = points.setdefault("%s/%s/%s/%s" % (name, "f64" if prec else "f32", "split" if layout else "interleaved",
                                                                   "2d" if twod else "1d"), [])
                        for a in SIDES:
                            for b in SIDES:
                                group.append([a, b] + ask(N, pair(N, prec, layout, twod, a, b)))
        finally:
            if key is not None:
                N.check(N.lib.mifft_debug_set(key, saved))
    return points, malformed(N)


def dump(points, bad, path=PATH):
    """one group per line, so that a change of the file reads as a change of those groups"""
    def js(v):
        return json.dumps(v, separators=(",", ":"))
    head = ['"forms":' + js(list(FORMS)), '"settings":' + js([list(s) for s in SETTINGS]), '"malformed":' + js(bad)]
    groups = ",\n".join("  %s:%s" % (js(k), js(points[k])) for k in sorted(points))
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(head) + ',\n"points":{\n' + groups + "\n}\n}\n")


def load(path=PATH):
    with open(path) as f:
        return json.load(f)


if __name__ == "__main__":
    dump(*enumerate_library())
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))
