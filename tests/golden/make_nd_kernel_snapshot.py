"""Generator of tests/golden/nd_kernel_snapshot.json.gz: which kernel form (MIFFT_ND_KERNEL_*) runs an MIFFT_PASS_ND pass, for both
precisions, the four layout classes (interleaved; planes on both sides; planes in only; planes out only), every power-of-two (x, y, z) of
up to 2^24 points, every alias combination the layout allows, MIFFT_FLAG_WRITE_THROUGH on and off, variant 0 and 1 -- under the default
development switches and under each of the five settings the rule reads, one at a time.  Only the points whose form is neither the
run-time-shaped kernel nor an error are listed; tests/test_host.py::test_nd_kernel_snapshot checks the rest by rule.

The committed file was written from the rule of the commit BEFORE the selection moved into one selector (validate()'s ND block and
launch_nd() of csrc/mifft_runtime.cpp, copied into a stand-alone program with every launch replaced by "return this form"), so it holds
the library to what that code launched.  This script regenerates it from mifft_nd_kernel and must reproduce it byte for byte.  Runs
without a GPU (the query touches no device):

    python tests/golden/make_nd_kernel_snapshot.py            # rewrites the json
"""
import ctypes
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nd_kernel_snapshot.json.gz")
MAX_LOG2_POINTS = 24
FORMS = ("wave", "nd2z", "nd2", "nd2zp", "nd2p", "nd2t", "nd")          # MIFFT_ND_KERNEL_* 1 ... 7
LAYOUTS = ("interleaved", "planes", "planes_in", "planes_out")
# (name, MIFFT_DEBUG_* key, value)
SETTINGS = (("default", None, 0), ("no_nd2", 0, 1), ("force_wave", 3, 1), ("alt_rows_6", 5, 6), ("alt_rows_7", 5, 7), ("narrow_tiles", 9, 1))


def shapes():
    for lx in range(MAX_LOG2_POINTS + 1):
        for ly in range(MAX_LOG2_POINTS + 1 - lx):
            for lz in range(MAX_LOG2_POINTS + 1 - lx - ly):
                yield 1 << lx, 1 << ly, 1 << lz


def group_key(setting, prec, layout, aliased, wt, variant):
    return "%s/%s/%s/aliased%d/wt%d/variant%d" % (setting, "f64" if prec else "f32", layout, aliased, wt, variant)


def enumerate_library(unlisted=None):
    """{group key: {form name: [[x, y, z], ...]}} of the points whose form is a fixed one; unlisted(prec, x, y, z, code) is called for
    every other point (code: MIFFT_ND_KERNEL_ND or a negative error code)"""
    from pyfft_amd import _native as N
    points = {}
    d = N.MifftPass()
    d.kind, d.outer, d.scale = N.PASS_ND, 4, 1.0
    d.tw_L = d.tw_lo = d.tw_hi = 4096                # (never read: the query touches no device)
    ref = ctypes.byref(d)
    query = N.lib.mifft_nd_kernel
    all_shapes = list(shapes())
    for name, key, value in SETTINGS:
        saved = N.lib.mifft_debug_get(key) if key is not None else 0
        if key is not None:
            N.check(N.lib.mifft_debug_set(key, value))
        try:
            for prec in (N.F32, N.F64):
                d.precision = prec
                for li, layout in enumerate(LAYOUTS):
                    d.layout = N.INTERLEAVED if li == 0 else N.SPLIT
                    side = N.FLAG_DST_INTERLEAVED if li == 2 else N.FLAG_SRC_INTERLEAVED if li == 3 else 0
                    for wt in (0, 1):
                        d.flags = side | (N.FLAG_WRITE_THROUGH if wt else 0)
                        for variant in (0, 1):
                            d.variant = variant
                            groups = [points.setdefault(group_key(name, prec, layout, a, wt, variant), {}) for a in range(4 if li == 1 else 2)]
                            for x, y, z in all_shapes:
                                d.L, d.M, d.S = x, y, z
                                d.outer_stride_in = d.outer_stride_out = max(2, x * y * z)
                                for aliased, group in enumerate(groups):
                                    code = query(ref, aliased)
                                    if 0 < code < N.ND_KERNEL_ND:
                                        group.setdefault(FORMS[code - 1], []).append([x, y, z])
                                    elif unlisted is not None:
                                        unlisted(prec, x, y, z, code)
        finally:
            if key is not None:
                N.check(N.lib.mifft_debug_set(key, saved))
    return dict((k, v) for k, v in points.items() if v)


def dump(points, path=PATH):
    text = json.dumps({"forms": list(FORMS), "settings": [list(s) for s in SETTINGS], "points": points}, sort_keys=True, separators=(",", ":"))
    with open(path, "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, compresslevel=9, mtime=0) as g:      # (no name, no time: byte-reproducible)
            g.write(text.encode("ascii"))


def load(path=PATH):
    with gzip.open(path, "rt") as f:
        return json.load(f)


if __name__ == "__main__":
    dump(enumerate_library())
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))
