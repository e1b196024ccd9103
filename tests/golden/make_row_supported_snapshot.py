"""Generator of tests/golden/row_supported_snapshot.json: which contiguous-axis row lengths each kernel family of the library has a kernel
for -- both precisions, every power of two from 2 to 2^18:

    pass_row, pass_row_interleaved_only   mifft_pass_supported(MIFFT_PASS_ROW, prec, L, 0 / MIFFT_VARIANT_INTERLEAVED_ONLY)
    real_row                              mifft_real_row_supported(prec, L)
    conv_row_complex, conv_row_real       mifft_conv_row_supported(prec, 0 / 1, L)
    r2r_row                               mifft_r2r_row_supported(prec, L)
    half_supported, half_kernel           mifft_half_supported(L, 1, 1), mifft_half_kernel(L, 1, 1, 0)   (complex32: no precision)

The committed file was written from the library of the commit BEFORE the row families took their work-group shapes from one table
(csrc/fft_row_shapes.hpp) and their lengths from per-family lists, so tests/test_host.py::test_row_supported_snapshot holds the library
to the sets that code supported.  Runs without a GPU (the queries touch no device):

    python tests/golden/make_row_supported_snapshot.py [path/to/libmifft.so]      # rewrites the json (default: the package's library)
"""
import ctypes
import json
import os
import sys

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "row_supported_snapshot.json")
LENGTHS = [1 << k for k in range(1, 19)]
F32, F64, PASS_ROW, VARIANT_INTERLEAVED_ONLY = 0, 1, 1, 2       # include/mifft.h (the test checks them against pyfft_amd._native)


def record(lib):
    """{"lengths": [...], "f32": {query: [answer per length]}, "f64": {...}, "complex32": {...}} from a loaded libmifft"""
    def per_precision(prec):
        return {
            "pass_row": [lib.mifft_pass_supported(PASS_ROW, prec, L, 0) for L in LENGTHS],
            "pass_row_interleaved_only": [lib.mifft_pass_supported(PASS_ROW, prec, L, VARIANT_INTERLEAVED_ONLY) for L in LENGTHS],
            "real_row": [lib.mifft_real_row_supported(prec, L) for L in LENGTHS],
            "conv_row_complex": [lib.mifft_conv_row_supported(prec, 0, L) for L in LENGTHS],
            "conv_row_real": [lib.mifft_conv_row_supported(prec, 1, L) for L in LENGTHS],
            "r2r_row": [lib.mifft_r2r_row_supported(prec, L) for L in LENGTHS],
        }
    return {
        "lengths": LENGTHS,
        "f32": per_precision(F32),
        "f64": per_precision(F64),
        "complex32": {
            "half_supported": [lib.mifft_half_supported(L, 1, 1) for L in LENGTHS],
            "half_kernel": [lib.mifft_half_kernel(L, 1, 1, 0) for L in LENGTHS],
        },
    }


def load(path=PATH):
    with open(path) as f:
        return json.load(f)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        lib = ctypes.CDLL(os.path.abspath(sys.argv[1]))        # (every argument and result of these queries is a C int: ctypes' default)
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
        from pyfft_amd import _native
        lib = _native.lib
    with open(PATH, "w") as f:
        json.dump(record(lib), f, sort_keys=True, indent=1)
        f.write("\n")
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))
