"""The index division of the mixed-radix kernels, checked exhaustively on the host.

csrc/fft_mixed.hpp computes q = a / d as fast_div(a, inv) = (int)(((float)a + 0.5f) * inv) with inv = 1.0f / d, and the stage loops of
fft_mixed.hip (rows, lines, long transforms, Bluestein) and fft_mixed_nd.hip divide every index that way: by n / R, by Ns, by the rows
of a tile, by `inner`.  Every numerator is a thread's work index j < the points of one tile (W * n, W * m, or the threads times the
butterflies each holds), every divisor at most that many points.  A later LDS or tile-size change that pushes these ranges past what
float32 divides exactly must fail here, not as a silently wrong index on the device."""
import os
import re

import numpy

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyfft_amd", "csrc")


def _constant(fname, name):
    src = open(os.path.join(CSRC, fname)).read()
    m = re.search(r"\b%s\s*=\s*([0-9 *]+)[,;]" % name, src)
    assert m, (fname, name)
    return int(eval(m.group(1), {}))


def tile_points():
    """the largest tile (points) any launcher forms: mixed rows / lines, the one-launch Bluestein kernel, the N-D kernel"""
    return max(_constant("fft_mixed.hpp", "kTilePoints32"), _constant("fft_mixed.hpp", "kTilePoints64"),
               _constant("fft_mixed.hip", "kBluePoints32"), _constant("fft_mixed.hip", "kBluePoints64"),
               _constant("fft_mixed_nd.hip", "kNdTilePoints32"), _constant("fft_mixed_nd.hip", "kNdTilePoints64"))


def fast_div(a, d):
    """the device's expression in float32: (float)a + 0.5f, times fl(1 / d), truncated"""
    inv = numpy.float32(1.0) / numpy.float32(d)
    return ((a.astype(numpy.float32) + numpy.float32(0.5)) * inv).astype(numpy.int64)


def test_fast_div_model_is_the_device_expression():
    src = open(os.path.join(CSRC, "fft_mixed.hpp")).read()
    assert "fast_div(int a, float inv) { return (int)(((float)a + 0.5f) * inv); }" in src


def test_fast_div_is_exact_over_every_range_the_launchers_form():
    """Every divisor d <= the largest tile and every numerator a < 2x the largest tile (both far below 2^22, where (float)a + 0.5f
    stops being exact).  (a + 0.5) * fl(1/d) rounded is non-decreasing in a, so q is correct for all a once it is correct at the
    boundaries k d - 1 and k d: those are checked, for every k."""
    top = tile_points()
    assert top < (1 << 22) and 2 * top < (1 << 22), top
    a_max = 2 * top                           # (work indices stay below one tile; the margin keeps a small tile increase in range)
    for d in range(1, top + 1):
        at = numpy.arange(0, a_max, d, dtype=numpy.int64)
        edges = numpy.concatenate([at, at[1:] - 1, [a_max - 1]])
        assert numpy.array_equal(fast_div(edges, d), edges // d), d


def test_fast_div_monotone_argument_holds_on_a_dense_sample():
    """the boundary argument above, checked against every numerator for a spread of divisors"""
    a = numpy.arange(0, 2 * tile_points(), dtype=numpy.int64)
    for d in (1, 2, 3, 5, 7, 9, 15, 49, 125, 243, 343, 1000, 2187, 3125, 4095, 5000, 9999, 10000, 16383, 16384):
        assert numpy.array_equal(fast_div(a, d), a // d), d
