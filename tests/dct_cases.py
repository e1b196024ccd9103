"""The cosine / sine transform plans' case lists, shared by tests/test_dct_cpu.py and tests/test_dct_gpu.py.  Every shape runs the
composed form (plan.r2r_form == "composed"): pre step, the inner complex plan of the packed shape, post step."""
import numpy

F32, F64 = numpy.float32, numpy.float64

# (dtype, n) of every one-launch row instance (mifft_r2r_row_supported == 0)
FUSED = ([(F32, n) for n in (4, 8, 16, 32, 64, 256, 1024, 2048, 8192)] + [(F64, 1 << e) for e in range(2, 14)])

# real-row lengths without a one-launch r2r row: they run the composed form.  Each names its line of profiles/r07_dct_transforms.log.
LEFT_OUT = {
    (F32, 128): "dropped f32 n=128",
    (F32, 512): "dropped f32 n=512",
    (F32, 4096): "dropped f32 n=4096",
    (F32, 16384): "dropped f32 n=16384",
    (F32, 32768): "dropped f32 n=32768",
    (F32, 65536): "dropped f32 n=65536",
    (F64, 16384): "dropped f64 n=16384",
    (F64, 32768): "dropped f64 n=32768",
}

# 1-D rows of every length a real-row kernel exists for (the inner plan is then a one-launch row of n / 2 points), and the shortest rows
ROWS = [(F32, 1 << e) for e in range(0, 17)] + [(F64, 1 << e) for e in range(0, 16)]

# (dtype, shape) of the N-D and long composed cases: the inner plans reach the N-D one-launch kernel ((8, 8), (64, 64)), the chain / pair
# kernels ((1024, 1024), (64, 64, 64)), the persistent 2^20 plan (2^21 reals) and unit axes
COMPOSED = [(F32, (8, 8)), (F64, (8, 8)), (F32, (64, 64)), (F64, (64, 64)), (F32, (1024, 1024)), (F32, (64, 64, 64)),
            (F64, (16, 32, 8)), (F32, (1 << 21,)), (F32, (1, 8)), (F32, (8, 1)), (F64, (1, 8)), (F64, (8, 1)), (F32, (4, 1, 2)),
            (F32, (2, 2)), (F32, (2, 16)), (F32, (32, 2)), (F32, (4, 4, 4)), (F32, (1, 1))]


def levels(shape):
    """the accuracy_bound levels of a transform of `shape`: the packed complex transform's log2(N / 2), one for the real separation or
    packing, and one twiddle butterfly per axis (tests/test_dct_cpu.py)"""
    n = int(numpy.prod(shape))
    return max(n.bit_length() - 1, 0) + len(shape)
