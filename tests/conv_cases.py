"""The convolution plans' case lists, shared by tests/test_conv_cpu.py (the planner and the coverage rule) and tests/test_conv_gpu.py
(one GPU case per fused instance)."""
import numpy

F32, F64 = numpy.float32, numpy.float64

# (dtype, real, n) of every one-launch instance: complex rows of n points, real rows of n reals
FUSED = ([(F32, False, 1 << e) for e in range(1, 16)] + [(F64, False, 1 << e) for e in range(1, 14)] +
         [(F32, True, 1 << e) for e in range(2, 15)] + [(F64, True, 1 << e) for e in range(2, 14)])

# lengths a row or real-row kernel exists for but the convolution has no one-launch instance: they run the composed form.  Each names the
# line of profiles/r07_conv_transforms.log that records why.
LEFT_OUT = {
    (F32, True, 32768): "dropped f32 real n=32768",
    (F32, True, 65536): "dropped f32 real n=65536",
    (F64, False, 16384): "dropped f64 complex n=16384",
    (F64, True, 16384): "dropped f64 real n=16384",
    (F64, True, 32768): "dropped f64 real n=32768",
}

# (dtype, real, shape) of the composed-form GPU cases
COMPOSED = [(numpy.complex64, False, (1 << 16,)), (numpy.complex64, False, (1 << 20,)), (numpy.complex64, False, (64, 64)),
            (numpy.complex64, False, (1024, 1024)), (numpy.complex64, False, (128, 128, 128)), (numpy.complex128, False, (1 << 16,)),
            (numpy.complex128, False, (64, 64)), (F32, True, (2048, 2048)), (F32, True, (1 << 21,)), (F32, True, (32768,)),
            (F64, True, (16, 64)), (F64, True, (32768,))]


def case_id(c):
    dt, real, n = c[:3]
    return "%s-%s-%s" % (numpy.dtype(dt).name, "real" if real else "complex", n)
