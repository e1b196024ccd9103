// f32 one-launch convolution rows (fft_conv_row.hpp): complex rows of L points and real rows of n = 2L reals, one instance per
// (complex / real, L); correlation and the spectrum pitch are run-time arguments.  Work-group shapes and forward radix lists:
// fft_row_shapes.hpp, so the LDS footprint matches the row kernels of L points.
#include "mifft_internal.h"
#include "fft_conv_row.hpp"
extern "C" int mifft_conv_row_dispatch_f32(int real, int L, const mifft::ConvRowArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    int rc = -2;
    // real rows of 32768 and 65536 reals: the pair epilogue spills beyond the real row kernels of the same length (500 / 540 bytes
    // of scratch against 376 / 348), so those lengths run the composed form (docs/extensions.md "Convolution plans") and build no real kernel
    for_length<2, 4, 8, 16, 32>(L, rc, [&](auto l) { return launch_conv_row_small<float, l>(real, a, s, query_only); }) ||
        for_length<64, 128, 256, 512, 1024, 2048, 4096, 8192>(L, rc, [&](auto l) { return launch_conv_row<float, l>(real, a, s, query_only); }) ||
        for_length<16384, 32768>(L, rc, [&](auto l) { return launch_conv_row<float, l, false>(real, a, s, query_only); });
    return rc;
}
