// f64 one-launch convolution rows (fft_conv_row.hpp): complex rows of L points and real rows of n = 2L reals, one instance per
// (complex / real, L); correlation and the spectrum pitch are run-time arguments.  Work-group shapes and forward radix lists:
// fft_row_shapes.hpp, so the LDS footprint matches the row kernels of L points.
#include "mifft_internal.h"
#include "fft_conv_row.hpp"
extern "C" int mifft_conv_row_dispatch_f64(int real, int L, const mifft::ConvRowArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    int rc = -2;
    // real rows of 16384 and 32768 reals spill (308 / 836 bytes of scratch against 0 / 168 for the real rows), and so does the
    // complex row of 16384 points (272 against 0): those run the composed form (docs/extensions.md "Convolution plans"); L = 8192
    // builds the complex kernel only
    for_length<2, 4, 8, 16, 32>(L, rc, [&](auto l) { return launch_conv_row_small<double, l>(real, a, s, query_only); }) ||
        for_length<64, 128, 256, 512, 1024, 2048, 4096>(L, rc, [&](auto l) { return launch_conv_row<double, l>(real, a, s, query_only); }) ||
        for_length<8192>(L, rc, [&](auto l) { return launch_conv_row<double, l, false>(real, a, s, query_only); });
    return rc;
}
