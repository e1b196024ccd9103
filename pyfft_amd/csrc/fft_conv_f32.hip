// f32 one-launch convolution rows (fft_conv_row.hpp): complex rows of L points and real rows of n = 2L reals, one instance per
// (complex / real, L); correlation and the spectrum pitch are run-time arguments.  The work-group shapes and forward radix lists are those
// of the real rows of L packed points (fft_real_row_f32.hip), so the LDS footprint matches the row kernels of L points.
#include "mifft_internal.h"
#include "fft_conv_row.hpp"
extern "C" int mifft_conv_row_dispatch_f32(int real, int L, const mifft::ConvRowArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    switch (L) {
        case 2: return launch_conv_row_small<float, 2>(real, a, s, query_only);
        case 4: return launch_conv_row_small<float, 4>(real, a, s, query_only);
        case 8: return launch_conv_row_small<float, 8>(real, a, s, query_only);
        case 16: return launch_conv_row_small<float, 16>(real, a, s, query_only);
        case 32: return launch_conv_row_small<float, 32>(real, a, s, query_only);
        case 64: return launch_conv_row<float, 64, 32, 256, RadixList<8, 8>>(real, a, s, query_only);
        case 128: return launch_conv_row<float, 128, 32, 256, RadixList<16, 8>>(real, a, s, query_only);
        case 256: return launch_conv_row<float, 256, 8, 256, RadixList<8, 8, 4>>(real, a, s, query_only);
        case 512: return launch_conv_row<float, 512, 8, 256, RadixList<16, 2, 16>>(real, a, s, query_only);
        case 1024: return launch_conv_row<float, 1024, 4, 256, RadixList<16, 4, 16>>(real, a, s, query_only);
        case 2048: return launch_conv_row<float, 2048, 1, 128, RadixList<16, 8, 16>>(real, a, s, query_only);
        case 4096: return launch_conv_row<float, 4096, 1, 256, RadixList<16, 16, 16>>(real, a, s, query_only);
        case 8192: return launch_conv_row<float, 8192, 1, 256, RadixList<16, 16, 32>, true>(real, a, s, query_only);
        // real rows of 32768 and 65536 reals: the pair epilogue spills beyond the real row kernels of the same length (500 / 540 bytes
        // of scratch against 376 / 348), so those lengths run the composed form (docs/extensions.md "Convolution plans")
        case 16384: return real ? -2 : launch_conv_row<float, 16384, 1, 512, RadixList<4, 16, 16, 16>, true, 4>(real, a, s, query_only);
        case 32768: return real ? -2 : launch_conv_row<float, 32768, 1, 1024, RadixList<32, 32, 32>, true, 4>(real, a, s, query_only);
    }
    return -2;
}
