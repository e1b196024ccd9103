// f32 one-launch cosine / sine rows (fft_r2r_row.hpp): every L = n / 2 whose real row (fft_real_row_f32.hip) exchanges full complex
// numbers through LDS, with that row's work-group shape and radix list.  The real rows with a half-width slab (HALF) are left to the
// composed form: profiles/r07_dct_transforms.log says why.
#include "mifft_internal.h"
#include "fft_r2r_row.hpp"
extern "C" int mifft_r2r_row_dispatch_f32(int L, int inverse, const mifft::TileArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    switch (L) {
        case 2: return launch_r2r_row_small<float, 2>(a, inverse, s, query_only);
        case 4: return launch_r2r_row_small<float, 4>(a, inverse, s, query_only);
        case 8: return launch_r2r_row_small<float, 8>(a, inverse, s, query_only);
        case 16: return launch_r2r_row_small<float, 16>(a, inverse, s, query_only);
        case 32: return launch_r2r_row_small<float, 32>(a, inverse, s, query_only);
        case 128: return launch_r2r_row<float, 128, 32, 256, RadixList<16, 8>>(a, inverse, s, query_only);
        case 512: return launch_r2r_row<float, 512, 8, 256, RadixList<16, 2, 16>>(a, inverse, s, query_only);
        case 1024: return launch_r2r_row<float, 1024, 4, 256, RadixList<16, 4, 16>>(a, inverse, s, query_only);
        case 4096: return launch_r2r_row<float, 4096, 1, 256, RadixList<16, 16, 16>>(a, inverse, s, query_only);
    }
    return -2;
}
