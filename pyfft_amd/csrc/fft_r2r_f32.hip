// f32 one-launch cosine / sine rows (fft_r2r_row.hpp): the L = n / 2 whose work-group shape (fft_row_shapes.hpp) exchanges full complex
// numbers through LDS.  The lengths with a half-width slab (HALF) and the others not listed are left to the composed form:
// profiles/r07_dct_transforms.log says why.
#include "mifft_internal.h"
#include "fft_r2r_row.hpp"
extern "C" int mifft_r2r_row_dispatch_f32(int L, int inverse, const mifft::TileArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    int rc = -2;
    for_length<2, 4, 8, 16, 32>(L, rc, [&](auto l) { return launch_r2r_row_small<float, l>(a, inverse, s, query_only); }) ||
        for_length<128, 512, 1024, 4096>(L, rc, [&](auto l) { return launch_r2r_row<float, l>(a, inverse, s, query_only); });
    return rc;
}
