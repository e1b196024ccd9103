// Instances of the row-first persistent 2-D kernel for split-complex fp32 planes (fft_fused2r.hpp): (ny, nx) in {256, 512, 1024}^2 --
// the chain's own order, ROW x from the planes in groups of 16 rows, COL y to the planes on tiles of 16 columns.
// MIFFT_DEBUG_NARROW_TILES = 1 / MIFFT_DEBUG_NO_ROWFIRST = 1: never (A/B against the forms it replaced).
// -fno-slp-vectorize: see fft_col2_f32.hip.
#include "../../include/mifft.h"
#include "mifft_internal.h"
#include "fft_fused2r.hpp"

extern "C" int mifft_fused2r_f32(int ny, int nx, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query,
                                 mifft_fused2_choice* c) {
    if (!split || mifft_debug_get(MIFFT_DEBUG_NARROW_TILES) == 1 || mifft_debug_get(MIFFT_DEBUG_NO_ROWFIRST)) return MIFFT_E_UNSUPPORTED;
#define RF(NY, NX) \
    if (ny == NY && nx == NX) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_2D_ROWFIRST, NY / 16, NX / 16, 256, mifft::fft_fused2r_kernel<NX, NY / 256>);
    RF(1024, 1024)
    RF(512, 512)
    RF(512, 1024)
    RF(1024, 512)
    RF(256, 256)
    RF(256, 512)
    RF(512, 256)
    RF(256, 1024)
    RF(1024, 256)
#undef RF
    return MIFFT_E_UNSUPPORTED;
}
