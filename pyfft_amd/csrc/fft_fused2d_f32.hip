// fp32 instances of the fused 2-D kernels for RECTANGLES (fft_fused2.hpp; round 4): (ny, nx) in {512, 1024, 2048}^2, ny != nx,
// interleaved.  Both sides up to 1024: 256-thread tiles (fft_fused2d_kernel); a 2048-point axis: 512-thread tiles
// (fft_fused3d_kernel, axis length 512 * A).  Pass 0 runs the y axis over nx / 16 column tiles, pass 1 the x axis over ny / 16.
// -fno-slp-vectorize: see fft_col2_f32.hip.
#include "../../include/mifft.h"
#include "mifft_internal.h"
#include "fft_fused2.hpp"

// (1 = not a rectangle of the 2-D form: mifft_fused2d_f32, fft_fused2_f32.hip, asks this list for every ny != nx)
extern "C" int mifft_fused2d_rect_f32(int ny, int nx, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query,
                                      mifft_fused2_choice* c) {
    if (split) return 1;
#define RECT2(NY, NX) \
    if (ny == NY && nx == NX) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_2D, NX / 16, NY / 16, 256, mifft::fft_fused2d_kernel<float, NY / 256, NX / 256, false, true>);
#define RECT3(NY, NX) \
    if (ny == NY && nx == NX) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_2D_BIG, NX / 16, NY / 16, 512, mifft::fft_fused3d_kernel<float, NY / 512, NX / 512, false, true>);
    RECT2(512, 1024)
    RECT2(1024, 512)
    RECT3(1024, 2048)
    RECT3(2048, 1024)
    RECT3(512, 2048)
    RECT3(2048, 512)
#undef RECT2
#undef RECT3
    return 1;
}

// 2-D shapes with a 256- or 512-point axis on 32-column tiles for that axis' pass (fft_fused2dw_kernel), interleaved: pass 0 (the y
// axis) moves 32 columns where ny <= 512, pass 1 (the x axis) where nx <= 512.  MIFFT_DEBUG_NARROW_TILES = 1: never
extern "C" int mifft_fused2dw_f32(int ny, int nx, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query,
                                  mifft_fused2_choice* c) {
    if (split || mifft_debug_get(MIFFT_DEBUG_NARROW_TILES) == 1) return MIFFT_E_UNSUPPORTED;
#define WIDE2D(NY, NX)                                                                                                             \
    if (ny == NY && nx == NX)                                                                                                      \
        MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_2D_WIDE, NX / (NY <= 512 ? 32 : 16), NY / (NX <= 512 ? 32 : 16), 256, mifft::fft_fused2dw_kernel<NY / 256, NX / 256>);
    WIDE2D(512, 512)
    WIDE2D(512, 1024)
    WIDE2D(1024, 512)
    // a 256-point axis (round 4, second batch): 64 KiB tiles of 32 columns, as in the 1-D kernel for N = 2^16
    WIDE2D(256, 256)
    WIDE2D(256, 512)
    WIDE2D(512, 256)
    WIDE2D(256, 1024)
    WIDE2D(1024, 256)
#undef WIDE2D
    return MIFFT_E_UNSUPPORTED;
}

// 1-D N = 2^16 ... 2^18 on the 32-column tiles (fft_fused2w_kernel): L0 >= L1 in {256, 512}, interleaved -- half as many tiles per
// pass as on 16 columns.  MIFFT_DEBUG_NARROW_TILES = 1: never
extern "C" int mifft_fused2w_f32(int L0, int L1, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query,
                                 mifft_fused2_choice* c) {
    if (split || mifft_debug_get(MIFFT_DEBUG_NARROW_TILES) == 1) return MIFFT_E_UNSUPPORTED;
#define WIDE(A0, A1) \
    if (L0 == 256 * A0 && L1 == 256 * A1) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_1D_WIDE, L1 / 32, L0 / 32, 256, mifft::fft_fused2w_kernel<A0, A1>);
    WIDE(1, 1)
    WIDE(2, 1)
    WIDE(2, 2)
#undef WIDE
    // 2^19, mixed: 16-column first pass, 32-column second pass
    if (L0 == 1024 && L1 == 512) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_1D_MIXED, L1 / 16, L0 / 32, 256, mifft::fft_fused2m_kernel<1>);
    return MIFFT_E_UNSUPPORTED;
}
