// fp32 instances of the fused two-pass kernel (fft_fused2.hpp).  -fno-slp-vectorize: see fft_col2_f32.hip.
#include "../../include/mifft.h"
#include "mifft_internal.h"
#include "fft_fused2.hpp"

namespace {
// The paired-lane forms of the 1024 x 1024 kernel (fft_col2.hpp PAIR_IN / PAIR_OUT; docs/persistent.md): form 0 moves 8 bytes per lane
// on all four streams of the kernel, form 3 -- the default -- sixteen on all four (forms 1 and 2, the ring side alone, were measured
// and not kept: docs/negative_results.md).  MIFFT_DEBUG_PAIR_LANES = n asks for form n - 1 (0: the default); a form this library has
// no instance of gets -2, never another kernel.
constexpr int kPairLanesDefault = 3;
int pair_lanes_form() {
    const int sw = mifft_debug_get(MIFFT_DEBUG_PAIR_LANES);
    return sw == 0 ? kPairLanesDefault : sw - 1;
}
// Form 0 is also what runs when a user buffer is not 16-byte aligned (the ring is the plan's own allocation and always is;
// mifft_launch_fused2 refuses such buffers today, so this is the kernel's own second line): a property of the launch, not of the query
int launch_1024(const mifft::FusedArgs* f, unsigned grid, hipStream_t s) {
    constexpr int kPairAll = mifft::kPairIn | mifft::kPairOut;
    int form = pair_lanes_form();
    if ((((uintptr_t)f->p0.in0 | (uintptr_t)f->p1.out0) & 15) != 0) form = 0;
    if (form == 3) hipLaunchKernelGGL((mifft::fft_fused2_kernel<float, 4, 4, false, 1, kPairAll, kPairAll>), dim3(grid), dim3(256), 0, s, *f);
    else hipLaunchKernelGGL((mifft::fft_fused2_kernel<float, 4, 4, false, 1>), dim3(grid), dim3(256), 0, s, *f);
    mifft_note_pair_lanes_form(form);
    return (int)hipGetLastError();
}
}  // namespace

// 1-D L0 x L1.  The forms plans choose for L0, L1 in {256, 512, 1024}, L0 >= L1 (the chain's factorisation puts the larger radix first):
// split planes on the lane-interleaved sibling tiles -- an item is the two sibling 16-column tiles side by side in one 512-thread
// work-group (fft_fused2s_kernel), so half as many tiles per pass -- and interleaved data with a 1024-point first pass on the
// 16-column tiles (shorter first passes run the 32-column tiles of fft_fused2d_f32.hip, which are asked first), both streamed
// non-temporally: non-temporal accesses on the streamed side (input of pass 0, output of pass 1) leave the Infinity Cache to the
// intermediate ring, C2 35.0 -> 36.6 %; split planes: whole lines per wave instruction, 2^20 0.366 -> 0.420.  A development switch that
// asks for another form of these (MIFFT_DEBUG_NARROW_TILES = 1, MIFFT_DEBUG_STORE = 2 / 3) gets -2.
// 2048 x 2048 and 2048 x 1024: 512-thread tiles (fft_col3.hpp), either layout (planes: non-temporal, 0.302 -> 0.312).
extern "C" int mifft_fused2_f32(int L0, int L1, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query,
                                mifft_fused2_choice* c) {
#define BIG(A0, A1)                                                                                                                             \
    if (L0 == 512 * A0 && L1 == 512 * A1) {                                                                                                     \
        if (split) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_1D_BIG, L1 / 16, L0 / 16, 512, mifft::fft_fused3_kernel<float, A0, A1, true, true>);    \
        MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_1D_BIG, L1 / 16, L0 / 16, 512, mifft::fft_fused3_kernel<float, A0, A1, false, true>);              \
    }
    BIG(4, 4)
    BIG(4, 2)
#undef BIG
    const int store = mifft_debug_get(MIFFT_DEBUG_STORE);
    if (mifft_debug_get(MIFFT_DEBUG_NARROW_TILES) == 1 || store == 2 || store == 3) return MIFFT_E_UNSUPPORTED;
#define SIBLINGS(A0, A1) \
    if (split && L0 == 256 * A0 && L1 == 256 * A1) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_1D_SIBLINGS, L1 / 32, L0 / 32, 512, mifft::fft_fused2s_kernel<A0, A1, false, true>);
#define TILES16(A1) \
    if (!split && L0 == 1024 && L1 == 256 * A1) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_1D, L1 / 16, L0 / 16, 256, mifft::fft_fused2_kernel<float, 4, A1, false, 1>);
    SIBLINGS(1, 1)
    SIBLINGS(2, 1)
    SIBLINGS(2, 2)
    SIBLINGS(4, 1)
    SIBLINGS(4, 2)
    SIBLINGS(4, 4)
    TILES16(1)
    TILES16(2)      // (never reached: 1024 x 512 runs the mixed tiles, which are asked first, and the switch that takes those away refuses above)
#undef SIBLINGS
#undef TILES16
    if (!split && L0 == 1024 && L1 == 1024) {
        const int form = pair_lanes_form();
        if (form != 0 && form != 3) return MIFFT_E_UNSUPPORTED;
        *c = {MIFFT_FUSED2_KERNEL_1D, (unsigned)L1 / 16, (unsigned)L0 / 16};
        return query ? 0 : launch_1024(f, grid, s);
    }
    return MIFFT_E_UNSUPPORTED;
}

// interleaved 2-D squares: 1024 on the 16-column tiles (fft_fused2d_kernel), 2048 on the 512-thread ones (fft_fused3d_kernel); the
// rectangles live in fft_fused2d_f32.hip.  The 512 square and the split-complex squares are shapes of the 2-D form without an instance
// HERE (-2, not 1): they run the 32-column tiles (mifft_fused2dw_f32) / the row-first kernel (mifft_fused2r_f32), which are asked
// first, and nothing when a switch takes those away -- as the split-complex 2048 square, which had its kernel until the row-first one
// replaced the sibling tiles of the smaller squares
extern "C" int mifft_fused2d_f32(int ny, int nx, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query,
                                 mifft_fused2_choice* c) {
    if (ny != nx) return mifft_fused2d_rect_f32(ny, nx, split, f, grid, s, query, c);
    if (!split && ny == 2048) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_2D_BIG, nx / 16, ny / 16, 512, mifft::fft_fused3d_kernel<float, 4, 4, false, true>);
    if (!split && ny == 1024) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_2D, nx / 16, ny / 16, 256, mifft::fft_fused2d_kernel<float, 4, 4, false, true>);
    return ny == 512 || ny == 1024 || ny == 2048 ? MIFFT_E_UNSUPPORTED : 1;
}
