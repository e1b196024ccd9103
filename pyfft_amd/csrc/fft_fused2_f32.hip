// fp32 instances of the fused two-pass kernel (fft_fused2.hpp).  -fno-slp-vectorize: see fft_col2_f32.hip.
#include "../../include/mifft.h"
#include "mifft_internal.h"
#include "fft_fused2.hpp"

namespace {
// The forms plans choose: split planes on the lane-interleaved sibling tiles, interleaved data with a 1024-point pass on the 16-column
// tiles (shorter passes run the 32-column tiles of fft_fused2d_f32.hip), both streamed non-temporally, L0 >= L1 (the chain's
// factorisation puts the larger radix first).  A development switch that asks for another form (MIFFT_NARROW_TILES=1, MIFFT_STORE)
// gets -2.
// The paired-lane forms of the 1024 x 1024 kernel (fft_col2.hpp PAIR_IN / PAIR_OUT; docs/persistent.md): form 0 moves 8 bytes per lane
// on all four streams of the kernel, form 3 -- the default -- sixteen on all four (forms 1 and 2, the ring side alone, were measured
// and not kept: docs/negative_results.md).  Form 0 is also what runs when a user buffer is not 16-byte aligned (the ring is the
// plan's own allocation and always is; mifft_launch_fused2 refuses such buffers today, so this is the kernel's own second line).
// MIFFT_DEBUG_PAIR_LANES = n asks for form n - 1 (0: the default); a form this library has no instance of gets -2, never another kernel.
constexpr int kPairLanesDefault = 3;
int launch_1024(const mifft::FusedArgs* f, unsigned grid, hipStream_t s) {
    constexpr int kPairAll = mifft::kPairIn | mifft::kPairOut;
    const int sw = mifft_debug_get(MIFFT_DEBUG_PAIR_LANES);
    int form = sw == 0 ? kPairLanesDefault : sw - 1;
    if (form != 0 && form != 3) return -2;
    if ((((uintptr_t)f->p0.in0 | (uintptr_t)f->p1.out0) & 15) != 0) form = 0;
    if (form == 3) hipLaunchKernelGGL((mifft::fft_fused2_kernel<float, 4, 4, false, 1, kPairAll, kPairAll>), dim3(grid), dim3(256), 0, s, *f);
    else hipLaunchKernelGGL((mifft::fft_fused2_kernel<float, 4, 4, false, 1>), dim3(grid), dim3(256), 0, s, *f);
    mifft_note_pair_lanes_form(form);
    return (int)hipGetLastError();
}

template <int A0, int A1> int launch(const mifft::FusedArgs* f, int split, unsigned grid, hipStream_t s) {
    if constexpr (A0 < A1) {
        return -2;
    } else {
        // non-temporal accesses on the streamed side (input of pass 1, output of pass 2) leave the Infinity Cache to the
        // intermediate ring: C2 35.0 -> 36.6 %; split planes: whole lines per wave instruction, 2^20 0.366 -> 0.420
        const int store = mifft_debug_get(MIFFT_DEBUG_STORE);
        if (mifft_debug_get(MIFFT_DEBUG_NARROW_TILES) == 1 || store == 2 || store == 3) return -2;
        if (split) {
            hipLaunchKernelGGL((mifft::fft_fused2s_kernel<A0, A1, false, true>), dim3(grid), dim3(512), 0, s, *f);
        } else if constexpr (A0 == 4 && A1 == 4) {
            return launch_1024(f, grid, s);
        } else if constexpr (A0 == 4) {
            hipLaunchKernelGGL((mifft::fft_fused2_kernel<float, A0, A1, false, 1>), dim3(grid), dim3(256), 0, s, *f);
        } else {
            return -2;     // (interleaved L0, L1 <= 512: the 32-column tiles, mifft_fused2w_f32_launch)
        }
        return (int)hipGetLastError();
    }
}
}  // namespace

extern "C" int mifft_fused2_f32_launch(int L0, int L1, const mifft::FusedArgs* f, int split, unsigned grid, hipStream_t s) {
    if (L0 == 2048 && L1 == 2048) {   // 512-thread tiles (fft_col3.hpp)
        if (split) hipLaunchKernelGGL((mifft::fft_fused3_kernel<float, 4, 4, true, true>), dim3(grid), dim3(512), 0, s, *f);   // (planes: non-temporal, 0.302 -> 0.312)
        else hipLaunchKernelGGL((mifft::fft_fused3_kernel<float, 4, 4, false, true>), dim3(grid), dim3(512), 0, s, *f);
        return (int)hipGetLastError();
    }
    if (L0 == 2048 && L1 == 1024) {
        if (split) hipLaunchKernelGGL((mifft::fft_fused3_kernel<float, 4, 2, true, true>), dim3(grid), dim3(512), 0, s, *f);
        else hipLaunchKernelGGL((mifft::fft_fused3_kernel<float, 4, 2, false, true>), dim3(grid), dim3(512), 0, s, *f);
        return (int)hipGetLastError();
    }
    const int key = (L0 / 256) * 10 + (L1 / 256);
    switch (key) {
        case 11: return launch<1, 1>(f, split, grid, s);
        case 12: return launch<1, 2>(f, split, grid, s);
        case 14: return launch<1, 4>(f, split, grid, s);
        case 21: return launch<2, 1>(f, split, grid, s);
        case 22: return launch<2, 2>(f, split, grid, s);
        case 24: return launch<2, 4>(f, split, grid, s);
        case 41: return launch<4, 1>(f, split, grid, s);
        case 42: return launch<4, 2>(f, split, grid, s);
        case 44: return launch<4, 4>(f, split, grid, s);
    }
    return -2;
}

// interleaved 2-D squares: 1024 on the 16-column tiles (fft_fused2d_kernel), 2048 on the 512-thread ones (fft_fused3d_kernel); 512 and
// the rectangles live in fft_fused2d_f32.hip, split-complex squares run the row-first kernel (fft_fused2r_f32.hip)
extern "C" int mifft_fused2d_rect_f32_launch(int ny, int nx, const mifft::FusedArgs* f, unsigned grid, hipStream_t s);
extern "C" int mifft_fused2d_f32_launch(int ny, int nx, const mifft::FusedArgs* f, int split, unsigned grid, hipStream_t s) {
    if (ny != nx) return split ? MIFFT_E_UNSUPPORTED : mifft_fused2d_rect_f32_launch(ny, nx, f, grid, s);
    const int L = nx;
    if (split) return MIFFT_E_UNSUPPORTED;
    if (L == 2048) hipLaunchKernelGGL((mifft::fft_fused3d_kernel<float, 4, 4, false, true>), dim3(grid), dim3(512), 0, s, *f);
    else if (L == 1024) hipLaunchKernelGGL((mifft::fft_fused2d_kernel<float, 4, 4, false, true>), dim3(grid), dim3(256), 0, s, *f);
    else return MIFFT_E_UNSUPPORTED;
    return (int)hipGetLastError();
}
