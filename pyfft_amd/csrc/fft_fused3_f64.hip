// fp64 instances of the fused persistent two-pass kernels (fft_fused2.hpp), 16-column tiles in both passes, either layout unless a row
// says otherwise.  -fno-slp-vectorize: see fft_col2_f32.hip.
#include "../../include/mifft.h"
#include "mifft_internal.h"
#include "fft_fused2.hpp"

// 1-D L0 x L1.  Round 4: N = 2^16 ... 2^18 with L0 >= L1 in {256, 512} on the 256-thread two-phase tiles (fft_fused2_kernel<double>:
// 16-byte points cross LDS one component at a time, write-through intermediate by 16-byte sc1 stores; split planes, second batch of
// round 4: 16 columns of an fp64 plane are a whole 128-byte line, streamed non-temporally).  2^19 and 2^20 on the 512-thread tiles of
// fft_col3.hpp (2^19: the 512-point pass too, 2 x 256 by decimation in time; split planes: non-temporal loads and stores of the planes
// since the second batch of round 4 -- fft_col3.hpp honoured neither hint for planes before: 2^20 0.373 -> 0.406,
// profiles/r04_aj_split_nt_ab.log)
extern "C" int mifft_fused3_f64(int L0, int L1, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query,
                                mifft_fused2_choice* c) {
// (L0 / 256, L1 / 256, form, threads, kernel template, its NT argument, its A0, A1: fft_fused3_kernel counts an axis in 512s)
#define ONE_D(A0, A1, FORM, THREADS, KERNEL, NT, ...)                                                                   \
    if (L0 == 256 * A0 && L1 == 256 * A1) {                                                                             \
        if (split) MIFFT_FUSED2_RUN(FORM, L1 / 16, L0 / 16, THREADS, mifft::KERNEL<double, __VA_ARGS__, true, NT>);     \
        MIFFT_FUSED2_RUN(FORM, L1 / 16, L0 / 16, THREADS, mifft::KERNEL<double, __VA_ARGS__, false, NT>);               \
    }
    ONE_D(2, 2, MIFFT_FUSED2_KERNEL_1D, 256, fft_fused2_kernel, 1, 2, 2)
    ONE_D(2, 1, MIFFT_FUSED2_KERNEL_1D, 256, fft_fused2_kernel, 1, 2, 1)
    ONE_D(1, 1, MIFFT_FUSED2_KERNEL_1D, 256, fft_fused2_kernel, 1, 1, 1)
    ONE_D(4, 2, MIFFT_FUSED2_KERNEL_1D_BIG, 512, fft_fused3_kernel, true, 2, 1)
    ONE_D(4, 4, MIFFT_FUSED2_KERNEL_1D_BIG, 512, fft_fused3_kernel, true, 2, 2)
#undef ONE_D
    return MIFFT_E_UNSUPPORTED;
}

// 2-D (ny, nx), pass 0 over nx / 16 column tiles, pass 1 over ny / 16.  Interleaved: {256, 512}^2 (round 4; a 256-point axis: its second
// batch) on the 256-thread two-phase tiles (fft_fused2d_kernel<double>), a 1024-point side on the 512-thread tiles (fft_fused3d_kernel,
// axis length 512 * A).  Split planes: 1024 x 1024 (0.374 -> 0.423).  Every shape the 2-D form names in fp64 has its instance: 1 otherwise
extern "C" int mifft_fused3d_f64(int ny, int nx, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query,
                                 mifft_fused2_choice* c) {
#define SMALL2D(NY, NX) \
    if (!split && ny == NY && nx == NX) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_2D, NX / 16, NY / 16, 256, mifft::fft_fused2d_kernel<double, NY / 256, NX / 256, false, true>);
#define BIG2D(NY, NX, SPLIT) \
    if (split == SPLIT && ny == NY && nx == NX) MIFFT_FUSED2_RUN(MIFFT_FUSED2_KERNEL_2D_BIG, NX / 16, NY / 16, 512, mifft::fft_fused3d_kernel<double, NY / 512, NX / 512, SPLIT != 0, true>);
    SMALL2D(512, 512)
    SMALL2D(256, 256)
    SMALL2D(256, 512)
    SMALL2D(512, 256)
    BIG2D(512, 1024, 0)
    BIG2D(1024, 512, 0)
    BIG2D(1024, 1024, 0)
    BIG2D(1024, 1024, 1)
#undef SMALL2D
#undef BIG2D
    return 1;
}
