// Internal glue between the C-ABI runtime (mifft_runtime.cpp) and the per-precision kernel tables.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mifft.h"
#include "fft_tile.hpp"
#include "fft_fused2.hpp"
#include "fft_nd.hpp"
#include "fft_wave.hpp"
#include "fft_pair.hpp"
#include "fft_nd2t.hpp"
#include "fft_fusedp.hpp"

// Each returns 0 on success, MIFFT_E_UNSUPPORTED (-2) when no kernel is compiled for (L, tr, variant),
// or a hipError_t.  With query_only != 0 nothing is launched.
extern "C" {
int mifft_dispatch_col_f32(int L, int tr, int variant, const mifft::TileArgs* a, hipStream_t s, int query_only);
int mifft_dispatch_row_f32(int L, int variant, const mifft::TileArgs* a, hipStream_t s, int query_only);
int mifft_dispatch_col_f64(int L, int tr, int variant, const mifft::TileArgs* a, hipStream_t s, int query_only);
int mifft_dispatch_row_f64(int L, int variant, const mifft::TileArgs* a, hipStream_t s, int query_only);
int mifft_nd_max_points(int f64);
int mifft_nd_launch(int f64, long long n, const mifft::NdArgs* a, hipStream_t s);
int mifft_nd2_f32_supported(int x, int y, int z);
int mifft_nd2_f32_launch(int x, int y, int z, const mifft::TileArgs* a, hipStream_t s);
int mifft_nd2_f64_supported(int x, int y, int z);
int mifft_nd2_f64_launch(int x, int y, int z, const mifft::TileArgs* a, hipStream_t s);
void mifft_note_pair_lanes_form(int form);    // mifft_runtime.cpp: what mifft_debug_last_pair_lanes_form answers on this thread
// The units of the persistent two-pass launch (docs/persistent.md has the table of forms).  Each answers from the instance list it
// launches from, for (a, b) = (L0, L1) of a 1-D pair / (ny, nx) of a 2-D one and the layout of the user's buffers, under the calling
// thread's development switches: the form (MIFFT_FUSED2_KERNEL_*) and the work-list tiles per transform go to *c, then -- query == 0 --
// the kernel is launched.  0, MIFFT_E_UNSUPPORTED without such an instance, or a hipError_t.  The 2-D launchers of a precision
// (mifft_fused2d_f32, mifft_fused3d_f64) answer 1 for a shape the 2-D form does not name at all.
struct mifft_fused2_choice {
    int form;
    unsigned tiles0, tiles1;
};
typedef int mifft_fused2_unit(int a, int b, int split, const mifft::FusedArgs* f, unsigned grid, hipStream_t s, int query, mifft_fused2_choice* c);
mifft_fused2_unit mifft_fused2r_f32, mifft_fused2dw_f32, mifft_fused2d_rect_f32, mifft_fused2d_f32, mifft_fused3d_f64;      // 2-D
mifft_fused2_unit mifft_fused2w_f32, mifft_fused2_f32, mifft_fusedx_f64, mifft_fused3_f64;                                  // 1-D
int mifft_aux_copy_launch(const struct mifft_copy* c, const void* s0, const void* s1, void* d0, void* d1, hipStream_t s);
int mifft_aux_mul_rows_launch(int f64, void* a, const void* b, long long rows, long long n, hipStream_t s);
// data[i][j] = scale * data[i][j] * S[i * spectrum_pitch + j] (S = conj(spectrum) when correlate); 0 launched, -1 grid too large
int mifft_aux_mul_spectrum_launch(int f64, void* data, const void* spectrum, long long items, long long points, long long spectrum_pitch,
                                  int correlate, double scale, hipStream_t s);
int mifft_aux_mismatch_launch(const void* a, const void* b, unsigned long long words, unsigned long long* count, hipStream_t s);
int mifft_aux_zero_launch(void* p, unsigned long long nbytes, hipStream_t s);     // nbytes a multiple of 16, p 16-byte aligned
int mifft_wave_supported(int f64, int N);
int mifft_wave_launch(int f64, int N, const mifft::WaveArgs* a, int max_blocks, hipStream_t s);
int mifft_wave_16x16_launch(const mifft::WaveArgs* a, int max_blocks, hipStream_t s);
int mifft_pair_f64(int kind, int k0, int k1, int k2, int split, const mifft::PairArgs* a, hipStream_t s, int query, int* width);
int mifft_pair_f32(int kind, int k0, int k1, int k2, int split, const mifft::PairArgs* a, hipStream_t s, int query, int* width);
int mifft_fusedp(int f64, int split, int x, int y, int z, const mifft::FusedPairArgs* f, unsigned grid, hipStream_t s, int query, int* r0,
                 unsigned* tiles0, unsigned* tiles1);
int mifft_fusedp_more(int f64, int split, int x, int y, int z, const mifft::FusedPairArgs* f, unsigned grid, hipStream_t s, int query, int* r0,
                      unsigned* tiles0, unsigned* tiles1);
int mifft_nd2t(int f64, int x, int y, int z, const mifft::TileArgs* a, const mifft::TiledGeom* g, hipStream_t s, int query);
int mifft_nd2t_split_in(int f64, int x, int y, int z, const mifft::TileArgs* a, const mifft::TiledGeom* g, hipStream_t s, int query);
int mifft_nd2t_split(int f64, int x, int y, int z, const mifft::TileArgs* a, const mifft::TiledGeom* g, hipStream_t s, int query);
int mifft_nd2p(int f64, int x, int y, int z, const mifft::TileArgs* a, hipStream_t s, int query);     // fft_nd2p.hip: dense planes, 16-byte accesses
int mifft_nd2zp(int f64, int x, int y, int z, const mifft::TileArgs* a, hipStream_t s, int query);    // fft_nd2zp.hip: the same with several work-groups per transform (out of place)
int mifft_mixed_supported_impl(int f64, int n);
int mifft_mixed_radices_impl(int n, int32_t* radix);
int mifft_mixed_launch(int f64, int n, long long rows, long long stride_in, long long stride_out, long long inner, const void* in,
                       void* out, const void* tw, int flags, double scale, hipStream_t s);
int mifft_mixed_long_split_impl(int f64, long long n, int* n1, int* n2);
int mifft_mixed_long_launch(int f64, int n1, int n2, long long batch, const void* in, void* mid, void* out, const void* tw1, const void* tw2,
                            const void* tw_lo, const void* tw_hi, int tw_shift, int flags, double scale, hipStream_t s);
int mifft_bluestein_padded_impl(int f64, int n);
int mifft_bluestein_len_supported_impl(int f64, int m);
int mifft_mixed_nd_supported_impl(int f64, int nx, int ny, int nz);
int mifft_mixed_nd_rows_ok_impl(int f64, int n);
int mifft_mixed_nd_launch(int f64, int nx, int ny, int nz, long long transforms, const void* in, void* out, const void* twx, const void* twy,
                          const void* twz, int flags, double scale, hipStream_t s);
int mifft_bluestein_launch(int f64, int n, int m, long long rows, long long stride_in, long long stride_out, const void* in, void* out,
                           const void* tw, const void* chirp, const void* bhat, int flags, double scale, hipStream_t s);
// fft_r2r.hip: the pre / post steps of the cosine and sine transforms; 0 launched, -1 grid too large, else a hipError_t
int mifft_r2r_step_launch(int f64, int post, int inverse, int kind, int nd, const int* n, long long outer, const void* in, void* out,
                          const void* tw, double scale, hipStream_t s);
// fft_r2r_f32.hip / _f64.hip: one-launch cosine / sine rows of L = n / 2 packed points; 0 launched (query: a kernel exists), -2 none,
// -1 grid too large
int mifft_r2r_row_dispatch_f32(int L, int inverse, const mifft::TileArgs* a, hipStream_t s, int query_only);
int mifft_r2r_row_dispatch_f64(int L, int inverse, const mifft::TileArgs* a, hipStream_t s, int query_only);
// fft_real.hip: separation / packing step of the real-input transforms; 0 launched, -1 grid too large, else a hipError_t
int mifft_real_post_launch(int f64, int inverse, int nx, int ny, int nz, long long outer, long long stride_in, long long stride_out,
                           const void* in, void* out, const void* tw, double scale, hipStream_t s);
// fft_real_row_f32.hip / _f64.hip: one-launch real rows of L = n / 2 packed points; 0 launched (query: a kernel exists), -2 none, -1 grid too large
int mifft_real_row_dispatch_f32(int L, int inverse, const mifft::TileArgs* a, hipStream_t s, int query_only);
int mifft_real_row_dispatch_f64(int L, int inverse, const mifft::TileArgs* a, hipStream_t s, int query_only);
// fft_conv_f32.hip / _f64.hip: one-launch convolution rows of L complex (real: packed) points; 0 launched (query: a kernel exists), -2 none,
// -1 grid too large
namespace mifft { struct ConvRowArgs; }
int mifft_conv_row_dispatch_f32(int real, int L, const mifft::ConvRowArgs* a, hipStream_t s, int query_only);
int mifft_conv_row_dispatch_f64(int real, int L, const mifft::ConvRowArgs* a, hipStream_t s, int query_only);
// fft_fir_f32.hip / _f64.hip: one-launch overlap-save FIR rows, blocks of L complex (real: packed) points; 0 launched (query: a kernel
// exists), -2 none, -1 grid too large.  mifft_fir_pad_launch: out[f][j] = j < taps ? in[f * taps + j] : 0, j < n, in scalars of the
// precision, n a multiple of 16 bytes' worth, out 16-byte aligned
namespace mifft { struct FirRowArgs; }
int mifft_fir_row_dispatch_f32(int real, int L, const mifft::FirRowArgs* a, hipStream_t s, int query_only);
int mifft_fir_row_dispatch_f64(int real, int L, const mifft::FirRowArgs* a, hipStream_t s, int query_only);
int mifft_fir_pad_launch(int f64, const void* in, void* out, long long filters, int n, int taps, hipStream_t s);
// fft_nd2z.hip: 0 = launched (query 1: a kernel exists; query 2: one that is preferred at every buffer size), -2 = none, -1 = grid too large
int mifft_nd2z(int f64, int x, int y, int z, const mifft::TileArgs* a, hipStream_t s, int query);
// fft_half.hip / fft_nd2_c32_*.hip: complex32 twins of the fp32 one-launch kernels; 0 launched (query: a kernel exists), -2 none, -1 grid too large
int mifft_c32_row_dispatch(int L, const mifft::TileArgs* a, hipStream_t s, int query_only);
int mifft_c32_nd_launch(long long n, const mifft::NdArgs* a, hipStream_t s);
int mifft_nd2_c32_supported(int x, int y, int z);
int mifft_nd2_c32_launch(int x, int y, int z, const mifft::TileArgs* a, hipStream_t s);
}

// one row of a mifft_fused2_unit's instance list: the form and its tiles per transform, then the launch of the kernel on THREADS threads
#define MIFFT_FUSED2_RUN(FORM, T0, T1, THREADS, ...)                             \
    do {                                                                         \
        *c = {FORM, (unsigned)(T0), (unsigned)(T1)};                             \
        if (query) return 0;                                                     \
        hipLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(THREADS), 0, s, *f);  \
        return (int)hipGetLastError();                                           \
    } while (0)

namespace mifft {
template <typename T, int L, int W, int NT, bool ROW, bool TR, typename RL>
static inline int launch_tile(const TileArgs* a, hipStream_t s, int query_only) {
    return launch_groups(a, &TileArgs::total, W, query_only, [&](dim3 grid) {
        hipLaunchKernelGGL((fft_tile_kernel<T, L, W, NT, ROW, TR, RL>), grid, dim3(NT), 0, s, *a);
    });
}
}  // namespace mifft

#define MIFFT_COL_CASE(T, Lv, Wv, NTv, ...)                                                             \
    case Lv:                                                                                            \
        return tr ? mifft::launch_tile<T, Lv, Wv, NTv, false, true, mifft::RadixList<__VA_ARGS__>>(a, s, query_only) \
                  : mifft::launch_tile<T, Lv, Wv, NTv, false, false, mifft::RadixList<__VA_ARGS__>>(a, s, query_only);
#define MIFFT_ROW_CASE(T, Lv, Wv, NTv, ...)                                                             \
    case Lv:                                                                                            \
        return mifft::launch_tile<T, Lv, Wv, NTv, true, false, mifft::RadixList<__VA_ARGS__>>(a, s, query_only);
// the fp32 ROW tiles below the register-edged rows (L < 256): fft_row_f32.hip expands them for float, fft_half.hip for Complex32<float>
#define MIFFT_ROW_CASES_F32_SHORT(T)       \
    MIFFT_ROW_CASE(T, 2, 2048, 256, 2)     \
    MIFFT_ROW_CASE(T, 4, 1024, 256, 4)     \
    MIFFT_ROW_CASE(T, 8, 512, 256, 8)      \
    MIFFT_ROW_CASE(T, 16, 256, 256, 16)    \
    MIFFT_ROW_CASE(T, 32, 128, 256, 8, 4)  \
    MIFFT_ROW_CASE(T, 64, 64, 256, 8, 8)   \
    MIFFT_ROW_CASE(T, 128, 32, 256, 16, 8)
