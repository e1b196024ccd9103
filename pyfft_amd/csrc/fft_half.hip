// complex32 (fp16 interleaved) transforms, docs/extensions.md "Half-precision transforms": the complex32-storage twins of the fp32
// kernels that serve the same shapes in one launch.  Each twin is the fp32 kernel instantiated with TS = Complex32<float>
// (fft_tile.hpp): the first stage's loads widen fp16 to fp32, the last stage's stores round to fp16 (nearest even); the work-group,
// the stages, the LDS exchanges and the twiddle tables are those of the fp32 kernel.  The fixed-shape N-D twins are in the generated
// fft_nd2_c32_*.hip units.
#include "mifft_internal.h"
#include "fft_row2.hpp"

namespace {
using C32 = mifft::Complex32<float>;

template <int P, int NT> int launch_nd(const mifft::NdArgs* a, hipStream_t s) {
    const long long tiles = (a->total + P - 1) / P;
    if (tiles <= 0) return 0;
    if (tiles > 2147483647ll) return -1;
    hipLaunchKernelGGL((mifft::fft_nd_kernel<C32, P, NT>), dim3((unsigned)tiles), dim3(NT), 0, s, *a);
    return (int)hipGetLastError();
}
}  // namespace

// Rows of L points, interleaved both sides: the configurations of mifft_dispatch_row_f32's interleaved kernels -- register-edged
// (fft_row2.hpp) for L >= 256, LDS-staged ROW tiles (fft_tile.hpp) below.  0 launched (query: a kernel exists), -2 none, -1 grid
// too large
extern "C" int mifft_c32_row_dispatch(int L, const mifft::TileArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    switch (L) {
        case 32768: return launch_row2<C32, 32768, 1, 1024, RadixList<32, 32, 32>, true, 4>(a, s, query_only);
        case 16384: return launch_row2<C32, 16384, 1, 512, RadixList<4, 16, 16, 16>, true, 4>(a, s, query_only);
        case 8192: return launch_row2<C32, 8192, 1, 256, RadixList<16, 16, 32>, true>(a, s, query_only);
        case 4096: return launch_row2<C32, 4096, 1, 256, RadixList<16, 16, 16>>(a, s, query_only);
        case 2048: return launch_row2<C32, 2048, 1, 128, RadixList<16, 8, 16>>(a, s, query_only);
        case 1024: return launch_row2<C32, 1024, 4, 256, RadixList<16, 4, 16>>(a, s, query_only);
        case 512: return launch_row2<C32, 512, 8, 256, RadixList<16, 2, 16>>(a, s, query_only);
        case 256: return launch_row2<C32, 256, 8, 256, RadixList<8, 8, 4>>(a, s, query_only);
        MIFFT_ROW_CASE(C32, 2, 2048, 256, 2)
        MIFFT_ROW_CASE(C32, 4, 1024, 256, 4)
        MIFFT_ROW_CASE(C32, 8, 512, 256, 8)
        MIFFT_ROW_CASE(C32, 16, 256, 256, 16)
        MIFFT_ROW_CASE(C32, 32, 128, 256, 8, 4)
        MIFFT_ROW_CASE(C32, 64, 64, 256, 8, 8)
        MIFFT_ROW_CASE(C32, 128, 32, 256, 16, 8)
    }
    return -2;
}

// The run-time-shaped N-D kernel (fft_nd.hpp) for n = x*y*z <= 16384 points: the tiles of mifft_nd_launch's fp32 instances
extern "C" int mifft_c32_nd_launch(long long n, const mifft::NdArgs* a, hipStream_t s) {
    if (n <= 4096) return launch_nd<4096, 256>(a, s);
    if (n <= 8192) return launch_nd<8192, 512>(a, s);
    return launch_nd<16384, 1024>(a, s);
}
