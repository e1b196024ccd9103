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
    return mifft::launch_groups(a, &mifft::NdArgs::total, P, 0, [&](dim3 grid) {
        hipLaunchKernelGGL((mifft::fft_nd_kernel<C32, P, NT>), grid, dim3(NT), 0, s, *a);
    });
}
}  // namespace

// Rows of L points, interleaved both sides: the lengths of mifft_dispatch_row_f32's interleaved kernels -- register-edged (fft_row2.hpp,
// float's shapes of fft_row_shapes.hpp) for L >= 256, the fp32 LDS-staged ROW tiles (fft_tile.hpp) below.  0 launched (query: a kernel
// exists), -2 none, -1 grid too large
extern "C" int mifft_c32_row_dispatch(int L, const mifft::TileArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    int rc;
    if (for_length<256, 512, 1024, 2048, 4096, 8192, 16384, 32768>(L, rc, [&](auto l) { return launch_row2<C32, l>(a, s, query_only); })) return rc;
    switch (L) {
        MIFFT_ROW_CASES_F32_SHORT(C32)
    }
    return -2;
}

// The run-time-shaped N-D kernel (fft_nd.hpp) for n = x*y*z <= 16384 points: the tiles of mifft_nd_launch's fp32 instances
extern "C" int mifft_c32_nd_launch(long long n, const mifft::NdArgs* a, hipStream_t s) {
    if (n <= 4096) return launch_nd<4096, 256>(a, s);
    if (n <= 8192) return launch_nd<8192, 512>(a, s);
    return launch_nd<16384, 1024>(a, s);
}
