// f32 one-launch overlap-save FIR rows (fft_fir_row.hpp): blocks of L complex points and of n = 2L reals, one instance per
// (complex / real, L) -- the convolution rows' instances on the Row2Stages path (L >= 64; fft_conv_f32.hip), with their work-group
// shapes and radix lists (fft_row_shapes.hpp) -- and the padding launch of filter_spectrum.
#include "mifft_internal.h"
#include "fft_fir_row.hpp"
extern "C" int mifft_fir_row_dispatch_f32(int real, int L, const mifft::FirRowArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    int rc = -2;
    // (real blocks of 32768 and 65536 reals: no convolution row to follow, fft_conv_f32.hip)
    for_length<64, 128, 256, 512, 1024, 2048, 4096, 8192>(L, rc, [&](auto l) { return launch_fir_row<float, l>(real, a, s, query_only); }) ||
        for_length<16384, 32768>(L, rc, [&](auto l) { return launch_fir_row<float, l, false>(real, a, s, query_only); });
    return rc;
}

// scalars: a complex filter is 2 * taps of them in a row of 2 * n
extern "C" int mifft_fir_pad_launch(int f64, const void* in, void* out, long long filters, int n, int taps, hipStream_t s) {
    using namespace mifft;
    const int V = f64 ? 2 : 4;
    FirPadArgs a = {in, out, filters * (n / V), n, taps};
    if (a.total <= 0) return 0;
    const long long want = (a.total + 255) / 256;
    const dim3 grid((unsigned)(want < 8192 ? want : 8192));
    if (f64) hipLaunchKernelGGL((fir_pad_kernel<double, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((fir_pad_kernel<float, 4>), grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
}
