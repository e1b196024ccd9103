// f64 one-launch overlap-save FIR rows (fft_fir_row.hpp): blocks of L complex points and of n = 2L reals, one instance per
// (complex / real, L) -- the convolution rows' instances on the Row2Stages path (L >= 64; fft_conv_f64.hip), with their work-group
// shapes and radix lists (fft_row_shapes.hpp).
#include "mifft_internal.h"
#include "fft_fir_row.hpp"
extern "C" int mifft_fir_row_dispatch_f64(int real, int L, const mifft::FirRowArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    int rc = -2;
    // (real blocks of 16384 reals and beyond, complex blocks of 16384 points: no convolution row to follow, fft_conv_f64.hip)
    for_length<64, 128, 256, 512, 1024, 2048, 4096>(L, rc, [&](auto l) { return launch_fir_row<double, l>(real, a, s, query_only); }) ||
        for_length<8192>(L, rc, [&](auto l) { return launch_fir_row<double, l, false>(real, a, s, query_only); });
    return rc;
}
