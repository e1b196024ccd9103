// f64 one-launch real-input rows (fft_real_row.hpp): every L = n / 2 that has a ROW kernel, forward and inverse.  The work-group shapes
// are those of the complex rows of L points (fft_row_f64.hip), so LDS footprint and occupancy match them.
#include "mifft_internal.h"
#include "fft_real_row.hpp"
extern "C" int mifft_real_row_dispatch_f64(int L, int inverse, const mifft::TileArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    switch (L) {
        case 2: return launch_real_row_small<double, 2>(a, inverse, s, query_only);
        case 4: return launch_real_row_small<double, 4>(a, inverse, s, query_only);
        case 8: return launch_real_row_small<double, 8>(a, inverse, s, query_only);
        case 16: return launch_real_row_small<double, 16>(a, inverse, s, query_only);
        case 32: return launch_real_row_small<double, 32>(a, inverse, s, query_only);
        case 64: return launch_real_row<double, 64, 32, 256, RadixList<8, 8>>(a, inverse, s, query_only);
        case 128: return launch_real_row<double, 128, 32, 256, RadixList<16, 8>>(a, inverse, s, query_only);
        case 256: return launch_real_row<double, 256, 8, 256, RadixList<8, 8, 4>>(a, inverse, s, query_only);
        case 512: return launch_real_row<double, 512, 8, 256, RadixList<16, 2, 16>>(a, inverse, s, query_only);
        case 1024: return launch_real_row<double, 1024, 4, 256, RadixList<16, 4, 16>>(a, inverse, s, query_only);
        case 2048: return launch_real_row<double, 2048, 1, 128, RadixList<16, 8, 16>>(a, inverse, s, query_only);
        case 4096: return launch_real_row<double, 4096, 1, 256, RadixList<16, 16, 16>>(a, inverse, s, query_only);
        case 8192: return launch_real_row<double, 8192, 1, 512, RadixList<2, 16, 16, 16>, true>(a, inverse, s, query_only);
        case 16384: return launch_real_row<double, 16384, 1, 1024, RadixList<4, 16, 16, 16>, true, 4>(a, inverse, s, query_only);
    }
    return -2;
}
