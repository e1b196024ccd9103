// f64 one-launch real-input rows (fft_real_row.hpp): every L = n / 2 that has a ROW kernel, forward and inverse, in the work-group shape
// of the complex row of L points (fft_row_shapes.hpp), so LDS footprint and occupancy match it.
#include "mifft_internal.h"
#include "fft_real_row.hpp"
extern "C" int mifft_real_row_dispatch_f64(int L, int inverse, const mifft::TileArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    int rc = -2;
    for_length<2, 4, 8, 16, 32>(L, rc, [&](auto l) { return launch_real_row_small<double, l>(a, inverse, s, query_only); }) ||
        for_length<64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384>(L, rc, [&](auto l) { return launch_real_row<double, l>(a, inverse, s, query_only); });
    return rc;
}
