// fp32 contiguous-axis (ROW) kernels: register-edged form (fft_row2.hpp; shapes: fft_row_shapes.hpp) for interleaved L >= 256 and
// planes L >= 512, LDS-staged tile kernels (fft_tile.hpp; W rows of L points per work-group, 16 points per thread) for the rest.
#include "mifft_internal.h"
#include "fft_row2.hpp"
#include "../../include/mifft.h"
extern "C" int mifft_dispatch_row_f32(int L, int variant, const mifft::TileArgs* a, hipStream_t s, int query_only) {
    using namespace mifft;
    if (variant != 0 && variant != 2) return -2;
    int rc;
    // L = 32768 exists in the register-edged half-exchange form only (128 KiB of LDS as scalars, one work-group per CU):
    // interleaved data on both sides; a query with variant 2 (MIFFT_VARIANT_INTERLEAVED_ONLY) asks for exactly that
    // (second batch of round 4: planes too -- the first stage loads and the last stage stores either layout, the exchanges are the same)
    if (L == 32768) {
        if (query_only) return 0;
        if (!a || (!a->split && a->split_out)) return -2;
        if (a->split) return launch_row2_lay<float, 32768>(a, s, 0);
        if (mifft_debug_get(MIFFT_DEBUG_ALT_ROWS)) return -2;    // (the alternative stage lists were A/B forms, measured and not adopted)
        return launch_row2<float, 32768>(a, s, 0);
    }
    // Split-complex planes (second batch of round 4): the register-edged kernels with the first-stage operands loaded from / the
    // last-stage results stored to the two planes -- planes -> planes (a single-pass plan) and planes -> interleaved (the first pass of a
    // multi-pass plan); rounds 1-3 sent every split row to the LDS-staged tile kernels below (1024 x 4096 planes, the reference's
    // 32 MiB protocol: 0.515 against 0.809 interleaved; 8192: 0.418 / 0.645 -- profiles/r04_at_rows_split.log)
    if (a && !(!a->split && a->split_out) && (a->split || a->split_out) && mifft_debug_get(MIFFT_DEBUG_NARROW_TILES) != 1) {
        if (for_length<512, 1024, 2048, 4096, 8192, 16384>(L, rc, [&](auto l) { return launch_row2_lay<float, l>(a, s, query_only); })) return rc;
    }
    // both sides interleaved
    if (a && !a->split && !a->split_out) {
        if (for_length<256, 512, 1024, 2048, 4096, 8192, 16384>(L, rc, [&](auto l) { return launch_row2<float, l>(a, s, query_only); })) return rc;
    }
    switch (L) {
        MIFFT_ROW_CASES_F32_SHORT(float)
        MIFFT_ROW_CASE(float, 256, 16, 256, 16, 16)
        MIFFT_ROW_CASE(float, 512, 8, 256, 8, 8, 8)
        MIFFT_ROW_CASE(float, 1024, 4, 256, 16, 16, 4)
        MIFFT_ROW_CASE(float, 2048, 2, 256, 16, 16, 8)
        MIFFT_ROW_CASE(float, 4096, 1, 256, 16, 16, 16)
        MIFFT_ROW_CASE(float, 8192, 1, 512, 16, 16, 16, 2)
        MIFFT_ROW_CASE(float, 16384, 1, 1024, 16, 16, 16, 4)
    }
    return -2;
}
