// The work-group shape of a register-edged contiguous-axis row of L points (fft_row2.hpp): THE table.  Every kernel family built on
// those stages -- complex rows (fft_row_f32.hip / _f64.hip), their complex32 twins (fft_half.hip), real rows (fft_real_row_*.hip),
// convolution rows (fft_conv_*.hip), cosine / sine rows (fft_r2r_*.hip) and pass 0 of the row-first persistent 2-D kernel
// (fft_fused2r.hpp) -- takes W, NT, RL, HALF and OCC of a length from here, so LDS footprint, occupancy class and stage order of
// one length are the same in all of them, and a retune is one line.  WHICH lengths a family instantiates stays an explicit list in
// that family's file (for_length below): that is the family's own decision, with its own evidence.
#pragma once
#include <type_traits>
#include "fft_tile.hpp"

namespace mifft {

// W rows per work-group, NT threads (NT / W per row), the stages' radices, HALF: the exchanges move real and imaginary parts one
// after the other through a slab of L scalars (fft_row2.hpp), OCC: waves per SIMD the register allocation must leave room for
template <int W_, int NT_, typename RL_, bool HALF_ = false, int OCC_ = 1> struct Row2ShapeOf {
    static constexpr int W = W_, NT = NT_, OCC = OCC_;
    static constexpr bool HALF = HALF_;
    using RL = RL_;
};

// T: the working precision (complex32 storage works in float: key on StorageOf<TS>::work).  Chosen by measurement (1 GiB buffers,
// tools/row_probe.py; docs/kernels.md "fft_row2_kernel").
template <typename T, int L> struct Row2Shape;
// L = 64, 128: the extension rows only (real, convolution, cosine / sine) -- the complex ROW dispatch runs the LDS-staged tile kernel
// there, which has no register epilogue.  Complex rows start at 256 (fp32; planes at 512: the LDS-staged kernel measured faster for
// planes at L = 256, 0.740 against 0.716) and at 1024 (fp64: for L <= 512 the LDS-staged tile kernels measure faster for 16-byte points).
template <typename T> struct Row2Shape<T, 64> : Row2ShapeOf<32, 256, RadixList<8, 8>> {};
template <typename T> struct Row2Shape<T, 128> : Row2ShapeOf<32, 256, RadixList<16, 8>> {};
template <typename T> struct Row2Shape<T, 256> : Row2ShapeOf<8, 256, RadixList<8, 8, 4>> {};
template <typename T> struct Row2Shape<T, 512> : Row2ShapeOf<8, 256, RadixList<16, 2, 16>> {};
template <typename T> struct Row2Shape<T, 1024> : Row2ShapeOf<4, 256, RadixList<16, 4, 16>> {};
template <typename T> struct Row2Shape<T, 2048> : Row2ShapeOf<1, 128, RadixList<16, 8, 16>> {};
template <typename T> struct Row2Shape<T, 4096> : Row2ShapeOf<1, 256, RadixList<16, 16, 16>> {};
// The half-exchange form wins where it raises the work-groups per CU, the plain form everywhere else: fp32 8192 2 -> 3 and 16384
// 1 -> 2; fp64 8192 1 -> 2 (59 % -> 70 %).  The longest row of a precision (128 KiB of LDS as scalars, one work-group per CU) exists
// in this form only.
template <> struct Row2Shape<float, 8192> : Row2ShapeOf<1, 256, RadixList<16, 16, 32>, true> {};
template <> struct Row2Shape<float, 16384> : Row2ShapeOf<1, 512, RadixList<4, 16, 16, 16>, true, 4> {};
template <> struct Row2Shape<float, 32768> : Row2ShapeOf<1, 1024, RadixList<32, 32, 32>, true, 4> {};
template <> struct Row2Shape<double, 8192> : Row2ShapeOf<1, 512, RadixList<2, 16, 16, 16>, true> {};
template <> struct Row2Shape<double, 16384> : Row2ShapeOf<1, 1024, RadixList<4, 16, 16, 16>, true, 4> {};

// Run-time L -> compile-time L over a family's explicit list of lengths: rc = f(std::integral_constant<int, L>) for the L of the list
// that matches; false (rc untouched) when none does
template <int... Ls, typename F> static inline bool for_length(int L, int& rc, F&& f) {
    return ((L == Ls && (rc = f(std::integral_constant<int, Ls>{}), true)) || ...);
}

}  // namespace mifft
