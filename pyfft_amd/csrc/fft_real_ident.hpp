// The separation and packing identities of a real transform through its packed complex transform Z, L = n / 2 points (csrc/fft_real.hip
// derives them), written once for the streaming kernel of fft_real.hip and the one-launch rows (fft_real_row.hpp, fft_conv_row.hpp,
// fft_r2r_row.hpp).  All of them start from a point and its mirror: s = Z[k] + conj Z[L - k], d = Z[k] - conj Z[L - k]; w = w(n)^k.
// The parameters stand in the order of the formulas, w before d, by value (real_sd: its inputs by reference): the compiler orders the
// operands of the products by it before it inlines, and with another order the kernels compile to other instruction text
// (tools/device_code_diff.py, profiles/r12_row_sharing.log).
#pragma once
#include "fft_butterfly.hpp"

namespace mifft {

// s and d of the pair p = Z[k], q = Z[L - k] (the inverse: p = X[k], q = X[L - k])
template <typename T> __device__ __forceinline__ void real_sd(const cplx<T>& p, const cplx<T>& q, cplx<T>& s, cplx<T>& d) {
    s = cplx<T>{p.x + q.x, p.y - q.y};
    d = cplx<T>{p.x - q.x, p.y + q.y};
}

// t = w d of the separation
template <typename T> __device__ __forceinline__ cplx<T> real_wd(cplx<T> w, cplx<T> d) {
    return cplx<T>{w.x * d.x - w.y * d.y, w.x * d.y + w.y * d.x};
}

// separation: X[k] = h (s - i t), h = scale / 2
template <typename T> __device__ __forceinline__ cplx<T> real_sep(cplx<T> s, cplx<T> w, cplx<T> d, T h) {
    const cplx<T> t = real_wd<T>(w, d);
    return cplx<T>{(s.x + t.y) * h, (s.y - t.x) * h};
}

// the mirrored point from the same s, d: X[L - k] = conj(h (s + i t))
template <typename T> __device__ __forceinline__ cplx<T> real_sep_mirror(cplx<T> s, cplx<T> w, cplx<T> d, T h) {
    const cplx<T> t = real_wd<T>(w, d);
    return cplx<T>{(s.x - t.y) * h, -(s.y + t.x) * h};
}

// the k = 0 edge: X[L] = h (s + i d) from the s, d of k = 0 (w(n)^L = -1)
template <typename T> __device__ __forceinline__ cplx<T> real_sep_edge(cplx<T> s, cplx<T> d, T h) {
    return cplx<T>{(s.x - d.y) * h, (s.y + d.x) * h};
}

// packing: Z'[k] = s + i conj(w) d, s and d from the pair X[k], X[L - k]
template <typename T> __device__ __forceinline__ cplx<T> real_pack(cplx<T> s, cplx<T> w, cplx<T> d) {
    const cplx<T> t = {w.x * d.x + w.y * d.y, w.x * d.y - w.y * d.x};    // conj(w) d
    return cplx<T>{s.x - t.y, s.y + t.x};
}

}  // namespace mifft
