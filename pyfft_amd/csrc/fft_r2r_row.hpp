// One-launch cosine / sine rows (Plan(n, r2r=...) where mifft_r2r_row_supported is 0): Makhoul's algorithm (csrc/fft_r2r.hip,
// tests/dct_model.py) around the stages of fft_row2.hpp in ONE work-group, so that a row crosses HBM once: n s bytes in, n s out.
//   forward  load prologue: one 16-byte read of x[4j .. 4j + 3] is z[j] = (x[4j], x[4j + 2]) and z[L - 1 - j] = (x[4j + 3], x[4j + 1])
//            of the packed permuted row (DST: the odd samples negated); both go to the row's LDS slab, and every thread fetches its
//            first-stage points from there.  The stages of the complex row of L = n / 2 points run.  The epilogue exchanges the
//            transform through the slab once more (Z[k] needs Z[L - k]: real_mirror_pairs, as RealSepEpi), forms 2 V[k] and stores
//            y[k] = Re(t[k] 2V[k]) and y[n - k] = -Im(t[k] 2V[k]) (DST: at n - 1 - k and k - 1): one ascending and one descending run.
//   inverse  every thread loads the orbit {Y[k], Y[n - k], Y[L + k], Y[L - k]} of its first-stage points (ascending and descending
//            runs), forms V[k] = u[k] (Y[k] - i Y[n - k]) and V[L + k], and packs Z'[k] = (V[k] + V[L + k]) + i w(n)^-k (V[k] - V[L + k]);
//            the inverse stages run; the epilogue puts the packed result through the slab and stores x[4j .. 4j + 3] as one 16-byte
//            write (the un-permutation).
// Rows of L <= 32 packed points: one thread per row, the whole transform in registers (Dft<L>).
// Tables: a.tw_L = w(L)^k (the stages), a.tw_lo = w(n)^k (k < L, the separation / packing), a.tw_hi = forward t[k] = 2 g c[k] w(4n)^k
// (k <= L) or inverse u[k] = g w(4n)^-k / 2c[k] (k < n), g the plan's factor; a.has_tw = kind (0 DCT, 1 DST).  The row kernels support the
// work-group shapes whose real row exchanges full complex numbers through LDS (no HALF slab): fp32 and fp64 n <= 8192.
#pragma once
#include "fft_real_row.hpp"

namespace mifft {

template <typename T> struct R2rVec4 { T v[4]; };
template <typename T> __device__ __forceinline__ R2rVec4<T> r2r_load4(const T* p) {
    if constexpr (sizeof(T) == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        return {{q.x, q.y, q.z, q.w}};
    } else {
        const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
        return {{a.x, a.y, b.x, b.y}};
    }
}
template <typename T> __device__ __forceinline__ void r2r_store4(T* p, T a, T b, T c, T d) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = float4{a, b, c, d};
    } else {
        reinterpret_cast<double2*>(p)[0] = double2{a, b};
        reinterpret_cast<double2*>(p)[1] = double2{c, d};
    }
}

template <typename T> __device__ __forceinline__ cplx<T> r2r_cmul(cplx<T> a, cplx<T> b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// forward outputs of the point pair (Z[k], Z[L - k]) given as its s, d (real_sd): y[k], y[n - k] (k > 0), and y[L] from k = 0.  2V[k]
// and 2V[L] are real_sep and real_sep_edge with h = 1, written out with r2r_cmul: through those functions the kernels schedule differently
template <typename T, int L>
__device__ __forceinline__ void r2r_fwd_emit(T* out, const cplx<T>* sep, const cplx<T>* tab, int dst, int k, cplx<T> s, cplx<T> d) {
    constexpr int n = 2 * L;
    const cplx<T> t = r2r_cmul(sep[k], d);
    const cplx<T> u = r2r_cmul(tab[k], cplx<T>{s.x + t.y, s.y - t.x});     // t[k] 2V[k]
    out[dst ? n - 1 - k : k] = u.x;
    if (k != 0) out[dst ? k - 1 : n - k] = -u.y;
    else out[dst ? L - 1 : L] = r2r_cmul(tab[L], cplx<T>{s.x - d.y, s.y + d.x}).x;   // 2V[L]: w(n)^L = -1
}

// inverse packing of point k from the Y orbit: Z'[k]
template <typename T, int L>
__device__ __forceinline__ cplx<T> r2r_inv_pack(const T* y, const cplx<T>* sep, const cplx<T>* tab, int dst, int k) {
    constexpr int n = 2 * L;
    auto at = [&](int j) __attribute__((always_inline)) { return y[dst ? n - 1 - j : j]; };
    const T ya = at(k), yb = k ? at(n - k) : (T)0, yc = at(L + k), yd = at(L - k);
    const cplx<T> va = r2r_cmul(tab[k], cplx<T>{ya, -yb});                   // u[k] (Y[k] - i Y[n - k])
    const cplx<T> vc = r2r_cmul(tab[L + k], cplx<T>{yc, -yd});               // u[L + k] (Y[L + k] - i Y[L - k])
    const cplx<T> w = sep[k];
    const cplx<T> df = r2r_cmul(cplx<T>{w.x, -w.y}, cplx<T>{va.x - vc.x, va.y - vc.y});
    return cplx<T>{va.x + vc.x - df.y, va.y + vc.y + df.x};
}

template <typename T, int L> struct R2rFwdEpi {
    template <int NB, int R, int TPR, int LR, typename LdsT>
    static __device__ __forceinline__ void run(LdsT* lds, cplx<T>* v, const TileArgs& a, int tid, char* outb, bool valid) {
        const cplx<T>* sep = reinterpret_cast<const cplx<T>*>(a.tw_lo);
        const cplx<T>* tab = reinterpret_cast<const cplx<T>*>(a.tw_hi);
        T* out = reinterpret_cast<T*>(outb);
        real_mirror_pairs<T, L, false, NB, R, TPR, LR>(lds, v, tid, valid, [&](auto, int idx, cplx<T> s, cplx<T> d) __attribute__((always_inline)) {
            r2r_fwd_emit<T, L>(out, sep, tab, a.has_tw, idx, s, d);
        });
    }
};

template <typename T, int L> struct R2rInvEpi {
    template <int NB, int R, int TPR, int LR, typename LdsT>
    static __device__ __forceinline__ void run(LdsT* lds, cplx<T>* v, const TileArgs& a, int tid, char* outb, bool valid) {
        T* out = reinterpret_cast<T*>(outb);
        const T so = a.has_tw ? (T)-1 : (T)1;
        __syncthreads();
        static_for<NB>([&](auto bb) {
            static_for<R>([&](auto kk) {
                constexpr int b = bb, k = kk;
                const cplx<T> p = v[b * R + k];
                lds[row2_pad(b * TPR + k * LR + tid)] = cplx<T>{p.x, -p.y};   // the inverse ran as a conjugated forward transform
            });
        });
        __syncthreads();
        if (!valid) return;
        static_for<L / (2 * TPR)>([&](auto tt) {
            constexpr int t = tt;
            const int j = t * TPR + tid;
            const cplx<T> e = lds[row2_pad(j)], m = lds[row2_pad(L - 1 - j)];
            r2r_store4<T>(out + 4 * j, e.x, so * m.y, e.y, so * m.x);
        });
    }
};

template <typename T, int L, int W, int NT, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) r2r_row_fwd_kernel(const TileArgs a) {
    using G = Row2Geom<L, W, NT>;
    constexpr int TPR = G::TPR, PPT = G::PPT, LP = G::LP;
    constexpr int R0 = FirstRadix<RL>::value;
    constexpr int LR0 = L / R0;
    static_assert(PPT % 2 == 0, "the load prologue / store epilogue moves four reals per step");
    __shared__ __attribute__((aligned(16))) cplx<T> lds[W * LP];
    const Row2Lane g = G::lane(a.total);
    const int u = g.u;
    const bool valid = g.valid;
    const T* x = reinterpret_cast<const T*>(a.in0) + g.row * (2 * L);
    cplx<T>* slab = lds + g.c * LP;
    const T so = a.has_tw ? (T)-1 : (T)1;
    static_for<PPT / 2>([&](auto tt) {
        constexpr int t = tt;
        const int j = t * TPR + u;
        R2rVec4<T> q = {{(T)0, (T)0, (T)0, (T)0}};
        if (valid) q = r2r_load4<T>(x + 4 * j);
        slab[row2_pad(j)] = cplx<T>{q.v[0], q.v[2]};
        slab[row2_pad(L - 1 - j)] = cplx<T>{so * q.v[3], so * q.v[1]};
    });
    __syncthreads();
    cplx<T> v[PPT];
    static_for<PPT>([&](auto ii) {
        constexpr int i = ii, b = i / R0, k = i % R0;
        v[i] = slab[row2_pad(b * TPR + k * LR0 + u)];
    });
    __syncthreads();       // the first stage's exchange writes the slab
    char* outb = reinterpret_cast<char*>(reinterpret_cast<T*>(a.out0) + g.row * (2 * L));
    Row2Stages<T, L, TPR, 1, true, false, RL, 0, R2rFwdEpi<T, L>>::template run<true>(slab, v, a, u, nullptr, outb, 0, valid);
}

template <typename T, int L, int W, int NT, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) r2r_row_inv_kernel(const TileArgs a) {
    using G = Row2Geom<L, W, NT>;
    constexpr int TPR = G::TPR, PPT = G::PPT, LP = G::LP;
    constexpr int R0 = FirstRadix<RL>::value;
    constexpr int LR0 = L / R0;
    static_assert(PPT % 2 == 0, "the load prologue / store epilogue moves four reals per step");
    __shared__ __attribute__((aligned(16))) cplx<T> lds[W * LP];
    const Row2Lane g = G::lane(a.total);
    const int u = g.u;
    const T* y = reinterpret_cast<const T*>(a.in0) + g.row * (2 * L);
    const cplx<T>* sep = reinterpret_cast<const cplx<T>*>(a.tw_lo);
    const cplx<T>* tab = reinterpret_cast<const cplx<T>*>(a.tw_hi);
    cplx<T> v[PPT];
    static_for<PPT>([&](auto i) { v[i] = cplx<T>{(T)0, (T)0}; });
    if (g.valid) {
        static_for<PPT>([&](auto ii) {
            constexpr int i = ii, b = i / R0, k = i % R0;
            v[i] = r2r_inv_pack<T, L>(y, sep, tab, a.has_tw, b * TPR + k * LR0 + u);
        });
    }
    char* outb = reinterpret_cast<char*>(reinterpret_cast<T*>(a.out0) + g.row * (2 * L));
    Row2Stages<T, L, TPR, 1, true, false, RL, 0, R2rInvEpi<T, L>>::template run<true>(lds + g.c * LP, v, a, u, nullptr, outb, 0, g.valid);
}

// ---- L <= 32: one thread per row -------------------------------------------------------------------------------------------------
// the x sample held at real position p (2j = Re, 2j + 1 = Im of z[j]) of the packed permuted row; an odd sample carries the DST's sign
constexpr int r2r_perm(int L, int p) { return p < L ? 2 * p : 2 * (2 * L - 1 - p) + 1; }

template <typename T, int L, bool INV>
__global__ void __launch_bounds__(256) r2r_row_small_kernel(const TileArgs a) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= a.total) return;
    const cplx<T>* sep = reinterpret_cast<const cplx<T>*>(a.tw_lo);
    const cplx<T>* tab = reinterpret_cast<const cplx<T>*>(a.tw_hi);
    const T so = a.has_tw ? (T)-1 : (T)1;
    const T* in = reinterpret_cast<const T*>(a.in0) + row * (2 * L);
    T* out = reinterpret_cast<T*>(a.out0) + row * (2 * L);
    cplx<T> v[L];
    if constexpr (!INV) {
        T xr[2 * L];
        static_for<2 * L>([&](auto i) { xr[i] = in[i]; });
        static_for<L>([&](auto jj) {
            constexpr int j = jj, s0 = r2r_perm(L, 2 * j), s1 = r2r_perm(L, 2 * j + 1);
            v[j] = cplx<T>{(s0 & 1) ? so * xr[s0] : xr[s0], (s1 & 1) ? so * xr[s1] : xr[s1]};
        });
        Dft<L, T>::run(v);
        static_for<L>([&](auto kk) {
            constexpr int k = kk;
            cplx<T> s, d;
            real_sd<T>(v[k], v[(L - k) & (L - 1)], s, d);
            r2r_fwd_emit<T, L>(out, sep, tab, a.has_tw, k, s, d);
        });
    } else {
        T yr[2 * L];
        static_for<2 * L>([&](auto i) { yr[i] = in[i]; });
        static_for<L>([&](auto k) {
            const cplx<T> z = r2r_inv_pack<T, L>(yr, sep, tab, a.has_tw, k);
            v[k] = cplx<T>{z.x, -z.y};                                    // conjugated: the inverse as a forward DFT
        });
        Dft<L, T>::run(v);
        static_for<L>([&](auto jj) {
            constexpr int j = jj, s0 = r2r_perm(L, 2 * j), s1 = r2r_perm(L, 2 * j + 1);
            out[s0] = (s0 & 1) ? so * v[j].x : v[j].x;
            out[s1] = (s1 & 1) ? -so * v[j].y : -v[j].y;
        });
    }
}

// (the kernels exchange full complex numbers: a length whose Row2Shape is HALF has no r2r row)
template <typename T, int L>
static inline int launch_r2r_row(const TileArgs* a, int inverse, hipStream_t s, int query_only) {
    using S = Row2Shape<T, L>;
    static_assert(!S::HALF, "r2r rows have no half-width exchange");
    return launch_row_pair(r2r_row_fwd_kernel<T, L, S::W, S::NT, S::OCC, typename S::RL>,
                           r2r_row_inv_kernel<T, L, S::W, S::NT, S::OCC, typename S::RL>, S::W, S::NT, a, inverse, s, query_only);
}

template <typename T, int L>
static inline int launch_r2r_row_small(const TileArgs* a, int inverse, hipStream_t s, int query_only) {
    return launch_row_pair(r2r_row_small_kernel<T, L, false>, r2r_row_small_kernel<T, L, true>, 256, 256, a, inverse, s, query_only);
}

}  // namespace mifft
