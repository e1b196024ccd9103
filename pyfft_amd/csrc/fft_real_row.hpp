// One-launch real-input rows (Plan(n, real=True) for 4 <= n <= 65536 fp32 / 32768 fp64): the row transform of the L = n / 2 packed
// points z[m] = x[2m] + i x[2m + 1] and the separation into the half spectrum (csrc/fft_real.hip derives the identities,
// fft_real_ident.hpp holds them) in ONE work-group, so that a row crosses HBM once: n s bytes in, (L + 1) 2s bytes out (s the scalar size).
//   forward  the stages of fft_row2.hpp (Row2Shape of fft_row_shapes.hpp: the complex row's work-group shape, LDS and occupancy); instead of the
//            last stage's stores, RealSepEpi exchanges the transform through the row's LDS slab once more (real_mirror_pairs: each point
//            needs its mirror Z[L - k], held by another thread) and stores X[k], k < L, plus X[L] from the thread that holds Z[0]
//   inverse  every thread loads the half-spectrum points its first stage needs and their mirrors X[L - k] (the same row read
//            backwards: a wave's mirrored loads are one descending contiguous run), packs them in registers (X[0], X[L] through their
//            real parts -- the Hermitian rule on a 1-D row), and the fft_row2.hpp stages run the inverse L-point transform
// Rows of L <= 32 packed points: one thread per row, the whole transform in registers (Dft<L>).
// Tables: a.tw_L = w(L)^k (L entries, the stages), a.tw_lo = w(n)^k (L + 1 entries, the separation).
#pragma once
#include <type_traits>
#include "fft_row2.hpp"
#include "fft_real_ident.hpp"

namespace mifft {

// The mirror exchange of an epilogue (EPI of Row2Stages: v[b*R + k] = point idx = b*TPR + k*LR + tid of the transform Z): the transform
// goes through the row's LDS slab once more, so that the thread that holds Z[idx] also gets Z[L - idx], and every register i is handed
// on as f(IC<i>, idx, s, d), s = Z[idx] + conj Z[L - idx], d = Z[idx] - conj Z[L - idx].  `live`: IC<1>{} (every row; a compile-time
// constant, so that no branch is ever emitted) or a bool, under which s and d are formed and f is called (a row outside the launch).
// HALF: the slab holds L scalars: real parts, then imaginary parts.  After the first round v[i].x holds s.x and dx[i] d.x.
template <typename T, int L, bool HALF, int NB, int R, int TPR, int LR, typename LdsT, typename Live, typename F>
__device__ __forceinline__ void real_mirror_pairs(LdsT* lds, cplx<T>* v, int tid, Live live, F&& f) {
    auto each = [&](auto&& g) __attribute__((always_inline)) {       // g(IC<i>, idx) for every register of the thread
        static_for<NB>([&](auto bb) {
            static_for<R>([&](auto kk) {
                constexpr int b = bb, k = kk;
                g(IC<b * R + k>{}, b * TPR + k * LR + tid);
            });
        });
    };
    auto mirror = [&](int idx) __attribute__((always_inline)) { return lds[row2_pad((L - idx) & (L - 1))]; };
    __syncthreads();       // every thread has fetched its last-stage operands: the slab is free
    if constexpr (!HALF) {
        each([&](auto i, int idx) { lds[row2_pad(idx)] = v[i]; });
        __syncthreads();
        each([&](auto i, int idx) {
            const cplx<T> q = mirror(idx);
            if (live) {
                cplx<T> s, d;
                real_sd<T>(v[i], q, s, d);
                f(i, idx, s, d);
            }
        });
    } else {
        T dx[NB * R];
        each([&](auto i, int idx) { lds[row2_pad(idx)] = v[i].x; });
        __syncthreads();
        each([&](auto i, int idx) {
            const T qx = mirror(idx);
            dx[i] = v[i].x - qx;
            v[i].x += qx;
        });
        __syncthreads();
        each([&](auto i, int idx) { lds[row2_pad(idx)] = v[i].y; });
        __syncthreads();
        each([&](auto i, int idx) {
            const T qy = mirror(idx);
            const T py = v[i].y;
            if (live) f(i, idx, cplx<T>{v[i].x, py - qy}, cplx<T>{dx[i], py + qy});
        });
    }
}

template <typename T, int L, bool HALF> struct RealSepEpi {
    template <int NB, int R, int TPR, int LR, typename LdsT>
    static __device__ __forceinline__ void run(LdsT* lds, cplx<T>* v, const TileArgs& a, int tid, char* outb, bool valid) {
        const cplx<T>* tw = reinterpret_cast<const cplx<T>*>(a.tw_lo);
        cplx<T>* out = reinterpret_cast<cplx<T>*>(outb);
        const T h = (T)(0.5 * a.scale);
        real_mirror_pairs<T, L, HALF, NB, R, TPR, LR>(lds, v, tid, IC<1>{}, [&](auto, int idx, cplx<T> s, cplx<T> d) __attribute__((always_inline)) {
            if (!valid) return;       // (s and d formed all the same, as the stages before them: `valid` as the predicate changes the code)
            out[idx] = real_sep<T>(s, tw[idx], d, h);
            if (idx == 0) out[L] = real_sep_edge<T>(s, d, h);
        });
    }
};

// ---- forward: W rows of L packed points per work-group (the complex row's shape) -------------------------------------------------
template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) real_row_fwd_kernel(const TileArgs a) {
    using G = Row2Geom<L, W, NT>;
    constexpr int TPR = G::TPR, PPT = G::PPT, LP = G::LP;
    using LdsT = typename std::conditional<HALF, T, cplx<T>>::type;
    __shared__ __attribute__((aligned(16))) LdsT lds[W * LP];
    const Row2Lane g = G::lane(a.total);
    const char* inb = reinterpret_cast<const char*>(reinterpret_cast<const cplx<T>*>(a.in0) + g.row * L);
    char* outb = reinterpret_cast<char*>(reinterpret_cast<cplx<T>*>(a.out0) + g.row * (L + 1));
    unsigned voff = (unsigned)g.u * (unsigned)sizeof(cplx<T>);
    row2_fold_offset<W>(voff, inb);
    cplx<T> v[PPT];
    Row2Stages<T, L, TPR, 1, true, HALF, RL, 0, RealSepEpi<T, L, HALF>>::run(lds + g.c * LP, v, a, g.u, inb, outb, voff, g.valid);
}

// ---- inverse: pack in registers, then the inverse L-point stages store the n reals ------------------------------------------------
template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) real_row_inv_kernel(const TileArgs a) {
    using G = Row2Geom<L, W, NT>;
    constexpr int TPR = G::TPR, PPT = G::PPT, LP = G::LP;
    constexpr int R0 = FirstRadix<RL>::value;
    constexpr int LR0 = L / R0;
    using LdsT = typename std::conditional<HALF, T, cplx<T>>::type;
    __shared__ __attribute__((aligned(16))) LdsT lds[W * LP];
    const Row2Lane g = G::lane(a.total);
    const int u = g.u;
    const cplx<T>* x = reinterpret_cast<const cplx<T>*>(a.in0) + g.row * (L + 1);
    const cplx<T>* tw = reinterpret_cast<const cplx<T>*>(a.tw_lo);
    char* outb = reinterpret_cast<char*>(reinterpret_cast<cplx<T>*>(a.out0) + g.row * L);
    unsigned voff = (unsigned)u * (unsigned)sizeof(cplx<T>);
    row2_fold_offset<W>(voff, outb);
    cplx<T> v[PPT];
    static_for<PPT>([&](auto i) { v[i] = cplx<T>{(T)0, (T)0}; });
    if (g.valid) {
        cplx<T> q[PPT];
        // all loads in flight before the packing arithmetic: the points of the first stage, then their mirrors
        static_for<PPT>([&](auto ii) {
            constexpr int i = ii, b = i / R0, k = i % R0;
            v[i] = x[b * TPR + k * LR0 + u];
        });
        static_for<PPT>([&](auto ii) {
            constexpr int i = ii, b = i / R0, k = i % R0;
            q[i] = x[L - (b * TPR + k * LR0 + u)];
        });
        static_for<PPT>([&](auto ii) {
            constexpr int i = ii, b = i / R0, k = i % R0;
            const int idx = b * TPR + k * LR0 + u;
            cplx<T> p = v[i], m = q[i], s, d;
            if (idx == 0) {                       // X[0] and X[L] through their real parts
                p.y = 0;
                m.y = 0;
            }
            real_sd<T>(p, m, s, d);
            v[i] = real_pack<T>(s, tw[idx], d);
        });
    }
    Row2Stages<T, L, TPR, 1, true, HALF, RL>::template run<true>(lds + g.c * LP, v, a, u, nullptr, outb, voff, g.valid);
}

// ---- L <= 32: one thread per row -------------------------------------------------------------------------------------------------
template <typename T, int L, bool INV>
__global__ void __launch_bounds__(256) real_row_small_kernel(const TileArgs a) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= a.total) return;
    const cplx<T>* tw = reinterpret_cast<const cplx<T>*>(a.tw_lo);
    cplx<T> v[L];
    if constexpr (!INV) {
        const cplx<T>* in = reinterpret_cast<const cplx<T>*>(a.in0) + row * L;
        cplx<T>* out = reinterpret_cast<cplx<T>*>(a.out0) + row * (L + 1);
        static_for<L>([&](auto k) { v[k] = in[k]; });
        Dft<L, T>::run(v);
        const T h = (T)(0.5 * a.scale);
        static_for<L + 1>([&](auto kk) {
            constexpr int k = kk;
            cplx<T> s, d;
            real_sd<T>(v[k & (L - 1)], v[(L - k) & (L - 1)], s, d);
            out[k] = real_sep<T>(s, tw[k], d, h);
        });
    } else {
        const cplx<T>* in = reinterpret_cast<const cplx<T>*>(a.in0) + row * (L + 1);
        cplx<T>* out = reinterpret_cast<cplx<T>*>(a.out0) + row * L;
        cplx<T> x[L + 1];
        static_for<L + 1>([&](auto k) { x[k] = in[k]; });
        x[0].y = 0;
        x[L].y = 0;
        static_for<L>([&](auto kk) {
            constexpr int k = kk;
            cplx<T> s, d;
            real_sd<T>(x[k], x[L - k], s, d);
            const cplx<T> z = real_pack<T>(s, tw[k], d);
            v[k] = cplx<T>{z.x, -z.y};                                            // conjugated: the inverse as a forward DFT
        });
        Dft<L, T>::run(v);
        const T sc = (T)a.scale;
        static_for<L>([&](auto k) { out[k] = cplx<T>{v[k].x * sc, -v[k].y * sc}; });
    }
}

template <typename T, int L>
static inline int launch_real_row(const TileArgs* a, int inverse, hipStream_t s, int query_only) {
    using S = Row2Shape<T, L>;
    return launch_row_pair(real_row_fwd_kernel<T, L, S::W, S::NT, S::HALF, S::OCC, typename S::RL>,
                           real_row_inv_kernel<T, L, S::W, S::NT, S::HALF, S::OCC, typename S::RL>, S::W, S::NT, a, inverse, s, query_only);
}

template <typename T, int L>
static inline int launch_real_row_small(const TileArgs* a, int inverse, hipStream_t s, int query_only) {
    return launch_row_pair(real_row_small_kernel<T, L, false>, real_row_small_kernel<T, L, true>, 256, 256, a, inverse, s, query_only);
}

}  // namespace mifft
