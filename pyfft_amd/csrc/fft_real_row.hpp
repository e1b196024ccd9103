// One-launch real-input rows (Plan(n, real=True) for 4 <= n <= 65536 fp32 / 32768 fp64): the row transform of the L = n / 2 packed
// points z[m] = x[2m] + i x[2m + 1] and the separation into the half spectrum (csrc/fft_real.hip states the identity) in ONE
// work-group, so that a row crosses HBM once: n s bytes in, (L + 1) 2s bytes out (s the scalar size).
//   forward  the stages of fft_row2.hpp (Row2Shape of fft_row_shapes.hpp: the complex row's work-group shape, LDS and occupancy); instead of the
//            last stage's stores, RealSepEpi exchanges the transform through the row's LDS slab once more (each point needs its mirror
//            Z[L - k], held by another thread) and stores X[k], k < L, plus X[L] from the thread that holds Z[0]
//   inverse  every thread loads the half-spectrum points its first stage needs and their mirrors X[L - k] (the same row read
//            backwards: a wave's mirrored loads are one descending contiguous run), packs them in registers (X[0], X[L] through their
//            real parts -- the Hermitian rule on a 1-D row), and the fft_row2.hpp stages run the inverse L-point transform
// Rows of L <= 32 packed points: one thread per row, the whole transform in registers (Dft<L>).
// Tables: a.tw_L = w(L)^k (L entries, the stages), a.tw_lo = w(n)^k (L + 1 entries, the separation).
#pragma once
#include <type_traits>
#include "fft_row2.hpp"

namespace mifft {

// X[k] = 1/2 (s - i w(n)^k d), s = Z[k] + conj Z[L - k], d = Z[k] - conj Z[L - k]; h = scale / 2
template <typename T> __device__ __forceinline__ cplx<T> real_sep(cplx<T> s, cplx<T> d, cplx<T> w, T h) {
    const cplx<T> t = {w.x * d.x - w.y * d.y, w.x * d.y + w.y * d.x};
    return cplx<T>{(s.x + t.y) * h, (s.y - t.x) * h};
}

template <typename T, int L, bool HALF> struct RealSepEpi {
    template <int NB, int R, int TPR, int LR, typename LdsT>
    static __device__ __forceinline__ void run(LdsT* lds, cplx<T>* v, const TileArgs& a, int tid, char* outb, bool valid) {
        const cplx<T>* tw = reinterpret_cast<const cplx<T>*>(a.tw_lo);
        cplx<T>* out = reinterpret_cast<cplx<T>*>(outb);
        const T h = (T)(0.5 * a.scale);
        auto emit = [&](int idx, cplx<T> s, cplx<T> d) __attribute__((always_inline)) {
            if (!valid) return;
            out[idx] = real_sep<T>(s, d, tw[idx], h);
            if (idx == 0) out[L] = cplx<T>{(s.x - d.y) * h, (s.y + d.x) * h};    // w(n)^L = -1
        };
        __syncthreads();       // every thread has fetched its last-stage operands: the slab is free
        if constexpr (!HALF) {
            static_for<NB>([&](auto bb) {
                static_for<R>([&](auto kk) {
                    constexpr int b = bb, k = kk;
                    lds[row2_pad(b * TPR + k * LR + tid)] = v[b * R + k];
                });
            });
            __syncthreads();
            static_for<NB>([&](auto bb) {
                static_for<R>([&](auto kk) {
                    constexpr int b = bb, k = kk;
                    const int idx = b * TPR + k * LR + tid;
                    const cplx<T> p = v[b * R + k], q = lds[row2_pad((L - idx) & (L - 1))];
                    emit(idx, cplx<T>{p.x + q.x, p.y - q.y}, cplx<T>{p.x - q.x, p.y + q.y});
                });
            });
        } else {
            // the slab holds L scalars: real parts, then imaginary parts.  After the first round v[i].x holds s.x and dx[i] d.x.
            T dx[NB * R];
            static_for<NB>([&](auto bb) {
                static_for<R>([&](auto kk) {
                    constexpr int b = bb, k = kk;
                    lds[row2_pad(b * TPR + k * LR + tid)] = v[b * R + k].x;
                });
            });
            __syncthreads();
            static_for<NB>([&](auto bb) {
                static_for<R>([&](auto kk) {
                    constexpr int b = bb, k = kk;
                    const int idx = b * TPR + k * LR + tid;
                    const T qx = lds[row2_pad((L - idx) & (L - 1))];
                    dx[b * R + k] = v[b * R + k].x - qx;
                    v[b * R + k].x += qx;
                });
            });
            __syncthreads();
            static_for<NB>([&](auto bb) {
                static_for<R>([&](auto kk) {
                    constexpr int b = bb, k = kk;
                    lds[row2_pad(b * TPR + k * LR + tid)] = v[b * R + k].y;
                });
            });
            __syncthreads();
            static_for<NB>([&](auto bb) {
                static_for<R>([&](auto kk) {
                    constexpr int b = bb, k = kk;
                    const int idx = b * TPR + k * LR + tid;
                    const T qy = lds[row2_pad((L - idx) & (L - 1))];
                    const T py = v[b * R + k].y;
                    emit(idx, cplx<T>{v[b * R + k].x, py - qy}, cplx<T>{dx[b * R + k], py + qy});
                });
            });
        }
    }
};

// ---- forward: W rows of L packed points per work-group (the complex row's shape) -------------------------------------------------
template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) real_row_fwd_kernel(const TileArgs a) {
    using G = Row2Geom<L, W, NT>;
    constexpr int TPR = G::TPR, PPT = G::PPT, LP = G::LP;
    using LdsT = typename std::conditional<HALF, T, cplx<T>>::type;
    __shared__ __attribute__((aligned(16))) LdsT lds[W * LP];
    const int c = W == 1 ? 0 : threadIdx.x / TPR, u = W == 1 ? threadIdx.x : threadIdx.x % TPR;
    const long long row = (long long)blockIdx.x * W + c;
    const bool valid = row < a.total;
    const char* inb = reinterpret_cast<const char*>(reinterpret_cast<const cplx<T>*>(a.in0) + row * L);
    char* outb = reinterpret_cast<char*>(reinterpret_cast<cplx<T>*>(a.out0) + row * (L + 1));
    unsigned voff = (unsigned)u * (unsigned)sizeof(cplx<T>);
    if constexpr (W > 1) {
        inb += voff;
        voff = 0;
    }
    cplx<T> v[PPT];
    Row2Stages<T, L, TPR, 1, true, HALF, RL, 0, RealSepEpi<T, L, HALF>>::run(lds + c * LP, v, a, u, inb, outb, voff, valid);
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
    const int c = W == 1 ? 0 : threadIdx.x / TPR, u = W == 1 ? threadIdx.x : threadIdx.x % TPR;
    const long long row = (long long)blockIdx.x * W + c;
    const bool valid = row < a.total;
    const cplx<T>* x = reinterpret_cast<const cplx<T>*>(a.in0) + row * (L + 1);
    const cplx<T>* tw = reinterpret_cast<const cplx<T>*>(a.tw_lo);
    char* outb = reinterpret_cast<char*>(reinterpret_cast<cplx<T>*>(a.out0) + row * L);
    unsigned voff = (unsigned)u * (unsigned)sizeof(cplx<T>);
    if constexpr (W > 1) {
        outb += voff;
        voff = 0;
    }
    cplx<T> v[PPT];
    static_for<PPT>([&](auto i) { v[i] = cplx<T>{(T)0, (T)0}; });
    if (valid) {
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
            cplx<T> p = v[i], m = q[i];
            if (idx == 0) {                       // X[0] and X[L] through their real parts
                p.y = 0;
                m.y = 0;
            }
            const cplx<T> s = {p.x + m.x, p.y - m.y}, d = {p.x - m.x, p.y + m.y};
            const cplx<T> w = tw[idx];
            const cplx<T> t = {w.x * d.x + w.y * d.y, w.x * d.y - w.y * d.x};    // conj(w) d
            v[i] = cplx<T>{s.x - t.y, s.y + t.x};                                 // s + i t
        });
    }
    Row2Stages<T, L, TPR, 1, true, HALF, RL>::template run<true>(lds + c * LP, v, a, u, nullptr, outb, voff, valid);
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
            const cplx<T> p = v[k & (L - 1)], q = v[(L - k) & (L - 1)];
            out[k] = real_sep<T>(cplx<T>{p.x + q.x, p.y - q.y}, cplx<T>{p.x - q.x, p.y + q.y}, tw[k], h);
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
            const cplx<T> p = x[k], m = x[L - k];
            const cplx<T> s = {p.x + m.x, p.y - m.y}, d = {p.x - m.x, p.y + m.y};
            const cplx<T> w = tw[k];
            const cplx<T> t = {w.x * d.x + w.y * d.y, w.x * d.y - w.y * d.x};
            v[k] = cplx<T>{s.x - t.y, -(s.y + t.x)};                              // conjugated: the inverse as a forward DFT
        });
        Dft<L, T>::run(v);
        const T sc = (T)a.scale;
        static_for<L>([&](auto k) { out[k] = cplx<T>{v[k].x * sc, -v[k].y * sc}; });
    }
}

template <typename T, int L>
static inline int launch_real_row(const TileArgs* a, int inverse, hipStream_t s, int query_only) {
    using S = Row2Shape<T, L>;
    return launch_groups(a, &TileArgs::total, S::W, query_only, [&](dim3 grid) {
        if (inverse) hipLaunchKernelGGL((real_row_inv_kernel<T, L, S::W, S::NT, S::HALF, S::OCC, typename S::RL>), grid, dim3(S::NT), 0, s, *a);
        else hipLaunchKernelGGL((real_row_fwd_kernel<T, L, S::W, S::NT, S::HALF, S::OCC, typename S::RL>), grid, dim3(S::NT), 0, s, *a);
    });
}

template <typename T, int L>
static inline int launch_real_row_small(const TileArgs* a, int inverse, hipStream_t s, int query_only) {
    return launch_groups(a, &TileArgs::total, 256, query_only, [&](dim3 grid) {
        if (inverse) hipLaunchKernelGGL((real_row_small_kernel<T, L, true>), grid, dim3(256), 0, s, *a);
        else hipLaunchKernelGGL((real_row_small_kernel<T, L, false>), grid, dim3(256), 0, s, *a);
    });
}

}  // namespace mifft
