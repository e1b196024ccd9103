// One-launch convolution rows (Plan(n, convolve=True), docs/extensions.md "Convolution plans"): y = scale * IFFT(FFT(x) * S) per row,
// S = H or conj(H), in ONE work-group, so that a row crosses HBM once: n s bytes in, n s bytes out, plus the spectrum (from L2 / MALL
// when it is shared by every row).
//   complex  the fft_row2.hpp stages of the forward L = n point transform; instead of the last stage's stores ConvEpi multiplies every
//            point by S[idx] in the thread that holds it (register i = b*R + k is point b*TPR + k*LR + tid), then the inverse runs as a
//            forward transform of the conjugate, IFFT(Y) = conj(FFT(conj Y)) / n, through the preloaded stage entry with
//            TileArgs::inverse set: its first stage negates the imaginary parts in registers, its stores negate them again and apply
//            the scale (1/n folded in by the host), so one twiddle table serves both directions.
//            The inverse takes the REVERSED radix list: its first radix is the forward's last, so the forward's last-stage register
//            layout is the inverse's first-stage load layout for every list, and no LDS exchange joins the two transforms.
//   real     n real points as L = n / 2 packed complex points (csrc/fft_real.hip derives the identities, fft_real_ident.hpp holds them).
//            The forward packed stages run; one mirror exchange through the row's LDS slab (real_mirror_pairs, as RealSepEpi) gives the
//            thread that holds Z[k] also Z[L - k]; from that pair it derives X[k] and X[L - k], multiplies them by S[k] and S[L - k] and packs Z'[k] from the two products -- exactly
//            the pair the packing identity needs, so no second exchange.  Index 0 takes X[0] and X[L] through their real parts (the
//            edge rule of real_row_inv_kernel, numpy's irfft).  The inverse L-point stages store the n reals.
// Rows of L <= 32 (complex or packed points): one thread per row, both transforms in registers (Dft<L>), as real_row_small_kernel.
// Work-group shapes and forward radix lists: Row2Shape (fft_row_shapes.hpp), as for the real rows of L packed points.
#pragma once
#include <type_traits>
#include "fft_real_row.hpp"

namespace mifft {

struct ConvRowArgs {
    const void* in;          // rows of L complex numbers (complex) or n = 2L reals (real), dense
    void* out;               // the same layout; may equal `in`
    const void* spec;        // interleaved complex: L (complex) or L + 1 (real) points per spectrum
    const void* tw;          // w(L)^k, L entries (the stages)
    const void* tw_sep;      // real: w(n)^k, L + 1 entries (separation / packing); complex: unused
    long long rows;
    long long spec_pitch;    // complex numbers between the spectra of consecutive rows; 0 = one spectrum shared by every row
    int correlate;           // 1: S = conj(H)
    double scale;            // final factor of the inverse stores (the user's scale, times 1/n when normalising)
};

template <typename RL, typename Acc = RadixList<>> struct ReverseRadices;
template <int... A> struct ReverseRadices<RadixList<>, RadixList<A...>> { using type = RadixList<A...>; };
template <int R, int... Rs, int... A> struct ReverseRadices<RadixList<R, Rs...>, RadixList<A...>> {
    using type = typename ReverseRadices<RadixList<Rs...>, RadixList<R, A...>>::type;
};

// The epilogues read, from the row's TileArgs copy, fields no row stage reads: in1 = the row's spectrum, tw_lo = the separation table,
// has_tw = correlate.
template <typename T> __device__ __forceinline__ cplx<T> conv_spec(const TileArgs& a, int idx, bool valid) {
    if (!valid) return cplx<T>{(T)0, (T)0};
    cplx<T> h = reinterpret_cast<const cplx<T>*>(a.in1)[idx];
    if (a.has_tw) h.y = -h.y;
    return h;
}

// Between two butterflies' worth of spectrum products (real rows: between two points): keeps the scheduler from hoisting every spectrum
// load of the row above the first product, which would hold PPT more complex numbers live (three times that on the real rows, with the
// separation twiddles)
__device__ __forceinline__ void conv_group_fence() { __builtin_amdgcn_sched_barrier(0); }

// The inverse transform of the registers (already in its first-stage layout) with the final stores.  voff: the thread's byte offset
// within the row (0 where the kernel folded it into outb).  STORE: the EPI of the inverse's last stage (fft_fir_row.hpp: the masked
// stores of an overlap-save block); void: the plain stores.
template <typename T, int L, int W, bool HALF, typename RL, int TPR, typename STORE = void, typename LdsT>
__device__ __forceinline__ void conv_inverse(LdsT* lds, cplx<T>* v, const TileArgs& a, int tid, char* outb, bool valid) {
    using Inv = typename ReverseRadices<RL>::type;
    TileArgs c = a;
    c.inverse = 1;
    const unsigned voff = W > 1 ? 0u : (unsigned)tid * (unsigned)sizeof(cplx<T>);
    __syncthreads();       // every thread is done with the slab (the forward's last operands, the mirrors): the inverse may spill
    Row2Stages<T, L, TPR, 1, true, HALF, Inv, 0, STORE>::template run<true>(lds, v, c, tid, nullptr, outb, voff, valid);
}

template <typename T, int L, int W, bool HALF, typename RL, typename STORE = void> struct ConvEpi {
    template <int NB, int R, int TPR, int LR, typename LdsT>
    static __device__ __forceinline__ void run(LdsT* lds, cplx<T>* v, const TileArgs& a, int tid, char* outb, bool valid) {
        static_assert(FirstRadix<typename ReverseRadices<RL>::type>::value == R, "the inverse starts with the forward's last radix");
        static_for<NB>([&](auto bb) {
            static_for<R>([&](auto kk) {
                constexpr int b = bb, k = kk;
                v[b * R + k] = cmul<T>(v[b * R + k], conv_spec<T>(a, b * TPR + k * LR + tid, valid));
            });
            conv_group_fence();
        });
        conv_inverse<T, L, W, HALF, RL, TPR, STORE>(lds, v, a, tid, outb, valid);
    }
};

// Z'[k] from the s, d of the packed forward transform Z at idx = k: the separated pair X[k], X[L - k];  Y = X * S;  at k = 0 the pair is
// X[0], X[L], real parts only;  Z'[k] packed from the s, d of the pair Y[k], Y[L - k].  The unnormalised inverse transform of Z' is n
// times the inverse real transform of Y, packed.
template <typename T, int L>
__device__ __forceinline__ cplx<T> conv_real_pair(cplx<T> s, cplx<T> d, int idx, const TileArgs& a, bool valid) {
    const cplx<T> w = reinterpret_cast<const cplx<T>*>(a.tw_lo)[idx];
    const T h = (T)0.5;
    cplx<T> y1 = cmul<T>(real_sep<T>(s, w, d, h), conv_spec<T>(a, idx, valid));
    cplx<T> y2 = cmul<T>(real_sep_mirror<T>(s, w, d, h), conv_spec<T>(a, L - idx, valid));
    if (idx == 0) {
        y1.y = 0;
        y2.y = 0;
    }
    cplx<T> sm, df;
    real_sd<T>(y1, y2, sm, df);
    return real_pack<T>(sm, w, df);
}

template <typename T, int L, int W, bool HALF, typename RL, typename STORE = void> struct ConvRealEpi {
    template <int NB, int R, int TPR, int LR, typename LdsT>
    static __device__ __forceinline__ void run(LdsT* lds, cplx<T>* v, const TileArgs& a, int tid, char* outb, bool valid) {
        static_assert(FirstRadix<typename ReverseRadices<RL>::type>::value == R, "the inverse starts with the forward's last radix");
        // every row is live: one outside the launch carries zeros (conv_spec) into the inverse stages
        real_mirror_pairs<T, L, HALF, NB, R, TPR, LR>(lds, v, tid, IC<1>{}, [&](auto i, int idx, cplx<T> s, cplx<T> d) __attribute__((always_inline)) {
            v[i] = conv_real_pair<T, L>(s, d, idx, a, valid);
            conv_group_fence();
        });
        conv_inverse<T, L, W, HALF, RL, TPR, STORE>(lds, v, a, tid, outb, valid);
    }
};

// The row's TileArgs: what the stages read (tw_L, inverse, nt, scale) and what the epilogues read (in1, tw_lo, has_tw)
__device__ __forceinline__ TileArgs conv_tile_args(const ConvRowArgs& a, const void* spec_row) {
    TileArgs t = {};
    t.in0 = a.in;
    t.in1 = spec_row;
    t.out0 = a.out;
    t.tw_L = a.tw;
    t.tw_lo = a.tw_sep;
    t.total = a.rows;
    t.has_tw = a.correlate;
    t.scale = a.scale;
    return t;
}

// W rows of L complex (REAL: packed) points per work-group, NT threads; NT == W: one thread per row (L <= 32), both transforms in registers
template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL, bool REAL>
__device__ __forceinline__ void conv_row_body(const ConvRowArgs& a) {
    constexpr int TPR = NT / W;
    if constexpr (TPR == 1) {
        const long long row = (long long)blockIdx.x * NT + threadIdx.x;
        if (row >= a.rows) return;
        const cplx<T>* in = reinterpret_cast<const cplx<T>*>(a.in) + row * L;
        cplx<T>* out = reinterpret_cast<cplx<T>*>(a.out) + row * L;
        const TileArgs t = conv_tile_args(a, reinterpret_cast<const cplx<T>*>(a.spec) + row * a.spec_pitch);
        cplx<T> v[L];
        static_for<L>([&](auto k) { v[k] = in[k]; });
        Dft<L, T>::run(v);
        if constexpr (!REAL) {
            static_for<L>([&](auto k) {
                const cplx<T> y = cmul<T>(v[k], conv_spec<T>(t, k, true));
                v[k] = cplx<T>{y.x, -y.y};
            });
        } else {
            cplx<T> z[L];
            static_for<L>([&](auto kk) {
                constexpr int k = kk;
                cplx<T> s, d;
                real_sd<T>(v[k], v[(L - k) & (L - 1)], s, d);
                const cplx<T> y = conv_real_pair<T, L>(s, d, k, t, true);
                z[k] = cplx<T>{y.x, -y.y};
            });
            static_for<L>([&](auto k) { v[k] = z[k]; });
        }
        Dft<L, T>::run(v);        // the conjugate's forward transform
        const T sc = (T)a.scale;
        static_for<L>([&](auto k) { out[k] = cplx<T>{v[k].x * sc, -v[k].y * sc}; });
    } else {
        using G = Row2Geom<L, W, NT>;
        constexpr int PPT = G::PPT, LP = G::LP;
        using LdsT = typename std::conditional<HALF, T, cplx<T>>::type;
        __shared__ __attribute__((aligned(16))) LdsT lds[W * LP];
        // (the row preamble written out, not Row2Geom::lane: through the function the W > 1 kernels schedule differently)
        const int c = W == 1 ? 0 : threadIdx.x / TPR, u = W == 1 ? threadIdx.x : threadIdx.x % TPR;
        const long long row = (long long)blockIdx.x * W + c;
        const bool valid = row < a.rows;
        const TileArgs t = conv_tile_args(a, reinterpret_cast<const cplx<T>*>(a.spec) + (valid ? row * a.spec_pitch : 0));
        const char* inb = reinterpret_cast<const char*>(reinterpret_cast<const cplx<T>*>(a.in) + row * L);
        char* outb = reinterpret_cast<char*>(reinterpret_cast<cplx<T>*>(a.out) + row * L);
        unsigned voff = (unsigned)u * (unsigned)sizeof(cplx<T>);
        row2_fold_offset<W>(voff, inb, outb);
        using Epi = typename std::conditional<REAL, ConvRealEpi<T, L, W, HALF, RL>, ConvEpi<T, L, W, HALF, RL>>::type;
        cplx<T> v[PPT];
        Row2Stages<T, L, TPR, 1, true, HALF, RL, 0, Epi>::run(lds + c * LP, v, t, u, inb, outb, voff, valid);
    }
}

template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) conv_row_kernel(const ConvRowArgs a) {
    conv_row_body<T, L, W, NT, HALF, OCC, RL, false>(a);
}

template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) conv_row_real_kernel(const ConvRowArgs a) {
    conv_row_body<T, L, W, NT, HALF, OCC, RL, true>(a);
}

// real != 0: L packed points (n = 2L reals); 0 launched (query: a kernel exists), -2 none, -1 grid too large
// REAL_ROWS false: this length has complex rows only, and no real kernel is built for it
template <typename T, int L, bool REAL_ROWS = true, typename S = Row2Shape<T, L>>
static inline int launch_conv_row(int real, const ConvRowArgs* a, hipStream_t s, int query_only) {
    if (real && !REAL_ROWS) return -2;
    return launch_groups(a, &ConvRowArgs::rows, S::W, query_only, [&](dim3 grid) {
        auto kernel = conv_row_kernel<T, L, S::W, S::NT, S::HALF, S::OCC, typename S::RL>;
        if constexpr (REAL_ROWS) {
            if (real) kernel = conv_row_real_kernel<T, L, S::W, S::NT, S::HALF, S::OCC, typename S::RL>;
        }
        hipLaunchKernelGGL(kernel, grid, dim3(S::NT), 0, s, *a);
    });
}

// L <= 32: one thread per row
template <typename T, int L>
static inline int launch_conv_row_small(int real, const ConvRowArgs* a, hipStream_t s, int query_only) {
    return launch_conv_row<T, L, true, Row2ShapeOf<256, 256, RadixList<L>>>(real, a, s, query_only);
}

}  // namespace mifft
