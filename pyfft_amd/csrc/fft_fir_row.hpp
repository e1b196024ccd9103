// One-launch overlap-save FIR rows (Plan(n, convolve=True, taps=m), docs/extensions.md "FIR filtering plans"): every block of n
// points of a long signal runs transform -> product with the filter's spectrum -> inverse in ONE work-group, exactly as a convolution
// row (fft_conv_row.hpp: the same stages, the same ConvEpi / ConvRealEpi product, the same work-group shapes), but the block is a WINDOW
// of the signal and only its valid part is stored, so the signal crosses HBM once in and once out whatever its length.
//
// Index algebra, in points (complex numbers; real plans: packed pairs of reals), L per block, ov = overlap, hop = L - ov:
//   row = item * blocks + r;  block r of an item starts at point  start = r * hop - ov  of the item (negative for r = 0)
//   load   local point p is the item's point start + p, taken if 0 <= start + p and it lies inside the item's `length`, else 0
//          -> the window [plo, phi) of local points, plo = max(0, -start) (ov for r = 0: hop > ov), phi = min(L, whole points of the
//          item from `start` on)
//   store  local point p >= ov of the block's circular convolution is the item's output point start + p, stored if inside `length`
//          -> the window [ov, phi): the same upper end
//   real plans: `length` counts reals and may be odd: the pair that straddles the item's end (local point phi, `half` set) loads and
//          stores its first real only.
// A lane outside the window issues no access at all (the branch masks it); a row outside the launch has an empty window (phi = 0).
// The loads put the block into the first-stage register layout of Row2Stages (load_regs: v[b*R + k] = point b*TPR + k*LR + tid), the
// forward runs through the PRELOADED entry, and the inverse's last stage stores through FirStoreEpi (its EPI).
#pragma once
#include <type_traits>
#include "fft_conv_row.hpp"

namespace mifft {

struct FirRowArgs {
    const void* in;          // items of `length` complex numbers (complex) or reals (real), `pitch` points apart
    void* out;               // the same layout; never the input
    const void* spec;        // interleaved complex: L (complex) or L + 1 (real) points per spectrum
    const void* tw;          // w(L)^k, L entries (the stages)
    const void* tw_sep;      // real: w(n)^k, L + 1 entries (separation / packing); complex: unused
    long long rows;          // items * blocks
    long long blocks;        // blocks per item
    long long pitch;         // points between two items (real: pairs)
    long long length;        // complex numbers (complex) or reals (real) per item
    long long spec_pitch;    // complex numbers between the spectra of consecutive ITEMS; 0 = one spectrum shared by every item
    int ov;                  // points of a block that repeat the previous block's end (real: pairs)
    double scale;            // final factor of the inverse stores (the user's scale, times 1/n when normalising)
};

// The store window travels to the inverse's last stage in fields of the row's TileArgs copy that no row stage reads: logMS = ov,
// logS = phi - ov (0 for a row outside the launch), tw_shift = half.
// A window test is one add and one unsigned compare on a per-thread base (tid - ov here, tid - plo for the loads): written with the
// point index p itself, the compiler keeps the PPT values of p alive from the loads to the stores (+16 VGPRs at PPT = 16).
template <typename T, int W, bool REAL> struct FirStoreEpi {
    template <int NB, int R, int TPR, int LR, typename LdsT>
    static __device__ __forceinline__ void run(LdsT*, cplx<T>* v, const TileArgs& a, int tid, char* outb, bool) {
        // (no `valid`: a row outside the launch has an empty window and half = 0)
        const T sx = (T)a.scale;
        const T sy = a.inverse ? -sx : sx;     // the conjugation and the scale of the plain stores
        const unsigned rel = (unsigned)(tid - a.logMS), width = (unsigned)a.logS;
        const unsigned voff = W > 1 ? 0u : (unsigned)tid * (unsigned)sizeof(cplx<T>);
        static_for<NB>([&](auto bb) {
            static_for<R>([&](auto kk) {
                constexpr int b = bb, k = kk;
                const unsigned q = rel + (unsigned)(b * TPR + k * LR);       // p - ov, p = b * TPR + k * LR + tid
                cplx<T> y = v[b * R + k];
                y.x *= sx;
                y.y *= sy;
                char* at = outb + (size_t)(b * TPR + k * LR) * sizeof(cplx<T>) + voff;
                if (q < width) *reinterpret_cast<cplx<T>*>(at) = y;
                else if (REAL && a.tw_shift && q == width) *reinterpret_cast<T*>(at) = y.x;
            });
        });
    }
};

// W blocks of L complex (REAL: packed) points per work-group, NT threads: the geometry of conv_row_body
template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL, bool REAL>
__device__ __forceinline__ void fir_row_body(const FirRowArgs& a) {
    using G = Row2Geom<L, W, NT>;
    constexpr int TPR = G::TPR, PPT = G::PPT, LP = G::LP;
    constexpr int R0 = FirstRadix<RL>::value, LR0 = L / R0;
    constexpr int SC = REAL ? 2 : 1;       // scalars of `length` per point
    using LdsT = typename std::conditional<HALF, T, cplx<T>>::type;
    __shared__ __attribute__((aligned(16))) LdsT lds[W * LP];
    const int c = W == 1 ? 0 : threadIdx.x / TPR, u = W == 1 ? threadIdx.x : threadIdx.x % TPR;
    const long long row = (long long)blockIdx.x * W + c;
    const bool valid = row < a.rows;
    // the flat row index: a work-group of W > 1 blocks may hold blocks of two items
    const long long item = valid ? row / a.blocks : 0;
    const long long r = valid ? row - item * a.blocks : 0;
    const long long start = r * (L - a.ov) - a.ov;              // the block's first point within its item
    const long long rest = a.length - SC * start;               // scalars of the item from there on (>= SC * ov + 1: r < blocks)
    const int lim = valid ? (int)(rest < (long long)SC * L ? rest : (long long)SC * L) : 0;
    const int plo = r == 0 ? a.ov : 0, phi = lim / SC;          // (valid: phi >= ov >= plo)
    const bool half = REAL && (lim & 1);
    const unsigned rel = (unsigned)(u - plo), width = valid ? (unsigned)(phi - plo) : 0u;

    TileArgs t = {};
    t.in1 = reinterpret_cast<const cplx<T>*>(a.spec) + item * a.spec_pitch;
    t.tw_L = a.tw;
    t.tw_lo = a.tw_sep;
    t.total = a.rows;
    t.scale = a.scale;
    t.logMS = a.ov;
    t.logS = valid ? phi - a.ov : 0;
    t.tw_shift = half;

    const long long first = item * a.pitch + start;             // (points; every access adds at least plo >= -start to it)
    const char* inb = reinterpret_cast<const char*>(reinterpret_cast<const cplx<T>*>(a.in) + first);
    char* outb = reinterpret_cast<char*>(reinterpret_cast<cplx<T>*>(a.out) + first);
    unsigned voff = (unsigned)u * (unsigned)sizeof(cplx<T>);
    row2_fold_offset<W>(voff, inb, outb);

    // the masked first-stage loads, all in flight before the first butterfly
    cplx<T> v[PPT];
    static_for<PPT>([&](auto ii) {
        constexpr int i = ii, b = i / R0, k = i % R0;
        const unsigned q = rel + (unsigned)(b * TPR + k * LR0);      // p - plo, p = b * TPR + k * LR0 + u
        const char* at = inb + (size_t)(b * TPR + k * LR0) * sizeof(cplx<T>) + voff;
        v[i] = cplx<T>{(T)0, (T)0};
        if (q < width) v[i] = *reinterpret_cast<const cplx<T>*>(at);
        else if (half && q == width) v[i].x = *reinterpret_cast<const T*>(at);
    });
    using Store = FirStoreEpi<T, W, REAL>;
    using Epi = typename std::conditional<REAL, ConvRealEpi<T, L, W, HALF, RL, Store>, ConvEpi<T, L, W, HALF, RL, Store>>::type;
    Row2Stages<T, L, TPR, 1, true, HALF, RL, 0, Epi>::template run<true>(lds + c * LP, v, t, u, nullptr, outb, voff, valid);
}

template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) fir_row_kernel(const FirRowArgs a) {
    fir_row_body<T, L, W, NT, HALF, OCC, RL, false>(a);
}

template <typename T, int L, int W, int NT, bool HALF, int OCC, typename RL>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(OCC))) fir_row_real_kernel(const FirRowArgs a) {
    fir_row_body<T, L, W, NT, HALF, OCC, RL, true>(a);
}

// real != 0: L packed points (n = 2L reals); 0 launched (query: a kernel exists), -2 none, -1 grid too large
// REAL_ROWS false: this length has complex blocks only, and no real kernel is built for it
template <typename T, int L, bool REAL_ROWS = true, typename S = Row2Shape<T, L>>
static inline int launch_fir_row(int real, const FirRowArgs* a, hipStream_t s, int query_only) {
    if (real && !REAL_ROWS) return -2;
    return launch_groups(a, &FirRowArgs::rows, S::W, query_only, [&](dim3 grid) {
        auto kernel = fir_row_kernel<T, L, S::W, S::NT, S::HALF, S::OCC, typename S::RL>;
        if constexpr (REAL_ROWS) {
            if (real) kernel = fir_row_real_kernel<T, L, S::W, S::NT, S::HALF, S::OCC, typename S::RL>;
        }
        hipLaunchKernelGGL(kernel, grid, dim3(S::NT), 0, s, *a);
    });
}

// filter_spectrum's padding launch: out[f][j] = j < taps ? in[f * taps + j] : 0, j < n, for `filters` filters of E-typed elements (the
// precision's complex number or real).  One thread writes 16 bytes (V elements) with one vector store; the taps are read one by one
// (a filter's first tap has no alignment beyond its element).
struct FirPadArgs {
    const void* in;
    void* out;           // 16-byte aligned
    long long total;     // filters * n / V
    int n, taps;
};

template <typename E, int V> __global__ void __launch_bounds__(256) fir_pad_kernel(const FirPadArgs a) {
    typedef E VT __attribute__((ext_vector_type(V)));
    const E* in = reinterpret_cast<const E*>(a.in);
    const long long stride = (long long)gridDim.x * 256;
    const int per = a.n / V;
    for (long long id = (long long)blockIdx.x * 256 + threadIdx.x; id < a.total; id += stride) {
        const long long f = id / per;
        const int j = (int)(id - f * per) * V;
        VT q;
#pragma unroll
        for (int e = 0; e < V; ++e) q[e] = j + e < a.taps ? in[f * a.taps + j + e] : (E)0;
        reinterpret_cast<VT*>(a.out)[id] = q;
    }
}

}  // namespace mifft
