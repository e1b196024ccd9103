// Cosine and sine transforms (DCT-II / DST-II forward, type III inverse): the steps around a complex transform of the packed data, by
// Makhoul's algorithm (docs/extensions.md "Real-to-real transforms", tests/dct_model.py).  Per axis of n points:
//   v = [x0, x2, x4, ..., x5, x3, x1] (DST: x[j] times (-1)^j first),   V = FFT(v),   Y[k] = t[k] V[k] + conj(t[k]) V[-k]
// with t[k] = c[k] w(4n)^k (c: the ortho weight, or 1), and the inverse V[k] = u[k] (Y[k] - i Y[n - k]), Y[n] = 0, u[k] = w(4n)^-k / 2c[k].
// DST-II is the DCT-II of the signed input read backwards on every axis.  Over several axes both formulas apply axis by axis.  The real
// v read as interleaved complex numbers is the packed z of shape (..., nx / 2), so the FFT is a complex transform of z plus the real
// separation (forward) or packing (inverse) of fft_real.hip, here fused with the twiddles into one launch.
//   permutation steps  forward pre (x -> v) and inverse post (v -> x): a pure gather / scatter, one thread per 4 (or 1) contiguous x
//   orbit steps        forward post (Z -> Y) and inverse pre (Y -> Z'): one thread per orbit {k, n - k} on every leading axis and
//                      {kx, n - kx, L - kx, L + kx} on the contiguous one; it reads the 2^(d-1) x 2 points of Z (the 2^(d-1) x 4 points
//                      of Y) the orbit needs and stores each output of the orbit once
// A wave's loads and stores on the contiguous axis are ascending or descending contiguous runs.  The global factor (scale, the
// normalisation, the dropped unit axes, the separation's 1/2) is folded into the last axis's table, so no multiply is added for it.
#include <hip/hip_runtime.h>
#include "mifft_internal.h"

namespace {

template <typename T> using cx = mifft::cplx<T>;

struct R2rPermArgs {
    const void* in;
    void* out;
    double scale;
    long long total;       // threads
    int log_cw;            // log2(threads per row)
    int log_rows;          // log2(rows per item) = log2(n0 n1)
    int n0, n1;            // leading axes (1 when absent)
    int log_n1;
    int nl;                // contiguous axis
    int dst;
};

struct R2rOrbitArgs {
    const void* in;
    void* out;
    const void* tab[3];    // per-axis tables (t or u), the last axis's with the global factor
    const void* sep;       // w(nl)^k, k = 0 .. L / 2
    long long rows;        // items x leading orbits
    unsigned lead_count;   // prod (n_a / 2 + 1) over the leading axes
    int n0, n1;            // leading axes (1 when absent)
    int c1;                // n1 / 2 + 1
    int nl, L;
    int cx;                // threads per row: L / 2 (the kx = 0 thread also runs the orbit of L / 2) when L / 2 fills a wave, else L / 2 + 1
    int fold;
    int lanes, log_lanes;
    unsigned rows_per_block, blocks_per_row_group;
    int dst;
};

__device__ __forceinline__ int perm_of(int i, int n) { return (i & 1) ? n - 1 - (i >> 1) : (i >> 1); }

template <typename T> struct Vec4 { T v[4]; };
template <typename T> __device__ __forceinline__ Vec4<T> load4(const T* p);
template <> __device__ __forceinline__ Vec4<float> load4(const float* p) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    return {{q.x, q.y, q.z, q.w}};
}
template <> __device__ __forceinline__ Vec4<double> load4(const double* p) {
    const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
    return {{a.x, a.y, b.x, b.y}};
}
template <typename T> __device__ __forceinline__ void store4(T* p, const Vec4<T>& q);
template <> __device__ __forceinline__ void store4(float* p, const Vec4<float>& q) {
    *reinterpret_cast<float4*>(p) = float4{q.v[0], q.v[1], q.v[2], q.v[3]};
}
template <> __device__ __forceinline__ void store4(double* p, const Vec4<double>& q) {
    reinterpret_cast<double2*>(p)[0] = double2{q.v[0], q.v[1]};
    reinterpret_cast<double2*>(p)[1] = double2{q.v[2], q.v[3]};
}

// INV = false: out = v (the permuted, signed x);  INV = true: out = x from v.  G = 4: one thread per x[4j .. 4j + 3] (a 16-byte aligned
// x and nl % 4 == 0), whose places in v are v[2j], v[2j + 1] and v[nl - 2 - 2j], v[nl - 1 - 2j]: two 2-element runs.  G = 1: one point.
template <typename T, bool INV, int G>
__global__ void __launch_bounds__(256) r2r_perm_kernel(const R2rPermArgs a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.total) return;
    const long long row = t >> a.log_cw;
    const int j = (int)(t & ((1ll << a.log_cw) - 1));
    const long long item = row >> a.log_rows;
    const int r = (int)(row & ((1ll << a.log_rows) - 1));
    const int i1 = r & (a.n1 - 1), i0 = r >> a.log_n1;
    const long long base = item << a.log_rows;
    const long long xrow = (base + r) * a.nl;
    const long long vrow = (base + (long long)perm_of(i0, a.n0) * a.n1 + perm_of(i1, a.n1)) * a.nl;
    const T s = (a.dst && ((i0 + i1) & 1)) ? -(T)a.scale : (T)a.scale;     // the sign of the row's even points
    const T so = a.dst ? -s : s;                                           // of its odd points
    const T* src = reinterpret_cast<const T*>(a.in);
    T* dst = reinterpret_cast<T*>(a.out);
    if constexpr (G == 4) {
        const int lo = 2 * j, hi = a.nl - 2 - 2 * j;
        if constexpr (!INV) {
            const Vec4<T> x = load4(src + xrow + 4 * j);
            dst[vrow + lo] = s * x.v[0];
            dst[vrow + lo + 1] = s * x.v[2];
            dst[vrow + hi] = so * x.v[3];
            dst[vrow + hi + 1] = so * x.v[1];
        } else {
            const T e0 = src[vrow + lo], e2 = src[vrow + lo + 1], e3 = src[vrow + hi], e1 = src[vrow + hi + 1];
            store4(dst + xrow + 4 * j, Vec4<T>{{s * e0, so * e1, s * e2, so * e3}});
        }
    } else {
        const T f = (j & 1) ? so : s;
        const int p = perm_of(j, a.nl);
        if constexpr (!INV) dst[vrow + p] = f * src[xrow + j];
        else dst[xrow + j] = f * src[vrow + p];
    }
}

template <typename T> __device__ __forceinline__ cx<T> cmul(cx<T> a, cx<T> b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <typename T> __device__ __forceinline__ cx<T> conj_(cx<T> a) { return {a.x, -a.y}; }

// One orbit of the forward post step (INV = false: Z -> Y) or the inverse pre step (INV = true: Y -> Z').  D leading axes; k[] the
// orbit's leading indices (0 <= k <= n / 2), kx its contiguous one (0 <= kx <= L / 2).  Slot bit `ax` of s picks k or -k on leading axis
// ax; q picks kx, -kx, L - kx, L + kx (mod nl) on the contiguous axis.
template <typename T, int D, bool INV>
__device__ __forceinline__ void r2r_orbit(const R2rOrbitArgs& a, long long item, const int* k, int kx) {
    constexpr int S = 1 << D;
    const int nl = a.nl, L = a.L;
    const int nlead[2] = {a.n0, a.n1};
    int idx[2][2];
    bool wr[2];                                 // slot 1 of the axis holds an output of its own
    for (int ax = 0; ax < D; ++ax) {
        idx[ax][0] = k[ax];
        idx[ax][1] = (nlead[ax] - k[ax]) & (nlead[ax] - 1);
        wr[ax] = k[ax] != 0 && 2 * k[ax] != nlead[ax];
    }
    long long roff[S];                          // leading row of each slot combination
    for (int s = 0; s < S; ++s) {
        long long r = 0;
        for (int ax = 0; ax < D; ++ax) r = r * nlead[ax] + idx[ax][(s >> ax) & 1];
        roff[s] = r;
    }
    const int jq[4] = {kx, (nl - kx) & (nl - 1), L - kx, (L + kx) & (nl - 1)};
    const bool wq[4] = {true, kx != 0, L == 1 || 2 * kx != L, kx != 0 && 2 * kx != L};
    const cx<T> W = reinterpret_cast<const cx<T>*>(a.sep)[kx];
    const long long half_item = (long long)(nl / 2) * (long long)(D >= 1 ? nlead[0] : 1) * (D >= 2 ? nlead[1] : 1);
    cx<T> V[S][4];
    if constexpr (!INV) {
        const cx<T>* Z = reinterpret_cast<const cx<T>*>(a.in) + item * half_item;
        const int m0 = kx & (L - 1), m1 = (L - kx) & (L - 1);
        cx<T> z0[S], z1[S];
        for (int s = 0; s < S; ++s) {
            z0[s] = Z[roff[s] * L + m0];
            z1[s] = Z[roff[s] * L + m1];
        }
        const cx<T> W2 = {-W.x, W.y};           // w(nl)^(L - kx) = -conj(w(nl)^kx)
        for (int s = 0; s < S; ++s) {
            const int sm = s ^ (S - 1);         // the orbit's -kp
            // 2 V[kp, j] = (p + conj q) - i w(nl)^j (p - conj q),  p = Z[kp, j], q = Z[-kp, L - j]
            const cx<T> pq[2][2] = {{z0[s], z1[sm]}, {z1[s], z0[sm]}};
            for (int h = 0; h < 2; ++h) {
                const cx<T> p = pq[h][0], q = pq[h][1];
                const cx<T> sm_ = {p.x + q.x, p.y - q.y}, df = {p.x - q.x, p.y + q.y};
                const cx<T> t = cmul(h ? W2 : W, df);
                V[s][2 * h] = cx<T>{sm_.x + t.y, sm_.y - t.x};
            }
        }
        for (int s = 0; s < S; ++s) {           // V[kp, n - j] = conj V[-kp, j]
            V[s ^ (S - 1)][1] = conj_(V[s][0]);
            V[s ^ (S - 1)][3] = conj_(V[s][2]);
        }
        // leading axes: Y[k] = t[k] V[k] + conj(t[k]) V[-k]
        for (int ax = 0; ax < D; ++ax) {
            const cx<T>* tab = reinterpret_cast<const cx<T>*>(a.tab[ax]);
            const cx<T> t0 = tab[idx[ax][0]], t1 = tab[idx[ax][1]];
            for (int s = 0; s < S; ++s) {
                if ((s >> ax) & 1) continue;
                const int s1 = s | (1 << ax);
                for (int q = 0; q < 4; ++q) {
                    const cx<T> x0 = V[s][q], x1 = V[s1][q];
                    const cx<T> a0 = cmul(t0, x0), b0 = cmul(conj_(t0), x1);
                    const cx<T> a1 = cmul(t1, x1), b1 = cmul(conj_(t1), x0);
                    V[s][q] = cx<T>{a0.x + b0.x, a0.y + b0.y};
                    V[s1][q] = cx<T>{a1.x + b1.x, a1.y + b1.y};
                }
            }
        }
        // contiguous axis, real part only; pairs (kx, -kx) and (L - kx, L + kx)
        const cx<T>* tl = reinterpret_cast<const cx<T>*>(a.tab[D]);
        T* Y = reinterpret_cast<T*>(a.out) + item * 2 * half_item;
        for (int s = 0; s < S; ++s) {
            bool skip = false;
            long long orow = 0;
            for (int ax = 0; ax < D; ++ax) {
                const int bit = (s >> ax) & 1;
                if (bit && !wr[ax]) skip = true;
                const int i = idx[ax][bit];
                orow = orow * nlead[ax] + (a.dst ? nlead[ax] - 1 - i : i);
            }
            if (skip) continue;
            T* yrow = Y + orow * nl;
            for (int h = 0; h < 2; ++h) {
                const cx<T> ta = tl[jq[2 * h]], tb = tl[jq[2 * h + 1]];
                const cx<T> x0 = V[s][2 * h], x1 = V[s][2 * h + 1];
                const T y0 = ta.x * x0.x - ta.y * x0.y + ta.x * x1.x + ta.y * x1.y;
                const T y1 = tb.x * x1.x - tb.y * x1.y + tb.x * x0.x + tb.y * x0.y;
                if (wq[2 * h]) yrow[a.dst ? nl - 1 - jq[2 * h] : jq[2 * h]] = y0;
                if (wq[2 * h + 1]) yrow[a.dst ? nl - 1 - jq[2 * h + 1] : jq[2 * h + 1]] = y1;
            }
        }
    } else {
        const T* Y = reinterpret_cast<const T*>(a.in) + item * 2 * half_item;
        for (int s = 0; s < S; ++s) {
            bool zero = false;                  // Y[n] = 0 on an axis where the orbit's k is 0
            long long irow = 0;
            for (int ax = 0; ax < D; ++ax) {
                const int bit = (s >> ax) & 1;
                if (bit && k[ax] == 0) zero = true;
                const int i = idx[ax][bit];
                irow = irow * nlead[ax] + (a.dst ? nlead[ax] - 1 - i : i);
            }
            const T* yrow = Y + irow * nl;
            for (int q = 0; q < 4; ++q) {
                const bool zq = zero || (q == 1 && kx == 0);
                V[s][q] = cx<T>{zq ? (T)0 : yrow[a.dst ? nl - 1 - jq[q] : jq[q]], (T)0};
            }
        }
        // every axis: V[k] = u[k] (Y[k] - i Y[-k]),  V[-k] = u[-k] (Y[-k] - i Y[k])
        for (int ax = 0; ax <= D; ++ax) {
            const cx<T>* tab = reinterpret_cast<const cx<T>*>(a.tab[ax]);
            if (ax < D) {
                const cx<T> u0 = tab[idx[ax][0]], u1 = tab[idx[ax][1]];
                for (int s = 0; s < S; ++s) {
                    if ((s >> ax) & 1) continue;
                    const int s1 = s | (1 << ax);
                    for (int q = 0; q < 4; ++q) {
                        const cx<T> x0 = V[s][q], x1 = V[s1][q];
                        V[s][q] = cmul(u0, cx<T>{x0.x + x1.y, x0.y - x1.x});
                        V[s1][q] = cmul(u1, cx<T>{x1.x + x0.y, x1.y - x0.x});
                    }
                }
            } else {
                for (int h = 0; h < 2; ++h) {
                    const cx<T> u0 = tab[jq[2 * h]], u1 = tab[jq[2 * h + 1]];
                    for (int s = 0; s < S; ++s) {
                        const cx<T> x0 = V[s][2 * h], x1 = V[s][2 * h + 1];
                        V[s][2 * h] = cmul(u0, cx<T>{x0.x + x1.y, x0.y - x1.x});
                        V[s][2 * h + 1] = cmul(u1, cx<T>{x1.x + x0.y, x1.y - x0.x});
                    }
                }
            }
        }
        // packing: Z'[kx] = (V[kx] + V[L + kx]) + i w(nl)^-kx (V[kx] - V[L + kx]);  Z'[L - kx] from V[L - kx], V[n - kx] with
        // w(nl)^-(L - kx) = -w(nl)^kx
        cx<T>* Zo = reinterpret_cast<cx<T>*>(a.out) + item * half_item;
        const bool second = kx != 0 && 2 * kx != L;
        for (int s = 0; s < S; ++s) {
            bool skip = false;
            for (int ax = 0; ax < D; ++ax)
                if (((s >> ax) & 1) && !wr[ax]) skip = true;
            if (skip) continue;
            cx<T>* zrow = Zo + roff[s] * L;
            {
                const cx<T> p = V[s][0], q = V[s][3];
                const cx<T> df = cmul(conj_(W), cx<T>{p.x - q.x, p.y - q.y});
                zrow[kx] = cx<T>{p.x + q.x - df.y, p.y + q.y + df.x};
            }
            if (second) {
                const cx<T> p = V[s][2], q = V[s][1];
                const cx<T> df = cmul(cx<T>{-W.x, -W.y}, cx<T>{p.x - q.x, p.y - q.y});
                zrow[L - kx] = cx<T>{p.x + q.x - df.y, p.y + q.y + df.x};
            }
        }
    }
}

template <typename T, int D, bool INV>
__global__ void __launch_bounds__(256) r2r_orbit_kernel(const R2rOrbitArgs a) {
    const unsigned b = blockIdx.x;
    const unsigned grp = b / a.blocks_per_row_group, part = b - grp * a.blocks_per_row_group;
    const long long row = (long long)grp * a.rows_per_block + (threadIdx.x >> a.log_lanes);
    const int kx0 = (int)(part << a.log_lanes) + (int)(threadIdx.x & (a.lanes - 1));
    if (row >= a.rows || kx0 >= a.cx) return;
    const long long item = row / a.lead_count;
    const unsigned l = (unsigned)(row - item * a.lead_count);
    int k[2] = {0, 0};
    if constexpr (D == 1) k[0] = (int)l;
    if constexpr (D == 2) {
        k[0] = (int)(l / (unsigned)a.c1);
        k[1] = (int)(l - (unsigned)k[0] * (unsigned)a.c1);
    }
    r2r_orbit<T, D, INV>(a, item, k, kx0);
    if (a.fold && kx0 == 0) r2r_orbit<T, D, INV>(a, item, k, a.L / 2);
}

int ilog2i(long long v) {
    int r = 0;
    while (v > 1) { v >>= 1; ++r; }
    return r;
}

template <typename T>
int launch_perm(int inverse, int nd, const int* n, long long outer, const void* in, void* out, double scale, int dst, hipStream_t s) {
    R2rPermArgs a;
    a.in = in;
    a.out = out;
    a.scale = scale;
    a.dst = dst;
    a.nl = n[nd - 1];
    a.n0 = nd >= 3 ? n[0] : 1;
    a.n1 = nd >= 2 ? n[nd - 2] : 1;
    a.log_n1 = ilog2i(a.n1);
    a.log_rows = ilog2i((long long)a.n0 * a.n1);
    const uintptr_t x = (uintptr_t)(inverse ? out : in);
    const bool vec = a.nl % 4 == 0 && (x & 15) == 0;
    a.log_cw = ilog2i(vec ? a.nl / 4 : a.nl);
    a.total = (outer << a.log_rows) << a.log_cw;
    if (a.total == 0) return 0;
    const long long blocks = (a.total + 255) / 256;
    if (blocks > 2147483647ll) return -1;
    if (vec) {
        if (inverse) hipLaunchKernelGGL((r2r_perm_kernel<T, true, 4>), dim3((unsigned)blocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((r2r_perm_kernel<T, false, 4>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    } else {
        if (inverse) hipLaunchKernelGGL((r2r_perm_kernel<T, true, 1>), dim3((unsigned)blocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((r2r_perm_kernel<T, false, 1>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

template <typename T, bool INV>
int launch_orbit(int nd, const int* n, long long outer, const void* in, void* out, const void* tw, int dst, hipStream_t s) {
    R2rOrbitArgs a;
    a.in = in;
    a.out = out;
    a.dst = dst;
    const cx<T>* t = reinterpret_cast<const cx<T>*>(tw);
    for (int ax = 0; ax < 3; ++ax) a.tab[ax] = nullptr;
    for (int ax = 0; ax < nd; ++ax) {
        a.tab[ax] = t;
        t += n[ax];
    }
    a.sep = t;
    a.n0 = nd >= 2 ? n[0] : 1;
    a.n1 = nd >= 3 ? n[1] : 1;
    a.c1 = a.n1 / 2 + 1;
    a.lead_count = 1;
    for (int ax = 0; ax < nd - 1; ++ax) a.lead_count *= (unsigned)(n[ax] / 2 + 1);
    a.nl = n[nd - 1];
    a.L = a.nl / 2;
    // a row of at least a wave's orbits gives the L / 2 orbit to its kx = 0 thread (one doubled lane in L / 128 waves); a shorter row
    // gives it a lane of its own, so that no wave carries a second orbit in every row
    a.fold = a.L / 2 >= 64;
    a.cx = a.L >= 2 ? (a.fold ? a.L / 2 : a.L / 2 + 1) : 1;
    int lanes = 1;
    while (lanes < a.cx && lanes < 256) lanes *= 2;
    a.lanes = lanes;
    a.log_lanes = ilog2i(lanes);
    a.rows_per_block = 256u / (unsigned)lanes;
    a.blocks_per_row_group = (unsigned)((a.cx + lanes - 1) / lanes);
    a.rows = outer * (long long)a.lead_count;
    if (a.rows == 0) return 0;
    const long long groups = (a.rows + a.rows_per_block - 1) / a.rows_per_block;
    const long long blocks = groups * a.blocks_per_row_group;
    if (blocks > 2147483647ll) return -1;
    const dim3 g((unsigned)blocks), b(256);
    if (nd == 1) hipLaunchKernelGGL((r2r_orbit_kernel<T, 0, INV>), g, b, 0, s, a);
    else if (nd == 2) hipLaunchKernelGGL((r2r_orbit_kernel<T, 1, INV>), g, b, 0, s, a);
    else hipLaunchKernelGGL((r2r_orbit_kernel<T, 2, INV>), g, b, 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace

// 0 launched, -1 grid too large, or a hipError_t.  Arguments were checked by mifft_launch_r2r_pre / _post.
// post = 0: the pre step (forward: permutation; inverse: orbit), post = 1: the post step (forward: orbit; inverse: permutation)
extern "C" int mifft_r2r_step_launch(int f64, int post, int inverse, int kind, int nd, const int* n, long long outer, const void* in, void* out,
                                     const void* tw, double scale, hipStream_t s) {
    const int dst = kind == 1;
    if (post == inverse) {                      // the permutation steps: forward pre, inverse post
        return f64 ? launch_perm<double>(inverse, nd, n, outer, in, out, scale, dst, s)
                   : launch_perm<float>(inverse, nd, n, outer, in, out, scale, dst, s);
    }
    if (inverse) return f64 ? launch_orbit<double, true>(nd, n, outer, in, out, tw, dst, s) : launch_orbit<float, true>(nd, n, outer, in, out, tw, dst, s);
    return f64 ? launch_orbit<double, false>(nd, n, outer, in, out, tw, dst, s) : launch_orbit<float, false>(nd, n, outer, in, out, tw, dst, s);
}
