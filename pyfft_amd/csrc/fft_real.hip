// Real-input transforms: the separation (forward) and packing (inverse) steps around a complex transform of the packed data.
// A real array x of shape (..., nx) viewed as interleaved complex numbers is z[..., m] = x[..., 2m] + i x[..., 2m + 1], an array of
// shape (..., L) with L = nx / 2; Z = FFT(z) over all axes.  With k = (kp, kx) and -k = (-kp mod np, (L - kx) mod L) over ALL axes:
//   forward  X[kp, kx] = 1/2 (Z[k] + conj Z[-k]) - 1/2 i w(nx)^kx (Z[k] - conj Z[-k]),          0 <= kx <= L   (half spectrum)
//   inverse  Z[kp, kx] = (X[k] + conj X'[k]) + i w(nx)^-kx (X[k] - conj X'[k]),  X'[k] = X[-kp, L - kx],  0 <= kx < L
// (fft_real_ident.hpp holds both as functions of s = a + conj b, d = a - conj b of a point a and its mirror b, for this file and the
// one-launch rows: forward 1/2 (s - i w d), and 1/2 (s + i d) at kx = L from the pair of kx = 0, w(nx)^L = -1; inverse s + i conj(w) d)
// and the unnormalised inverse complex transform of that Z is the unnormalised inverse real transform, packed the same way.  The inverse
// reads the two edge planes kx = 0 and kx = L through their Hermitian parts 1/2 (X[kp, e] + conj X[-kp, e]): the leading axes' inverse
// transforms of a non-Hermitian edge plane would otherwise leave imaginary parts that a real result has to drop (what numpy's irfftn
// does after its leading inverse transforms).
// A streaming kernel: one thread per packed point reads its own point and the mirrored one (the forward's kx = 0 thread writes X[kp, 0]
// and X[kp, L], both from the same two points); the mirrored half is the same rows read
// backwards, so a wave's mirrored loads are one descending contiguous run (coalesced), and the second read of every line finds it in
// the L2 / Infinity Cache behind the first.
#include <hip/hip_runtime.h>
#include "mifft_internal.h"
#include "fft_real_ident.hpp"

namespace {

struct RealPostArgs {
    const void* in;
    void* out;
    const void* tw;            // L + 1 entries w(nx)^k
    long long stride_in;       // item pitch, complex numbers
    long long stride_out;
    double scale;
    unsigned rows_per_item;    // ny * nz
    int log_ny;
    int ny, nz;
    int L;                     // nx / 2
    int lanes;                 // threads per row segment (a power of two)
    int log_lanes;
    unsigned rows_per_block;   // 256 / lanes
    unsigned blocks_per_row_group;
    long long rows;            // outer * ny * nz
};

template <typename T> using cx = mifft::cplx<T>;

template <typename T, bool INV>
__global__ void __launch_bounds__(256) real_post_kernel(const RealPostArgs a) {
    const unsigned b = blockIdx.x;
    const unsigned grp = b / a.blocks_per_row_group, part = b - grp * a.blocks_per_row_group;
    const long long row = (long long)grp * a.rows_per_block + (threadIdx.x >> a.log_lanes);
    const int kx = (int)(part << a.log_lanes) + (int)(threadIdx.x & (a.lanes - 1));
    const int L = a.L;
    if (row >= a.rows || kx >= L) return;       // one thread per packed point: kx = 0 also writes the forward's X[kp, L]
    const long long item = row / a.rows_per_item;
    const unsigned r = (unsigned)(row - item * a.rows_per_item);
    const int iy = (int)(r & (unsigned)(a.ny - 1)), iz = (int)(r >> a.log_ny);
    const int my = (a.ny - iy) & (a.ny - 1), mz = (a.nz - iz) & (a.nz - 1);
    const long long mrow = (long long)mz * a.ny + my;
    const cx<T>* tw = reinterpret_cast<const cx<T>*>(a.tw);
    const T s = (T)a.scale;
    if constexpr (!INV) {
        // Z rows at pitch L, X rows at pitch L + 1
        const cx<T>* zi = reinterpret_cast<const cx<T>*>(a.in) + item * a.stride_in;
        const cx<T> p = zi[(long long)r * L + (kx & (L - 1))];
        const cx<T> q = zi[mrow * L + ((L - kx) & (L - 1))];
        const cx<T> w = tw[kx];
        cx<T> sm, df;
        mifft::real_sd<T>(p, q, sm, df);                    // Z[k] + conj Z[-k], Z[k] - conj Z[-k]
        const T h = (T)0.5 * s;
        const cx<T> o = mifft::real_sep<T>(sm, w, df, h);
        cx<T>* xo = reinterpret_cast<cx<T>*>(a.out) + item * a.stride_out + (long long)r * (L + 1);
        xo[kx] = o;
        if (kx == 0) xo[L] = mifft::real_sep_edge<T>(sm, df, h);   // the same two points
    } else {
        const cx<T>* xi = reinterpret_cast<const cx<T>*>(a.in) + item * a.stride_in;
        const int P = L + 1;
        cx<T> p = xi[(long long)r * P + kx];
        cx<T> q = xi[mrow * P + (L - kx)];
        if (kx == 0) {
            // the edge planes through their Hermitian parts: p = X[kp, 0], q = X[-kp, L]
            const cx<T> pm = xi[mrow * P];                  // X[-kp, 0]
            const cx<T> qm = xi[(long long)r * P + L];      // X[kp, L]
            p = cx<T>{(T)0.5 * (p.x + pm.x), (T)0.5 * (p.y - pm.y)};
            q = cx<T>{(T)0.5 * (q.x + qm.x), (T)0.5 * (q.y - qm.y)};
        }
        const cx<T> w = tw[kx];
        cx<T> sm, df;
        mifft::real_sd<T>(p, q, sm, df);                    // X[k] + conj X'[k], X[k] - conj X'[k]
        const cx<T> o = mifft::real_pack<T>(sm, w, df);
        reinterpret_cast<cx<T>*>(a.out)[item * a.stride_out + (long long)r * L + kx] = cx<T>{o.x * s, o.y * s};
    }
}

int ilog2i(long long v) {
    int r = 0;
    while (v > 1) { v >>= 1; ++r; }
    return r;
}

}  // namespace

// 0 launched, -1 grid too large, or a hipError_t.  Arguments were checked by mifft_launch_real_post.
extern "C" int mifft_real_post_launch(int f64, int inverse, int nx, int ny, int nz, long long outer, long long stride_in,
                                      long long stride_out, const void* in, void* out, const void* tw, double scale, hipStream_t s) {
    RealPostArgs a;
    a.in = in;
    a.out = out;
    a.tw = tw;
    a.stride_in = stride_in;
    a.stride_out = stride_out;
    a.scale = scale;
    a.ny = ny;
    a.nz = nz;
    a.log_ny = ilog2i(ny);
    a.rows_per_item = (unsigned)ny * (unsigned)nz;
    a.L = nx / 2;
    const int width = a.L;                      // threads per row (the forward's X[kp, L] comes from the kx = 0 thread)
    int lanes = 1;
    while (lanes < width && lanes < 256) lanes *= 2;
    a.lanes = lanes;
    a.log_lanes = ilog2i(lanes);
    a.rows_per_block = 256u / (unsigned)lanes;
    a.blocks_per_row_group = (unsigned)((width + lanes - 1) / lanes);
    a.rows = outer * (long long)a.rows_per_item;
    if (a.rows == 0) return 0;
    const long long groups = (a.rows + a.rows_per_block - 1) / a.rows_per_block;
    const long long blocks = groups * a.blocks_per_row_group;
    if (blocks > 2147483647ll) return -1;
    if (f64) {
        if (inverse) hipLaunchKernelGGL((real_post_kernel<double, true>), dim3((unsigned)blocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((real_post_kernel<double, false>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    } else {
        if (inverse) hipLaunchKernelGGL((real_post_kernel<float, true>), dim3((unsigned)blocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((real_post_kernel<float, false>), dim3((unsigned)blocks), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}
