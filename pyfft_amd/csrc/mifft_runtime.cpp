// C-ABI runtime shim + pass launchers of libmifft.so (see include/mifft.h for the contract and for
// the reference interfaces each entry point replaces).
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <initializer_list>

#include "../../include/mifft.h"
#include "mifft_internal.h"
#include "fft_conv_row.hpp"
#include "fft_fir_row.hpp"

namespace {

thread_local char g_err[512] = "";
// the library's only process-wide state: the DEFAULTS of the development switches (all zero in production) and a per-device
// compute-unit count.  The switches: a process default (mifft_debug_set_default) under a per-thread override (mifft_debug_set) -- a switch flipped
// by one thread never changes what another thread's plan launches
std::atomic<int> g_debug_default[MIFFT_DEBUG_KEYS];
thread_local int t_debug_value[MIFFT_DEBUG_KEYS];
thread_local unsigned t_debug_mask = 0;
thread_local int t_pair_lanes_form = -1;   // form of this thread's last fp32 1-D 1024 x 1024 persistent launch (mifft_debug_last_pair_lanes_form)
struct DebugSwitches {
    int operator[](int key) const {
        return ((t_debug_mask >> key) & 1u) ? t_debug_value[key] : g_debug_default[key].load(std::memory_order_relaxed);
    }
};
const DebugSwitches g_debug;

int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    return set_err((int)e, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

// what a kernel launcher of this library returned (0, -1 = grid too large, else a hipError_t) as the entry point's result; a launcher's
// -2 ("no such kernel") is the caller's to name
int launched(int rc) {
    if (rc == -1) return set_err(MIFFT_E_INVALID, "grid too large");
    return hip_check((hipError_t)rc, "kernel launch");
}

bool is_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }
bool bad_precision(int precision) { return precision != MIFFT_F32 && precision != MIFFT_F64; }
long long complex_bytes(int precision) { return precision == MIFFT_F64 ? 16 : 8; }
// is one of the addresses no multiple of mask + 1 (null counts as aligned)
bool misaligned(uintptr_t mask, std::initializer_list<const void*> ptrs) {
    uintptr_t all = 0;
    for (const void* p : ptrs) all |= (uintptr_t)p;
    return (all & mask) != 0;
}
bool misaligned_complex(int precision, std::initializer_list<const void*> ptrs) { return misaligned((uintptr_t)complex_bytes(precision) - 1, ptrs); }
// do the byte ranges [a, a + na) and [b, b + nb) share a byte
bool overlap(const void* a, uintptr_t na, const void* b, uintptr_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; }
// the two sides of a pass: scalar planes, or interleaved (always for MIFFT_INTERLEAVED; for MIFFT_SPLIT the plan's temp buffer)
bool planes_in(const mifft_pass* p) { return p->layout == MIFFT_SPLIT && !(p->flags & MIFFT_FLAG_SRC_INTERLEAVED); }
bool planes_out(const mifft_pass* p) { return p->layout == MIFFT_SPLIT && !(p->flags & MIFFT_FLAG_DST_INTERLEAVED); }
// a * b * c (all >= 0) without overflow, or -1
long long mul3_checked(long long a, long long b, long long c) {
    long long ab, abc;
    if (__builtin_mul_overflow(a, b, &ab) || __builtin_mul_overflow(ab, c, &abc)) return -1;
    return abc;
}
// rows of the mixed-radix / Bluestein launchers: interleaved complex numbers, 8-byte (fp32) / 16-byte (fp64) aligned; an in-place call
// must keep every row where it is (a work-group stores its rows while others have not loaded theirs yet)
const char* check_rows(int precision, const void* in, const void* out, long long rows, long long n, long long stride_in, long long stride_out) {
    if (misaligned_complex(precision, {in, out})) return "data buffers must be aligned to one complex number";
    if (in == out && stride_in != stride_out) return "an in-place call needs equal row strides on both sides";
    if (mul3_checked(rows, stride_in > stride_out ? stride_in : stride_out, complex_bytes(precision)) < 0) return "rows * stride overflows";
    (void)n;
    return nullptr;
}
int ilog2(long long v) {
    int r = 0;
    while (v > 1) {
        v >>= 1;
        ++r;
    }
    return r;
}

// ---- which kernel form runs an MIFFT_PASS_ND pass ---------------------------------------------------------------------------------
// One gate per form that has instances of its own: the form's development switches, its instance query and its minimum-row-bytes rule.
// select_nd() (what a launch runs), nd_has_kernel() (what validate() accepts) and mifft_nd_shape_supported() (what a planner is told)
// are all written in terms of these.  MIFFT_DEBUG_NO_ND2: the run-time-shaped kernel only.

// fixed shapes, interleaved on both sides (fft_nd2.hpp; the generated tables fft_nd2_<prec>_*.hip).  The instance query alone: the
// switch acts when a pass is launched (select_nd), not on what the planner is told
bool nd2_instance(bool f64, int x, int y, int z) { return (f64 ? mifft_nd2_f64_supported(x, y, z) : mifft_nd2_f32_supported(x, y, z)) == 0; }

// several work-groups per transform, interleaved on both sides, out of place only (fft_nd2z.hpp, round 5).  It is only instantiated where
// it measured faster, at 32 MiB and at 1 GiB per side.  level 1: a kernel exists -- what a shape without another one-launch kernel runs
// (FOUR two-per-CU tiles; the plan only builds such a pass for its out-of-place executes), and what runs in SMALL launches (the plan marks
// those with MIFFT_FLAG_WRITE_THROUGH: up to half the last-level cache per side); level 2: one that is preferred at every buffer size (the
// one-tile-per-CU shapes).  A/B: MIFFT_DEBUG_ALT_ROWS = 6 never
bool nd2z_gate(bool f64, int x, int y, int z, int level) {
    return g_debug[MIFFT_DEBUG_NO_ND2] == 0 && g_debug[MIFFT_DEBUG_ALT_ROWS] != 6 && mifft_nd2z(f64 ? 1 : 0, x, y, z, nullptr, nullptr, level) == 0;
}

// planes on BOTH sides of a published shape, dense, 16 bytes per lane and plane (fft_nd2p.hpp, round 6); the tiled kernel below moves one
// scalar per lane and plane through the tiling's address arithmetic (0.69-0.86 of the interleaved twin at 1 GiB).  level 1: an instance
// exists; 2: it is also the choice for small launches.  MIFFT_DEBUG_ALT_ROWS = 7: the tiled kernel (A/B)
bool nd2p_gate(bool f64, int x, int y, int z, int level) {
    return g_debug[MIFFT_DEBUG_NO_ND2] == 0 && g_debug[MIFFT_DEBUG_NARROW_TILES] != 1 && g_debug[MIFFT_DEBUG_ALT_ROWS] != 7 &&
           mifft_nd2p(f64 ? 1 : 0, x, y, z, nullptr, nullptr, level) == 0;
}

// ... and its one-tile-per-CU shapes as two half-size work-groups per transform, out of place (fft_nd2zp.hpp; levels as for nd2z_gate;
// MIFFT_DEBUG_ALT_ROWS = 6: never several work-groups per transform, as for interleaved data)
bool nd2zp_gate(bool f64, int x, int y, int z, int level) {
    return g_debug[MIFFT_DEBUG_NO_ND2] == 0 && g_debug[MIFFT_DEBUG_NARROW_TILES] != 1 && g_debug[MIFFT_DEBUG_ALT_ROWS] != 7 &&
           g_debug[MIFFT_DEBUG_ALT_ROWS] != 6 && mifft_nd2zp(f64 ? 1 : 0, x, y, z, nullptr, nullptr, level) == 0;
}

// planes on the input side (planes -> planes: a single-pass N-D plan; planes -> interleaved: the plane pass of a split-complex multi-pass
// plan, fft_nd2t_split_in.hip): the fixed-shape stage chain exists for planes in its TILED form (fft_nd2t.hpp, second batch of round 4)
// -- a dense batch is the tiling with one tile per "parent".  (128, 128) planes at 1 GiB: 0.471 on the run-time-shaped kernel -> 0.653
// (interleaved fixed-shape kernel 0.700), (64, 64) 0.535 -> 0.597, fp64 16^3 0.510 -> 0.584; shapes whose x rows are shorter than 128 bytes
// per plane stay on the run-time-shaped kernel -- fp32 (16, 16) 0.717 against 0.460, 16^3 0.674 against 0.475: their tiles move scalars over
// short runs (profiles/r04_at_rows_split.log).  min_row_bytes: 128 to RUN it; 256 to PREFER it to two passes when planning (fp64
// (128, 128) 0.374 as two passes -> 0.568, (16, 32, 32) 0.338 -> 0.499; fp32 32^3, 128-byte rows, measured 0.285 against 0.307 for its
// two passes and keeps them -- same log)
bool nd2t_gate(bool f64, int x, int y, int z, int min_row_bytes) {
    return g_debug[MIFFT_DEBUG_NO_ND2] == 0 && g_debug[MIFFT_DEBUG_NARROW_TILES] != 1 && x * (f64 ? 8 : 4) >= min_row_bytes &&
           mifft_nd2t_split(f64, x, y, z, nullptr, nullptr, nullptr, 1) == 0;
}

// validate(): is there a kernel for the pass's shape and sides at all.  Beyond the run-time-shaped kernel's tile: a fixed instance of the
// sides' own (planes on the input side: the tiled kernel's planning threshold, or a dense planes instance), or one that exists out of
// place only -- select_nd refuses an in-place call of those, with its own message
bool nd_has_kernel(const mifft_pass* p) {
    const bool f64 = p->precision == MIFFT_F64;
    const int x = p->L, y = (int)p->M, z = (int)p->S;
    const long long n = mul3_checked(p->L, p->M, p->S);
    if (n >= 0 && n <= mifft_nd_max_points(f64)) return true;
    if (!planes_in(p)) return !planes_out(p) && (nd2_instance(f64, x, y, z) || nd2z_gate(f64, x, y, z, 1));
    return nd2t_gate(f64, x, y, z, 256) || nd2p_gate(f64, x, y, z, 1) || (planes_out(p) && nd2zp_gate(f64, x, y, z, 1));
}

int validate(const mifft_pass* p) {
    if (!p) return set_err(MIFFT_E_INVALID, "null pass descriptor");
    if (p->kind != MIFFT_PASS_COL && p->kind != MIFFT_PASS_ROW && p->kind != MIFFT_PASS_ND) return set_err(MIFFT_E_INVALID, "bad pass kind %d", p->kind);
    if (bad_precision(p->precision)) return set_err(MIFFT_E_INVALID, "bad precision %d", p->precision);
    if (p->layout != MIFFT_INTERLEAVED && p->layout != MIFFT_SPLIT) return set_err(MIFFT_E_INVALID, "bad layout %d", p->layout);
    if (!is_pow2(p->L) || (p->L < 2 && p->kind != MIFFT_PASS_ND)) return set_err(MIFFT_E_INVALID, "L=%d is not a power of two >= 2", p->L);
    if (p->outer < 0) return set_err(MIFFT_E_INVALID, "negative outer count");
    if (p->kind == MIFFT_PASS_ND) {
        if (!is_pow2(p->M) || !is_pow2(p->S)) return set_err(MIFFT_E_INVALID, "ND pass: y and z must be powers of two");
        const long long n = (long long)p->L * p->M * p->S;
        if (n < 4 || !nd_has_kernel(p))
            return set_err(MIFFT_E_UNSUPPORTED, "ND pass: no kernel for %d x %lld x %lld (%lld points)", p->L, (long long)p->M, (long long)p->S, n);
        if ((p->L > 1 && !p->tw_L) || (p->M > 1 && !p->tw_lo) || (p->S > 1 && !p->tw_hi)) return set_err(MIFFT_E_INVALID, "ND pass: twiddle table missing");
        return 0;
    }
    if (!p->tw_L) return set_err(MIFFT_E_INVALID, "tw_L table missing");
    if (p->kind == MIFFT_PASS_COL) {
        if (!is_pow2(p->M) || !is_pow2(p->S)) return set_err(MIFFT_E_INVALID, "M and S must be powers of two");
        if (p->M * p->S < 2) return set_err(MIFFT_E_INVALID, "a COL pass needs M*S >= 2 (use a ROW pass)");
        if ((long long)p->L * p->M > (1ll << 30)) return set_err(MIFFT_E_INVALID, "axis longer than 2^30");
        if (p->M > 1) {
            if (!p->tw_lo || !p->tw_hi) return set_err(MIFFT_E_INVALID, "inter-pass twiddle tables missing (M > 1)");
            if (p->tw_shift < 0 || p->tw_shift > 30) return set_err(MIFFT_E_INVALID, "bad tw_shift");
        }
    } else {
        if (p->M != 1 || p->S != 1) return set_err(MIFFT_E_INVALID, "a ROW pass has M == S == 1");
    }
    return 0;
}

// development switch MIFFT_DEBUG_STORE: overrides the store side of a TileArgs.nt / PairArgs.nt for A/B measurements
int store_override(int nt) {
    const int how = g_debug[MIFFT_DEBUG_STORE];
    return how == 1 ? (nt & 1) | 2 : how == 2 ? (nt & 1) | 4 : how == 3 ? nt & 1 : nt;
}
// TileArgs.nt from the MIFFT_FLAG_STREAM_* hints: bit 0 non-temporal loads, bit 1 non-temporal stores, bit 2 write-through stores
int stream_policy(int flags) {
    int nt = ((flags & MIFFT_FLAG_STREAM_SRC) ? 1 : 0) | ((flags & MIFFT_FLAG_STREAM_DST) ? 2 : 0);
    if (flags & MIFFT_FLAG_WRITE_THROUGH) nt = (nt & 1) | 4;
    return store_override(nt);
}

void fill_args(const mifft_pass* p, const void* in0, const void* in1, void* out0, void* out1, mifft::TileArgs* pa) {
    mifft::TileArgs& a = *pa;
    a.in0 = in0;
    a.in1 = in1;
    a.out0 = out0;
    a.out1 = out1;
    a.tw_L = p->tw_L;
    a.tw_lo = p->tw_lo;
    a.tw_hi = p->tw_hi;
    a.ostride_in = p->outer_stride_in;
    a.ostride_out = p->outer_stride_out;
    if (p->kind == MIFFT_PASS_COL) {
        a.total = p->outer * p->M * p->S;
        a.logMS = ilog2(p->M * p->S);
        a.logS = ilog2(p->S);
    } else {
        a.total = p->outer;
        a.logMS = 0;
        a.logS = 0;
    }
    a.tw_shift = p->tw_shift;
    a.split = planes_in(p) ? 1 : 0;
    a.split_out = planes_out(p) ? 1 : 0;
    a.inverse = p->inverse ? 1 : 0;
    a.has_tw = (p->kind == MIFFT_PASS_COL && p->M > 1) ? 1 : 0;
    a.nt = stream_policy(p->flags);
    a.scale = p->scale;
}

// radix list of one axis for the in-LDS N-D kernel (each radix <= maxr, a power of two)
int nd_radices(int L, int maxr, int* out) {
    int n = 0;
    while (L > 1) {
        int r = maxr;
        while (r > L) r >>= 1;
        // avoid a trailing radix 2 after big radices: prefer e.g. 32 = 8 * 4 over 16 * 2
        if (L > r && L / r == 2 && r >= 8) r >>= 1;
        out[n++] = r;
        L /= r;
    }
    return n;
}

// compute units of the CURRENT device (cached per device index: a process may drive several different devices)
int current_cus() {
    static std::atomic<int> cached[64];
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < 64 && (cus = cached[dev].load(std::memory_order_relaxed)) > 0) return cus;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) return 256;
    if (dev >= 0 && dev < 64) cached[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

// grid cap of the grid-stride wave kernels: 8 work-groups of 4 waves per CU
int wave_max_blocks() { return current_cus() * 8; }

long long wave_bytes(const mifft_pass* p, const mifft::TileArgs* a) {   // bytes of one side of a dense ROW pass
    return a->total * p->L * (p->precision == MIFFT_F64 ? 16ll : 8ll);
}

// the stage list of the run-time-shaped N-D kernel (fft_nd.hpp) for the axes dims (x, y, z): axis geometry, radices, nstages, and the
// register edge -- the last stage of all writes runs of (L / radix) * S points, straight to HBM when that is >= 128 bytes (interleaved
// output only: the caller clears edge_out for planes); -1 if it needs more than kNdMaxStages stages
int nd_stage_list(const long long dims[3], bool f64, mifft::NdArgs* a) {
    int logs = 0, ns = 0;
    for (int ax = 0; ax < 3; ++ax) {
        a->logL[ax] = ilog2(dims[ax]);
        a->logS[ax] = logs;
        logs += a->logL[ax];
        int rad[16];
        const int nr = nd_radices((int)dims[ax], f64 ? 8 : 16, rad);
        int logNs = 0;
        for (int i = 0; i < nr; ++i) {
            if (ns >= mifft::kNdMaxStages) return -1;
            a->st_axis[ns] = (unsigned char)ax;
            a->st_radix[ns] = (unsigned char)rad[i];
            a->st_logNs[ns] = (unsigned char)logNs;
            logNs += ilog2(rad[i]);
            ++ns;
        }
    }
    a->nstages = ns;
    if (ns >= 1) {
        const int axn = a->st_axis[ns - 1];
        a->edge_out = ((dims[axn] / a->st_radix[ns - 1]) << a->logS[axn]) * (f64 ? 16 : 8) >= 128 ? 1 : 0;
    }
    return 0;
}

// The kernel form (MIFFT_ND_KERNEL_*) a validated ND pass runs -- a pure function of the descriptor, of which of the two buffer pairs
// alias (bit 0: in0 == out0, bit 1: in1 == out1) and of the calling thread's development switches -- or a negative error code with its
// message.  The planes of a side that has them are never null here (mifft_launch_pass refuses that first), so the forms ask for none.
int select_nd(const mifft_pass* p, int aliased) {
    const bool f64 = p->precision == MIFFT_F64, small_launch = (p->flags & MIFFT_FLAG_WRITE_THROUGH) != 0;
    const int x = p->L, y = (int)p->M, z = (int)p->S;
    const bool interleaved = !planes_in(p) && !planes_out(p), planes = planes_in(p) && planes_out(p);
    // the (16, 16) fp32 plane, interleaved: wave-autonomous kernel (no LDS, DPP exchange; csrc/fft_wave.hpp)
    // -- measured slower than the fixed-shape LDS kernel at the reference's 32 MiB buffer (0.62 vs 0.68 of the roofline) and
    // equal at 128 MiB (profiles/r02_h_small_n.log), so it only runs on request (MIFFT_DEBUG_FORCE_WAVE; parity-tested)
    if (!f64 && x == 16 && y == 16 && z == 1 && g_debug[MIFFT_DEBUG_FORCE_WAVE] && interleaved) return MIFFT_ND_KERNEL_WAVE;
    // variant 1 of the pass: the run-time-shaped kernel only (the plan asks for it where that kernel measured faster than the shape's
    // fixed instance: pyfft_amd/tuning_gfx950.json, "nd_generic")
    if (p->variant != 1) {
        if (interleaved) {
            // the one-tile-per-CU shapes always, the two-per-CU shapes in small launches, and shapes without a fixed instance
            const bool have_nd2 = nd2_instance(f64, x, y, z);
            if (!(aliased & 1) && nd2z_gate(f64, x, y, z, have_nd2 && !small_launch ? 2 : 1)) return MIFFT_ND_KERNEL_ND2Z;
            if (have_nd2 && g_debug[MIFFT_DEBUG_NO_ND2] == 0) return MIFFT_ND_KERNEL_ND2;
        }
        if (planes && !(aliased & 3) && nd2zp_gate(f64, x, y, z, 1)) return MIFFT_ND_KERNEL_ND2ZP;
        if (planes && nd2p_gate(f64, x, y, z, small_launch ? 2 : 1)) return MIFFT_ND_KERNEL_ND2P;
        if (planes_in(p) && nd2t_gate(f64, x, y, z, 128)) return MIFFT_ND_KERNEL_ND2T;
    }
    if ((long long)p->L * p->M * p->S > mifft_nd_max_points(f64))
        return set_err(MIFFT_E_UNSUPPORTED, "ND pass %d x %d x %d: this shape has a one-launch kernel out of place only, for interleaved data or planes on both sides "
                       "(several work-groups per transform, mifft_nd_shape_supported with MIFFT_VARIANT_OUT_OF_PLACE_ONLY / _SPLIT_OUT_OF_PLACE)",
                       z, y, x);
    return MIFFT_ND_KERNEL_ND;
}

int launch_nd(const mifft_pass* p, const void* in0, const void* in1, void* out0, void* out1, hipStream_t s) {
    const int form = select_nd(p, (in0 == out0 ? 1 : 0) | (in1 == out1 ? 2 : 0));
    if (form < 0) return form;
    const bool f64 = p->precision == MIFFT_F64;
    const int x = p->L, y = (int)p->M, z = (int)p->S;
    if (form == MIFFT_ND_KERNEL_WAVE) {
        mifft::WaveArgs w;
        w.in = in0; w.out = out0;
        w.pieces = p->outer * 128;
        w.inverse = p->inverse ? 1 : 0;
        w.nt = stream_policy(p->flags);
        w.scale = p->scale;
        return hip_check((hipError_t)mifft_wave_16x16_launch(&w, wave_max_blocks(), s), "kernel launch");
    }
    if (form == MIFFT_ND_KERNEL_ND) {
        mifft::NdArgs a;
        memset(&a, 0, sizeof(a));
        a.in0 = in0; a.in1 = in1; a.out0 = out0; a.out1 = out1;
        a.tw[0] = p->tw_L; a.tw[1] = p->tw_lo; a.tw[2] = p->tw_hi;
        const long long dims[3] = {p->L, p->M, p->S};
        a.total = p->outer * dims[0] * dims[1] * dims[2];
        if (nd_stage_list(dims, f64, &a) != 0) return set_err(MIFFT_E_UNSUPPORTED, "ND pass: too many stages");
        a.split = planes_in(p) ? 1 : 0;
        a.split_out = planes_out(p) ? 1 : 0;
        if (a.split_out) a.edge_out = 0;
        a.inverse = p->inverse ? 1 : 0;
        a.scale = p->scale;
        // small launches: write-through stores of the result (the store phase -- planes always go through it; an interleaved result that
        // leaves by the register edge keeps plain stores).  MIFFT_NARROW_TILES = 1: off (A/B)
        a.wt = ((stream_policy(p->flags) & 4) && g_debug[MIFFT_DEBUG_NARROW_TILES] != 1) ? 1 : 0;
        return launched(mifft_nd_launch(f64 ? 1 : 0, dims[0] * dims[1] * dims[2], &a, s));
    }
    mifft::TileArgs t;
    memset(&t, 0, sizeof(t));
    t.in0 = in0; t.in1 = in1; t.out0 = out0; t.out1 = out1;
    t.split = planes_in(p) ? 1 : 0;
    t.split_out = planes_out(p) ? 1 : 0;
    t.tw_L = p->tw_L; t.tw_lo = p->tw_lo; t.tw_hi = p->tw_hi;
    t.total = p->outer * p->L * p->M * p->S;
    t.inverse = p->inverse ? 1 : 0;
    t.scale = p->scale;
    t.nt = stream_policy(p->flags);
    if (form == MIFFT_ND_KERNEL_ND2Z) return launched(mifft_nd2z(f64 ? 1 : 0, x, y, z, &t, s, 0));
    if (form == MIFFT_ND_KERNEL_ND2) return launched(f64 ? mifft_nd2_f64_launch(x, y, z, &t, s) : mifft_nd2_f32_launch(x, y, z, &t, s));
    if (form == MIFFT_ND_KERNEL_ND2ZP) return launched(mifft_nd2zp(f64 ? 1 : 0, x, y, z, &t, s, 0));
    if (form == MIFFT_ND_KERNEL_ND2P) return launched(mifft_nd2p(f64 ? 1 : 0, x, y, z, &t, s, 0));
    // the tiled kernel on a dense batch: one tile per "parent"; it counts tiles, not points, and knows the write-through form of the
    // small launches only
    t.total = 0;
    t.nt &= 4;
    mifft::TiledGeom g;
    g.pitch_y = p->L; g.pitch_z = (long long)p->L * p->M; g.parent = (long long)p->L * p->M * p->S; g.tiles = p->outer;
    g.cx = g.cy = g.cz = 1;
    return launched((planes_out(p) ? mifft_nd2t_split : mifft_nd2t_split_in)(f64, x, y, z, &t, &g, s, 0));
}

int dispatch(const mifft_pass* p, const mifft::TileArgs* a, hipStream_t s, int query_only) {
    const int tr = (p->kind == MIFFT_PASS_COL && p->S == 1) ? 1 : 0;
    int rc;
    // short dense interleaved rows: wave-autonomous kernel (no LDS, DPP exchange; csrc/fft_wave.hpp)
    // up to 128 MiB per side (both sides then fit the 256 MiB Infinity Cache: 0.72-0.84 of the roofline against 0.57-0.69
    // for the LDS-staged kernels at the reference's 32 MiB buffer, 0.90-0.99 against 0.83-0.90 at 128 MiB); larger
    // buffers are HBM-bound and the LDS kernels are 0-5 points ahead (profiles/r02_h_small_n.log)
    if (!query_only && p->kind == MIFFT_PASS_ROW && a && !a->split && !a->split_out && a->ostride_in == p->L &&
        a->ostride_out == p->L && !g_debug[MIFFT_DEBUG_NO_WAVE] && mifft_wave_supported(p->precision == MIFFT_F64, p->L) == 0 &&
        (g_debug[MIFFT_DEBUG_FORCE_WAVE] ||
         (wave_bytes(p, a) <= (128ll << 20) && !(p->precision == MIFFT_F32 && p->L == 32 && wave_bytes(p, a) < (64ll << 20))))) {
        mifft::WaveArgs w;
        w.in = a->in0; w.out = a->out0;
        w.pieces = a->total * p->L * (p->precision == MIFFT_F64 ? 16 : 8) / 16;
        w.inverse = a->inverse;
        w.nt = a->nt;
        w.scale = a->scale;
        rc = mifft_wave_launch(p->precision == MIFFT_F64, p->L, &w, wave_max_blocks(), s);
        return hip_check((hipError_t)rc, "kernel launch");
    }
    if (p->kind == MIFFT_PASS_COL)
        rc = p->precision == MIFFT_F32 ? mifft_dispatch_col_f32(p->L, tr, p->variant, a, s, query_only)
                                       : mifft_dispatch_col_f64(p->L, tr, p->variant, a, s, query_only);
    else
        rc = p->precision == MIFFT_F32 ? mifft_dispatch_row_f32(p->L, p->variant, a, s, query_only)
                                       : mifft_dispatch_row_f64(p->L, p->variant, a, s, query_only);
    if (rc == MIFFT_E_UNSUPPORTED)
        return set_err(rc, "no compiled kernel for kind=%d precision=%d L=%d variant=%d", p->kind, p->precision, p->L, p->variant);
    return launched(rc);
}

// ---- pass pairs (fft_pair.hpp) -------------------------------------------------------------------------------------
// kind 0 = XY (ROW x + COL y R0), kind 1 = YZ (COL y R1 + COL z); keys as in mifft_pair_f64; *split = the user-facing side of
// the launch is two scalar planes (XY: its input, YZ: its output; the side between the two launches is always interleaved).
// Returns 0 and fills kind / keys / split, or MIFFT_E_UNSUPPORTED when (p0, p1) is not a pair shape.
int classify_pair(const mifft_pass* p0, const mifft_pass* p1, int* kind, int key[3], int* split) {
    if (!p0 || !p1) return MIFFT_E_INVALID;
    if (p0->precision != p1->precision || p0->inverse != p1->inverse || p0->layout != p1->layout) return MIFFT_E_UNSUPPORTED;
    const bool inter_in = p0->layout != MIFFT_SPLIT || (p0->flags & MIFFT_FLAG_SRC_INTERLEAVED);
    const bool inter_out = p1->layout != MIFFT_SPLIT || (p1->flags & MIFFT_FLAG_DST_INTERLEAVED);
    if (p0->kind == MIFFT_PASS_ROW && p1->kind == MIFFT_PASS_COL && p1->M > 1 && p1->S == p0->L) {
        const long long plane = (long long)p0->L * p1->L * p1->M;            // nx * ny
        if (!inter_out || p1->outer_stride_in != plane || p1->outer_stride_out != plane || p0->outer != p1->outer * p1->L * p1->M ||
            p0->outer_stride_in != p0->L || p0->outer_stride_out != p0->L || p1->M > (1 << 20))
            return MIFFT_E_UNSUPPORTED;
        *kind = 0;
        *split = inter_in ? 0 : 1;
        key[0] = p0->L; key[1] = p1->L; key[2] = (int)p1->M;
        return 0;
    }
    if (p0->kind == MIFFT_PASS_COL && p1->kind == MIFFT_PASS_COL && p0->M == 1 && p1->M == 1 && p1->S == p0->S * p0->L) {
        const long long xform = p1->S * p1->L;                                // nx * ny * nz
        if (!inter_in || p1->outer_stride_in != xform || p1->outer_stride_out != xform || p0->outer != p1->outer * p1->L ||
            p0->outer_stride_in != p1->S || p0->outer_stride_out != p1->S || p0->S > (1 << 30))
            return MIFFT_E_UNSUPPORTED;
        *kind = 1;
        *split = inter_out ? 0 : 1;
        key[0] = (int)p0->S; key[1] = p0->L; key[2] = p1->L;
        return 0;
    }
    return MIFFT_E_UNSUPPORTED;
}

int pair_call(int precision, int kind, const int key[3], int split, const mifft::PairArgs* a, hipStream_t s, int query, int* width) {
    if (precision == MIFFT_F64) return mifft_pair_f64(kind, key[0], key[1], key[2], split, a, s, query, width);
    if (precision == MIFFT_F32) return mifft_pair_f32(kind, key[0], key[1], key[2], split, a, s, query, width);
    return MIFFT_E_UNSUPPORTED;
}

// Last-level cache size and XCD count of a HIP device: HIP has no attribute for either, the HSA agent behind the device has
// (matched by PCI domain / bus / device / function).  HSA is already initialised by the HIP runtime; hsa_init / hsa_shut_down only
// move its reference count.
struct HsaProbe {
    uint32_t domain, bdf;
    uint32_t cache[4];
    uint32_t xcc;
    bool found;
};
hsa_status_t hsa_probe_agent(hsa_agent_t agent, void* data) {
    HsaProbe* p = static_cast<HsaProbe*>(data);
    hsa_device_type_t type;
    if (hsa_agent_get_info(agent, HSA_AGENT_INFO_DEVICE, &type) != HSA_STATUS_SUCCESS || type != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
    uint32_t bdf = 0, domain = 0;
    if (hsa_agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    (void)hsa_agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &domain);
    if (bdf != p->bdf || domain != p->domain) return HSA_STATUS_SUCCESS;
    uint32_t cache[4] = {0, 0, 0, 0}, xcc = 0;
    if (hsa_agent_get_info(agent, HSA_AGENT_INFO_CACHE_SIZE, cache) == HSA_STATUS_SUCCESS) memcpy(p->cache, cache, sizeof(cache));
    if (hsa_agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_NUM_XCC, &xcc) == HSA_STATUS_SUCCESS) p->xcc = xcc;
    p->found = true;
    return HSA_STATUS_INFO_BREAK;
}
void probe_memory_system(const hipDeviceProp_t& hp, int64_t* llc_bytes, int32_t* num_xcc) {
    HsaProbe probe;
    memset(&probe, 0, sizeof(probe));
    probe.domain = (uint32_t)hp.pciDomainID;
    probe.bdf = ((uint32_t)hp.pciBusID << 8) | ((uint32_t)hp.pciDeviceID << 3);
    if (hsa_init() == HSA_STATUS_SUCCESS) {
        (void)hsa_iterate_agents(hsa_probe_agent, &probe);
        (void)hsa_shut_down();
    }
    *llc_bytes = probe.found ? (int64_t)probe.cache[2] : 0;
    *num_xcc = (probe.found && probe.xcc >= 1) ? (int32_t)probe.xcc : 0;
    // a partition (CPX / DPX / QPX: an agent of 1, 2 or 4 of the 8 XCDs) may still report the whole part's Infinity Cache; the other
    // partitions stream through it too, so the planner gets this agent's FAIR SHARE (not verified on partitioned hardware: the sizes
    // derived from it are only ever too small, never too large)
    if (probe.found && probe.xcc >= 1 && probe.xcc < 8 && hp.multiProcessorCount < 228 && *llc_bytes >= (int64_t)(256ll << 20) &&
        (strncmp(hp.gcnArchName, "gfx94", 5) == 0 || strncmp(hp.gcnArchName, "gfx95", 5) == 0))
        *llc_bytes = *llc_bytes * (int64_t)probe.xcc / 8;
    if (*llc_bytes == 0 && (strncmp(hp.gcnArchName, "gfx94", 5) == 0 || strncmp(hp.gcnArchName, "gfx95", 5) == 0)) {
        // no answer from HSA on a CDNA3/4 part: the documented 256 MiB per 8 XCDs, scaled to the partition this device is
        *llc_bytes = (int64_t)(256ll << 20) * (hp.multiProcessorCount >= 228 ? 8 : (hp.multiProcessorCount + 37) / 38) / 8;
    }
    if (*num_xcc == 0) *num_xcc = hp.multiProcessorCount >= 228 ? 8 : (hp.multiProcessorCount >= 64 ? hp.multiProcessorCount / 32 : 1);
}

// which kernel runs dense smooth rows of n points by default (profiles/r04_j_mixed_rows_ab.log): fp64 the single-buffer tile kernel
// (N = 1000 0.503 -> 0.569, 2000 0.382 -> 0.460, 100 0.661 -> 0.685); fp32 the two-buffer row kernel (N = 1000 0.513 against 0.445)
// except for the longest rows, which fill its tile alone (N = 4000 0.279 -> 0.337; 3125 0.313 / 0.305, 3000 0.340 / 0.316)
bool mixed_rows_prefer_nd(bool f64, int n) {
    return f64 || n > 3200;
}

// keys 1, 4 and 11 are retired: they selected kernel forms this library no longer has (include/mifft.h)
bool debug_key_ok(int key) { return key >= 0 && key < MIFFT_DEBUG_KEYS && key != 1 && key != 4 && key != 11; }

// The kernel form of a persistent two-pass launch (mifft_fused2_kernel, mifft_launch_fused2): validates the two descriptors, then a
// pure function of them and of the calling thread's development switches.  Which shapes have a kernel, and on which tiles, is asked
// of the units -- each answers from the list it launches from (mifft_internal.h) -- in the order of preference; 0 with *c filled, or a
// negative error code with its message.
int select_fused2(const mifft_pass* p0, const mifft_pass* p1, mifft_fused2_choice* c) {
    int rc = validate(p0);
    if (!rc) rc = validate(p1);
    if (rc) return rc;
    if (p0->precision != p1->precision) return set_err(MIFFT_E_INVALID, "fused2: passes of two precisions");
    const bool f64 = p0->precision == MIFFT_F64;
    const int split = p0->layout == MIFFT_SPLIT ? 1 : 0;
    auto has = [&](mifft_fused2_unit* unit, int a, int b) { return (rc = unit(a, b, split, nullptr, 0, nullptr, 1, c)) == 0; };
    if (p0->kind == MIFFT_PASS_ROW) {
        // 2-D form: the ROW pass (x axis, length nx) and the strided COL pass (y axis, length ny) of a 2-D plan: the row-first kernel,
        // else two transposing column passes -- on 32-column tiles, else on the tiles of the precision's 2-D launcher
        const int nx = p0->L, ny = p1->L;
        const bool plan2d = p1->kind == MIFFT_PASS_COL && p1->S == nx && p1->M == 1 && p0->outer == p1->outer * ny &&
                            p0->layout == p1->layout && p0->inverse == p1->inverse;
        if (plan2d && (f64 ? has(mifft_fused3d_f64, ny, nx) : has(mifft_fused2r_f32, ny, nx) || has(mifft_fused2dw_f32, ny, nx) || has(mifft_fused2d_f32, ny, nx)))
            return 0;
        if (!plan2d || rc != MIFFT_E_UNSUPPORTED)
            return set_err(MIFFT_E_UNSUPPORTED, "fused2: the 2-D form takes (ny, nx) in {512, 1024, 2048}^2 (fp32; interleaved: also a 256-point side next to one <= 1024; split planes: {256, 512, 1024}^2 and the 2048 square) / {256, 512, 1024}^2 (fp64; split planes: 1024 x 1024; 256 only next to <= 512)");
    } else {
        if (p0->kind != MIFFT_PASS_COL || p1->kind != MIFFT_PASS_COL || p0->S != 1 || p0->M != p1->L || p1->M != 1 ||
            p1->S != p0->L || p0->outer != p1->outer || p0->layout != p1->layout || p0->inverse != p1->inverse)
            return set_err(MIFFT_E_INVALID, "fused2: passes are not the two passes of one long contiguous axis");
        // 32-column and mixed tiles, the fp64 stage-chain tiles, else the tiles of the precision's 1-D launcher
        if (f64 ? has(mifft_fusedx_f64, p0->L, p1->L) || has(mifft_fused3_f64, p0->L, p1->L)
                : has(mifft_fused2w_f32, p0->L, p1->L) || has(mifft_fused2_f32, p0->L, p1->L))
            return 0;
    }
    return set_err(MIFFT_E_UNSUPPORTED, "fused2: no kernel for %d x %d", p0->L, p1->L);
}

// work-list control block of a persistent launch from the caller's mifft_fused_sync (include/mifft.h): validates, zeroes the
// counters on `stream` when the caller does not alternate between two sets
int fill_ctl(mifft::FusedCtl* c, const mifft_fused_sync* sync, long long outer, int lag, int ring_slots, unsigned tiles0, unsigned tiles1,
             hipStream_t stream, const char* who) {
    static_assert(mifft::kFusedCS == MIFFT_FUSED2_COUNTER_STRIDE, "counter stride");
    if (!sync || !sync->counters) return set_err(MIFFT_E_INVALID, "%s: null counters", who);
    if (misaligned(255, {sync->counters, sync->counters_next})) return set_err(MIFFT_E_INVALID, "%s: counter buffers must be 256-byte aligned", who);
    if (misaligned(3, {sync->error_word})) return set_err(MIFFT_E_INVALID, "%s: misaligned error word", who);
    if (sync->counters_next == sync->counters) return set_err(MIFFT_E_INVALID, "%s: counters_next must be a second buffer", who);
    if (outer > 0x3fffffff) return set_err(MIFFT_E_INVALID, "%s: batch too large", who);
    if (sync->counters_next) {
        // the launch zeroes words 0 and 1 of EVERY line of counters_next -- word 1 of line 0 is the default error word of the launch
        // that ran on that set, so a time-out report would vanish with the next launch
        if (!sync->error_word) return set_err(MIFFT_E_INVALID, "%s: alternating counter sets need an error word of their own", who);
        // a CAPTURED launch replays on the same set every time, while the two-set form relies on the host alternating the sets per
        // launch: the second replay would start on non-zero counters.  Captured launches take the single-set form, whose memset
        // becomes a node of the graph in front of the kernel
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &st) == hipSuccess && st == hipStreamCaptureStatusActive)
            return set_err(MIFFT_E_INVALID, "%s: a launch on a capturing stream must use the single-set form (counters_next = NULL)", who);
    }
    c->counters = (unsigned*)sync->counters;
    c->counters_next = (unsigned*)sync->counters_next;
    c->err = sync->error_word ? (unsigned*)sync->error_word : (unsigned*)sync->counters + 1;
    c->lines = (unsigned)(9 + 2 * outer);
    c->batch = (unsigned)outer;
    c->lag = (unsigned)lag;
    c->ring = (unsigned)ring_slots;
    c->tiles0 = tiles0;
    c->tiles1 = tiles1;
    if (!sync->counters_next) {
        // single-set form: zero the set in front of the launch.  On a CAPTURING stream with a kernel of our own (a kernel node) instead
        // of a memset node: see mifft_aux_zero_launch (csrc/fft_aux.hip)
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &st) == hipSuccess && st == hipStreamCaptureStatusActive) {
            const int rz = mifft_aux_zero_launch(sync->counters, MIFFT_FUSED2_COUNTER_BYTES(outer), stream);
            return hip_check((hipError_t)rz, "kernel launch");
        }
        return hip_check(hipMemsetAsync(sync->counters, 0, MIFFT_FUSED2_COUNTER_BYTES(outer), stream), "hipMemsetAsync");
    }
    return 0;
}

// the f32 or the f64 dispatcher of an extension row family (real, convolution, cosine / sine rows)
template <typename F> F* row_dispatcher(int32_t precision, F* f32, F* f64) { return precision == MIFFT_F64 ? f64 : f32; }

}  // namespace

extern "C" {

int mifft_abi_version(void) { return MIFFT_ABI_VERSION; }
int mifft_debug_set(int32_t key, int32_t value) {
    if (!debug_key_ok(key)) return set_err(MIFFT_E_INVALID, "bad debug key %d", key);
    t_debug_value[key] = value;
    t_debug_mask |= 1u << key;
    return 0;
}
int mifft_debug_set_default(int32_t key, int32_t value) {
    if (!debug_key_ok(key)) return set_err(MIFFT_E_INVALID, "bad debug key %d", key);
    g_debug_default[key].store(value, std::memory_order_relaxed);
    return 0;
}
int mifft_debug_get(int32_t key) { return (key >= 0 && key < MIFFT_DEBUG_KEYS) ? g_debug[key] : 0; }
void mifft_note_pair_lanes_form(int form) { t_pair_lanes_form = form; }
int mifft_debug_last_pair_lanes_form(void) { return t_pair_lanes_form; }
const char* mifft_last_error(void) { return g_err; }

int mifft_device_count(int* count) {
    if (!count) return set_err(MIFFT_E_INVALID, "null argument");
    hipError_t e = hipGetDeviceCount(count);
    if (e == hipErrorNoDevice) {
        *count = 0;
        (void)hipGetLastError();
        return 0;
    }
    return hip_check(e, "hipGetDeviceCount");
}
int mifft_set_device(int device) { return hip_check(hipSetDevice(device), "hipSetDevice"); }
int mifft_get_device(int* device) { return hip_check(hipGetDevice(device), "hipGetDevice"); }

int mifft_device_props_get(int device, mifft_device_props* props) {
    if (!props) return set_err(MIFFT_E_INVALID, "null argument");
    hipDeviceProp_t p;
    int rc = hip_check(hipGetDeviceProperties(&p, device), "hipGetDeviceProperties");
    if (rc) return rc;
    memset(props, 0, sizeof(*props));
    snprintf(props->name, sizeof(props->name), "%s", p.name);
    snprintf(props->gcn_arch, sizeof(props->gcn_arch), "%s", p.gcnArchName);
    props->compute_units = p.multiProcessorCount;
    props->wavefront_size = p.warpSize;
    props->max_threads_per_block = p.maxThreadsPerBlock;
    props->max_grid_x = p.maxGridSize[0];
    props->lds_bytes_per_block = (int64_t)p.sharedMemPerBlock;
    props->total_mem_bytes = (int64_t)p.totalGlobalMem;
    props->clock_khz = p.clockRate;
    props->l2_bytes = p.l2CacheSize;
    probe_memory_system(p, &props->llc_bytes, &props->num_xcc);
    return 0;
}

int mifft_malloc(void** ptr, size_t nbytes) {
    if (!ptr) return set_err(MIFFT_E_INVALID, "null argument");
    return hip_check(hipMalloc(ptr, nbytes ? nbytes : 1), "hipMalloc");
}
int mifft_free(void* ptr) { return hip_check(hipFree(ptr), "hipFree"); }
int mifft_memset(void* ptr, int value, size_t nbytes, mifft_stream_t stream) {
    return hip_check(hipMemsetAsync(ptr, value, nbytes, (hipStream_t)stream), "hipMemsetAsync");
}
int mifft_memcpy_h2d(void* dst, const void* src, size_t nbytes, mifft_stream_t stream) {
    int rc = hip_check(hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync(h2d)");
    if (rc) return rc;
    return hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
}
int mifft_memcpy_d2h(void* dst, const void* src, size_t nbytes, mifft_stream_t stream) {
    int rc = hip_check(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync(d2h)");
    if (rc) return rc;
    return hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
}
int mifft_memcpy_d2d(void* dst, const void* src, size_t nbytes, mifft_stream_t stream) {
    return hip_check(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "hipMemcpyAsync(d2d)");
}
int mifft_stream_create(mifft_stream_t* stream) {
    if (!stream) return set_err(MIFFT_E_INVALID, "null argument");
    hipStream_t s;
    // a BLOCKING stream, like PyCUDA's (cuda.py:94-96): null-stream copies (DeviceArray.get/set, the reference quick-start
    // doc/source/index.rst:61-92) and a framework's default-stream kernels order against the plan's work without a sync
    int rc = hip_check(hipStreamCreateWithFlags(&s, hipStreamDefault), "hipStreamCreate");
    if (rc) return rc;
    *stream = (mifft_stream_t)s;
    return 0;
}
int mifft_host_alloc(void** ptr, size_t nbytes) {
    if (!ptr) return set_err(MIFFT_E_INVALID, "null argument");
    return hip_check(hipHostMalloc(ptr, nbytes ? nbytes : 1, hipHostMallocDefault), "hipHostMalloc");
}
int mifft_host_free(void* ptr) { return hip_check(hipHostFree(ptr), "hipHostFree"); }
int mifft_memcpy_d2h_async(void* dst, const void* src, size_t nbytes, mifft_stream_t stream) {
    return hip_check(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync(d2h)");
}
int mifft_event_query(mifft_event_t event) {
    const hipError_t e = hipEventQuery((hipEvent_t)event);
    if (e == hipSuccess) return 0;
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        return 1;
    }
    return hip_check(e, "hipEventQuery");
}
int mifft_stream_wait_event(mifft_stream_t stream, mifft_event_t event) {
    return hip_check(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0), "hipStreamWaitEvent");
}
int mifft_stream_destroy(mifft_stream_t stream) { return hip_check(hipStreamDestroy((hipStream_t)stream), "hipStreamDestroy"); }
int mifft_stream_sync(mifft_stream_t stream) { return hip_check(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize"); }
int mifft_stream_is_capturing(mifft_stream_t stream, int32_t* capturing) {
    if (!capturing) return set_err(MIFFT_E_INVALID, "null argument");
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    const int rc = hip_check(hipStreamIsCapturing((hipStream_t)stream, &st), "hipStreamIsCapturing");
    if (rc) return rc;
    *capturing = st == hipStreamCaptureStatusActive ? 1 : 0;
    return 0;
}
int mifft_stream_begin_capture(mifft_stream_t stream) {
    if (!stream) return set_err(MIFFT_E_INVALID, "the default stream cannot be captured");
    return hip_check(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeRelaxed), "hipStreamBeginCapture");
}
int mifft_stream_end_capture(mifft_stream_t stream, mifft_graph_t* graph) {
    if (!graph) return set_err(MIFFT_E_INVALID, "null argument");
    hipGraph_t g = nullptr;
    int rc = hip_check(hipStreamEndCapture((hipStream_t)stream, &g), "hipStreamEndCapture");
    if (rc) return rc;
    hipGraphExec_t ge = nullptr;
    rc = hip_check(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0), "hipGraphInstantiate");
    (void)hipGraphDestroy(g);
    if (rc) return rc;
    *graph = (mifft_graph_t)ge;
    return 0;
}
int mifft_graph_launch(mifft_graph_t graph, mifft_stream_t stream) {
    if (!graph) return set_err(MIFFT_E_INVALID, "null graph");
    return hip_check(hipGraphLaunch((hipGraphExec_t)graph, (hipStream_t)stream), "hipGraphLaunch");
}
int mifft_graph_destroy(mifft_graph_t graph) {
    if (!graph) return 0;
    return hip_check(hipGraphExecDestroy((hipGraphExec_t)graph), "hipGraphExecDestroy");
}
int mifft_device_sync(void) { return hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize"); }
int mifft_event_create(mifft_event_t* event) {
    if (!event) return set_err(MIFFT_E_INVALID, "null argument");
    hipEvent_t e;
    int rc = hip_check(hipEventCreate(&e), "hipEventCreate");
    if (rc) return rc;
    *event = (mifft_event_t)e;
    return 0;
}
int mifft_event_destroy(mifft_event_t event) { return hip_check(hipEventDestroy((hipEvent_t)event), "hipEventDestroy"); }
int mifft_event_record(mifft_event_t event, mifft_stream_t stream) {
    return hip_check(hipEventRecord((hipEvent_t)event, (hipStream_t)stream), "hipEventRecord");
}
int mifft_event_sync(mifft_event_t event) { return hip_check(hipEventSynchronize((hipEvent_t)event), "hipEventSynchronize"); }
int mifft_event_elapsed_ms(float* ms, mifft_event_t start, mifft_event_t stop) {
    return hip_check(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop), "hipEventElapsedTime");
}

int mifft_nd_max_points_for(int32_t precision) { return mifft_nd_max_points(precision == MIFFT_F64); }

int mifft_nd_shape_supported(int32_t precision, int32_t x, int32_t y, int32_t z, int32_t variant) {
    if (bad_precision(precision)) return MIFFT_E_UNSUPPORTED;
    if (x < 1 || y < 1 || z < 1 || (x & (x - 1)) || (y & (y - 1)) || (z & (z - 1))) return MIFFT_E_UNSUPPORTED;
    const long long n = (long long)x * y * z;
    if (n <= mifft_nd_max_points(precision == MIFFT_F64)) return 0;
    const bool f64 = precision == MIFFT_F64;
    bool ok = false;
    if (variant == MIFFT_VARIANT_SPLIT_ONLY)      // planes on both sides: the tiled kernel where it beats two passes, or a dense planes instance
        ok = nd2t_gate(f64, x, y, z, 256) || nd2p_gate(f64, x, y, z, 1);
    else if (variant == MIFFT_VARIANT_OUT_OF_PLACE_ONLY || variant == MIFFT_VARIANT_OUT_OF_PLACE_ANY_SIZE)      // interleaved AND out of place
        ok = nd2z_gate(f64, x, y, z, variant == MIFFT_VARIANT_OUT_OF_PLACE_ONLY ? 1 : 2);
    else if (variant == MIFFT_VARIANT_SPLIT_OUT_OF_PLACE || variant == MIFFT_VARIANT_SPLIT_OUT_OF_PLACE_ANY_SIZE)   // planes AND out of place
        ok = nd2zp_gate(f64, x, y, z, variant == MIFFT_VARIANT_SPLIT_OUT_OF_PLACE ? 1 : 2);
    else if (variant == MIFFT_VARIANT_INTERLEAVED_ONLY)
        ok = nd2_instance(f64, x, y, z);
    return ok ? 0 : MIFFT_E_UNSUPPORTED;
}

int mifft_pass_supported(int32_t kind, int32_t precision, int32_t L, int32_t variant) {
    if (kind == MIFFT_PASS_ND) return (L >= 1 && L <= mifft_nd_max_points(precision == MIFFT_F64) && (L & (L - 1)) == 0) ? 0 : MIFFT_E_UNSUPPORTED;
    mifft_pass p;
    memset(&p, 0, sizeof(p));
    p.kind = kind;
    p.precision = precision;
    p.L = L;
    p.variant = variant;
    p.M = 1;
    p.S = (kind == MIFFT_PASS_COL) ? 2 : 1;
    int rc0 = dispatch(&p, nullptr, nullptr, 1);
    if (rc0 || kind != MIFFT_PASS_COL) return rc0;
    p.S = 1;  // transposing form
    p.M = 2;
    return dispatch(&p, nullptr, nullptr, 1);
}

// what mifft_launch_pass checks once the descriptor is valid and before it looks at a pointer
static int check_strides(const mifft_pass* p) {
    if ((p->outer_stride_in | p->outer_stride_out) & 1) return set_err(MIFFT_E_INVALID, "outer strides must be even");
    return 0;
}

int mifft_nd_kernel(const mifft_pass* p, int32_t aliased) {
    int rc = validate(p);
    if (rc) return rc;
    if (p->kind != MIFFT_PASS_ND) return set_err(MIFFT_E_INVALID, "mifft_nd_kernel: not an ND pass");
    rc = check_strides(p);
    if (rc) return rc;
    return select_nd(p, planes_in(p) && planes_out(p) ? aliased & 3 : aliased & 1);
}

int mifft_launch_pass(const mifft_pass* p, const void* in0, const void* in1, void* out0, void* out1, mifft_stream_t stream) {
    int rc = validate(p);
    if (rc) return rc;
    if (!in0 || !out0) return set_err(MIFFT_E_INVALID, "null data buffer");
    const bool split_in = planes_in(p), split_out = planes_out(p);
    if ((split_in && !in1) || (split_out && !out1)) return set_err(MIFFT_E_INVALID, "split layout needs imaginary planes");
    if (p->layout != MIFFT_SPLIT && (in1 || out1)) return set_err(MIFFT_E_INVALID, "interleaved layout takes no imaginary planes");
    if (!split_in) in1 = nullptr;
    if (!split_out) out1 = nullptr;
    if (misaligned(15, {in0, out0, in1, out1})) return set_err(MIFFT_E_INVALID, "data buffers must be 16-byte aligned");
    rc = check_strides(p);
    if (rc) return rc;
    if (p->kind == MIFFT_PASS_COL && p->M > 1 && (in0 == out0 || (split_in && split_out && in1 == out1)))
        return set_err(MIFFT_E_INVALID, "a COL pass with M > 1 cannot run in place");
    if (p->outer == 0) return 0;

    if (p->kind == MIFFT_PASS_ND) {
        if ((p->outer * p->L * p->M * p->S) & 3) return set_err(MIFFT_E_INVALID, "ND pass: total points must be a multiple of 4");
        return launch_nd(p, in0, in1, out0, out1, (hipStream_t)stream);
    }
    mifft::TileArgs a;
    fill_args(p, in0, in1, out0, out1, &a);
    return dispatch(p, &a, (hipStream_t)stream, 0);
}


int mifft_pair_split(int32_t precision, int32_t layout, int32_t x, int32_t y, int32_t z) {
    if (x < 2 || y < 2 || z < 2 || !is_pow2(x) || !is_pow2(y) || !is_pow2(z)) return 0;
    const int split = layout == MIFFT_SPLIT ? 1 : 0;
    // the development switch "no pass pairs" acts HERE, when a plan is built, and nowhere else: a plan that was built with pairs
    // keeps launching them whatever the switch says later
    if (g_debug[MIFFT_DEBUG_PAIR] == 1) return 0;
    // candidates in order of preference (measured: profiles/r03_b_c4_pair_split.log); MIFFT_DEBUG_PAIR = 2 swaps them
    int cand[2] = {32, 64};
    if (g_debug[MIFFT_DEBUG_PAIR] == 2) { cand[0] = 64; cand[1] = 32; }
    for (int r0 : cand) {
        if (y % r0 || y / r0 < 2) continue;
        const int kxy[3] = {x, r0, y / r0}, kyz[3] = {x * r0, y / r0, z};
        if (pair_call(precision, 0, kxy, split, nullptr, nullptr, 1, nullptr) == 0 &&
            pair_call(precision, 1, kyz, split, nullptr, nullptr, 1, nullptr) == 0)
            return r0;
    }
    return 0;
}

int mifft_pair_kernel_supported(int32_t precision, int32_t layout, int32_t kind, int32_t k0, int32_t k1, int32_t k2) {
    if (bad_precision(precision) || (layout != MIFFT_INTERLEAVED && layout != MIFFT_SPLIT) || (kind != 0 && kind != 1))
        return MIFFT_E_UNSUPPORTED;
    if (g_debug[MIFFT_DEBUG_PAIR] == 1) return MIFFT_E_UNSUPPORTED;      // (as mifft_pair_split: the switch acts when a plan is built)
    const int key[3] = {k0, k1, k2};
    return pair_call(precision, kind, key, layout == MIFFT_SPLIT ? 1 : 0, nullptr, nullptr, 1, nullptr) == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}

int mifft_pass_pair_supported(const mifft_pass* p0, const mifft_pass* p1) {
    int kind, key[3], split;
    int rc = classify_pair(p0, p1, &kind, key, &split);
    if (rc) return MIFFT_E_UNSUPPORTED;
    return pair_call(p0->precision, kind, key, split, nullptr, nullptr, 1, nullptr) == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}

int mifft_launch_pass_pair(const mifft_pass* p0, const mifft_pass* p1, const void* in0, const void* in1, void* out0, void* out1,
                           mifft_stream_t stream) {
    int rc = validate(p0);
    if (rc) return rc;
    rc = validate(p1);
    if (rc) return rc;
    int kind, key[3], split;
    if (classify_pair(p0, p1, &kind, key, &split) != 0)
        return set_err(MIFFT_E_UNSUPPORTED, "pass pair: not a (ROW x, COL y) / (COL y, COL z) pair of a dense batch with an interleaved intermediate");
    if (!in0 || !out0) return set_err(MIFFT_E_INVALID, "null data buffer");
    if (split && ((kind == 0 && !in1) || (kind == 1 && !out1))) return set_err(MIFFT_E_INVALID, "split layout needs imaginary planes");
    if (misaligned(15, {in0, out0, in1, out1})) return set_err(MIFFT_E_INVALID, "data buffers must be 16-byte aligned");
    if (kind == 0 && in0 == out0) return set_err(MIFFT_E_INVALID, "the (ROW x, COL y) pair cannot run in place");
    if (p1->outer == 0) return 0;
    int width = 0;
    if (pair_call(p0->precision, kind, key, split, nullptr, nullptr, 1, &width) != 0)
        return set_err(MIFFT_E_UNSUPPORTED, "pass pair: no kernel for kind %d keys (%d, %d, %d) split %d", kind, key[0], key[1], key[2], split);
    mifft::PairArgs a;
    memset(&a, 0, sizeof(a));
    a.in0 = in0;
    a.in1 = (kind == 0 && split) ? in1 : nullptr;
    a.out0 = out0;
    a.out1 = (kind == 1 && split) ? out1 : nullptr;
    if (kind == 0) {
        a.tw[0] = p0->tw_L;   // w(nx)
        a.tw[1] = p1->tw_L;   // w(R0)
        a.tw_lo = p1->tw_lo;  // w(ny), two-level
        a.tw_hi = p1->tw_hi;
        a.tw_shift = p1->tw_shift;
        a.tiles = p1->outer * p1->M;                 // planes * R1
    } else {
        a.tw[1] = p0->tw_L;   // w(R1)
        a.tw[2] = p1->tw_L;   // w(nz)
        a.tiles = p1->outer * (p0->S / width);       // transforms * groups of `width` adjacent columns
    }
    a.inverse = p0->inverse ? 1 : 0;
    // streamed sides: non-temporal loads of the plan's input, PLAIN stores on both launches (BASELINE config 4 at batch 64, one
    // box: plain 13.31 ms, write-through 14.44 ms; non-temporal stores measured below plain ones at batch 16 --
    // profiles/r03_c_store_policy.log)
    a.nt = store_override(((p0->flags & MIFFT_FLAG_STREAM_SRC) ? 1 : 0) | ((p1->flags & MIFFT_FLAG_WRITE_THROUGH) ? 4 : 0));
    a.scale = p0->scale * p1->scale;
    return launched(pair_call(p0->precision, kind, key, split, &a, (hipStream_t)stream, 0, nullptr));
}

// one unit of a chain: a single pass, or a pass pair (MIFFT_FLAG_PAIR_WITH_NEXT on the first); *consumed = descriptors used
static int launch_unit(const mifft_pass* passes, int32_t i, int32_t npasses, const void* in0, const void* in1, void* out0, void* out1,
                       mifft_stream_t stream, int* consumed) {
    const mifft_pass* p = &passes[i];
    if (p->flags & MIFFT_FLAG_PAIR_WITH_NEXT) {
        if (i + 1 >= npasses) return set_err(MIFFT_E_INVALID, "pass %d: MIFFT_FLAG_PAIR_WITH_NEXT on the last pass", i);
        *consumed = 2;
        return mifft_launch_pass_pair(p, &passes[i + 1], in0, in1, out0, out1, stream);
    }
    *consumed = 1;
    return mifft_launch_pass(p, in0, in1, out0, out1, stream);
}

int mifft_launch_chain(const mifft_pass* passes, int32_t npasses, void* const bufs0[3], void* const bufs1[3], mifft_stream_t stream) {
    if (npasses < 0 || (npasses > 0 && !passes) || !bufs0) return set_err(MIFFT_E_INVALID, "bad chain arguments");
    for (int i = 0; i < npasses; ++i) {
        const mifft_pass* p = &passes[i];
        if (p->src < 0 || p->src > 2 || p->dst < 0 || p->dst > 2) return set_err(MIFFT_E_INVALID, "pass %d: bad buffer index", i);
    }
    for (int i = 0; i < npasses;) {
        const mifft_pass* p = &passes[i];
        const mifft_pass* pl = (p->flags & MIFFT_FLAG_PAIR_WITH_NEXT) && i + 1 < npasses ? &passes[i + 1] : p;   // the unit writes pl->dst
        const void* i1 = bufs1 ? bufs1[p->src] : nullptr;
        void* o1 = bufs1 ? bufs1[pl->dst] : nullptr;
        int used = 1;
        int rc = launch_unit(passes, i, npasses, bufs0[p->src], i1, bufs0[pl->dst], o1, stream, &used);
        if (rc) return rc;
        i += used;
    }
    return 0;
}

int mifft_fused2_kernel(const mifft_pass* p0, const mifft_pass* p1, uint32_t* tiles0, uint32_t* tiles1) {
    mifft_fused2_choice c;
    const int rc = select_fused2(p0, p1, &c);
    if (rc) return rc;
    if (tiles0) *tiles0 = c.tiles0;
    if (tiles1) *tiles1 = c.tiles1;
    return c.form;
}

int mifft_launch_fused2(const mifft_pass* p0, const mifft_pass* p1, const void* in0, const void* in1, void* out0, void* out1,
                        void* ring0, void* ring1, int32_t ring_slots, int32_t lag, const mifft_fused_sync* sync, int32_t grid,
                        mifft_stream_t stream) {
    mifft_fused2_choice c;
    int rc = select_fused2(p0, p1, &c);
    if (rc) return rc;
    const bool f64 = p0->precision == MIFFT_F64, split = p0->layout == MIFFT_SPLIT;
    if (!in0 || !out0 || !ring0 || (split && (!in1 || !out1))) return set_err(MIFFT_E_INVALID, "fused2: null buffer");
    (void)ring1;  // the ring is always interleaved
    if (grid < 1) return set_err(MIFFT_E_INVALID, "fused2: grid >= 1");
    if (ring_slots < 2 || lag < 1 || lag >= ring_slots) return set_err(MIFFT_E_INVALID, "fused2: need 1 <= lag < ring_slots");
    if (misaligned(15, {in0, out0, ring0, in1, out1}))
        return set_err(MIFFT_E_INVALID, "data buffers must be 16-byte aligned");
    if (p1->outer == 0) return 0;
    const int64_t n = (int64_t)p0->L * p1->L;
    mifft::FusedArgs f;
    fill_args(p0, in0, in1, ring0, nullptr, &f.p0);
    fill_args(p1, ring0, nullptr, out0, out1, &f.p1);
    f.p0.ostride_out = n;  // ring slot pitch
    f.p1.ostride_in = n;
    const bool twod = p0->kind == MIFFT_PASS_ROW;
    const int a = twod ? p1->L : p0->L, b = twod ? p0->L : p1->L;            // what the units are keyed on: (L0, L1) / (ny, nx)
    mifft_fused2_unit* unit = f64 ? mifft_fused3_f64 : mifft_fused2_f32;      // the 1-D launcher of the precision, on the descriptors as they are
    switch (c.form) {
        case MIFFT_FUSED2_KERNEL_2D_ROWFIRST:
            unit = mifft_fused2r_f32;
            f.p0.nt = 4;                // the ring is written through (the consumers acquire it, fft_fused2.hpp)
            f.p0.scale = p0->scale;
            f.p1.logMS = f.p1.logS = ilog2(p0->L);   // M = 1, S = nx
            f.p1.has_tw = 0;
            break;
        case MIFFT_FUSED2_KERNEL_2D:
        case MIFFT_FUSED2_KERNEL_2D_WIDE:
        case MIFFT_FUSED2_KERNEL_2D_BIG:
            unit = c.form == MIFFT_FUSED2_KERNEL_2D_WIDE ? mifft_fused2dw_f32 : f64 ? mifft_fused3d_f64 : mifft_fused2d_f32;
            // pass 0 = the y axis as a transposing column pass over in[y][x] (ny rows of M = nx columns, S = 1) -> ring[x][ky], with the
            // COL pass's table w(ny); pass 1 = the x axis as the same pass over ring[x][ky] (nx rows of ny columns) -> out[ky][kx],
            // with the ROW pass's table w(nx)
            f.p0.tw_L = p1->tw_L;
            f.p1.tw_L = p0->tw_L;
            f.p0.ostride_in = p1->outer_stride_in;
            f.p0.logMS = ilog2(p0->L); f.p0.logS = 0; f.p0.has_tw = 0; f.p0.total = p1->outer * p0->L;
            f.p1.logMS = ilog2(p1->L); f.p1.logS = 0; f.p1.has_tw = 0; f.p1.total = p1->outer * p1->L;
            break;
        case MIFFT_FUSED2_KERNEL_1D_WIDE:
        case MIFFT_FUSED2_KERNEL_1D_MIXED: unit = mifft_fused2w_f32; break;
        case MIFFT_FUSED2_KERNEL_1D_CHAIN64: unit = mifft_fusedx_f64; break;
        default: break;
    }
    rc = fill_ctl(&f.c, sync, p1->outer, lag, ring_slots, c.tiles0, c.tiles1, (hipStream_t)stream, "fused2");
    if (rc) return rc;
    rc = unit(a, b, split ? 1 : 0, &f, (unsigned)grid, (hipStream_t)stream, 0, &c);
    // (the unit answered the selector under the same switches a moment ago; should it refuse now, that is still no HIP error)
    if (rc == MIFFT_E_UNSUPPORTED || rc == 1) return set_err(MIFFT_E_UNSUPPORTED, "fused2: no kernel for %d x %d", p0->L, p1->L);
    return hip_check((hipError_t)rc, "kernel launch");
}

int mifft_fused_pair_supported(int32_t precision, int32_t layout, int32_t x, int32_t y, int32_t z) {
    if (bad_precision(precision) || (layout != MIFFT_INTERLEAVED && layout != MIFFT_SPLIT)) return MIFFT_E_UNSUPPORTED;
    return mifft_fusedp(precision == MIFFT_F64, layout == MIFFT_SPLIT, x, y, z, nullptr, 0, nullptr, 1, nullptr, nullptr, nullptr) == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}

int mifft_fused_pair_split(int32_t precision, int32_t layout, int32_t x, int32_t y, int32_t z) {
    if (bad_precision(precision) || (layout != MIFFT_INTERLEAVED && layout != MIFFT_SPLIT)) return 0;
    int r0 = 0;
    if (mifft_fusedp(precision == MIFFT_F64, layout == MIFFT_SPLIT, x, y, z, nullptr, 0, nullptr, 1, &r0, nullptr, nullptr) != 0) return 0;
    return r0;
}

int mifft_launch_fused_pair(const mifft_pass* passes, const void* in0, const void* in1, void* out0, void* out1, void* ring0, int32_t ring_slots,
                            int32_t lag, const mifft_fused_sync* sync, int32_t grid, mifft_stream_t stream) {
    if (!passes) return set_err(MIFFT_E_INVALID, "fused pair: null pass list");
    for (int i = 0; i < 4; ++i) {
        const int rc = validate(&passes[i]);
        if (rc) return rc;
    }
    const mifft_pass *px = &passes[0], *py0 = &passes[1], *py1 = &passes[2], *pz = &passes[3];
    int kxy, kyz, keyxy[3], keyyz[3], sxy, syz;
    // split-complex plans: the XY pair reads the two planes, the YZ pair writes them, the ring between them is interleaved
    const bool split = px->layout == MIFFT_SPLIT;
    if (classify_pair(px, py0, &kxy, keyxy, &sxy) != 0 || classify_pair(py1, pz, &kyz, keyyz, &syz) != 0 || kxy != 0 || kyz != 1 ||
        sxy != (split ? 1 : 0) || syz != (split ? 1 : 0) || pz->layout != px->layout ||
        py1->S != (int64_t)px->L * py0->L || py1->L != py0->M || pz->outer != py0->outer / pz->L || py1->inverse != px->inverse)
        return set_err(MIFFT_E_INVALID, "fused pair: not the (ROW x, COL y R0) + (COL y R1, COL z) pairs of one dense 3-D batch with an interleaved buffer between them");
    const int nx = px->L, ny = py0->L * (int)py0->M, nz = pz->L;
    const bool f64 = px->precision == MIFFT_F64;
    int r0 = 0;
    unsigned tiles0 = 0, tiles1 = 0;
    if (mifft_fusedp(f64, split ? 1 : 0, nx, ny, nz, nullptr, 0, nullptr, 1, &r0, &tiles0, &tiles1) != 0 || r0 != py0->L)
        return set_err(MIFFT_E_UNSUPPORTED, "fused pair: no kernel for %d x %d x %d with y = %d x %lld%s", nz, ny, nx, py0->L, (long long)py0->M, split ? " (split planes)" : "");
    if (!in0 || !out0 || !ring0 || (split && (!in1 || !out1))) return set_err(MIFFT_E_INVALID, "fused pair: null buffer");
    if (misaligned(15, {in0, out0, ring0, in1, out1})) return set_err(MIFFT_E_INVALID, "data buffers must be 16-byte aligned");
    if (ring0 == in0 || ring0 == out0) return set_err(MIFFT_E_INVALID, "fused pair: the ring must be a buffer of its own");
    if (grid < 1) return set_err(MIFFT_E_INVALID, "fused pair: grid >= 1");
    const long long batch = pz->outer;
    if (ring_slots < 2 || lag < 1 || lag >= ring_slots) return set_err(MIFFT_E_INVALID, "fused pair: need 1 <= lag < ring_slots");
    if (batch == 0) return 0;
    mifft::FusedPairArgs f;
    memset(&f, 0, sizeof(f));
    f.n = (long long)nx * ny * nz;
    f.a0.in0 = in0;
    f.a0.in1 = split ? in1 : nullptr;
    f.a0.out0 = ring0;
    f.a0.tw[0] = px->tw_L;     // w(nx)
    f.a0.tw[1] = py0->tw_L;    // w(R0)
    f.a0.tw_lo = py0->tw_lo;   // w(ny), two-level
    f.a0.tw_hi = py0->tw_hi;
    f.a0.tw_shift = py0->tw_shift;
    f.a0.inverse = px->inverse ? 1 : 0;
    f.a0.scale = px->scale * py0->scale;
    f.a1.in0 = ring0;
    f.a1.out0 = out0;
    f.a1.out1 = split ? out1 : nullptr;
    f.a1.tw[1] = py1->tw_L;    // w(R1)
    f.a1.tw[2] = pz->tw_L;     // w(nz)
    f.a1.inverse = f.a0.inverse;
    f.a1.scale = py1->scale * pz->scale;
    int rc = fill_ctl(&f.c, sync, batch, lag, ring_slots, tiles0, tiles1, (hipStream_t)stream, "fused pair");
    if (rc) return rc;
    rc = mifft_fusedp(f64, split ? 1 : 0, nx, ny, nz, &f, (unsigned)grid, (hipStream_t)stream, 0, nullptr, nullptr, nullptr);
    return hip_check((hipError_t)rc, "kernel launch");
}

int mifft_launch_chain_pipelined(const mifft_pass* passes, int32_t npasses, void* const bufs0[3], void* const bufs1[3],
                                 int64_t batch, int64_t chunk, int64_t item_elems, mifft_stream_t stream,
                                 const mifft_stream_t* side, int32_t nside, const mifft_event_t* events) {
    if (npasses < 0 || (npasses > 0 && !passes) || !bufs0) return set_err(MIFFT_E_INVALID, "bad chain arguments");
    if (batch < 1 || chunk < 1 || item_elems < 1 || nside < 1 || !side || !events)
        return set_err(MIFFT_E_INVALID, "bad pipeline arguments");
    for (int i = 0; i < npasses; ++i) {
        const mifft_pass* p = &passes[i];
        if (p->src < 0 || p->src > 2 || p->dst < 0 || p->dst > 2) return set_err(MIFFT_E_INVALID, "pass %d: bad buffer index", i);
        if (p->outer % batch) return set_err(MIFFT_E_INVALID, "pass %d: outer is not a multiple of the batch", i);
    }
    if (npasses == 0) return 0;
    const bool f64 = passes[0].precision == MIFFT_F64;
    const bool split = passes[0].layout == MIFFT_SPLIT;
    const int64_t ebytes = (split ? 1 : 2) * (f64 ? 8 : 4);
    bool tmp_interleaved = !split;  // the temp buffer is interleaved when the passes touching it say so
    for (int i = 0; i < npasses; ++i) {
        if (passes[i].src == 2 && (passes[i].flags & MIFFT_FLAG_SRC_INTERLEAVED)) tmp_interleaved = true;
        if (passes[i].dst == 2 && (passes[i].flags & MIFFT_FLAG_DST_INTERLEAVED)) tmp_interleaved = true;
    }
    const int64_t tbytes = (tmp_interleaved ? 2 : 1) * (f64 ? 8 : 4);
    // nside == 1 with side[0] == stream: the chunks in order on the caller's own stream, no fork and no join (what a plan asks for when
    // its stream is being captured into a graph: a linear graph)
    const bool inline_chunks = nside == 1 && side[0] == stream;
    int rc = 0;
    const int64_t nchunks = (batch + chunk - 1) / chunk;
    const int used = (int)(nchunks < nside ? nchunks : nside);
    if (!inline_chunks) {
        rc = hip_check(hipEventRecord((hipEvent_t)events[0], (hipStream_t)stream), "hipEventRecord");
        if (rc) return rc;
        for (int s = 0; s < used; ++s) {
            rc = hip_check(hipStreamWaitEvent((hipStream_t)side[s], (hipEvent_t)events[0], 0), "hipStreamWaitEvent");
            if (rc) return rc;
        }
    }
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t nb = (c + 1) * chunk <= batch ? chunk : batch - c * chunk;
        const int slot = (int)(c % nside);
        const int64_t off_io = c * chunk * item_elems * ebytes;
        const int64_t off_tmp = (int64_t)slot * chunk * item_elems * tbytes;
        for (int i = 0; i < npasses;) {
            mifft_pass p[2] = {passes[i], passes[i + 1 < npasses ? i + 1 : i]};
            p[0].outer = p[0].outer / batch * nb;
            p[1].outer = p[1].outer / batch * nb;
            const bool pair = (p[0].flags & MIFFT_FLAG_PAIR_WITH_NEXT) && i + 1 < npasses;
            const int dst = pair ? p[1].dst : p[0].dst;
            auto at = [&](void* const* bufs, int idx) -> void* {
                if (!bufs || !bufs[idx]) return nullptr;
                return (char*)bufs[idx] + (idx == 2 ? off_tmp : off_io);
            };
            int used = 1;
            rc = launch_unit(p, 0, pair ? 2 : 1, at(bufs0, p[0].src), split ? at(bufs1, p[0].src) : nullptr, at(bufs0, dst),
                             split ? at(bufs1, dst) : nullptr, side[slot], &used);
            if (rc) return rc;
            i += used;
        }
    }
    for (int s = 0; s < used && !inline_chunks; ++s) {
        rc = hip_check(hipEventRecord((hipEvent_t)events[1 + s], (hipStream_t)side[s]), "hipEventRecord");
        if (rc) return rc;
        rc = hip_check(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)events[1 + s], 0), "hipStreamWaitEvent");
        if (rc) return rc;
    }
    return 0;
}

int mifft_nd_tiled_supported(int32_t precision, int32_t x, int32_t y, int32_t z) {
    if (bad_precision(precision)) return MIFFT_E_UNSUPPORTED;
    return mifft_nd2t(precision == MIFFT_F64, x, y, z, nullptr, nullptr, nullptr, 1) == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}

static int launch_nd_tiled(const mifft_pass* p, const mifft_tiling* t, const void* in0, const void* in1, void* out0, void* out1, bool split,
                           mifft_stream_t stream) {
    if (!p || !t) return set_err(MIFFT_E_INVALID, "nd_tiled: null argument");
    if (p->kind != MIFFT_PASS_ND) return set_err(MIFFT_E_INVALID, "nd_tiled: not an ND pass");
    if (bad_precision(p->precision)) return set_err(MIFFT_E_INVALID, "bad precision %d", p->precision);
    if (p->layout != (split ? MIFFT_SPLIT : MIFFT_INTERLEAVED))
        return set_err(split ? MIFFT_E_INVALID : MIFFT_E_UNSUPPORTED, split ? "nd_tiled_split: the pass must say MIFFT_SPLIT" : "nd_tiled: interleaved data only (split planes: mifft_launch_nd_tiled_split)");
    if (mifft_nd_tiled_supported(p->precision, p->L, (int32_t)p->M, (int32_t)p->S) != 0)
        return set_err(MIFFT_E_UNSUPPORTED, "nd_tiled: no kernel for tiles of %d x %lld x %lld", p->L, (long long)p->M, (long long)p->S);
    if (t->cx < 1 || t->cy < 1 || t->cz < 1 || t->pitch_y < (int64_t)p->L * t->cx || t->pitch_z < t->pitch_y * p->M * t->cy ||
        t->parent_elems < t->pitch_z * p->S * t->cz || (t->pitch_y & 1) || (t->pitch_z & 1) || (t->parent_elems & 1))
        return set_err(MIFFT_E_INVALID, "nd_tiled: inconsistent tiling");
    if (!in0 || !out0 || (split && (!in1 || !out1))) return set_err(MIFFT_E_INVALID, "null data buffer");
    if (misaligned(15, {in0, out0, in1, out1})) return set_err(MIFFT_E_INVALID, "data buffers must be 16-byte aligned");
    if ((p->L > 1 && !p->tw_L) || (p->M > 1 && !p->tw_lo) || (p->S > 1 && !p->tw_hi)) return set_err(MIFFT_E_INVALID, "ND pass: twiddle table missing");
    if (p->outer < 0) return set_err(MIFFT_E_INVALID, "negative outer count");
    if (p->outer == 0) return 0;
    mifft::TileArgs a;
    memset(&a, 0, sizeof(a));
    a.in0 = in0; a.in1 = in1; a.out0 = out0; a.out1 = out1;
    a.split = a.split_out = split ? 1 : 0;
    a.tw_L = p->tw_L; a.tw_lo = p->tw_lo; a.tw_hi = p->tw_hi;
    a.inverse = p->inverse ? 1 : 0;
    a.scale = p->scale;
    mifft::TiledGeom g;
    g.pitch_y = t->pitch_y; g.pitch_z = t->pitch_z; g.parent = t->parent_elems; g.tiles = p->outer;
    g.cx = t->cx; g.cy = t->cy; g.cz = t->cz;
    return launched((split ? mifft_nd2t_split : mifft_nd2t)(p->precision == MIFFT_F64, p->L, (int)p->M, (int)p->S, &a, &g, (hipStream_t)stream, 0));
}

int mifft_launch_nd_tiled(const mifft_pass* p, const mifft_tiling* t, const void* in, void* out, mifft_stream_t stream) {
    return launch_nd_tiled(p, t, in, nullptr, out, nullptr, false, stream);
}

int mifft_launch_nd_tiled_split(const mifft_pass* p, const mifft_tiling* t, const void* in_re, const void* in_im, void* out_re, void* out_im,
                                mifft_stream_t stream) {
    return launch_nd_tiled(p, t, in_re, in_im, out_re, out_im, true, stream);
}

int mifft_aux_copy(const mifft_copy* c, const void* src0, const void* src1, void* dst0, void* dst1, mifft_stream_t stream) {
    if (!c || c->ndim < 1 || c->ndim > 6) return set_err(MIFFT_E_INVALID, "aux_copy: bad descriptor");
    if (bad_precision(c->precision)) return set_err(MIFFT_E_INVALID, "aux_copy: bad precision");
    for (int d = 0; d < c->ndim; ++d)
        if (c->dims[d] < 1) return set_err(MIFFT_E_INVALID, "aux_copy: dims[%d] = %lld", d, (long long)c->dims[d]);
    if (!src0 || !dst0 || (c->src_split && !src1) || (c->dst_split && !dst1)) return set_err(MIFFT_E_INVALID, "aux_copy: null buffer");
    const int rc = mifft_aux_copy_launch(c, src0, src1, dst0, dst1, (hipStream_t)stream);
    return hip_check((hipError_t)rc, "kernel launch");
}

int mifft_aux_mul_rows(int32_t precision, void* a, const void* b, int64_t rows, int64_t n, mifft_stream_t stream) {
    if (!a || !b || rows < 0 || n < 1) return set_err(MIFFT_E_INVALID, "aux_mul_rows: bad arguments");
    const int rc = mifft_aux_mul_rows_launch(precision == MIFFT_F64, a, b, rows, n, (hipStream_t)stream);
    return hip_check((hipError_t)rc, "kernel launch");
}

int mifft_aux_count_mismatch(const void* a, const void* b, size_t nbytes, uint64_t* count, mifft_stream_t stream) {
    if (!a || !b || !count) return set_err(MIFFT_E_INVALID, "null argument");
    if ((nbytes & 15) || misaligned(15, {a, b}) || misaligned(7, {count}))
        return set_err(MIFFT_E_INVALID, "mifft_aux_count_mismatch: buffers and size in whole 16-byte words, an 8-byte aligned counter");
    const int rc = mifft_aux_mismatch_launch(a, b, (unsigned long long)(nbytes / 16), (unsigned long long*)count, (hipStream_t)stream);
    return hip_check((hipError_t)rc, "kernel launch");
}

int mifft_mixed_supported(int32_t precision, int32_t n) {
    if (bad_precision(precision)) return MIFFT_E_UNSUPPORTED;
    return mifft_mixed_supported_impl(precision == MIFFT_F64, n) == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}

int mifft_mixed_radices(int32_t precision, int32_t n, int32_t* radix) {
    if (bad_precision(precision)) return MIFFT_E_UNSUPPORTED;
    if (!radix) return set_err(MIFFT_E_INVALID, "mixed radices: null result pointer");
    if (n < 2 || n > (1 << 24)) return MIFFT_E_UNSUPPORTED;
    const int ns = mifft_mixed_radices_impl(n, radix);
    return ns > 0 ? ns : MIFFT_E_UNSUPPORTED;
}

int mifft_launch_mixed_rows(int32_t precision, int32_t n, int64_t rows, int64_t stride_in, int64_t stride_out, const void* in, void* out,
                            const void* tw, int32_t inverse, double scale, mifft_stream_t stream) {
    if (mifft_mixed_supported(precision, n) != 0) return set_err(MIFFT_E_UNSUPPORTED, "mixed rows: no kernel for n = %d", n);
    if (!in || !out || !tw) return set_err(MIFFT_E_INVALID, "mixed rows: null buffer");
    if (rows < 0 || stride_in < n || stride_out < n) return set_err(MIFFT_E_INVALID, "mixed rows: bad row count / stride");
    if (const char* why = check_rows(precision, in, out, rows, n, stride_in, stride_out)) return set_err(MIFFT_E_INVALID, "mixed rows: %s", why);
    if (rows == 0) return 0;
    // dense rows: the single-buffer tile kernel of fft_mixed_nd.hip (one axis) where it is the faster one (development switch
    // MIFFT_DEBUG_ROWS_ND: 1 never, 2 wherever it fits)
    if (stride_in == n && stride_out == n && g_debug[MIFFT_DEBUG_ROWS_ND] != 1 && mifft_mixed_nd_rows_ok_impl(precision == MIFFT_F64, n) == 0 &&
        (g_debug[MIFFT_DEBUG_ROWS_ND] == 2 || mixed_rows_prefer_nd(precision == MIFFT_F64, n))) {
        const int rcn = mifft_mixed_nd_launch(precision == MIFFT_F64, n, 1, 1, rows, in, out, tw, nullptr, nullptr, inverse ? 3 : 0, scale, (hipStream_t)stream);
        if (rcn != -2) return launched(rcn);
    }
    return launched(mifft_mixed_launch(precision == MIFFT_F64, n, rows, stride_in, stride_out, 1, in, out, tw, inverse ? 3 : 0, scale, (hipStream_t)stream));
}

int mifft_launch_mixed_lines(int32_t precision, int32_t n, int64_t outer, int64_t inner, const void* in, void* out, const void* tw,
                             int32_t conj_in, int32_t conj_out, double scale, mifft_stream_t stream) {
    if (mifft_mixed_supported(precision, n) != 0) return set_err(MIFFT_E_UNSUPPORTED, "mixed lines: no kernel for n = %d", n);
    if (!in || !out || !tw) return set_err(MIFFT_E_INVALID, "mixed lines: null buffer");
    if (outer < 0 || inner < 1) return set_err(MIFFT_E_INVALID, "mixed lines: bad index space");
    if (mul3_checked(outer, inner, (long long)n * complex_bytes(precision)) < 0)
        return set_err(MIFFT_E_INVALID, "mixed lines: outer * inner * n overflows");
    if (const char* why = check_rows(precision, in, out, 0, n, n, n)) return set_err(MIFFT_E_INVALID, "mixed lines: %s", why);
    if (outer == 0) return 0;
    const int flags = (conj_in ? 1 : 0) | (conj_out ? 2 : 0);
    return launched(mifft_mixed_launch(precision == MIFFT_F64, n, outer * inner, n, n, inner, in, out, tw, flags, scale, (hipStream_t)stream));
}

int mifft_mixed_long_split(int32_t precision, int64_t n, int32_t* n1, int32_t* n2) {
    if (bad_precision(precision)) return MIFFT_E_UNSUPPORTED;
    if (!n1 || !n2) return set_err(MIFFT_E_INVALID, "mixed long: null result pointer");
    int a = 0, b = 0;
    if (mifft_mixed_long_split_impl(precision == MIFFT_F64, n, &a, &b) != 0) return MIFFT_E_UNSUPPORTED;
    *n1 = a; *n2 = b;
    return 0;
}

int mifft_launch_mixed_long(int32_t precision, int32_t n1, int32_t n2, int64_t batch, const void* in, void* mid, void* out, const void* tw1,
                            const void* tw2, const void* tw_lo, const void* tw_hi, int32_t tw_shift, int32_t inverse, double scale,
                            mifft_stream_t stream) {
    if (mifft_mixed_supported(precision, n1) != 0 || mifft_mixed_supported(precision, n2) != 0)
        return set_err(MIFFT_E_UNSUPPORTED, "mixed long: no kernel for %d x %d", n1, n2);
    if (!in || !mid || !out || !tw1 || !tw2 || !tw_lo || !tw_hi) return set_err(MIFFT_E_INVALID, "mixed long: null buffer");
    if (mid == in) return set_err(MIFFT_E_INVALID, "mixed long: the first pass transposes, `mid` must not be the input");
    if (batch < 0 || tw_shift < 1 || tw_shift > 23) return set_err(MIFFT_E_INVALID, "mixed long: bad batch / table shift");
    if ((long long)n1 * n2 > (1ll << 24)) return set_err(MIFFT_E_INVALID, "mixed long: n1 * n2 = %lld exceeds 2^24", (long long)n1 * n2);
    if (mul3_checked(batch, (long long)n1 * n2, complex_bytes(precision)) < 0) return set_err(MIFFT_E_INVALID, "mixed long: batch * n overflows");
    if (misaligned_complex(precision, {in, mid, out})) return set_err(MIFFT_E_INVALID, "mixed long: data buffers must be aligned to one complex number");
    if (batch == 0) return 0;
    return launched(mifft_mixed_long_launch(precision == MIFFT_F64, n1, n2, batch, in, mid, out, tw1, tw2, tw_lo, tw_hi, tw_shift,
                                           inverse ? 3 : 0, scale, (hipStream_t)stream));
}

int mifft_bluestein_padded(int32_t precision, int32_t n, int32_t* m) {
    if (bad_precision(precision)) return MIFFT_E_UNSUPPORTED;
    if (!m) return set_err(MIFFT_E_INVALID, "bluestein: null result pointer");
    const int v = mifft_bluestein_padded_impl(precision == MIFFT_F64, n);
    if (v <= 0) return MIFFT_E_UNSUPPORTED;
    *m = v;
    return 0;
}

int mifft_launch_bluestein_rows(int32_t precision, int32_t n, int32_t m, int64_t rows, int64_t stride_in, int64_t stride_out, const void* in,
                                void* out, const void* tw, const void* chirp, const void* bhat, int32_t inverse, double scale,
                                mifft_stream_t stream) {
    if (bad_precision(precision)) return MIFFT_E_UNSUPPORTED;
    if (n < 2 || m < 2 * (int64_t)n - 1 || mifft_bluestein_len_supported_impl(precision == MIFFT_F64, m) != 0)
        return set_err(MIFFT_E_UNSUPPORTED, "bluestein rows: no kernel for n = %d padded to %d", n, m);
    if (!in || !out || !tw || !chirp || !bhat) return set_err(MIFFT_E_INVALID, "bluestein rows: null buffer");
    if (rows < 0 || stride_in < n || stride_out < n) return set_err(MIFFT_E_INVALID, "bluestein rows: bad row count / stride");
    if (const char* why = check_rows(precision, in, out, rows, n, stride_in, stride_out)) return set_err(MIFFT_E_INVALID, "bluestein rows: %s", why);
    if (rows == 0) return 0;
    const int rc = mifft_bluestein_launch(precision == MIFFT_F64, n, m, rows, stride_in, stride_out, in, out, tw, chirp, bhat,
                                          inverse ? 3 : 0, scale, (hipStream_t)stream);
    if (rc == -2) return set_err(MIFFT_E_UNSUPPORTED, "bluestein rows: no kernel for n = %d padded to %d", n, m);
    return launched(rc);
}

int mifft_mixed_nd_supported(int32_t precision, int32_t x, int32_t y, int32_t z) {
    if (bad_precision(precision)) return MIFFT_E_UNSUPPORTED;
    return mifft_mixed_nd_supported_impl(precision == MIFFT_F64, x, y, z) == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}

int mifft_launch_mixed_nd(int32_t precision, int32_t x, int32_t y, int32_t z, int64_t transforms, const void* in, void* out, const void* tw_x,
                          const void* tw_y, const void* tw_z, int32_t inverse, double scale, mifft_stream_t stream) {
    if (mifft_mixed_nd_supported(precision, x, y, z) != 0) return set_err(MIFFT_E_UNSUPPORTED, "mixed nd: no kernel for %d x %d x %d", z, y, x);
    if (!in || !out || (x > 1 && !tw_x) || (y > 1 && !tw_y) || (z > 1 && !tw_z)) return set_err(MIFFT_E_INVALID, "mixed nd: null buffer");
    if (const char* why = check_rows(precision, in, out, 0, 0, 0, 0)) return set_err(MIFFT_E_INVALID, "mixed nd: %s", why);
    if (transforms < 0 || mul3_checked(transforms, (long long)x * y * z, complex_bytes(precision)) < 0)
        return set_err(MIFFT_E_INVALID, "mixed nd: bad transform count");
    if (transforms == 0) return 0;
    // inverse: 0 forward, 1 inverse = conjugate on load and on store; 2 / 4: on load / on store only (one end of a composition)
    const int flags = inverse == 1 ? 3 : inverse == 2 ? 1 : inverse == 4 ? 2 : 0;
    if (inverse != 0 && inverse != 1 && inverse != 2 && inverse != 4) return set_err(MIFFT_E_INVALID, "mixed nd: inverse must be 0, 1, 2 or 4");
    const int rc = mifft_mixed_nd_launch(precision == MIFFT_F64, x, y, z, transforms, in, out, tw_x, tw_y, tw_z, flags, scale, (hipStream_t)stream);
    if (rc == -2) return set_err(MIFFT_E_UNSUPPORTED, "mixed nd: no kernel for %d x %d x %d", z, y, x);
    return launched(rc);
}

int mifft_launch_real_post(const mifft_real_post* d, mifft_stream_t stream) {
    if (!d) return set_err(MIFFT_E_INVALID, "real post: null descriptor");
    if (bad_precision(d->precision)) return set_err(MIFFT_E_INVALID, "real post: bad precision %d", d->precision);
    if (d->inverse != 0 && d->inverse != 1) return set_err(MIFFT_E_INVALID, "real post: inverse must be 0 or 1");
    if (d->nx < 2 || !is_pow2(d->nx) || !is_pow2(d->ny) || !is_pow2(d->nz))
        return set_err(MIFFT_E_INVALID, "real post: shape %d x %d x %d is not powers of two with nx >= 2", d->nz, d->ny, d->nx);
    if (d->outer < 0) return set_err(MIFFT_E_INVALID, "real post: negative item count");
    if (!d->in || !d->out || !d->tw) return set_err(MIFFT_E_INVALID, "real post: null buffer");
    if (d->reserved != 0) return set_err(MIFFT_E_INVALID, "real post: reserved field must be 0");
    const long long L = d->nx / 2, rows = (long long)d->ny * d->nz;
    const long long n_in = rows * (d->inverse ? L + 1 : L), n_out = rows * (d->inverse ? L : L + 1);
    if (d->stride_in < n_in || d->stride_out < n_out) return set_err(MIFFT_E_INVALID, "real post: item pitch below the item's size");
    const long long esz = complex_bytes(d->precision);
    if (misaligned_complex(d->precision, {d->in, d->out, d->tw}))
        return set_err(MIFFT_E_INVALID, "real post: buffers must be aligned to one complex number");
    if (mul3_checked(d->outer, d->stride_in, esz) < 0 || mul3_checked(d->outer, d->stride_out, esz) < 0)
        return set_err(MIFFT_E_INVALID, "real post: items * pitch overflows");
    if (d->outer == 0) return 0;
    if (overlap(d->in, (uintptr_t)(((d->outer - 1) * d->stride_in + n_in) * esz), d->out, (uintptr_t)(((d->outer - 1) * d->stride_out + n_out) * esz)))
        return set_err(MIFFT_E_INVALID, "real post: input and output overlap (out of place only)");
    return launched(mifft_real_post_launch(d->precision == MIFFT_F64, d->inverse, d->nx, d->ny, d->nz, d->outer, d->stride_in, d->stride_out,
                                          d->in, d->out, d->tw, d->scale, (hipStream_t)stream));
}
int mifft_real_row_supported(int32_t precision, int32_t n) {
    if (bad_precision(precision) || n < 4 || !is_pow2(n)) return MIFFT_E_UNSUPPORTED;
    const int rc = row_dispatcher(precision, mifft_real_row_dispatch_f32, mifft_real_row_dispatch_f64)(n / 2, 0, nullptr, nullptr, 1);
    return rc == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}
int mifft_launch_real_row(int32_t precision, int32_t n, int32_t inverse, int64_t rows, const void* in, void* out, const void* tw_half,
                          const void* tw_sep, double scale, mifft_stream_t stream) {
    if (bad_precision(precision)) return set_err(MIFFT_E_INVALID, "real row: bad precision %d", precision);
    if (n < 2 || !is_pow2(n)) return set_err(MIFFT_E_INVALID, "real row: n = %d is not a power of two >= 2", n);
    if (mifft_real_row_supported(precision, n) != 0) return set_err(MIFFT_E_UNSUPPORTED, "real row: no kernel for n = %d", n);
    if (inverse != 0 && inverse != 1) return set_err(MIFFT_E_INVALID, "real row: inverse must be 0 or 1");
    if (rows < 0) return set_err(MIFFT_E_INVALID, "real row: negative row count");
    if (!in || !out || !tw_half || !tw_sep) return set_err(MIFFT_E_INVALID, "real row: null buffer");
    const long long esz = complex_bytes(precision);
    if (misaligned_complex(precision, {in, out, tw_half, tw_sep}))
        return set_err(MIFFT_E_INVALID, "real row: buffers must be aligned to one complex number");
    const long long L = n / 2, n_in = inverse ? L + 1 : L, n_out = inverse ? L : L + 1;
    if (mul3_checked(rows, n_in + n_out, esz) < 0) return set_err(MIFFT_E_INVALID, "real row: rows * n overflows");
    if (rows == 0) return 0;
    if (overlap(in, (uintptr_t)(rows * n_in * esz), out, (uintptr_t)(rows * n_out * esz))) return set_err(MIFFT_E_INVALID, "real row: input and output overlap (out of place only)");
    mifft::TileArgs a = {};
    a.in0 = in;
    a.out0 = out;
    a.tw_L = tw_half;
    a.tw_lo = tw_sep;
    a.total = rows;
    a.inverse = inverse;
    a.scale = scale;
    const int rc = row_dispatcher(precision, mifft_real_row_dispatch_f32, mifft_real_row_dispatch_f64)((int)L, inverse, &a, (hipStream_t)stream, 0);
    if (rc == -2) return set_err(MIFFT_E_UNSUPPORTED, "real row: no kernel for n = %d", n);
    return launched(rc);
}
// convolution rows (fft_conv_row.hpp): complex rows of n points (L = n), real rows of n reals (L = n / 2 packed points)
int mifft_conv_row_supported(int32_t precision, int32_t real, int32_t n) {
    if (bad_precision(precision) || (real != 0 && real != 1) || n < 2 || !is_pow2(n)) return MIFFT_E_UNSUPPORTED;
    if (real && n < 4) return MIFFT_E_UNSUPPORTED;
    const int L = real ? n / 2 : n;
    const int rc = row_dispatcher(precision, mifft_conv_row_dispatch_f32, mifft_conv_row_dispatch_f64)(real, L, nullptr, nullptr, 1);
    return rc == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}
int mifft_launch_conv_row(int32_t precision, int32_t real, int32_t n, int64_t rows, const void* in, void* out, const void* spectrum,
                          int64_t spectrum_pitch, int32_t correlate, const void* tw, const void* tw_sep, double scale, mifft_stream_t stream) {
    if (bad_precision(precision)) return set_err(MIFFT_E_INVALID, "conv row: bad precision %d", precision);
    if (real != 0 && real != 1) return set_err(MIFFT_E_INVALID, "conv row: real must be 0 or 1");
    if (n < 2 || !is_pow2(n)) return set_err(MIFFT_E_INVALID, "conv row: n = %d is not a power of two >= 2", n);
    if (mifft_conv_row_supported(precision, real, n) != 0) return set_err(MIFFT_E_UNSUPPORTED, "conv row: no kernel for n = %d", n);
    if (correlate != 0 && correlate != 1) return set_err(MIFFT_E_INVALID, "conv row: correlate must be 0 or 1");
    if (rows < 0) return set_err(MIFFT_E_INVALID, "conv row: negative row count");
    if (!in || !out || !spectrum || !tw || (real && !tw_sep)) return set_err(MIFFT_E_INVALID, "conv row: null buffer");
    const long long esz = complex_bytes(precision);
    if (misaligned_complex(precision, {in, out, spectrum, tw, tw_sep}))
        return set_err(MIFFT_E_INVALID, "conv row: buffers must be aligned to one complex number");
    const long long L = real ? n / 2 : n, sp = real ? L + 1 : L;
    if (spectrum_pitch != 0 && spectrum_pitch < sp)
        return set_err(MIFFT_E_INVALID, "conv row: spectrum_pitch %lld is neither 0 (shared) nor at least %lld", (long long)spectrum_pitch, sp);
    if (mul3_checked(rows, L, esz) < 0 || mul3_checked(rows, spectrum_pitch > sp ? spectrum_pitch : sp, esz) < 0)
        return set_err(MIFFT_E_INVALID, "conv row: rows * n overflows");
    if (rows == 0) return 0;
    const uintptr_t bytes = (uintptr_t)(rows * L * esz), sbytes = (uintptr_t)(((spectrum_pitch ? (rows - 1) * spectrum_pitch : 0) + sp) * esz);
    if (in != out && overlap(in, bytes, out, bytes)) return set_err(MIFFT_E_INVALID, "conv row: input and output overlap without being equal");
    if (overlap(spectrum, sbytes, in, bytes) || overlap(spectrum, sbytes, out, bytes)) return set_err(MIFFT_E_INVALID, "conv row: the spectrum overlaps the data");
    mifft::ConvRowArgs a = {};
    a.in = in;
    a.out = out;
    a.spec = spectrum;
    a.tw = tw;
    a.tw_sep = tw_sep;
    a.rows = rows;
    a.spec_pitch = spectrum_pitch;
    a.correlate = correlate;
    a.scale = scale;
    const int rc = row_dispatcher(precision, mifft_conv_row_dispatch_f32, mifft_conv_row_dispatch_f64)(real, (int)L, &a, (hipStream_t)stream, 0);
    if (rc == -2) return set_err(MIFFT_E_UNSUPPORTED, "conv row: no kernel for n = %d", n);
    return launched(rc);
}
// overlap-save FIR rows (fft_fir_row.hpp): blocks of n complex points (L = n) or n reals (L = n / 2 packed points)
int mifft_fir_row_supported(int32_t precision, int32_t real, int32_t n) {
    if (bad_precision(precision) || (real != 0 && real != 1) || n < 4 || !is_pow2(n)) return MIFFT_E_UNSUPPORTED;
    const int rc = row_dispatcher(precision, mifft_fir_row_dispatch_f32, mifft_fir_row_dispatch_f64)(real, real ? n / 2 : n, nullptr, nullptr, 1);
    return rc == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}
int mifft_launch_fir_row(int32_t precision, int32_t real, int32_t n, int32_t ov, int64_t length, int64_t pitch, int64_t items, const void* in,
                         void* out, const void* spectrum, int64_t spectrum_pitch, const void* tw, const void* tw_sep, double scale,
                         mifft_stream_t stream) {
    if (bad_precision(precision)) return set_err(MIFFT_E_INVALID, "fir row: bad precision %d", precision);
    if (real != 0 && real != 1) return set_err(MIFFT_E_INVALID, "fir row: real must be 0 or 1");
    if (n < 4 || !is_pow2(n)) return set_err(MIFFT_E_INVALID, "fir row: n = %d is not a power of two >= 4", n);
    if (mifft_fir_row_supported(precision, real, n) != 0) return set_err(MIFFT_E_UNSUPPORTED, "fir row: no kernel for n = %d", n);
    if (ov < 0 || ov > n / 2 || (real && (ov & 1)))
        return set_err(MIFFT_E_INVALID, "fir row: overlap %d is not in 0 .. n / 2%s", ov, real ? ", or is odd" : "");
    if (length < 1) return set_err(MIFFT_E_INVALID, "fir row: length must be at least 1");
    if (pitch < length || (real && (pitch & 1))) return set_err(MIFFT_E_INVALID, "fir row: pitch %lld is below the length%s", (long long)pitch, real ? ", or is odd" : "");
    if (items < 0) return set_err(MIFFT_E_INVALID, "fir row: negative item count");
    if (!in || !out || !spectrum || !tw || (real && !tw_sep)) return set_err(MIFFT_E_INVALID, "fir row: null buffer");
    const long long esz = complex_bytes(precision), ssz = real ? esz / 2 : esz;     // a point (real: one pair), an element
    if (misaligned_complex(precision, {in, out, spectrum, tw, tw_sep}))
        return set_err(MIFFT_E_INVALID, "fir row: buffers must be aligned to one complex number (real data: one pair)");
    const long long L = real ? n / 2 : n, sp = real ? L + 1 : L, hop = n - ov, blocks = (length + hop - 1) / hop;
    if (spectrum_pitch != 0 && spectrum_pitch < sp)
        return set_err(MIFFT_E_INVALID, "fir row: spectrum_pitch %lld is neither 0 (shared) nor at least %lld", (long long)spectrum_pitch, sp);
    if (mul3_checked(items, pitch, ssz) < 0 || mul3_checked(items, blocks, n) < 0 || mul3_checked(items, spectrum_pitch > sp ? spectrum_pitch : sp, esz) < 0)
        return set_err(MIFFT_E_INVALID, "fir row: items * pitch overflows");
    if (items == 0) return 0;
    const uintptr_t bytes = (uintptr_t)(((items - 1) * pitch + length) * ssz), sbytes = (uintptr_t)(((spectrum_pitch ? (items - 1) * spectrum_pitch : 0) + sp) * esz);
    if (overlap(in, bytes, out, bytes)) return set_err(MIFFT_E_INVALID, "fir row: input and output overlap (out of place only)");
    if (overlap(spectrum, sbytes, in, bytes) || overlap(spectrum, sbytes, out, bytes)) return set_err(MIFFT_E_INVALID, "fir row: the spectrum overlaps the data");
    mifft::FirRowArgs a = {};
    a.in = in;
    a.out = out;
    a.spec = spectrum;
    a.tw = tw;
    a.tw_sep = tw_sep;
    a.rows = items * blocks;
    a.blocks = blocks;
    a.pitch = real ? pitch / 2 : pitch;
    a.length = length;
    a.spec_pitch = spectrum_pitch;
    a.ov = real ? ov / 2 : ov;
    a.scale = scale;
    const int rc = row_dispatcher(precision, mifft_fir_row_dispatch_f32, mifft_fir_row_dispatch_f64)(real, (int)L, &a, (hipStream_t)stream, 0);
    if (rc == -2) return set_err(MIFFT_E_UNSUPPORTED, "fir row: no kernel for n = %d", n);
    return launched(rc);
}
int mifft_launch_fir_pad(int32_t precision, int32_t real, int32_t n, int32_t taps, int64_t filters, const void* in, void* out, mifft_stream_t stream) {
    if (bad_precision(precision)) return set_err(MIFFT_E_INVALID, "fir pad: bad precision %d", precision);
    if (real != 0 && real != 1) return set_err(MIFFT_E_INVALID, "fir pad: real must be 0 or 1");
    if (n < 4 || !is_pow2(n)) return set_err(MIFFT_E_INVALID, "fir pad: n = %d is not a power of two >= 4", n);
    if (taps < 1 || taps > n) return set_err(MIFFT_E_INVALID, "fir pad: taps = %d is not in 1 .. n", taps);
    if (filters < 0) return set_err(MIFFT_E_INVALID, "fir pad: negative filter count");
    if (!in || !out) return set_err(MIFFT_E_INVALID, "fir pad: null buffer");
    const long long esz = real ? complex_bytes(precision) / 2 : complex_bytes(precision);
    if (misaligned((uintptr_t)esz - 1, {in}) || misaligned(15, {out}))
        return set_err(MIFFT_E_INVALID, "fir pad: the taps must be aligned to one element, the output to 16 bytes");
    if (mul3_checked(filters, n, esz) < 0) return set_err(MIFFT_E_INVALID, "fir pad: filters * n overflows");
    if (filters == 0) return 0;
    if (overlap(in, (uintptr_t)(filters * taps * esz), out, (uintptr_t)(filters * n * esz)))
        return set_err(MIFFT_E_INVALID, "fir pad: input and output overlap (out of place only)");
    const int sc = real ? 1 : 2;
    return launched(mifft_fir_pad_launch(precision == MIFFT_F64, in, out, filters, n * sc, taps * sc, (hipStream_t)stream));
}
int mifft_aux_mul_spectrum(int32_t precision, void* data, const void* spectrum, int64_t items, int64_t points, int64_t spectrum_pitch,
                           int32_t correlate, double scale, mifft_stream_t stream) {
    if (bad_precision(precision)) return set_err(MIFFT_E_INVALID, "mul_spectrum: bad precision %d", precision);
    if (!data || !spectrum) return set_err(MIFFT_E_INVALID, "mul_spectrum: null buffer");
    if (items < 0 || points < 1 || (spectrum_pitch != 0 && spectrum_pitch < points) || (correlate != 0 && correlate != 1))
        return set_err(MIFFT_E_INVALID, "mul_spectrum: bad arguments");
    if (misaligned_complex(precision, {data, spectrum}))
        return set_err(MIFFT_E_INVALID, "mul_spectrum: buffers must be aligned to one complex number");
    if (mul3_checked(items, points, complex_bytes(precision)) < 0) return set_err(MIFFT_E_INVALID, "mul_spectrum: items * points overflows");
    return launched(mifft_aux_mul_spectrum_launch(precision == MIFFT_F64, data, spectrum, items, points, spectrum_pitch, correlate, scale,
                                                 (hipStream_t)stream));
}
// cosine and sine transforms (fft_r2r.hip): the steps around the complex transform of the packed data
static int r2r_step(const mifft_r2r_step* d, int post, mifft_stream_t stream) {
    const char* what = post ? "r2r post" : "r2r pre";
    if (!d) return set_err(MIFFT_E_INVALID, "%s: null descriptor", what);
    if (bad_precision(d->precision)) return set_err(MIFFT_E_INVALID, "%s: bad precision %d", what, d->precision);
    if (d->inverse != 0 && d->inverse != 1) return set_err(MIFFT_E_INVALID, "%s: inverse must be 0 or 1", what);
    if (d->kind != 0 && d->kind != 1) return set_err(MIFFT_E_INVALID, "%s: kind must be 0 (DCT) or 1 (DST)", what);
    if (d->ndim < 1 || d->ndim > 3) return set_err(MIFFT_E_INVALID, "%s: ndim must be 1, 2 or 3", what);
    if (d->reserved != 0) return set_err(MIFFT_E_INVALID, "%s: reserved field must be 0", what);
    const bool perm = post == d->inverse;       // forward pre, inverse post: the permutation steps
    const bool single = perm && d->ndim == 1 && d->n[0] == 1;
    long long pts = 1;
    for (int a = 0; a < d->ndim; ++a) {
        if (!single && (d->n[a] < 2 || !is_pow2(d->n[a])))
            return set_err(MIFFT_E_INVALID, "%s: axis %d has %d points, not a power of two >= 2", what, a, d->n[a]);
        pts *= d->n[a];
    }
    if (d->outer < 0) return set_err(MIFFT_E_INVALID, "%s: negative item count", what);
    if (!d->in || !d->out || (!perm && !d->tw)) return set_err(MIFFT_E_INVALID, "%s: null buffer", what);
    const long long rsz = d->precision == MIFFT_F64 ? 8 : 4;
    // the packed side (v, Z, Z') is whole complex numbers; the user side real numbers
    const void* packed = perm ? (d->inverse ? d->in : d->out) : (d->inverse ? d->out : d->in);
    if (misaligned((uintptr_t)rsz - 1, {d->in, d->out}) || (!single && misaligned_complex(d->precision, {packed})) ||
        (!perm && misaligned_complex(d->precision, {d->tw})))
        return set_err(MIFFT_E_INVALID, "%s: buffers must be aligned to one real (packed side: one complex) number", what);
    if (mul3_checked(d->outer, pts, rsz) < 0) return set_err(MIFFT_E_INVALID, "%s: items * points overflows", what);
    if (d->outer == 0) return 0;
    const uintptr_t bytes = (uintptr_t)(d->outer * pts * rsz);
    if (!(single && d->in == d->out) && overlap(d->in, bytes, d->out, bytes))
        return set_err(MIFFT_E_INVALID, "%s: input and output overlap (out of place only)", what);
    const int n[3] = {d->n[0], d->n[1], d->n[2]};
    return launched(mifft_r2r_step_launch(d->precision == MIFFT_F64, post, d->inverse, d->kind, d->ndim, n, d->outer, d->in, d->out, d->tw,
                                         d->scale, (hipStream_t)stream));
}
// one-launch cosine / sine rows (fft_r2r_row.hpp): rows of n reals, L = n / 2 packed points
int mifft_r2r_row_supported(int32_t precision, int32_t n) {
    if (bad_precision(precision) || n < 4 || !is_pow2(n)) return MIFFT_E_UNSUPPORTED;
    const int rc = row_dispatcher(precision, mifft_r2r_row_dispatch_f32, mifft_r2r_row_dispatch_f64)(n / 2, 0, nullptr, nullptr, 1);
    return rc == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}
int mifft_launch_r2r_row(int32_t precision, int32_t n, int32_t inverse, int32_t kind, int64_t rows, const void* in, void* out,
                         const void* tw_stage, const void* tw_sep, const void* tab, mifft_stream_t stream) {
    if (bad_precision(precision)) return set_err(MIFFT_E_INVALID, "r2r row: bad precision %d", precision);
    if (n < 4 || !is_pow2(n)) return set_err(MIFFT_E_INVALID, "r2r row: n = %d is not a power of two >= 4", n);
    if (mifft_r2r_row_supported(precision, n) != 0) return set_err(MIFFT_E_UNSUPPORTED, "r2r row: no kernel for n = %d", n);
    if (inverse != 0 && inverse != 1) return set_err(MIFFT_E_INVALID, "r2r row: inverse must be 0 or 1");
    if (kind != 0 && kind != 1) return set_err(MIFFT_E_INVALID, "r2r row: kind must be 0 (DCT) or 1 (DST)");
    if (rows < 0) return set_err(MIFFT_E_INVALID, "r2r row: negative row count");
    if (!in || !out || !tw_stage || !tw_sep || !tab) return set_err(MIFFT_E_INVALID, "r2r row: null buffer");
    const long long rsz = precision == MIFFT_F64 ? 8 : 4;
    if (misaligned(15, {in, out}) || misaligned_complex(precision, {tw_stage, tw_sep, tab}))
        return set_err(MIFFT_E_INVALID, "r2r row: data must be 16-byte aligned, tables aligned to one complex number");
    if (mul3_checked(rows, n, rsz) < 0) return set_err(MIFFT_E_INVALID, "r2r row: rows * n overflows");
    if (rows == 0) return 0;
    const uintptr_t bytes = (uintptr_t)(rows * n * rsz);
    if (in != out && overlap(in, bytes, out, bytes))
        return set_err(MIFFT_E_INVALID, "r2r row: input and output overlap without being the same buffer");
    mifft::TileArgs a = {};
    a.in0 = in;
    a.out0 = out;
    a.tw_L = tw_stage;
    a.tw_lo = tw_sep;
    a.tw_hi = tab;
    a.has_tw = kind;
    a.total = rows;
    a.inverse = inverse;
    a.scale = 1.0;
    const int rc = row_dispatcher(precision, mifft_r2r_row_dispatch_f32, mifft_r2r_row_dispatch_f64)(n / 2, inverse, &a, (hipStream_t)stream, 0);
    if (rc == -2) return set_err(MIFFT_E_UNSUPPORTED, "r2r row: no kernel for n = %d", n);
    return launched(rc);
}
int mifft_launch_r2r_pre(const mifft_r2r_step* desc, mifft_stream_t stream) { return r2r_step(desc, 0, stream); }
int mifft_launch_r2r_post(const mifft_r2r_step* desc, mifft_stream_t stream) { return r2r_step(desc, 1, stream); }
// complex32 transforms: the one-launch shape set of interleaved fp32 data (1-D rows up to 32768 points, the N-D shapes of
// mifft_nd_shape_supported with MIFFT_VARIANT_INTERLEAVED_ONLY), unit axes taken as given
int mifft_half_supported(int32_t x, int32_t y, int32_t z) {
    if (x < 1 || y < 1 || z < 1 || !is_pow2(x) || !is_pow2(y) || !is_pow2(z)) return MIFFT_E_UNSUPPORTED;
    if (y == 1 && z == 1) return (x >= 2 && mifft_c32_row_dispatch(x, nullptr, nullptr, 1) == 0) ? 0 : MIFFT_E_UNSUPPORTED;
    return mifft_nd_shape_supported(MIFFT_F32, x, y, z, MIFFT_VARIANT_INTERLEAVED_ONLY) == 0 ? 0 : MIFFT_E_UNSUPPORTED;
}
// the kernel family a supported shape runs (after dropping its unit axes): the ROW tile, the register-edged row, the fixed-shape N-D
// kernel or the run-time-shaped one (variant 1: the latter wherever it takes the shape, as variant 1 of an fp32 ND pass)
int mifft_half_kernel(int32_t x, int32_t y, int32_t z, int32_t variant) {
    if (mifft_half_supported(x, y, z) != 0 || (variant != 0 && variant != 1)) return MIFFT_E_UNSUPPORTED;
    int d[3] = {1, 1, 1}, nd = 0;
    for (int v : {x, y, z})
        if (v > 1) d[nd++] = v;
    if (nd <= 1) return d[0] >= 256 ? MIFFT_HALF_KERNEL_ROW : MIFFT_HALF_KERNEL_TILE;
    if (variant == 1 && (long long)d[0] * d[1] * d[2] <= mifft_nd_max_points(0)) return MIFFT_HALF_KERNEL_ND;
    return mifft_nd2_c32_supported(d[0], d[1], d[2]) == 0 ? MIFFT_HALF_KERNEL_ND2 : MIFFT_HALF_KERNEL_ND;
}
int mifft_launch_half(int32_t x, int32_t y, int32_t z, int32_t variant, int32_t inverse, int64_t transforms, const void* in, void* out, const void* tw_x,
                      const void* tw_y, const void* tw_z, double scale, mifft_stream_t stream) {
    if (x < 1 || y < 1 || z < 1 || !is_pow2(x) || !is_pow2(y) || !is_pow2(z))
        return set_err(MIFFT_E_INVALID, "half: shape %d x %d x %d is not powers of two", z, y, x);
    if (variant != 0 && variant != 1) return set_err(MIFFT_E_INVALID, "half: variant must be 0 or 1");
    const int kind = mifft_half_kernel(x, y, z, variant);
    if (kind < 0) return set_err(MIFFT_E_UNSUPPORTED, "half: no one-launch kernel for %d x %d x %d", z, y, x);
    if (inverse != 0 && inverse != 1) return set_err(MIFFT_E_INVALID, "half: inverse must be 0 or 1");
    if (transforms < 0) return set_err(MIFFT_E_INVALID, "half: negative transform count");
    if (!in || !out) return set_err(MIFFT_E_INVALID, "half: null buffer");
    // unit axes dropped: the data of (x, 1, z) is that of (x, z, 1); every remaining axis needs its table
    long long d[3] = {1, 1, 1};
    const void* tw[3] = {nullptr, nullptr, nullptr};
    int nd = 0;
    const int32_t dims_in[3] = {x, y, z};
    const void* tw_in[3] = {tw_x, tw_y, tw_z};
    for (int ax = 0; ax < 3; ++ax)
        if (dims_in[ax] > 1) {
            if (!tw_in[ax]) return set_err(MIFFT_E_INVALID, "half: null twiddle table for an axis of %d points", dims_in[ax]);
            d[nd] = dims_in[ax];
            tw[nd++] = tw_in[ax];
        }
    if (misaligned(15, {in, out})) return set_err(MIFFT_E_INVALID, "half: buffers must be 16-byte aligned");
    if (misaligned(7, {tw[0], tw[1], tw[2]})) return set_err(MIFFT_E_INVALID, "half: tables must be 8-byte aligned");
    const long long n = d[0] * d[1] * d[2];
    if (mul3_checked(transforms, n, 4) < 0) return set_err(MIFFT_E_INVALID, "half: transforms * points overflows");
    if (transforms == 0) return 0;
    const uintptr_t bytes = (uintptr_t)(transforms * n * 4);
    if (in != out && overlap(in, bytes, out, bytes))
        return set_err(MIFFT_E_INVALID, "half: input and output overlap (in place is exact aliasing only)");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (kind == MIFFT_HALF_KERNEL_ND) {
        mifft::NdArgs a;
        memset(&a, 0, sizeof(a));
        a.in0 = in; a.out0 = out;
        a.tw[0] = tw[0]; a.tw[1] = tw[1]; a.tw[2] = tw[2];
        a.total = transforms * n;
        // (with the register edge of the fp32 twin: the last stage writes runs of >= 16 points straight to HBM)
        if (nd_stage_list(d, false, &a) != 0) return set_err(MIFFT_E_UNSUPPORTED, "half: too many stages");
        a.inverse = inverse;
        a.scale = scale;
        rc = mifft_c32_nd_launch(n, &a, s);
    } else {
        mifft::TileArgs a;
        memset(&a, 0, sizeof(a));
        a.in0 = in; a.out0 = out;
        a.tw_L = tw[0]; a.tw_lo = tw[1]; a.tw_hi = tw[2];
        a.inverse = inverse;
        a.scale = scale;
        if (kind == MIFFT_HALF_KERNEL_ND2) {
            a.total = transforms * n;                        // points
            rc = mifft_nd2_c32_launch((int)d[0], (int)d[1], (int)d[2], &a, s);
        } else {
            a.total = transforms;                            // rows
            a.ostride_in = a.ostride_out = n;
            rc = mifft_c32_row_dispatch((int)n, &a, s, 0);
        }
    }
    if (rc == -2) return set_err(MIFFT_E_UNSUPPORTED, "half: no kernel for %d x %d x %d", z, y, x);
    return launched(rc);
}
int mifft_time_chain(const mifft_pass* passes, int32_t npasses, void* const bufs0[3], void* const bufs1[3], mifft_stream_t stream,
                     int32_t repeats, float* ms_total) {
    if (!ms_total || repeats < 1) return set_err(MIFFT_E_INVALID, "bad timing arguments");
    hipEvent_t e0, e1;
    int rc = hip_check(hipEventCreate(&e0), "hipEventCreate");
    if (rc) return rc;
    rc = hip_check(hipEventCreate(&e1), "hipEventCreate");
    if (rc) {
        (void)hipEventDestroy(e0);
        return rc;
    }
    rc = hip_check(hipEventRecord(e0, (hipStream_t)stream), "hipEventRecord");
    for (int r = 0; r < repeats && !rc; ++r) rc = mifft_launch_chain(passes, npasses, bufs0, bufs1, stream);
    if (!rc) rc = hip_check(hipEventRecord(e1, (hipStream_t)stream), "hipEventRecord");
    if (!rc) rc = hip_check(hipEventSynchronize(e1), "hipEventSynchronize");
    if (!rc) rc = hip_check(hipEventElapsedTime(ms_total, e0, e1), "hipEventElapsedTime");
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

}  // extern "C"
