/*
 * mifft.h -- C ABI of libmifft.so, the MI355X (gfx950) batched power-of-two c2c FFT engine
 * behind pyfft's Plan()/execute() API.
 *
 * This is the drop-in boundary.  In the reference (fjarri-attic/pyfft 0.3.9) the host side
 * (pyfft/plan.py, pyfft/kernel.py) reaches the device through a duck-typed
 * Context / Module / Function protocol implemented on PyCUDA (pyfft/cuda.py:19-113):
 *
 *   context.allocate(nbytes)                          cuda.py:85-89     -> mifft_malloc / mifft_free
 *   context.compile(src, fast_math) -> Module         cuda.py:52-61,91  -> (none: kernels are AOT-compiled
 *   module.getFunction(name, split, block) -> Function cuda.py:19-30        into this library; a pass is
 *   func.isExecutable()                               cuda.py:48-49         selected by mifft_pass_supported)
 *   func.prepare(grid, S); func(stream, *ptrs)        cuda.py:32-46     -> mifft_launch_pass / mifft_launch_chain
 *   context.createQueue()/wait()/flush()/getQueue()   cuda.py:94-107    -> mifft_stream_create / _sync / _destroy
 *   device limits read in Context.__init__            cuda.py:72-83     -> mifft_device_props
 *
 * and the generated kernels have the signature fft{Fwd,Inv}(in, out, int S) or
 * (in_re, in_im, out_re, out_im, int S) (pyfft/kernel.mako:690-697).  A `mifft_pass` describes one
 * such launch: one Stockham pass of pyfft/kernel.mako:805-1047 (globalKernel) or a whole LDS-resident
 * transform along the contiguous axis (kernel.mako:725-803, localKernel).
 *
 * Conventions
 *   - plain C, no C++ types or exceptions cross the boundary;
 *   - every function returns 0 on success, a positive hipError_t, or a negative MIFFT_E_* code, and
 *     records a thread-local message readable with mifft_last_error();
 *   - all device buffers (user data, temp, twiddle tables) are owned by the caller and only borrowed for
 *     the duration of the enqueued work; the library keeps no per-plan or per-call state (process-wide are only the
 *     DEFAULTS of the development switches, mifft_debug_set_default; mifft_debug_set itself is per thread);
 *   - launches are asynchronous on the caller's stream; nothing here synchronises except the *_sync calls.
 */
#ifndef MIFFT_H
#define MIFFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: mifft_launch_fused2's counter buffer is MIFFT_FUSED2_COUNTER_BYTES (one 256-byte line per counter) and is zeroed by the
 * call; streams are blocking streams; mifft_stream_wait_event
 * 3: the persistent launches take a mifft_fused_sync: two alternating counter sets, error word anywhere the device can write;
 * mifft_device_props carries the last-level cache size and the XCD count; mifft_launch_fused_pair
 * 6: mifft_has_feature, mifft_launch_xcd2 and mifft_launch_fused2x are gone; debug keys 1, 4 and 11 are retired; the persistent
 * launchers refuse lag == 0 */
#define MIFFT_ABI_VERSION 6

/* negative library error codes (positive values are hipError_t) */
#define MIFFT_E_INVALID      (-1)  /* malformed descriptor / argument              */
#define MIFFT_E_UNSUPPORTED  (-2)  /* no compiled kernel for this (precision, L, mode) */
#define MIFFT_E_NODEVICE     (-3)  /* no HIP device visible                         */

/* precision of the arithmetic and of the buffers */
#define MIFFT_F32 0
#define MIFFT_F64 1

/* buffer layout: interleaved (re,im) pairs, or two scalar planes
 * (pyfft/plan.py:26-35: complex dtypes -> interleaved, float dtypes -> split) */
#define MIFFT_INTERLEAVED 0
#define MIFFT_SPLIT       1

/* mifft_pass.flags (only meaningful with layout == MIFFT_SPLIT): the buffer read / written by this pass is
 * interleaved although the plan's layout is split.  Used for the plan-owned temp buffer, which is always
 * interleaved: 16 columns of one fp32 plane are only 64 bytes per row, so every side kept interleaved streams
 * at the full rate (src/dst plane pointer of that side is ignored and may be NULL). */
#define MIFFT_FLAG_SRC_INTERLEAVED 1
#define MIFFT_FLAG_DST_INTERLEAVED 2
/* hints for multi-pass plans: the source of this pass is read once and not needed again (the plan's first pass) /
   the destination is not re-read by the plan (its last pass): kernels that honour them use non-temporal accesses,
   which leaves the Infinity Cache to the intermediate of the pipelined strategy.  Results are unaffected. */
#define MIFFT_FLAG_STREAM_SRC 4
#define MIFFT_FLAG_STREAM_DST 8
/* this pass and the NEXT one of the chain are run by one launch (a "pass pair", csrc/fft_pair.hpp): the launch reads the
   buffer `src` of this pass and writes the buffer `dst` of the next one; the chain launchers skip the second descriptor.
   Only set where mifft_pass_pair_supported() says so. */
#define MIFFT_FLAG_PAIR_WITH_NEXT 16
/* small launches: store the destination WRITE-THROUGH.  A kernel's plain stores stay dirty in the eight L2s (32 MiB) until the
   end-of-kernel write-back, which runs alone: ~4 us behind a launch whose whole output fits the L2s -- a third of a 32 MiB
   launch (profiles/r03_l_small_launch_write_through.log).  Set by the planner for launches of <= 128 MiB; kernels without a
   write-through form ignore it.  Results are unaffected. */
#define MIFFT_FLAG_WRITE_THROUGH 32

/* pass kinds */
#define MIFFT_PASS_COL 0  /* strided pass: [outer][L][M*S] -> [outer][M][L][S]  (kernel.mako:805-1047) */
#define MIFFT_PASS_ROW 1  /* contiguous pass: `outer` rows of L points, in place  (kernel.mako:725-803)  */
#define MIFFT_PASS_ND  2  /* whole small 2-D/3-D transform in LDS: L = x, M = y, S = z (x contiguous), `outer`
                            transforms back to back; tw_L / tw_lo / tw_hi = w(x)^k / w(y)^k / w(z)^k tables (NULL for an
                            axis of length 1); shape accepted by mifft_nd_shape_supported().  In place capable.
                            Replaces the reference's local kernel + one global chain per further axis (plan.py:111-123) */

typedef void *mifft_stream_t; /* hipStream_t; NULL = the default stream */
typedef void *mifft_event_t;  /* hipEvent_t */

/*
 * One launch.  With w(m) = exp(-2*pi*i/m) (forward; the inverse conjugates input and output):
 *
 *   MIFFT_PASS_COL  in  viewed as [outer][L][M][S]
 *                   out viewed as [outer][M][L][S]
 *       out[o][l][q][j] = scale * w(L*M)^(l*q) * sum_r in[o][r][l][j] * w(L)^(r*q)
 *     M == 1  -> plain strided transform (last pass of an axis), in-place capable;
 *     S == 1  -> first pass of a long contiguous axis: the write is a transposition.
 *
 *   MIFFT_PASS_ROW  in/out viewed as [outer][L]:  out[o][q] = scale * sum_r in[o][r] * w(L)^(r*q)
 *
 *   MIFFT_PASS_ND   in/out viewed as [outer][S][M][L] (z, y, x):  out[o] = scale * DFT3(in[o])
 *
 * Matrix `o` starts at element o*outer_stride_{in,out} (elements of the complex type; for split layout
 * the same offset applies to both planes).  Sizes are powers of two except `outer`.
 */
typedef struct mifft_pass {
    int32_t kind;        /* MIFFT_PASS_COL | MIFFT_PASS_ROW | MIFFT_PASS_ND */
    int32_t precision;   /* MIFFT_F32 | MIFFT_F64 */
    int32_t layout;      /* MIFFT_INTERLEAVED | MIFFT_SPLIT (same for input and output) */
    int32_t inverse;     /* 0 forward (numpy.fft.fft sign), 1 inverse (unnormalised unless `scale`) */
    int32_t L;           /* transform length of this launch (the radix of the pass) */
    int32_t variant;     /* kernel variant selector: 0 = library default; 1 = the generic kernel of the kind (COL / ROW: the LDS tile kernel; ND: the
                          * run-time-shaped kernel instead of the shape's fixed instance -- the plan's choice for the shapes listed in the tuning table) */
    int64_t M;           /* not-yet-transformed extent of the axis after this pass (COL), 1 for ROW */
    int64_t S;           /* extent of everything faster than the digit being transformed (COL), 1 for ROW */
    int64_t outer;       /* number of independent matrices / rows */
    int64_t outer_stride_in;   /* elements between consecutive matrices in the input  */
    int64_t outer_stride_out;  /* elements between consecutive matrices in the output */
    double  scale;       /* every output is multiplied by this (1.0 except in a plan's last pass,
                            pyfft/kernel.py:23-37, pyfft/plan.py:125-128) */
    const void *tw_L;    /* device: L entries w(L)^k, complex of `precision` */
    const void *tw_lo;   /* device: 2^tw_shift entries w(L*M)^k            (NULL when M == 1) */
    const void *tw_hi;   /* device: (L*M)>>tw_shift entries w(L*M)^(k<<tw_shift) (NULL when M == 1) */
    int32_t tw_shift;
    int32_t src;         /* for mifft_launch_chain: index of the buffer read  (0 in, 1 out, 2 temp) */
    int32_t dst;         /* for mifft_launch_chain: index of the buffer written */
    int32_t flags;       /* MIFFT_FLAG_*: per-side layout overrides for a plan's internal temp buffer */
} mifft_pass;

typedef struct mifft_device_props {
    char    name[256];
    char    gcn_arch[64];
    int32_t compute_units;
    int32_t wavefront_size;
    int32_t max_threads_per_block;
    int32_t max_grid_x;
    int64_t lds_bytes_per_block;
    int64_t total_mem_bytes;
    int32_t clock_khz;
    int32_t l2_bytes;        /* L2 of ONE XCD (hipDeviceProp_t::l2CacheSize) */
    int64_t llc_bytes;       /* last-level cache in front of HBM (the Infinity Cache / MALL: 256 MiB on MI355X) from the HSA agent
                                (HSA_AGENT_INFO_CACHE_SIZE[2]); 0 = none or unknown.  The planner sizes the rings of the persistent
                                launches, the pipelined chunks and the write-through rule from it instead of from literals */
    int32_t num_xcc;         /* XCDs (chiplets with their own L2) the device spans (HSA_AMD_AGENT_INFO_NUM_XCC); 1 if unknown */
    int32_t reserved0;
} mifft_device_props;

/* ---- library ------------------------------------------------------------------------------------- */
int         mifft_abi_version(void);
const char *mifft_last_error(void);
/* development switches (all 0 in production; pyfft_amd/_debug.py maps environment variables onto them) */
#define MIFFT_DEBUG_NO_ND2 0       /* run-time-shaped N-D kernel only */
#define MIFFT_DEBUG_NO_WAVE 2      /* no wave-autonomous small-transform kernels */
#define MIFFT_DEBUG_FORCE_WAVE 3   /* wave-autonomous kernels wherever one exists, whatever the buffer size */
#define MIFFT_DEBUG_ALT_ROWS 5     /* alternative stage lists of the longest fp32 rows (A/B measurements) */
#define MIFFT_DEBUG_PAIR 6         /* pass pairs: 0 = default split, 1 = off, 2 = the alternative y split, 3 = the first tile forms of the persistent two-pair kernel (A/B measurements) */
#define MIFFT_DEBUG_STORE 7        /* streamed output stores (A/B): 0 = default, 1 = non-temporal, 2 = write-through (sc1), 3 = plain */
#define MIFFT_DEBUG_ROWS_ND 8      /* dense smooth rows: 0 = default, 1 = two-buffer row kernel only, 2 = single-buffer tile kernel wherever it fits (A/B) */
#define MIFFT_DEBUG_NARROW_TILES 9 /* A/B of the round-4 tile forms: 1 = the rounds 1-3 forms -- fp32 L = 256 / 512 on 16-column tiles also in the persistent
                                    * kernel, and for split-complex planes no lane-interleaved double tiles, no register-edged rows, no fixed-shape N-D
                                    * route, no row-first 2-D kernel, no write-through in the run-time-shaped N-D kernel; 3 = 16-column tiles also for strided passes
                                    * whose rows lie >= 2^16 points apart (round 6: those run on 32-column tiles by default) */
#define MIFFT_DEBUG_NO_ROWFIRST 10 /* split-complex fp32 2-D persistent launches: 1 = two transposing passes on sibling tiles instead of the row-first kernel (A/B) */
#define MIFFT_DEBUG_PAIR_LANES 12  /* fp32 interleaved 1-D 2^20 = 1024 x 1024 persistent launches: n = paired-lane form n - 1 of the kernel (A/B): 1 = form 0,
                                    * 8-byte lanes on every stream; 4 = form 3, 16-byte lanes on every stream (the default, 0) */
/* keys 1, 4 and 11 are retired (they selected kernel forms that were measured and not adopted): mifft_debug_set and
 * mifft_debug_set_default refuse them with MIFFT_E_INVALID */
#define MIFFT_DEBUG_KEYS 13
/* mifft_debug_set changes a switch for the CALLING THREAD only (a thread that never set a key sees the process default), so a
 * measurement that flips a switch in one thread cannot change the kernels another thread's plan gets; mifft_debug_set_default sets
 * the process default (what the environment variables of pyfft_amd/_debug.py do once, when the library is loaded).  A switch must
 * not change between the support queries a plan is built from and that plan's launches: the launch then fails with
 * MIFFT_E_UNSUPPORTED instead of running another kernel. */
int mifft_debug_set(int32_t key, int32_t value);
int mifft_debug_set_default(int32_t key, int32_t value);
int mifft_debug_get(int32_t key);
/* the paired-lane form (MIFFT_DEBUG_PAIR_LANES) the calling thread's last fp32 1-D 1024 x 1024 persistent launch took, -1 before the first */
int mifft_debug_last_pair_lanes_form(void);

/* ---- runtime shim (replaces cuda.py Context: allocate / stream lifecycle / device limits) ---------- */
int mifft_device_count(int *count);
int mifft_set_device(int device);
int mifft_get_device(int *device);
int mifft_device_props_get(int device, mifft_device_props *props);
int mifft_malloc(void **ptr, size_t nbytes);
int mifft_free(void *ptr);
int mifft_memset(void *ptr, int value, size_t nbytes, mifft_stream_t stream);
int mifft_memcpy_h2d(void *dst, const void *src, size_t nbytes, mifft_stream_t stream);
int mifft_memcpy_d2h(void *dst, const void *src, size_t nbytes, mifft_stream_t stream);
int mifft_memcpy_d2d(void *dst, const void *src, size_t nbytes, mifft_stream_t stream);
/* pinned host memory + a copy that does NOT synchronise: how a plan reads a persistent kernel's error word without
 * stalling the stream (the copy is enqueued behind the launch, the host looks at it once mifft_event_query says so) */
int mifft_host_alloc(void **ptr, size_t nbytes);
int mifft_host_free(void *ptr);
int mifft_memcpy_d2h_async(void *dst, const void *src, size_t nbytes, mifft_stream_t stream);
/* streams are BLOCKING streams (they order against the legacy null stream, like PyCUDA's: cuda.py:94-96) */
int mifft_stream_create(mifft_stream_t *stream);
int mifft_stream_destroy(mifft_stream_t stream);
int mifft_stream_sync(mifft_stream_t stream);
int mifft_device_sync(void);
/*
 * Stream capture / hipGraph replay of the calls a plan enqueues (HIP graphs are how a launch-bound inner loop is replayed on this
 * part; the reference's execute is an asynchronous enqueue on the caller's stream, pyfft/plan.py:250-259, and a torch-ROCm caller
 * may capture that stream).  Every launcher of this library may be called on a capturing stream; the persistent launches then
 * REQUIRE the single-set form of their mifft_fused_sync argument -- counters_next == NULL --, see there.
 *   mifft_stream_is_capturing   *capturing = 1 while `stream` records into a graph
 *   mifft_stream_begin_capture  start recording the work enqueued on `stream` (relaxed mode; not the default stream)
 *   mifft_stream_end_capture    stop recording and instantiate: *graph is an executable graph (hipGraphExec_t)
 *   mifft_graph_launch          replay it on `stream`; mifft_graph_destroy frees it
 */
typedef void *mifft_graph_t; /* hipGraphExec_t */
int mifft_stream_is_capturing(mifft_stream_t stream, int32_t *capturing);
int mifft_stream_begin_capture(mifft_stream_t stream);
int mifft_stream_end_capture(mifft_stream_t stream, mifft_graph_t *graph);
int mifft_graph_launch(mifft_graph_t graph, mifft_stream_t stream);
int mifft_graph_destroy(mifft_graph_t graph);
int mifft_event_create(mifft_event_t *event);
int mifft_event_destroy(mifft_event_t event);
int mifft_event_record(mifft_event_t event, mifft_stream_t stream);
int mifft_event_sync(mifft_event_t event);
int mifft_event_query(mifft_event_t event); /* 0 = completed, 1 = not yet, else an error code */
/* work enqueued on `stream` after this call starts only when `event` has completed (hipStreamWaitEvent): how a plan whose
 * caller switches streams between asynchronous executes orders the second stream behind the first on its scratch */
int mifft_stream_wait_event(mifft_stream_t stream, mifft_event_t event);
int mifft_event_elapsed_ms(float *ms, mifft_event_t start, mifft_event_t stop);

/* ---- pass launchers (replace cuda.py Function.__call__, cuda.py:35-46) ----------------------------- */

/* largest x*y*z a MIFFT_PASS_ND launch accepts for ANY power-of-two shape and either layout of the precision */
int mifft_nd_max_points_for(int32_t precision);

/* 0 if one MIFFT_PASS_ND launch can transform the (z, y, x) shape, else MIFFT_E_UNSUPPORTED: every shape up to
 * mifft_nd_max_points_for(); with variant MIFFT_VARIANT_INTERLEAVED_ONLY also the larger fixed shapes that exist for
 * interleaved data on both sides only; with MIFFT_VARIANT_SPLIT_ONLY those that exist for split-complex planes on BOTH
 * sides (a single-pass plan of a split-complex layout); with MIFFT_VARIANT_OUT_OF_PLACE_ONLY (round 5) those whose kernel runs several
 * work-groups per transform (csrc/fft_nd2z.hpp): interleaved data on both sides AND input != output -- a caller keeps another chain for
 * its in-place executes.  (No counterpart in the reference, whose kernels are generated per plan.) */
#define MIFFT_VARIANT_SPLIT_ONLY 3
#define MIFFT_VARIANT_OUT_OF_PLACE_ONLY 4
#define MIFFT_VARIANT_OUT_OF_PLACE_ANY_SIZE 5 /* ... and that kernel is the better choice at EVERY buffer size (else: beyond half the last-level cache per side) */
#define MIFFT_VARIANT_SPLIT_OUT_OF_PLACE 6 /* round 6: the same for split-complex planes on both sides (csrc/fft_nd2zp.hpp) ... */
#define MIFFT_VARIANT_SPLIT_OUT_OF_PLACE_ANY_SIZE 7 /* ... and at every buffer size */
int mifft_nd_shape_supported(int32_t precision, int32_t x, int32_t y, int32_t z, int32_t variant);

/* 0 if a compiled kernel exists for (kind, precision, L, variant), else MIFFT_E_UNSUPPORTED.
 * Counterpart of Function.isExecutable (cuda.py:48-49) for AOT kernels.  variant 0: a kernel that takes either layout;
 * MIFFT_VARIANT_INTERLEAVED_ONLY (ROW passes): also count kernels that need interleaved data on both sides.
 * The query knows no layout: the longest rows (32768 points fp32, 16384 fp64) exist for interleaved -> interleaved, planes -> planes and
 * planes -> interleaved; an interleaved -> planes ROW pass of that length (MIFFT_FLAG_SRC_INTERLEAVED without _DST_INTERLEAVED on a
 * MIFFT_SPLIT pass) is refused by mifft_launch_pass with MIFFT_E_UNSUPPORTED although the query says 0 -- no plan builds one (a ROW pass
 * is a plan's first pass: its input is the user's layout). */
#define MIFFT_VARIANT_INTERLEAVED_ONLY 2
int mifft_pass_supported(int32_t kind, int32_t precision, int32_t L, int32_t variant);

/* Enqueue one pass.  in1/out1 are the imaginary planes for MIFFT_SPLIT and must be NULL for
 * MIFFT_INTERLEAVED.  In-place (out == in) is allowed for MIFFT_PASS_ROW, MIFFT_PASS_ND and for
 * MIFFT_PASS_COL with M == 1 (pyfft/kernel.py:144,238-241). */
int mifft_launch_pass(const mifft_pass *pass, const void *in0, const void *in1, void *out0, void *out1,
                      mifft_stream_t stream);

/* Which kernel form mifft_launch_pass runs for a MIFFT_PASS_ND descriptor: a pure query (it never touches a device), the one selector
 * the launch itself goes through.  aliased: bit 0 = the call would have in0 == out0, bit 1 = in1 == out1 (planes on both sides only).
 * The answer also depends on the calling thread's development switches.  Returns a MIFFT_ND_KERNEL_* constant, else the error code (with
 * its message) mifft_launch_pass gives for that descriptor before it touches data: an invalid descriptor, a shape without a kernel, a
 * shape whose kernel exists out of place only asked for in place. */
#define MIFFT_ND_KERNEL_WAVE  1 /* wave-autonomous (16, 16) fp32 plane (fft_wave.hpp): MIFFT_DEBUG_FORCE_WAVE only */
#define MIFFT_ND_KERNEL_ND2Z  2 /* several work-groups per transform, interleaved, out of place (fft_nd2z.hpp) */
#define MIFFT_ND_KERNEL_ND2   3 /* fixed shape, interleaved on both sides (fft_nd2.hpp) */
#define MIFFT_ND_KERNEL_ND2ZP 4 /* several work-groups per transform, planes on both sides, out of place (fft_nd2zp.hpp) */
#define MIFFT_ND_KERNEL_ND2P  5 /* fixed shape, dense planes on both sides, 16-byte accesses (fft_nd2p.hpp) */
#define MIFFT_ND_KERNEL_ND2T  6 /* fixed shape in its tiled form, planes in (fft_nd2t.hpp: planes or interleaved out) */
#define MIFFT_ND_KERNEL_ND    7 /* run-time-shaped kernel (fft_nd.hpp), up to mifft_nd_max_points_for() points, any sides */
int mifft_nd_kernel(const mifft_pass *pass, int32_t aliased);

/*
 * Pass pairs: two CONSECUTIVE passes of a chain run by one launch on tiles that hold the points of both, so that a 3-D
 * transform whose (y, x) plane fits no work-group still crosses HBM twice instead of three times.  With the y axis
 * factored R0 * R1 as the chain factors a long axis (pyfft/kernel.py:259-283), the four passes
 *     ROW x | COL y (L = R0, M = R1, S = nx) | COL y (L = R1, M = 1, S = nx * R0) | COL z (L = nz, M = 1, S = nx * ny)
 * are the pairs (ROW x, COL y R0) -- out of place only -- and (COL y R1, COL z) -- in place capable.  Dense batches (outer
 * stride = the transform size) only.  The buffer BETWEEN the two launches is interleaved; with layout MIFFT_SPLIT the first
 * launch reads and the second writes two scalar planes (flags MIFFT_FLAG_DST_INTERLEAVED / _SRC_INTERLEAVED on the inner side).
 *   mifft_pair_split          R0 (> 0) if the library has both pair kernels for a (z, y, x) transform of that layout, else 0
 *   mifft_pass_pair_supported 0 if (p0, p1) is such a pair with a compiled kernel, else MIFFT_E_UNSUPPORTED
 *   mifft_launch_pass_pair    enqueue it: reads in0 / in1 (p0's input side), writes out0 / out1 (p1's output side); in1 / out1
 *                             are the imaginary planes of a split side, else ignored; scale = p0->scale * p1->scale
 */
int mifft_pair_split(int32_t precision, int32_t layout, int32_t x, int32_t y, int32_t z);
int mifft_pass_pair_supported(const mifft_pass *p0, const mifft_pass *p1);
/* Round 5: 0 if the library has the pass-pair kernel itself -- kind 0 = (ROW x, COL y R0) keyed by (nx, R0, R1 = ny / R0), kind 1 =
 * (COL y R1, COL z) keyed by (S0 = what is faster than the y digit, R1, nz) -- for interleaved data (layout MIFFT_SPLIT: planes on the
 * user side of the pair).  What a planner asks before it builds a chain around ONE pair: a 2-D shape with a y axis too long for one
 * strided pass (pair XY + one plain pass instead of three launches), a 3-D shape with short y and z behind a long x (ROW x + pair YZ). */
int mifft_pair_kernel_supported(int32_t precision, int32_t layout, int32_t kind, int32_t k0, int32_t k1, int32_t k2);
int mifft_launch_pass_pair(const mifft_pass *p0, const mifft_pass *p1, const void *in0, const void *in1, void *out0, void *out1,
                           mifft_stream_t stream);

/* Enqueue a whole plan: passes[i] reads bufs0/bufs1[passes[i].src] and writes [passes[i].dst]
 * (0 = data_in, 1 = data_out, 2 = temp -- the ping-pong loop of pyfft/plan.py:217-248 with the
 * schedule already decided by the Python plan).  bufs1 may be NULL for interleaved layout. */
int mifft_launch_chain(const mifft_pass *passes, int32_t npasses, void *const bufs0[3], void *const bufs1[3],
                       mifft_stream_t stream);

/*
 * Pipelined form of mifft_launch_chain for any multi-pass plan (counterpart of the batch loop the
 * reference runs inside each kernel grid, pyfft/kernel.py:99-121, re-cut for the MI355X memory system):
 * the batch is processed in chunks of `chunk` items; chunk i runs the whole pass chain on side stream
 * i % nside with temp slot i % nside, so the inter-pass intermediate of a chunk is consumed while it is still
 * in the 256 MiB Infinity Cache and kernels of different chunks overlap each other's launch tails.
 *   - `passes` describe the FULL batch (outer = outer_per_item * batch); `item_elems` = elements per batch item
 *     (per plane for split layout);  bufs*[2] (temp), when the schedule uses it, must hold nside * chunk items.
 *   - ordering: side streams wait for everything enqueued on `stream` so far; `stream` waits for all side
 *     streams before the call's work counts as done.  events[0..nside] are caller-owned scratch events.
 *   - nside == 1 with side[0] == stream: the chunks run in order on `stream` itself, no fork, no join, no event is touched -- what to
 *     pass while `stream` is being captured (a linear graph; forked captures of this launch crashed hipGraphLaunch now and then).
 */
int mifft_launch_chain_pipelined(const mifft_pass *passes, int32_t npasses, void *const bufs0[3], void *const bufs1[3],
                                 int64_t batch, int64_t chunk, int64_t item_elems, mifft_stream_t stream,
                                 const mifft_stream_t *side, int32_t nside, const mifft_event_t *events);

/*
 * Fused form of a two-pass long contiguous axis N = p0->L * p1->L: both Stockham passes of all `p0->outer` transforms in
 * ONE persistent launch, pass 1 of transform t trailing pass 0 by `lag` transforms, with the intermediate in a scratch
 * ring of `ring_slots` transforms (ring_slots > lag) that stays in the Infinity Cache.
 *   shapes    1-D form: p0 = the transposing first pass (COL, S == 1, M == p1->L), p1 = the plain strided last pass
 *             (COL, M == 1, S == p0->L).  2-D form: p0 = the ROW pass, p1 = the strided COL pass of the plan.  Which lengths
 *             have a kernel, per precision and layout: mifft_fused2_kernel below (the table of forms is in docs/persistent.md).
 *             Anything else: MIFFT_E_UNSUPPORTED.
 *   sync      counters + error word, see mifft_fused_sync below (one 256-byte line per counter, csrc/fft_fused2.hpp).  After
 *             completion a non-zero error word reports a dependency time-out (results invalid).
 *   ring      always interleaved (ring0; ring1 is ignored), also for split-plane in/out buffers.
 */
#define MIFFT_FUSED2_COUNTER_STRIDE 64u /* uint32 words between two counters */
#define MIFFT_FUSED2_COUNTER_BYTES(outer) ((size_t)MIFFT_FUSED2_COUNTER_STRIDE * 4u * (9u + 2u * (size_t)(outer)))
/*
 * Synchronisation state of one persistent launch (all caller-owned device-accessible memory):
 *   counters       MIFFT_FUSED2_COUNTER_BYTES(outer) bytes.  With counters_next == NULL the call zeroes them on `stream` in front
 *                  of the launch (hipMemsetAsync: ~5 us, what a 32 MiB execute cannot afford; on a CAPTURING stream a small kernel
 *                  of the library's own, i.e. a kernel node -- a memset node in front of the launch stopped zeroing once the process
 *                  built another plan under the HIP runtime PyTorch bundles, round 6).  The ONLY form allowed on a
 *                  capturing stream (a replayed graph runs on the same set every time): MIFFT_E_INVALID otherwise.
 *   counters_next  a second buffer of the same size: the caller guarantees that `counters` is ALL ZERO when the launch starts, and
 *                  THIS launch zeroes `counters_next` -- a plan that alternates between two sets (set A zeroes B, B zeroes A) after
 *                  one initial mifft_memset of both never pays the memset again.
 *   error_word     a uint32 the kernel sets (system-scope store) when a bounded dependency wait times out = results INVALID; any
 *                  address the device can write: pinned host memory from mifft_host_alloc (device-accessible under the same
 *                  pointer; the host then reads it without a copy), or NULL = word [1] of `counters` -- in the single-set form only:
 *                  with counters_next the next launch zeroes that word, so the two-set form REQUIRES an error word of its own
 *                  (MIFFT_E_INVALID otherwise).  A word of the caller's is never cleared by the library.
 */
typedef struct mifft_fused_sync {
    void *counters;
    void *counters_next;
    void *error_word;
} mifft_fused_sync;
/* 1 <= lag < ring_slots, MIFFT_E_INVALID otherwise.  A pair of descriptors without a kernel (mifft_fused2_kernel below) is refused
 * BEFORE `sync` is looked at: such a call neither validates the sync block nor zeroes a counter set, and a call with both a bad sync
 * block and a shape without a kernel reports the shape. */
int mifft_launch_fused2(const mifft_pass *p0, const mifft_pass *p1, const void *in0, const void *in1, void *out0,
                        void *out1, void *ring0, void *ring1, int32_t ring_slots, int32_t lag, const mifft_fused_sync *sync,
                        int32_t grid, mifft_stream_t stream);

/* Which kernel form mifft_launch_fused2 runs for the two descriptors: a pure query (it never touches a device), the one selector the
 * launch itself goes through.  The answer also depends on the calling thread's development switches.  Returns a MIFFT_FUSED2_KERNEL_*
 * constant and, through tiles0 / tiles1 (either may be NULL), the work-list tiles per transform of the two passes; else the error code
 * (with its message) mifft_launch_fused2 gives for the descriptors before it looks at a buffer.  docs/persistent.md has the table of
 * forms, their work-groups, tile widths and shapes. */
#define MIFFT_FUSED2_KERNEL_1D          1  /* 1-D, 256-thread tiles of 16 columns in both passes (fft_fused2_kernel) */
#define MIFFT_FUSED2_KERNEL_1D_SIBLINGS 2  /* 1-D fp32 planes, two sibling 16-column tiles per 512-thread work-group (fft_fused2s_kernel) */
#define MIFFT_FUSED2_KERNEL_1D_WIDE     3  /* 1-D fp32 interleaved, 256-thread tiles of 32 columns in both passes (fft_fused2w_kernel) */
#define MIFFT_FUSED2_KERNEL_1D_MIXED    4  /* 1-D fp32 interleaved 1024 x 512: 16 columns, then 32 (fft_fused2m_kernel) */
#define MIFFT_FUSED2_KERNEL_2D          5  /* 2-D as two transposing passes, 256-thread tiles of 16 columns (fft_fused2d_kernel) */
#define MIFFT_FUSED2_KERNEL_2D_WIDE     6  /* ... fp32 interleaved, 32 columns in the pass of an axis <= 512 (fft_fused2dw_kernel) */
#define MIFFT_FUSED2_KERNEL_1D_BIG      7  /* 1-D, 512-thread tiles of 16 columns (fft_fused3_kernel) */
#define MIFFT_FUSED2_KERNEL_2D_BIG      8  /* 2-D as two transposing passes, 512-thread tiles of 16 columns (fft_fused3d_kernel) */
#define MIFFT_FUSED2_KERNEL_2D_ROWFIRST 9  /* 2-D fp32 planes in the chain's order: groups of 16 rows, then 16-column tiles (fft_fused2r_kernel) */
#define MIFFT_FUSED2_KERNEL_1D_CHAIN64  10 /* 1-D fp64 2048-point first pass, 1024-thread stage-chain tiles of 8 / 16 columns (fft_fusedx64_kernel) */
int mifft_fused2_kernel(const mifft_pass *p0, const mifft_pass *p1, uint32_t *tiles0, uint32_t *tiles1);

/*
 * Persistent form of a 3-D plan made of two PASS PAIRS (mifft_pair_split > 0): passes[0..3] = ROW x | COL y (R0) | COL y (R1) |
 * COL z as the chain holds them.  Work list as in mifft_launch_fused2 with the (ROW x, COL y R0) tiles as first-pass items and the
 * (COL y R1, COL z) tiles as second-pass items; the buffer between the two pairs is a ring of `ring_slots` whole transforms
 * (interleaved) that stays in the last-level cache.  Exists for the cubes whose transform is a fraction of that cache:
 *   mifft_fused_pair_supported   0 if (precision, layout, x, y, z) has such a kernel, else MIFFT_E_UNSUPPORTED.  Split-complex user
 *                                buffers (in1 / out1 = the imaginary planes, layout MIFFT_SPLIT in the descriptors, the ring
 *                                interleaved: MIFFT_FLAG_DST_INTERLEAVED on passes[1], MIFFT_FLAG_SRC_INTERLEAVED on passes[2]):
 *                                the same shapes
 *   mifft_fused_pair_split       the factor R0 of the y axis that kernel is built for (y = R0 * R1), 0 if there is none.  For the
 *                                128^3 cubes it equals mifft_pair_split; the other shapes (64- and 128-point axes) have NO plain
 *                                pair launches -- their chain is a plane pass + a strided z pass -- and the caller builds the
 *                                four-pass list for this launch alone
 * Reference shape of the work: pyfft/plan.py:160-167 (one chain per axis), published row doc/source/index.rst:373 (128^3).
 */
int mifft_fused_pair_supported(int32_t precision, int32_t layout, int32_t x, int32_t y, int32_t z);
int mifft_fused_pair_split(int32_t precision, int32_t layout, int32_t x, int32_t y, int32_t z);
int mifft_launch_fused_pair(const mifft_pass *passes, const void *in0, const void *in1, void *out0, void *out1, void *ring0,
                            int32_t ring_slots, int32_t lag, const mifft_fused_sync *sync, int32_t grid, mifft_stream_t stream);

/*
 * ---- extensions the reference lists as TODO (TODO.txt:6-8): tiles of a bigger array, sizes that are not powers of two ----
 * Both are built from the power-of-two plans plus two streaming helpers (pyfft_amd/generic.py):
 *   mifft_aux_copy      general strided complex copy over an index space of up to 6 dimensions (dims[0] fastest): gathers the
 *                       tiles of a parent array, or the lines of one axis, into dense rows and scatters them back.  Element
 *                       = one complex number of `precision`; either side may be two scalar planes.  Optional, in this order:
 *                       zero fill for dims[0] indices >= src_valid0 (0 = no padding), conjugation of the input, a complex
 *                       multiplier mult[i0] (device table of dims[0] entries; the chirp of Bluestein's algorithm), a real
 *                       scale, conjugation of the output.  Strides are in elements.
 *   mifft_aux_mul_rows  a[r][j] *= b[j] for `rows` dense rows of n complex numbers (interleaved).
 */
/*
 * Tiled batches in ONE launch (csrc/fft_nd2t.hpp): a MIFFT_PASS_ND pass (L, M, S = the TILE's x, y, z; interleaved) whose
 * `outer` transforms are the non-overlapping tiles of `outer / (cx*cy*cz)` parent arrays, taken from and written to their places
 * in the parent -- tile g = item*(cx*cy*cz) + (iz*cy + iy)*cx + ix starts at item*parent_elems + iz*z*pitch_z + iy*y*pitch_y + ix*x.
 * In place or out of place (same geometry on both sides).  Exists for a list of tile shapes only:
 *   mifft_nd_tiled_supported  0 if the tile shape has such a kernel, else MIFFT_E_UNSUPPORTED
 * mifft_launch_nd_tiled_split is the same launch on split-complex parents (pass->layout = MIFFT_SPLIT; re / im planes with the
 * same element offsets on both sides), for the same list of tile shapes.
 */
typedef struct mifft_tiling {
    int64_t pitch_y;       /* elements between consecutive y of the parent array (its x extent) */
    int64_t pitch_z;       /* elements between consecutive z of the parent array (x extent * y extent) */
    int64_t parent_elems;  /* elements per parent array */
    int32_t cx, cy, cz;    /* tiles per parent axis */
} mifft_tiling;
int mifft_nd_tiled_supported(int32_t precision, int32_t x, int32_t y, int32_t z);
int mifft_launch_nd_tiled(const mifft_pass *pass, const mifft_tiling *tiling, const void *in, void *out, mifft_stream_t stream);
int mifft_launch_nd_tiled_split(const mifft_pass *pass, const mifft_tiling *tiling, const void *in_re, const void *in_im, void *out_re,
                                void *out_im, mifft_stream_t stream);

typedef struct mifft_copy {
    int32_t precision;          /* MIFFT_F32 | MIFFT_F64 */
    int32_t ndim;               /* 1 .. 6 */
    int64_t dims[6];
    int64_t src_stride[6];
    int64_t dst_stride[6];
    int64_t src_valid0;         /* source extent along dims[0]; larger indices read as zero (0: all valid) */
    int32_t src_split;          /* source is two scalar planes (src0 = re, src1 = im) */
    int32_t dst_split;
    int32_t conj_in;
    int32_t conj_out;
    const void *mult;           /* device: dims[0] complex multipliers, or NULL */
    double  scale;
} mifft_copy;
int mifft_aux_copy(const mifft_copy *copy, const void *src0, const void *src1, void *dst0, void *dst1, mifft_stream_t stream);
int mifft_aux_mul_rows(int32_t precision, void *a, const void *b, int64_t rows, int64_t n, mifft_stream_t stream);
/* Verification helper (round 6; no counterpart in the reference, whose tests copy everything to the host: test/test_errors.py:66-114):
 * ADDS to *count the number of 16-byte words in which a[0 .. nbytes) and b[0 .. nbytes) differ.  a, b 16-byte aligned device buffers,
 * nbytes a multiple of 16; count = any 8-byte aligned uint64 the device can add to atomically (device memory, or pinned host memory from
 * mifft_host_alloc, which the host then reads after synchronising `stream`).  Lets a caller check a periodic data set's result -- every
 * transform bit-identical to its period-mate -- over a buffer far too large to copy back. */
int mifft_aux_count_mismatch(const void *a, const void *b, size_t nbytes, uint64_t *count, mifft_stream_t stream);

/*
 * Mixed-radix rows (csrc/fft_mixed.hip; the reference's TODO.txt:8): `rows` contiguous transforms of SMOOTH length
 * n = 2^a 3^b 5^c 7^d, 2 <= n <= 4096 (fp32) / 2048 (fp64), interleaved, row r at element r * stride on either side, in place or
 * out of place; tw = device table of n entries w(n)^m.  out = scale * DFT(in) (inverse: conjugated in and out).
 *   mifft_mixed_supported  0 if rows of n points have such a kernel, else MIFFT_E_UNSUPPORTED
 */
int mifft_mixed_supported(int32_t precision, int32_t n);
/* The radix list the mixed-radix kernels run for a smooth length n (2 <= n <= 2^24), in stage order: host only, no device needed.
 * Returns the number of stages (at most MIFFT_MIXED_MAX_STAGES, written to radix[0 ..]) or MIFFT_E_UNSUPPORTED (n not smooth). */
#define MIFFT_MIXED_MAX_STAGES 12
int mifft_mixed_radices(int32_t precision, int32_t n, int32_t *radix);
int mifft_launch_mixed_rows(int32_t precision, int32_t n, int64_t rows, int64_t stride_in, int64_t stride_out, const void *in,
                            void *out, const void *tw, int32_t inverse, double scale, mifft_stream_t stream);
/* The same transform along ANY axis of a dense array viewed as [outer][n][inner] (inner = product of the faster axes; inner == 1
 * is the row form): line (o, j) starts at o*n*inner + j, its points are `inner` apart; a work-group takes adjacent lines, so the
 * accesses coalesce across lines.  conj_in / conj_out conjugate on load / store separately (an N-D inverse conjugates once at
 * either end of its chain of launches).  In place or out of place. */
int mifft_launch_mixed_lines(int32_t precision, int32_t n, int64_t outer, int64_t inner, const void *in, void *out, const void *tw,
                             int32_t conj_in, int32_t conj_out, double scale, mifft_stream_t stream);
/* LONG smooth lengths, N = n1 * n2 beyond one tile, in two launches (four-step form without a separate transposition): lines of n1
 * points n2 apart, stored as rows and multiplied by w(N)^(k1 * i2) into `mid`; then lines of n2 points n1 apart from `mid` to `out`
 * in place order = natural order.  `mid` must not be `in`; it may be `out` (out-of-place transforms need no scratch).
 *   mifft_mixed_long_split   0 and the factors (both with a mixed-radix kernel, as many adjacent lines per tile as possible) or
 *                            MIFFT_E_UNSUPPORTED (N not smooth, N > 2^24, or no split with >= 8 (fp64: 4) lines per tile)
 *   tables: tw1 / tw2 = w(n1)^m / w(n2)^m; w(N)^e = tw_lo[e & (2^tw_shift - 1)] * tw_hi[e >> tw_shift], e < N */
int mifft_mixed_long_split(int32_t precision, int64_t n, int32_t *n1, int32_t *n2);
int mifft_launch_mixed_long(int32_t precision, int32_t n1, int32_t n2, int64_t batch, const void *in, void *mid, void *out,
                            const void *tw1, const void *tw2, const void *tw_lo, const void *tw_hi, int32_t tw_shift,
                            int32_t inverse, double scale, mifft_stream_t stream);
/* Bluestein's algorithm in ONE launch for rows of ANY length n whose padded length fits the LDS of a CU twice (2 n - 1 <= 10000 fp32 /
 * 5000 fp64; up to 4096 / 2048 several rows share a work-group): both m-point transforms of the convolution run inside LDS
 * (csrc/fft_mixed.hip).
 *   mifft_bluestein_padded   0 and the padded length m (smooth, >= 2 n - 1, the cheapest one) or MIFFT_E_UNSUPPORTED
 *   tables: tw = w(m)^j (m entries); chirp c[j] = exp(-i pi j^2 / n) (n entries); bhat = FFT_m(b) / m with b[j] = conj(c[j]) for
 *   j < n, b[m - j] = b[j], zero between (m entries).  out = scale * DFT(in) (inverse: conjugated in and out). */
int mifft_bluestein_padded(int32_t precision, int32_t n, int32_t *m);
int mifft_launch_bluestein_rows(int32_t precision, int32_t n, int32_t m, int64_t rows, int64_t stride_in, int64_t stride_out,
                                const void *in, void *out, const void *tw, const void *chirp, const void *bhat, int32_t inverse,
                                double scale, mifft_stream_t stream);

/* Whole SMOOTH 2-D / 3-D transforms in one launch (csrc/fft_mixed_nd.hip): every axis of the (z, y, x) shape a smooth length (or 1), at
 * least two axes longer than 1, x * y * z <= 16384 points (fp32) / 8192 (fp64) -- the transform, or several, lives in one work-group's
 * LDS (one buffer; a stage holds its operands in registers across a barrier) between its first load and its last store.  `transforms` dense arrays one after the other, interleaved, in place or out of place;
 * tw_x / tw_y / tw_z = device tables w(len)^m of the axis lengths (NULL for an axis of length 1).  out = scale * DFT3(in);
 * inverse: 0 forward, 1 inverse (input and output conjugated), 2 / 4 conjugate the input / the output only (the first / last launch
 * of a composition, e.g. the (y, x) planes of a bigger 3-D shape followed by mifft_launch_mixed_lines along z).
 *   mifft_mixed_nd_supported  0 if the shape has this form, else MIFFT_E_UNSUPPORTED */
int mifft_mixed_nd_supported(int32_t precision, int32_t x, int32_t y, int32_t z);
int mifft_launch_mixed_nd(int32_t precision, int32_t x, int32_t y, int32_t z, int64_t transforms, const void *in, void *out,
                          const void *tw_x, const void *tw_y, const void *tw_z, int32_t inverse, double scale, mifft_stream_t stream);

/* Real-input transforms (docs/extensions.md "Real-input transforms").  A real array of shape (nz, ny, nx) read as interleaved complex
 * numbers is the packed array z of shape (nz, ny, nx / 2); a complex transform of z plus one separation step gives the half spectrum
 * X of shape (nz, ny, nx / 2 + 1) (numpy's rfftn layout), and one packing step plus an inverse complex transform undoes it.
 * mifft_launch_real_post enqueues that step, one streaming launch over `outer` items:
 *   inverse 0 (separation)  in = Z = FFT(z), nx / 2 complex numbers per row -> out = scale * X, nx / 2 + 1 per row
 *   inverse 1 (packing)     in = X -> out = scale * Z' with IFFT(Z') (unnormalised) = the unnormalised inverse real transform of X,
 *                           packed; the edge planes kx = 0 and kx = nx / 2 are read through their Hermitian parts
 * Rows are dense within an item; stride_in / stride_out are the item pitches in complex numbers (at least the item's size on that
 * side).  tw = device table w(nx)^k, k = 0 .. nx / 2 (nx / 2 + 1 entries, the precision's complex type).  Out of place only: in and out
 * must not overlap.  nx >= 2, ny, nz >= 1, all powers of two; buffers aligned to one complex number. */
typedef struct mifft_real_post {
    int32_t precision;   /* MIFFT_F32 / MIFFT_F64 */
    int32_t inverse;     /* 0 separation, 1 packing */
    int32_t nx, ny, nz;  /* REAL shape of one item: x contiguous */
    int32_t reserved;    /* 0 */
    int64_t outer;       /* items */
    int64_t stride_in;   /* item pitch of `in`, complex numbers */
    int64_t stride_out;  /* item pitch of `out`, complex numbers */
    const void *in;
    void *out;
    const void *tw;
    double scale;
} mifft_real_post;
int mifft_launch_real_post(const mifft_real_post *desc, mifft_stream_t stream);

/* One-launch real-input rows: forward, `rows` real rows of n points (dense, n reals each) -> their half spectra (dense, n / 2 + 1
 * complex numbers each), = scale * numpy.fft.rfft per row; inverse, half spectra -> real rows, = scale * the unnormalised inverse real
 * transform (X[0] and X[n / 2] through their real parts).  The row transform of the n / 2 packed points and the separation / packing
 * run in one work-group, so a row crosses HBM once.  tw_half = device table w(n / 2)^k (n / 2 entries), tw_sep = w(n)^k (n / 2 + 1
 * entries), the precision's complex type.  Out of place only.
 *   mifft_real_row_supported   0 if a kernel exists for the real length n (every n / 2 with a ROW kernel, n >= 4: up to 65536 fp32,
 *                              32768 fp64), else MIFFT_E_UNSUPPORTED */
int mifft_real_row_supported(int32_t precision, int32_t n);
int mifft_launch_real_row(int32_t precision, int32_t n, int32_t inverse, int64_t rows, const void *in, void *out, const void *tw_half,
                          const void *tw_sep, double scale, mifft_stream_t stream);

/* Convolution rows (docs/extensions.md "Convolution plans"): y = scale * IFFT(FFT(x) * S) per row in ONE launch, S = H or, with
 * correlate = 1, conj(H); IFFT unnormalised (the caller folds 1 / n into scale).  real = 0: rows of n interleaved complex numbers, H n
 * complex numbers; real = 1: rows of n reals, H the n / 2 + 1 point half spectrum (numpy's rfft layout; H[0] and H[n / 2] products
 * through their real parts, as numpy's irfft).  rows dense; in == out (in place) or disjoint.  spectrum_pitch: complex numbers between
 * the spectra of consecutive rows, 0 = one spectrum shared by every row; the spectrum must not overlap in or out and is never written.
 * tw = device table w(L)^k (L = n complex, n / 2 real), tw_sep = w(n)^k (n / 2 + 1 entries; real only), the precision's complex type.
 *   mifft_conv_row_supported   0 if a kernel exists for (precision, real, n), else MIFFT_E_UNSUPPORTED
 *   mifft_aux_mul_spectrum     data[i][j] *= scale * S[i * spectrum_pitch + j], items x points interleaved complex numbers (the composed
 *                              form's spectrum product) */
int mifft_conv_row_supported(int32_t precision, int32_t real, int32_t n);
int mifft_launch_conv_row(int32_t precision, int32_t real, int32_t n, int64_t rows, const void *in, void *out, const void *spectrum,
                          int64_t spectrum_pitch, int32_t correlate, const void *tw, const void *tw_sep, double scale, mifft_stream_t stream);
int mifft_aux_mul_spectrum(int32_t precision, void *data, const void *spectrum, int64_t items, int64_t points, int64_t spectrum_pitch,
                           int32_t correlate, double scale, mifft_stream_t stream);

/* Overlap-save FIR rows (docs/extensions.md "FIR filtering plans"): y[i][t] = scale * sum_j h[j] x[i][t - j], 0 <= t < length, x[i][< 0] = 0,
 * for `items` signals in ONE launch and without scratch.  Every block of n points (real = 1: n reals) runs as a convolution row
 * (transform, product with `spectrum`, unnormalised inverse: the caller folds 1 / n into scale); block r of an item starts at element
 * r * hop - overlap of the item, hop = n - overlap, takes zeros outside [0, length) and stores its elements overlap .. n - 1 that fall
 * inside [0, length).  No address outside [i * pitch, i * pitch + length) of either side is accessed.  overlap, length and pitch count
 * elements (complex numbers; real = 1: reals): 0 <= overlap <= n / 2 (the filter has at most overlap + 1 taps), length >= 1,
 * pitch >= length; real = 1: overlap and pitch even (length may be odd).  spectrum: the n (real = 1: n / 2 + 1) point spectrum of the
 * zero-padded taps; spectrum_pitch: complex numbers between the spectra of consecutive ITEMS, 0 = one shared by all; it must not
 * overlap in or out and is never written.  in and out must not overlap.  tw, tw_sep: as for mifft_launch_conv_row.  Bases aligned to
 * one complex number (real data: one pair of reals).
 *   mifft_fir_row_supported   0 if a kernel exists for (precision, real, n), else MIFFT_E_UNSUPPORTED
 *   mifft_launch_fir_pad      out[f][j] = j < taps ? in[f * taps + j] : 0, j < n: `filters` filters of `taps` elements (complex numbers;
 *                             real = 1: reals) zero-padded to n each; out 16-byte aligned, in aligned to one element, no overlap */
int mifft_fir_row_supported(int32_t precision, int32_t real, int32_t n);
int mifft_launch_fir_row(int32_t precision, int32_t real, int32_t n, int32_t overlap, int64_t length, int64_t pitch, int64_t items, const void *in,
                         void *out, const void *spectrum, int64_t spectrum_pitch, const void *tw, const void *tw_sep, double scale,
                         mifft_stream_t stream);
int mifft_launch_fir_pad(int32_t precision, int32_t real, int32_t n, int32_t taps, int64_t filters, const void *in, void *out, mifft_stream_t stream);

/* Cosine and sine transforms (docs/extensions.md "Real-to-real transforms"): DCT-II / DST-II forward and DCT-III / DST-III inverse
 * (scipy.fft's type 2 and 3) by Makhoul's algorithm, composed as pre step -> complex transform of the packed data -> post step.  An
 * item is a dense real array of shape n[0 .. ndim - 1] (numpy order, the last axis contiguous; every axis a power of two >= 2); v, its
 * per-axis permutation [x0, x2, x4, ..., x5, x3, x1] (DST: x[j] signed by (-1)^(sum of its indices) first), read as interleaved complex
 * numbers is the packed array z of shape (..., n_last / 2), the same bytes.
 *   mifft_launch_r2r_pre   inverse 0: in = x -> out = scale * v  (the permutation; ndim 1 with n[0] = 1 is a one-point item, in == out
 *                                     allowed)
 *                          inverse 1: in = Y -> out = Z' with IFFT(Z') (unnormalised) = the type III transform's packed v, times the
 *                                     factor the tables carry
 *   mifft_launch_r2r_post  inverse 0: in = Z = FFT(z) -> out = Y, the type II transform times the factor the tables carry
 *                          inverse 1: in = v -> out = scale * x  (the inverse permutation; the one-point item as above)
 * tw (the twiddle steps only): the per-axis tables in axis order, n[a] entries each -- forward t[k] = c[k] w(4n)^k, inverse
 * u[k] = w(4n)^-k / (2 c[k]), c the ortho weight or 1, the last axis's times the global factor (forward: 1/2 for the separation) --
 * followed by w(n_last)^k, k = 0 .. n_last / 4 (n_last / 4 + 1 entries; 1 for n_last = 2), the precision's complex type.
 * kind 0 DCT, 1 DST (Y read / written backwards on every axis).  Items dense on both sides; in and out must not overlap; real buffers
 * aligned to one real number, the packed side and tw to one complex number. */
typedef struct mifft_r2r_step {
    int32_t precision;   /* MIFFT_F32 / MIFFT_F64 */
    int32_t inverse;     /* 0 forward (type II), 1 inverse (type III) */
    int32_t kind;        /* 0 DCT, 1 DST */
    int32_t ndim;        /* 1 .. 3 */
    int32_t n[3];        /* the item's axes, numpy order */
    int32_t reserved;    /* 0 */
    int64_t outer;       /* items */
    const void *in;
    void *out;
    const void *tw;
    double scale;        /* the permutation steps' factor */
} mifft_r2r_step;
int mifft_launch_r2r_pre(const mifft_r2r_step *desc, mifft_stream_t stream);
int mifft_launch_r2r_post(const mifft_r2r_step *desc, mifft_stream_t stream);
/* One-launch cosine / sine rows: `rows` dense rows of n reals, forward y = the type II transform times the factor tab carries,
 * inverse x = the type III transform likewise (the same algorithm as the steps above, in one work-group: the row crosses HBM once).
 * tw_stage = w(n/2)^k (n/2 entries), tw_sep = w(n)^k (n/2 entries), tab = forward t'[k] = 2 g c[k] w(4n)^k (n/2 + 1 entries) or inverse
 * u[k] = g w(4n)^-k / 2c[k] (n entries), g the factor, c the ortho weight or 1; the precision's complex type.  kind 0 DCT, 1 DST.  in == out
 * (in place) or disjoint; in and out 16-byte aligned.
 *   mifft_r2r_row_supported   0 if a kernel exists for the real length n (4 ... 8192, fp32 and fp64), else MIFFT_E_UNSUPPORTED */
int mifft_r2r_row_supported(int32_t precision, int32_t n);
int mifft_launch_r2r_row(int32_t precision, int32_t n, int32_t inverse, int32_t kind, int64_t rows, const void *in, void *out,
                         const void *tw_stage, const void *tw_sep, const void *tab, mifft_stream_t stream);

/* Half-precision (complex32) transforms (docs/extensions.md "Half-precision transforms"): interleaved fp16 data, one fp16 real and one
 * fp16 imaginary part per point (4 bytes).  Loads widen to fp32 exactly, every stage runs in fp32 on the fp32 twiddle tables, and the
 * result (times scale, in fp32) is rounded to fp16 once, to nearest even, at the store: beyond +-65504 it is +-inf, NaN stays NaN.
 * One launch over `transforms` dense transforms of the (z, y, x) shape, x contiguous; in place (in == out) or out of place.
 *   mifft_half_supported   0 for the one-launch shapes of interleaved fp32 data -- 1-D rows (y = z = 1) of 2 ... 32768 points, and
 *                          every shape with y or z > 1 for which mifft_nd_shape_supported(MIFFT_F32, x, y, z,
 *                          MIFFT_VARIANT_INTERLEAVED_ONLY) is 0 -- else MIFFT_E_UNSUPPORTED
 *   mifft_half_kernel      the kernel family such a shape runs after its unit axes are dropped (MIFFT_HALF_KERNEL_*), else
 *                          MIFFT_E_UNSUPPORTED.  variant 0: the fixed-shape N-D kernel where one exists; variant 1: the run-time-
 *                          shaped one wherever it takes the shape (up to mifft_nd_max_points_for(MIFFT_F32) points), as variant 1
 *                          of an fp32 MIFFT_PASS_ND pass does; 1-D rows ignore it
 *   mifft_launch_half      tw_x / tw_y / tw_z = device tables w(len)^k, k < len, of complex64 numbers (8-byte aligned; null for an axis
 *                          of one point); in / out 16-byte aligned, equal or not overlapping; inverse 0 forward, 1 unnormalised
 *                          inverse (conjugate exponent), both times `scale`; variant as for mifft_half_kernel. */
#define MIFFT_HALF_KERNEL_TILE 1  /* LDS-staged ROW tile (fft_tile.hpp), rows of 2 ... 128 points */
#define MIFFT_HALF_KERNEL_ROW  2  /* register-edged row (fft_row2.hpp), 256 ... 32768 points */
#define MIFFT_HALF_KERNEL_ND2  3  /* fixed-shape N-D kernel (fft_nd2.hpp) */
#define MIFFT_HALF_KERNEL_ND   4  /* run-time-shaped N-D kernel (fft_nd.hpp), up to 16384 points */
int mifft_half_supported(int32_t x, int32_t y, int32_t z);
int mifft_half_kernel(int32_t x, int32_t y, int32_t z, int32_t variant);
int mifft_launch_half(int32_t x, int32_t y, int32_t z, int32_t variant, int32_t inverse, int64_t transforms, const void *in, void *out, const void *tw_x,
                      const void *tw_y, const void *tw_z, double scale, mifft_stream_t stream);

/* Same as mifft_launch_chain but brackets the chain with two events on `stream` and, after
 * synchronising, reports the elapsed device time of `repeats` back-to-back chains. (bench/test helper) */
int mifft_time_chain(const mifft_pass *passes, int32_t npasses, void *const bufs0[3], void *const bufs1[3],
                     mifft_stream_t stream, int32_t repeats, float *ms_total);

#ifdef __cplusplus
}
#endif
#endif /* MIFFT_H */
