// Fused two-pass kernels for a long contiguous axis N = L0 * L1 -- fp32: L0, L1 in {256, 512, 1024} on the 256-thread tiles
// of fft_col2.hpp, 2048 x 2048 / 2048 x 1024 on the 512-thread tiles of fft_col3.hpp; fp64: 1024 x 1024 -- and for the 2-D
// squares 512 / 1024 / 2048 (fp32) and 1024 (fp64): both Stockham
// passes of every transform run inside ONE persistent launch, in dependency order, so the inter-pass
// intermediate of a transform is consumed a few transforms later while it is still in the 256 MiB Infinity
// Cache, and there are no launch boundaries (with 128 KiB tiles a cache-sized chunk is only ~2 machine-waves
// of tiles, so per-chunk launches lose the cache gain to their tails).
//
// Work list (one global ticket counter): group g holds the pass-0 tiles of transform g interleaved with the
// pass-1 tiles of transform g - lag.  Dependencies, all on LOWER ticket numbers (=> no deadlock for any
// dispatch order / placement / residency):
//     pass-1 tile of t   waits until all pass-0 tiles of t have published            (wdone[t] == tiles0)
//     pass-0 tile of t   waits until all pass-1 tiles of t - ring have finished reading the ring slot it
//                        is about to overwrite                                       (rdone[t-ring] == tiles1)
// Hand-off (cdna_hip_programming.md Guideline 16, write-through form): the intermediate is written with
// agent-coherent write-through stores, every storing wave drains vmcnt, the work-group barrier, one lane bumps
// the counter (relaxed, agent scope); the consumer's one lane polls relaxed, ONE acquire fence, vmcnt drain,
// barrier, then plain loads.  (A release fence per tile -- buffer_wbl2 -- made this kernel 2x slower than two
// launches.)  The scratch ring is always interleaved, also for split-plane user buffers (SPLIT: the input of
// pass 0 and the output of pass 1 are two scalar planes).
// Every spin is bounded; on timeout an error word is set (the host checks it) instead of hanging the GPU.
#pragma once
#include "fft_col2.hpp"
#include "fft_col2w.hpp"
#include "fft_col3.hpp"

namespace mifft {

constexpr unsigned kFusedCS = 64u;   // words between two counters (= MIFFT_FUSED2_COUNTER_STRIDE)

// the work list and its synchronisation state (shared by every persistent kernel: fft_fused2 / fused3 / fusedp)
struct FusedCtl {
    unsigned* counters;  // [0] ticket, [1] error (when `err` points here), then one counter per CS = 64 words (256 bytes): wdone[t] at
                         // CS * (1 + t), rdone[t] at CS * (1 + batch + t); ALL ZERO when the launch starts
    unsigned* counters_next;   // nullptr, or a second counter set that THIS launch zeroes for the next one (round 4: a plan alternates
                               // between two sets, so no memset node precedes the launch)
    unsigned* err;       // error word, set on a dependency time-out (device-accessible: counters + 1, or pinned host memory)
    unsigned lines;      // counter lines per set (9 + 2 * batch)
    unsigned batch;      // number of transforms
    unsigned lag;        // pass 1 of transform t is queued with pass 0 of transform t + lag; 1 <= lag < ring (the launchers refuse 0)
    unsigned ring;       // scratch ring slots (transforms); ring > lag
    unsigned tiles0;     // tiles per transform in pass 0
    unsigned tiles1;     // tiles per transform in pass 1
};

struct FusedArgs {
    TileArgs p0;         // pass 0: in = user input,  out = scratch ring (matrix index = ring slot)
    TileArgs p1;         // pass 1: in = scratch ring, out = user output
    FusedCtl c;
};

// Deferred publish of a pass-0 tile: its write-through stores drain under the first poll of the NEXT item's dependency, and
// the counter is bumped BEFORE this work-group starts to wait.  (Publishing only after the wait has ended deadlocks: work-group
// X owes a tile of transform T and waits for U while Y owes a tile of U and waits for T -- measured as dependency time-outs.)
struct FusedPending {
    unsigned* ctr;   // wdone counter still to be bumped, or nullptr
};

// wait until *ctr >= target (one lane polls, bounded); ACQ: also make other work-groups' published data visible.
// `seen` is lane 0's EARLY poll of the same counter, issued from the middle of the previous tile (FusedHook below): an agent-scope load takes 1-3 us
// under load, and with the poll on the critical path of every item the kernel lost 16 % (C2: 22.5 ms; with no waits at all --
// wrong results, same traffic -- 18.9 ms).  The counters only grow, so a stale value can only under-estimate.
template <bool ACQ> __device__ __forceinline__ void fused_wait_ge(unsigned* ctr, unsigned target, unsigned seen, unsigned* err, FusedPending& pend) {
    if (pend.ctr != nullptr) {   // (uniform) the owed tile: every wave drains its stores, the barrier joins them, lane 0 publishes
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(pend.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pend.ctr = nullptr;
    }
    if (threadIdx.x == 0) {
        unsigned spins = 0;
        while (seen < target) {          // (the early value was not enough: look again, then sleep between polls)
            seen = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen >= target) break;
            __builtin_amdgcn_s_sleep(32);
            if (++spins > (1u << 22)) {  // ~ seconds: never hang the GPU
                __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (may be pinned host memory)
                break;
            }
        }
        if constexpr (ACQ) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
}

// publish now: every wave drains its own memory operations, the work-group barrier joins them, one lane bumps the counter.
// (The data a later tile depends on was written with write-through stores, so no release fence is needed.)
__device__ __forceinline__ void fused_flush(FusedPending& pend) {
    if (pend.ctr != nullptr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(pend.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pend.ctr = nullptr;
    }
}

// "this tile has finished READING" (pass 1 and its ring slot): every load has been consumed by the time the tile's last
// butterflies ran, so the stores of the result are not waited for.
__device__ __forceinline__ void fused_signal_read(unsigned* ctr) {
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Lane 0's view of the work list: the ticket of the next item (drawn at the top of this one) and the early poll of that item's
// dependency counter (issued from the middle of this tile, TileHook below).  Both returning atomics are consumed at the top of
// the next item, so neither latency is on the critical path.
struct FusedQueue {
    unsigned t1, seen1;
};

struct FusedItem {
    unsigned pass;     // 0, 1, or 2 = nothing to do (fill / drain of the pipeline)
    unsigned t;        // transform
    unsigned slot;     // its ring slot
    unsigned tile;
    unsigned* dep;     // counter this item waits for (nullptr: none)
    unsigned target;
};

// it.t is the transform, it.slot its ring slot
template <unsigned PER0, unsigned PER1>
__device__ __forceinline__ FusedItem fused_decode(const FusedCtl& f, unsigned item, unsigned gsize, unsigned* wdone, unsigned* rdone) {
    FusedItem it;
    it.dep = nullptr;
    it.target = 0;
    if (f.lag == 0u) {   // unreachable (the launchers refuse lag == 0); removing it changes the kernels: a follow-up with measurements
        const unsigned n0 = f.batch * f.tiles0;
        if (item < n0) {
            it.pass = 0u;
            it.t = item / f.tiles0;
            it.tile = item % f.tiles0;
        } else {
            it.pass = 1u;
            it.t = (item - n0) / f.tiles1;
            it.tile = (item - n0) % f.tiles1;
            it.dep = wdone + kFusedCS * it.t;
            it.target = f.tiles0;
        }
        it.slot = it.t;
        return it;
    }
    constexpr unsigned period = PER0 + PER1;
    const unsigned g = item / gsize, k = item % gsize, j = k / period, m = k % period;
    if (m < PER0) {
        it.pass = g < f.batch ? 0u : 2u;
        it.t = g;
        it.slot = g % f.ring;
        it.tile = j * PER0 + m;
        if (it.pass == 0u && g >= f.ring) {
            it.dep = rdone + kFusedCS * (g - f.ring);   // the ring slot it overwrites has been read
            it.target = f.tiles1;
        }
    } else {
        it.pass = g >= f.lag ? 1u : 2u;
        it.t = g - f.lag;
        it.slot = (g - f.lag) % f.ring;
        it.tile = j * PER1 + (m - PER0);
        if (it.pass == 1u) {
            it.dep = wdone + kFusedCS * it.t;           // every pass-0 tile of the transform has published
            it.target = f.tiles0;
        }
    }
    return it;
}

// lane 0 only: hand out this item's ticket and its early poll, draw the next ticket.  (`stat`: lag == 0, unreachable.)
__device__ __forceinline__ unsigned fused_advance(FusedQueue& q, unsigned& seen, unsigned total, unsigned* next, bool stat) {
    const unsigned item = q.t1;
    seen = q.seen1;
    q.seen1 = 0u;     // "not polled yet" (the hook of this item's tile sets it)
    if (item < total) q.t1 = stat ? item + gridDim.x : __hip_atomic_fetch_add(next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return item;
}

// The early poll.  A dependency is typically 20-50 us old when its consumer arrives (measured: 2 % younger than 10 us), so a
// poll from the middle of the previous tile (~8 us earlier) almost always sees it; one item earlier it fails three times in four.
template <unsigned PER0, unsigned PER1> struct FusedHook {
    const FusedCtl& f;
    FusedQueue& q;
    unsigned total, gsize;
    unsigned *wdone, *rdone;
    __device__ __forceinline__ void operator()() const {
        if (threadIdx.x == 0 && q.t1 < total) {
            const FusedItem nx = fused_decode<PER0, PER1>(f, q.t1, gsize, wdone, rdone);
            if (nx.dep != nullptr) q.seen1 = __hip_atomic_load(nx.dep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

// the work list, drained by this work-group together with every other one
template <unsigned PER0, unsigned PER1, bool EARLY, typename TILE0, typename TILE1>
__device__ __forceinline__ void fused_list(const FusedCtl& f, unsigned* s_item, TILE0& tile0, TILE1& tile1, FusedPending& pend) {
    unsigned* const err = f.err;
    unsigned* const next = f.counters;
    // One counter per 256-byte line: the counters of the few transforms in flight are polled and bumped by all 512 work-groups,
    // and packed 32 to a line they shared one memory channel's atomic unit (C2 with no polls at all -- wrong results, same
    // traffic -- ran 15 % faster; hiding the poll LATENCY changed nothing: it is the rate of same-line agent-scope accesses).
    unsigned* const wdone = f.counters + kFusedCS;
    unsigned* const rdone = wdone + kFusedCS * f.batch;
    // a group = the tiles0 pass-0 tiles of transform g and the tiles1 pass-1 tiles of transform g - lag, interleaved in their
    // ratio (tiles0 : tiles1 = PER0 : PER1), so that no ticket is an empty item
    const unsigned gsize = f.tiles0 + f.tiles1;
    const unsigned total = f.lag == 0u ? f.batch * gsize : (f.batch + f.lag) * gsize;   // (lag == 0: unreachable)

    const bool stat = f.lag == 0u;
    FusedQueue q = {0u, 0u};
    if (threadIdx.x == 0) q.t1 = stat ? blockIdx.x : __hip_atomic_fetch_add(next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const FusedHook<PER0, PER1> hook = {f, q, total, gsize, wdone, rdone};
    for (;;) {
        __syncthreads();  // the previous item's LDS traffic and its s_item read are over
        unsigned seen = 0;
        if (threadIdx.x == 0) *s_item = fused_advance(q, seen, total, next, stat);
        __syncthreads();
        const unsigned item = *s_item;
        if (item >= total) break;
        const FusedItem it = fused_decode<PER0, PER1>(f, item, gsize, wdone, rdone);
        if (it.pass == 2u) {             // fill / drain of the pipeline: nothing to do, but never sit on a publish
            fused_flush(pend);
            continue;
        }
        if (it.pass == 0u) {
            if (it.dep != nullptr) fused_wait_ge<false>(it.dep, it.target, seen, err, pend);
            else fused_flush(pend);
            if constexpr (EARLY) tile0(it.t, it.slot, it.tile, hook);
            else tile0(it.t, it.slot, it.tile, TileNoHook());
            pend.ctr = wdone + kFusedCS * it.t;     // published behind the next item's dependency wait (or at the end)
        } else {
            // (reading the ring with sc1 loads instead of the acquire fence measured the same, and 8-byte sc1 loads at two
            // work-groups per CU are outside the hand-off forms MI355X_MICROARCH.md lists as validated: the fence stays)
            fused_wait_ge<true>(it.dep, it.target, seen, err, pend);
            if constexpr (EARLY) tile1(it.slot, it.t, it.tile, hook);
            else tile1(it.slot, it.t, it.tile, TileNoHook());
            fused_signal_read(rdone + kFusedCS * it.t);
        }
    }
    fused_flush(pend);   // never carry a publish out of the kernel
}

// one persistent work-group: TILE0(t, slot, tile, hook) / TILE1(slot, t, tile, hook) run one tile of pass 0 / pass 1
template <unsigned PER0, unsigned PER1, bool EARLY, typename TILE0, typename TILE1>
__device__ __forceinline__ void fused_loop(const FusedCtl& f, unsigned* s_item, TILE0&& tile0, TILE1&& tile1) {
    // the counter set of the NEXT launch (words 0 and 1 of every line: a counter, or ticket + error / census)
    if (f.counters_next != nullptr) {
        for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < f.lines; i += gridDim.x * blockDim.x) {
            f.counters_next[i * kFusedCS] = 0u;
            f.counters_next[i * kFusedCS + 1u] = 0u;
        }
    }
    FusedPending pend = {};
    fused_list<PER0, PER1, EARLY>(f, s_item, tile0, tile1, pend);
}

// NT: 0 = plain accesses on the streamed side, 1 = non-temporal loads of the input and stores of the output, 2 = non-temporal
// loads and write-through (sc1) stores of the output (A/B; non-temporal loads of the RING in pass 1 measured 0.6 % slower on C2)
// PAIR0 / PAIR1: the paired-lane streams of pass 0 / pass 1 (kPairIn | kPairOut, col2_tile PAIR_IN / PAIR_OUT: 16 bytes per lane on
// that side of the pass); fp32 interleaved 1024 x 1024 only.  The ring side keeps the hand-off: sc1 stores (16 bytes: the raw-buffer
// form of the fp64 ring), plain loads behind the acquire.
constexpr int kPairIn = 1, kPairOut = 2;
template <typename T, int A0, int A1, bool SPLIT, int NT, int PAIR0 = 0, int PAIR1 = 0>
__global__ void __launch_bounds__(256, 2) fft_fused2_kernel(const FusedArgs f) {
    static_assert((PAIR0 | PAIR1) == 0 || (sizeof(T) == 4 && A0 == 4 && A1 == 4 && !SPLIT && NT == 1), "paired lanes: <float, 4, 4, false, 1> only");
    constexpr int E0 = Col2Lds<A0, true, sizeof(cplx<T>)>::ELEMS, E1 = Col2Lds<A1, false, sizeof(cplx<T>)>::ELEMS;
    __shared__ __attribute__((aligned(16))) cplx<T> lds[E0 > E1 ? E0 : E1];
    __shared__ unsigned s_item;
    constexpr unsigned per0 = A0 > A1 ? 1u : (unsigned)(A1 / A0);   // tiles0 : tiles1 = L1 : L0 = A1 : A0
    constexpr unsigned per1 = A1 > A0 ? 1u : (unsigned)(A0 / A1);
    fused_loop<per0, per1, !SPLIT && sizeof(T) == 4>(   // early poll: C2 19.49 -> 19.32 ms; split planes 26.7 -> 25.6 ms WITHOUT it; fp64: no register to spare
        f.c, &s_item,
        [&](unsigned t, unsigned slot, unsigned tile, auto hook) {
            col2_tile<T, A0, true, true, SPLIT, true, NT != 0, false, false, false, (PAIR0 & kPairIn) != 0, (PAIR0 & kPairOut) != 0>(
                f.p0, (long long)t, (long long)slot, (long long)tile * 16, lds, hook);
        },
        [&](unsigned slot, unsigned t, unsigned tile, auto hook) {
            col2_tile<T, A1, false, false, false, NT == 2, false, NT == 1, SPLIT, false, (PAIR1 & kPairIn) != 0, (PAIR1 & kPairOut) != 0>(
                f.p1, (long long)slot, (long long)t, (long long)tile * 16, lds, hook);
        });
}

// Split-complex fp32 with the SIBLING tiles side by side (second batch of round 4).  A 16-column tile touches 64 bytes per row of
// each plane -- half of a 128-byte line; on the global list the tile that owns the other half runs on whatever XCD drew its ticket
// and every input line crosses the fabric twice (PMC 2.48 x the algorithmic bytes, profiles/r04v_pmc_traffic_split.log).  Here a
// work-group is 512 threads = two 256-thread tiles in lock step (same code, same barriers), each on its own half of the LDS array,
// and an item is the sibling pair: both halves of every line are requested by the same CU at the same time.  One work-group per CU
// (the two tiles take the registers of two ordinary work-groups).  TWOD: the 2-D data flow (two transposing passes, no twiddle).
template <int A0, int A1, bool TWOD, bool NT = false, bool SPLIT = true>
__global__ void __launch_bounds__(512, 2) fft_fused2s_kernel(const FusedArgs f) {
    constexpr int E0 = Col2Lds<A0, true, sizeof(cplx<float>)>::ELEMS, E1 = Col2Lds<A1, TWOD, sizeof(cplx<float>)>::ELEMS;
    constexpr int E = E0 > E1 ? E0 : E1;
    __shared__ __attribute__((aligned(16))) cplx<float> lds[2 * E];
    __shared__ unsigned s_item;
    constexpr unsigned per0 = A0 > A1 ? 1u : (unsigned)(A1 / A0);
    constexpr unsigned per1 = A1 > A0 ? 1u : (unsigned)(A0 / A1);
    fused_loop<per0, per1, false>(
        f.c, &s_item,
        [&](unsigned t, unsigned slot, unsigned item, auto hook) {
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            col2_tile<float, A0, true, !TWOD, SPLIT, true, NT, false, false, true>(f.p0, (long long)t, (long long)slot, (long long)item * 32, lds, hook, tid);
        },
        [&](unsigned slot, unsigned t, unsigned item, auto hook) {
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            col2_tile<float, A1, TWOD, false, false, false, false, NT, SPLIT, true>(f.p1, (long long)slot, (long long)t, (long long)item * 32, lds, hook, tid);
        });
}

// The 1-D kernel on the 32-column tiles of fft_col2w.hpp (round 4): fp32 interleaved, L0 >= L1 in {256, 512} (N = 2^16 ... 2^18);
// a tile is 32 columns, so a transform has L1 / 32 first-pass and L0 / 32 second-pass tiles.
template <int A0, int A1>
__global__ void __launch_bounds__(256, 2) fft_fused2w_kernel(const FusedArgs f) {
    constexpr int E0 = Col2wLds<true>::ELEMS, E1 = Col2wLds<false>::ELEMS;
    __shared__ __attribute__((aligned(16))) cplx<float> lds[E0 > E1 ? E0 : E1];
    __shared__ unsigned s_item;
    constexpr unsigned per0 = A0 > A1 ? 1u : (unsigned)(A1 / A0);
    constexpr unsigned per1 = A1 > A0 ? 1u : (unsigned)(A0 / A1);
    fused_loop<per0, per1, (A0 == 1)>(     // (the early dependency poll only where registers are to spare: L = 512 sits at the 256-VGPR limit)
        f.c, &s_item,
        [&](unsigned t, unsigned slot, unsigned tile, auto hook) {
            col2w_tile<A0, true, true, true, true, false>(f.p0, (long long)t, (long long)slot, (long long)tile * 32, lds, hook);
        },
        [&](unsigned slot, unsigned t, unsigned tile, auto hook) {
            col2w_tile<A1, false, false, false, false, true>(f.p1, (long long)slot, (long long)t, (long long)tile * 32, lds, hook);
        });
}

// N = 2^19 = 1024 x 512 (round 4): the 1024-point pass on the 16-column tiles (64 points per thread: no room for a second column),
// the 512-point pass on the 32-column ones -- 32 + 32 tiles per transform
template <int NT>
__global__ void __launch_bounds__(256, 2) fft_fused2m_kernel(const FusedArgs f) {
    constexpr int E0 = Col2Lds<4, true>::ELEMS, E1 = Col2wLds<false>::ELEMS;
    __shared__ __attribute__((aligned(16))) cplx<float> lds[E0 > E1 ? E0 : E1];
    __shared__ unsigned s_item;
    fused_loop<1, 1, false>(
        f.c, &s_item,
        [&](unsigned t, unsigned slot, unsigned tile, auto hook) {
            col2_tile<float, 4, true, true, false, true, NT != 0, false, false>(f.p0, (long long)t, (long long)slot, (long long)tile * 16, lds, hook);
        },
        [&](unsigned slot, unsigned t, unsigned tile, auto hook) {
            col2w_tile<2, false, false, false, false, NT != 0>(f.p1, (long long)slot, (long long)t, (long long)tile * 32, lds, hook);
        });
}

// The 2-D form (BASELINE config 3: 1024 x 1024): a 2-D transform is two TRANSPOSING column passes without an inter-pass twiddle
// -- pass 0 transforms the y axis of in[y][x] and writes ring[x][ky], pass 1 transforms the x axis of that and writes
// out[ky][kx] -- i.e. the 1-D kernel above minus the twiddle, with contiguous 8 KiB runs on the output side.
// Round 4: rectangles.  A0 = ny / 256 (pass 0 transforms the y axis over nx / 16 tiles), A1 = nx / 256 (pass 1 the x axis over
// ny / 16 tiles); the two passes look their w(L) up in different tables (TileArgs.tw_L of p0 / p1).
// (The paired lanes of fft_fused2_kernel lost here: 2.46 against 2.43 ms on configuration 3, docs/negative_results.md.)
template <typename T, int A0, int A1, bool SPLIT, bool NT>
__global__ void __launch_bounds__(256, 2) fft_fused2d_kernel(const FusedArgs f) {
    constexpr int E0 = Col2Lds<A0, true, sizeof(cplx<T>)>::ELEMS, E1 = Col2Lds<A1, true, sizeof(cplx<T>)>::ELEMS;
    __shared__ __attribute__((aligned(16))) cplx<T> lds[E0 > E1 ? E0 : E1];
    __shared__ unsigned s_item;
    constexpr unsigned per0 = A0 > A1 ? 1u : (unsigned)(A1 / A0);   // tiles0 : tiles1 = nx : ny = A1 : A0
    constexpr unsigned per1 = A1 > A0 ? 1u : (unsigned)(A0 / A1);
    fused_loop<per0, per1, !SPLIT && sizeof(T) == 4>(
        f.c, &s_item,
        [&](unsigned t, unsigned slot, unsigned tile, auto hook) {
            col2_tile<T, A0, true, false, SPLIT, true, NT, false, false>(f.p0, (long long)t, (long long)slot, (long long)tile * 16, lds, hook);
        },
        [&](unsigned slot, unsigned t, unsigned tile, auto hook) {
            col2_tile<T, A1, true, false, false, false, false, NT, SPLIT>(f.p1, (long long)slot, (long long)t, (long long)tile * 16, lds, hook);
        });
}

// The 2-D form with 32-column tiles for a 512-point axis (round 4): (512, 512), (512, 1024), (1024, 512) fp32 interleaved.  W0 / W1 =
// columns per tile of pass 0 / pass 1: 32 where the pass transforms 512 points, 16 where it transforms 1024.
template <int A0, int A1>
__global__ void __launch_bounds__(256, 2) fft_fused2dw_kernel(const FusedArgs f) {
    constexpr bool WIDE0 = A0 <= 2, WIDE1 = A1 <= 2;
    constexpr int E0 = WIDE0 ? Col2wLds<true>::ELEMS : Col2Lds<A0, true>::ELEMS, E1 = WIDE1 ? Col2wLds<true>::ELEMS : Col2Lds<A1, true>::ELEMS;
    __shared__ __attribute__((aligned(16))) cplx<float> lds[E0 > E1 ? E0 : E1];
    __shared__ unsigned s_item;
    // tiles0 : tiles1 = nx / W0 : ny / W1 with nx = 256 A1, ny = 256 A0
    constexpr unsigned t0 = 256u * A1 / (WIDE0 ? 32u : 16u), t1 = 256u * A0 / (WIDE1 ? 32u : 16u);
    constexpr unsigned per0 = t0 >= t1 ? t0 / t1 : 1u, per1 = t1 > t0 ? t1 / t0 : 1u;
    fused_loop<per0, per1, false>(
        f.c, &s_item,
        [&](unsigned t, unsigned slot, unsigned tile, auto hook) {
            if constexpr (WIDE0) col2w_tile<A0, true, false, true, true, false>(f.p0, (long long)t, (long long)slot, (long long)tile * 32, lds, hook);
            else col2_tile<float, A0, true, false, false, true, true, false, false>(f.p0, (long long)t, (long long)slot, (long long)tile * 16, lds, hook);
        },
        [&](unsigned slot, unsigned t, unsigned tile, auto hook) {
            if constexpr (WIDE1) col2w_tile<A1, true, false, false, false, true>(f.p1, (long long)slot, (long long)t, (long long)tile * 32, lds, hook);
            else col2_tile<float, A1, true, false, false, false, false, true, false>(f.p1, (long long)slot, (long long)t, (long long)tile * 16, lds, hook);
        });
}

// The same work list with the 512-thread tiles of fft_col3.hpp (L = 512 * A): fp32 N = 2^22 = 2048 x 2048 (BASELINE config 5;
// one work-group per CU, the ring holds 7 transforms of 32 MiB), fp32 N = 2^21 = 2048 x 1024 and fp64 N = 2^20 = 1024 x 1024
// (14 transforms of 16 MiB).
template <typename T, int A0, int A1, bool SPLIT, bool NT>
__global__ void __launch_bounds__(512, 2) fft_fused3_kernel(const FusedArgs f) {
    constexpr int E0 = Col3Lds<T, true>::SCALARS, E1 = Col3Lds<T, false>::SCALARS;
    __shared__ __attribute__((aligned(16))) T lds[E0 > E1 ? E0 : E1];
    __shared__ unsigned s_item;
    constexpr unsigned per0 = A0 > A1 ? 1u : (unsigned)(A1 / A0);
    constexpr unsigned per1 = A1 > A0 ? 1u : (unsigned)(A0 / A1);
    fused_loop<per0, per1, false>(   // no early poll: the fp64 tiles have no register to spare for it, the fp32 ones measured equal
        f.c, &s_item,
        [&](unsigned t, unsigned slot, unsigned tile, auto hook) {
            col3_tile<T, A0, true, true, SPLIT, NT, false, false, true>(f.p0, (long long)t, (long long)slot, (long long)tile * 16, lds, hook);
        },
        [&](unsigned slot, unsigned t, unsigned tile, auto hook) {
            col3_tile<T, A1, false, false, false, false, NT, SPLIT>(f.p1, (long long)slot, (long long)t, (long long)tile * 16, lds, hook);
        });
}

// 2-D shapes on the 512-thread tiles (axis length 512 * A): fp64 1024 x 1024 (the published double-precision shape), fp32 with a
// 2048-point axis -- fft_fused2d_kernel's data flow
template <typename T, int A0, int A1, bool SPLIT, bool NT>
__global__ void __launch_bounds__(512, 2) fft_fused3d_kernel(const FusedArgs f) {
    __shared__ __attribute__((aligned(16))) T lds[Col3Lds<T, true>::SCALARS];
    __shared__ unsigned s_item;
    constexpr unsigned per0 = A0 > A1 ? 1u : (unsigned)(A1 / A0);
    constexpr unsigned per1 = A1 > A0 ? 1u : (unsigned)(A0 / A1);
    fused_loop<per0, per1, false>(
        f.c, &s_item,
        [&](unsigned t, unsigned slot, unsigned tile, auto hook) {
            col3_tile<T, A0, true, false, SPLIT, NT, false, false, true>(f.p0, (long long)t, (long long)slot, (long long)tile * 16, lds, hook);
        },
        [&](unsigned slot, unsigned t, unsigned tile, auto hook) {
            col3_tile<T, A1, true, false, false, false, NT, SPLIT>(f.p1, (long long)slot, (long long)t, (long long)tile * 16, lds, hook);
        });
}

}  // namespace mifft
