// lsr_key_emit.h — what a workgroup of a projection kernel does BEHIND the projection arithmetic (lsr_project.h), shared by
// k_preprocess (preprocess.hip) and the fused projection + SH kernel k_preprocess_sh (sh.hip):
//   * the per-tile pair histogram of a (view, Gaussian) and its binning record;
//   * the flush of the LDS-privatised histogram into the tile counts (two-phase binning), or
//   * single-pass binning (lsr_internal.h segment_capacity): the reservation of the workgroup's slots in the tiles' key
//     segments and the emission of its sort keys, one view at a time, through an LDS bucket pass;
//   * the tile scan folded into the last workgroup to arrive (lsr_tile_scan.h).
// The kernels differ in how a thread enumerates its Gaussians and in where their LDS areas come from; both are arguments
// here.  Everything is integer code and __forceinline__: the pointer parameters keep their address spaces (ds_* / global_*).
#pragma once
#include "lsr_blend.h"
#include "lsr_tile_scan.h"

namespace lsr {

struct TileRect { int x0, y0, x1, y1; };   // tiles [x0, x1) x [y0, y1)

// Per-tile pair counts of one (view, Gaussian) (also the compositing kernels' scheduling key: a finer work estimate —
// quadrants reached per entry — was measured to schedule no better).  `hist`: the view's row of the LDS histogram or of the
// global tile counts.  skip_none (LSR_FWD_REACHED_ONLY): only the tiles of the rectangle the footprint box reaches are pairs.
__device__ __forceinline__ void count_pairs(uint32_t *hist, int gx, TileRect r, uint32_t span, bool skip_none) {
    if (skip_none) reached_rect(span, r.x0, r.y0, r.x1, r.y1);
    for (int y = r.y0; y < r.y1; ++y)
        for (int x = r.x0; x < r.x1; ++x) atomicAdd(&hist[y * gx + x], 1u);
}

// Binning record of (view, Gaussian) slot `o` (BinRec / BinRecWide: lsr_internal.h); a culled one holds an empty rectangle
// and depth 0.
__device__ __forceinline__ void store_bin_record(char *binrec, int narrow, size_t o, bool ok, const TileRect &r, float tz, uint32_t span) {
    const float out_depth = ok ? tz : 0.0f;
    if (narrow) {
        BinRec br;
        br.rect = ok ? ((uint32_t)r.x0 | ((uint32_t)r.y0 << 8) | ((uint32_t)r.x1 << 16) | ((uint32_t)r.y1 << 24)) : 0u;
        br.depth = out_depth; br.span = span;
        ((BinRec *)binrec)[o] = br;
    } else {
        BinRecWide br;
        br.rect = ok ? make_ushort4((unsigned short)r.x0, (unsigned short)r.y0, (unsigned short)r.x1, (unsigned short)r.y1)
                     : make_ushort4(0, 0, 0, 0);
        br.depth = out_depth; br.span = span;
        ((BinRecWide *)binrec)[o] = br;
    }
}

// Two-phase binning: the workgroup's LDS histogram (n counters: its valid views x T tiles) is added to the tile counts.
template <int THREADS>
__device__ __forceinline__ void flush_counts(const uint32_t *s_hist, uint32_t *tile_count, int n) {
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += THREADS) {
        const uint32_t c = s_hist[t];
        if (c) atomicAdd(&tile_count[t], c);
    }
}

// Single-pass binning, reserve: count -> first slot of this workgroup in the tile's key segment.  The one global atomic
// per non-empty counter that used to add the count to the tile's total RETURNS the old total.
// Four counters per thread and round, their returning atomics in flight together: one round trip to the memory-side atomic
// unit per round instead of one per counter.  Only non-empty counters issue an atomic — adds of zero to a clamped address
// put thousands of same-address atomics of EVERY workgroup on one word: measured 5.5 ms instead of 0.15 for a
// one-view-per-workgroup launch.
template <int THREADS>
__device__ __forceinline__ void reserve_segments(const uint32_t *s_hist, uint32_t *s_first, uint32_t *tile_count, int n) {
    __syncthreads();
    for (int t0 = threadIdx.x; t0 < n; t0 += 4 * THREADS) {
        uint32_t c[4], first[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int t = t0 + k * THREADS; c[k] = t < n ? s_hist[t] : 0u; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = t0 + k * THREADS;
            if (c[k]) first[k] = __hip_atomic_fetch_add(&tile_count[t], c[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int t = t0 + k * THREADS; if (t < n) s_first[t] = first[k]; }
    }
    __syncthreads();
}

// The bucket arrays of the emission, carved out of an LDS area that is idle by then (k_preprocess: its record staging
// array; k_preprocess_sh: the coefficient rows): [T] s_delta | 8-byte aligned: [buf] keys | [buf] positions.
struct KeyBuckets {
    uint32_t *delta;   // [T] first slot in the segment minus local offset
    uint64_t *key;
    uint32_t *pos;
    uint32_t buf;      // slots: 12 bytes each
    __device__ __forceinline__ KeyBuckets(void *area, size_t bytes, int T) {
        const int kbase = (T * 4 + 7) & ~7;
        delta = (uint32_t *)area;
        key = (uint64_t *)((char *)area + kbase);
        buf = (uint32_t)((bytes - kbase) / 12);
        pos = (uint32_t *)((char *)area + kbase + (size_t)buf * 8);
    }
};

// Single-pass binning, emit: the sort keys `depth << 32 | index << key_shift | sub-block code` of ONE view of the workgroup,
// THROUGH LDS: the keys are first bucketed by tile in `kb` — a key's slot is its tile's local offset (exclusive scan of the
// workgroup's counts `cur`, which become the tiles' cursors) plus its arrival rank — together with their final positions,
// and then leave as one linear pass over the slots: every lane stores, and the lanes of a tile's run hit consecutive
// addresses.  Written straight from the item loop (the first version of this pass) the same keys were 7.4 M lane-scattered
// 8-byte stores at 31 % lane utilisation: 0.053 of k_preprocess' 0.155 ms (ablations in profiles/r05_ab_knobs.md).
//   cur / first : this view's rows of the workgroup's counts and first slots (reserve_segments);
//   seg_view    : the view's index in the whole call (its segments start at seg_view * T);
//   br / index / valid : the thread's N binning records of this view (the caller's own enumeration; loaded unconditionally
//                 at clamped addresses, all in flight together), their Gaussian indices, and whether each is a real item —
//                 a thread only ever reads records its own workgroup wrote.
template <int THREADS, int N>
__device__ __forceinline__ void emit_view_keys(uint32_t *cur, const uint32_t *first, const KeyBuckets &kb, const SegOut &seg,
                                               uint32_t seg_view, int T, int gx, bool skip_none,
                                               const uint3 (&br)[N], const int (&index)[N], const bool (&valid)[N]) {
    __shared__ uint32_t s_scanw[THREADS / LSR_WAVE];
    const int tpt = (T + THREADS - 1) / THREADS;             // tiles per thread of the scan (<= 4: T <= 1024)
    // local offsets of this view's tiles: a contiguous chunk of tiles per thread
    uint32_t cnt[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = (int)threadIdx.x * tpt + k;
        cnt[k] = (k < tpt && t < T) ? cur[t] : 0u;
        mine += cnt[k];
    }
    uint32_t n_v;
    uint32_t off = block_exclusive_scan<THREADS>(mine, s_scanw, n_v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = (int)threadIdx.x * tpt + k;
        if (k < tpt && t < T) { cur[t] = off; kb.delta[t] = first[t] - off; off += cnt[k]; }
    }
    __syncthreads();
    const uint32_t cap = seg.cap, seg0 = seg_view * (uint32_t)T;
#pragma unroll
    for (int it = 0; it < N; ++it) {
        const uint32_t rc = valid[it] ? br[it].x : 0u;           // (a culled record holds an empty rectangle)
        const int x0 = rc & 0xff, y0 = (rc >> 8) & 0xff, x1 = (rc >> 16) & 0xff, y1 = rc >> 24;
        const uint64_t key = ((uint64_t)br[it].y << 32) | ((uint32_t)index[it] << seg.key_shift);
        const uint32_t sp = br[it].z;
        int ex0 = x0, ey0 = y0, ex1 = x1, ey1 = y1;
        if (skip_none) reached_rect(sp, ex0, ey0, ex1, ey1);      // (the pairs count_pairs counted)
        for (int y = ey0; y < ey1; ++y)
            for (int x = ex0; x < ex1; ++x) {
                const int t = y * gx + x;
                const uint32_t code = seg.key_shift ? span_code(sp, x - x0, y - y0) : 0u;
                const uint32_t slot = atomicAdd(&cur[t], 1u);
                // position in the tile's segment, CLAMPED (not tested): the surplus keys of an overfull segment land
                // on its last slot; such a tile is binned again by the fallback scatter
                const uint32_t pos = (seg0 + (uint32_t)t) * cap + min(slot + kb.delta[t], cap - 1u);
                if (slot < kb.buf) { kb.key[slot] = key | code; kb.pos[slot] = pos; }
                else seg.keys[pos] = key | code;              // (more pairs in one view of this workgroup than the array holds)
            }
    }
    __syncthreads();
    const uint32_t nflush = min(n_v, kb.buf);
    for (uint32_t j = threadIdx.x; j < nflush; j += THREADS) seg.keys[kb.pos[j]] = kb.key[j];
    __syncthreads();
}

// The tile scan, folded in (round 4; it used to be a kernel of its own between the projection and k_scatter): the LAST
// workgroup to arrive scans the N = views x T tile counts, writes the tile offsets, the header, the compositing work items
// and the two numbers the synchronous forward's host is waiting for (lsr_tile_scan.h).
// The counts are only ever touched by agent-scope atomics, which are performed past the (mutually incoherent) per-XCD L2s:
// a workgroup waits until its own count updates have been acknowledged (vmcnt) and only then arrives at the counter, and
// the last workgroup reads the counts with agent-scope atomic loads.  No release fence: that would write back every record
// line the workgroup has just left dirty in L2 (measured in round 2: the forward went from 0.56 to 0.83 ms per step).
// The counts go through LDS (`s_counts`, at least kFoldTiles words of an area that is free by now): sixteen of them per
// thread in registers cost k_preprocess a wave per SIMD (85 instead of 77 VGPRs).
template <int THREADS>
__device__ __forceinline__ void folded_tile_scan(const FoldedScan &fs, uint32_t *header, const uint32_t *tile_count, int N,
                                                 uint32_t *s_counts, TileScanShared<THREADS> &s_scan) {
    __shared__ uint32_t s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t arrived = __hip_atomic_fetch_add(&header[kHdrPreDone], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = arrived == gridDim.x * gridDim.y - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    for (int i0 = threadIdx.x; i0 < N; i0 += 4 * THREADS) {     // four coalesced loads in flight per thread
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            c[k] = __hip_atomic_load(&tile_count[min(i0 + k * THREADS, N - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k * THREADS < N) s_counts[i0 + k * THREADS] = c[k];
    }
    __syncthreads();
    tile_scan_block<THREADS, 0, false>(s_counts, fs.tile_start, header, HostMirror{fs.host_words, fs.host_seq},
                                       fs.tile_order, N, fs.capacity, s_scan);
}

}  // namespace lsr
