// lsr_wave.h — the cross-lane and block-wide primitives of every kernel: single exchanges (DPP, readlane, ballot rank),
// reductions and scans over a DPP row, a wave and a workgroup.
// The results of this library are bit-reproducible without float atomics because every one of these exchanges combines
// its operands in a FIXED ORDER.  That order is stated at each primitive and is its contract: a caller's sums are formed
// in exactly that order, and a change of it changes results.
// All primitives expect every lane of the wave to be active and a workgroup of whole waves whose lane is threadIdx.x & 63.
#pragma once
#include "lsr_internal.h"

namespace lsr {

// ---- single exchanges ----

// The value of the lane that the DPP control names (32-bit T); lanes without a source, or in a row that ROW_MASK leaves
// out, read 0.
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false, class T>
__device__ __forceinline__ T dpp(T x) {
    static_assert(sizeof(T) == 4, "one register");
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf, BOUND_CTRL));
}
// x of one lane (wave-uniform index) as a uniform value (32-bit T)
template <class T>
__device__ __forceinline__ T readlane(T x, int lane) {
    static_assert(sizeof(T) == 4, "one register");
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}
// number of set ballot bits below this lane
__device__ __forceinline__ uint32_t lane_rank(uint64_t ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// ---- operators: op(mine, other) ----
struct Add { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct Or { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a | b; } };
struct Min {
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};
struct Max {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};

// ---- reductions ----

// All-reduce over the 8 lanes of every half DPP row / the 16 lanes of every DPP row; the result in each of those lanes.
// ORDER: x = op(x, x of lane ^ 1) [quad_perm 1,0,3,2]; then lane ^ 2 [quad_perm 2,3,0,1]; then the mirrored half row
// [row_half_mirror]; for the whole row then the mirrored row [row_mirror].  Both sides of every step combine the same
// pair, so with a commutative op all lanes return identical bits.
template <bool BOUND_CTRL = false, class T, class Op>
__device__ __forceinline__ T half_row_all(T x, Op op) {
    x = op(x, dpp<0xB1, 0xf, BOUND_CTRL>(x));
    x = op(x, dpp<0x4E, 0xf, BOUND_CTRL>(x));
    return op(x, dpp<0x141, 0xf, BOUND_CTRL>(x));
}
template <bool BOUND_CTRL = false, class T, class Op>
__device__ __forceinline__ T row_all(T x, Op op) {
    x = half_row_all<BOUND_CTRL>(x, op);
    return op(x, dpp<0x140, 0xf, BOUND_CTRL>(x));
}

// All-reduce over the 64 lanes of a wave: of several values in place, or of one value, returned.
// ORDER: the xor butterfly v = op(v, v of lane ^ off) for off = 32, 16, 8, 4, 2, 1; several values advance together, one
// step at a time, in argument order.
template <class Op, class... T>
__device__ __forceinline__ void wave_all_each(Op op, T &...v) {
#pragma unroll
    for (int off = LSR_WAVE / 2; off > 0; off >>= 1) ((v = op(v, __shfl_xor(v, off))), ...);
}
template <class T, class Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
    wave_all_each(op, v);
    return v;
}

// Sum of v[0..31] over the 64 lanes of a wave: recursive halving, 32 exchanges instead of 6 per value.
// Lane l returns the total of slot l & 31.
// ORDER: step H = 16, 8, 4, 2, 1 leaves in slot k (k < H) of a lane its own value of slot k (lanes without bit H) or
// k + H (lanes with it) plus the value that lane ^ H held of the same slot; then v[0] + v[0] of lane ^ 32.
// (one template instance per step: every index is a constant, the array stays in registers)
template <int H>
__device__ __forceinline__ void wave_halve(float (&v)[32], int lane) {
    const bool up = (lane & H) != 0;
#pragma unroll
    for (int k = 0; k < H; ++k) {
        const float send = up ? v[k] : v[k + H], keep = up ? v[k + H] : v[k];
        v[k] = keep + __shfl_xor(send, H);
    }
}
__device__ __forceinline__ float wave_sum32(float (&v)[32]) {
    const int lane = (int)(threadIdx.x & (LSR_WAVE - 1));
    wave_halve<16>(v, lane); wave_halve<8>(v, lane); wave_halve<4>(v, lane); wave_halve<2>(v, lane); wave_halve<1>(v, lane);
    return v[0] + __shfl_xor(v[0], 32);
}

// Sums of N doubles per lane over a workgroup of THREADS (one LDS hop, one barrier); s_red: THREADS / 64 rows of N.
// ORDER: wave_all of every value; lane 0 of wave w stores its N sums to s_red[w]; the barrier; then total k is
// s_red[0][k] + s_red[1][k] + ..., the waves in order from wave 0.
// The totals go to dst[k], which the caller passes (a workspace slot, a local array): with OWNERS = N thread k forms and
// stores total k; with OWNERS = 1 thread 0 forms all N side by side and stores them in k order.  No other thread touches
// dst, and s_red may be reused only after another barrier.
template <int THREADS, int N, int OWNERS = N>
__device__ __forceinline__ void block_sum(double (&v)[N], double (*s_red)[N], double *dst) {
    static_assert(THREADS % LSR_WAVE == 0 && (OWNERS == N || OWNERS == 1), "whole waves; a total per thread, or all in thread 0");
    constexpr int kWaves = THREADS / LSR_WAVE, kMine = N / OWNERS;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_all(v[k], Add());
    if ((threadIdx.x & (LSR_WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) s_red[threadIdx.x / LSR_WAVE][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < OWNERS) {
        const int first = OWNERS == 1 ? 0 : (int)threadIdx.x;
        double t[kMine];
#pragma unroll
        for (int j = 0; j < kMine; ++j) t[j] = s_red[0][first + j * OWNERS];
        for (int w = 1; w < kWaves; ++w)
#pragma unroll
            for (int j = 0; j < kMine; ++j) t[j] += s_red[w][first + j * OWNERS];
#pragma unroll
        for (int j = 0; j < kMine; ++j) dst[first + j * OWNERS] = t[j];
    }
}

// ---- scans ----

// Inclusive prefix sum over the 64 lanes of a wave.
// ORDER: the __shfl_up ladder, off = 1, 2, 4, 8, 16, 32: lanes >= off add the value of lane - off.
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & (LSR_WAVE - 1);
#pragma unroll
    for (int off = 1; off < LSR_WAVE; off <<= 1) {
        const T t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// Block-wide exclusive prefix sum of one value per thread: wave scans in registers + one LDS hop (two barriers).
// s_wave: THREADS / 64 values.  ORDER: wave_inclusive_scan; then the totals of the waves before this one, wave 0 first.
template <int THREADS, class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *s_wave, T &total) {
    constexpr int kWaves = THREADS / LSR_WAVE;
    const int lane = threadIdx.x & (LSR_WAVE - 1), wid = threadIdx.x / LSR_WAVE;
    const T incl = wave_inclusive_scan(v);
    if (lane == LSR_WAVE - 1) s_wave[wid] = incl;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const T x = s_wave[w];
        tot += x;
        base += w < wid ? x : T(0);
    }
    __syncthreads();   // s_wave may be reused
    total = tot;
    return base + incl - v;
}

// One workgroup of THREADS turns sums[chunks] into exclusive bases, in place; total = their sum.
// ORDER: thread t sums its ceil(chunks / THREADS) consecutive entries from the lowest up; block_exclusive_scan of those.
template <int THREADS, class T>
__device__ __forceinline__ void scan_chunk_sums(T *sums, int64_t chunks, T *s_wave, T &total) {
    const int64_t per = (chunks + THREADS - 1) / THREADS;
    const int64_t lo = threadIdx.x * per < chunks ? threadIdx.x * per : chunks, hi = lo + per < chunks ? lo + per : chunks;
    T mine = 0;
    for (int64_t i = lo; i < hi; ++i) mine += sums[i];
    T run = block_exclusive_scan<THREADS>(mine, s_wave, total);
    for (int64_t i = lo; i < hi; ++i) { const T c = sums[i]; sums[i] = run; run += c; }
}

}  // namespace lsr
