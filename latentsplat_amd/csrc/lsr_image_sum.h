// lsr_image_sum.h — what the fused image losses share after their main pass: the finishing launch that turns workspace
// slots into per-image values and the loss, and the decoding of a tile index.
//
// A loss's main kernel leaves N doubles per workgroup in that workgroup's own slot (block_sum of lsr_wave.h); the slots of
// one image are consecutive.  The finish is ONE workgroup of kFinishThreads = 1024, 16 waves:
//   * wave w takes the images w, w + 16, ...; for one image lane l adds the slots l, l + 64, ... from the lowest up and
//     the wave butterfly makes the image's N sums (image_slot_sums), the same in every lane;
//   * the caller's per-image step turns the sums into the image's M contributions to the loss and stores what belongs
//     to the image (per_view, a table row) from lane 0; a wave adds the contributions of its images in order;
//   * lane 0 of every wave leaves its M totals in LDS, and after one barrier thread 0 adds them in wave order from wave 0
//     and hands them to the caller's final step, which writes the loss.
// Every sum is in double and in that fixed order: no atomics, the same bits every call, and an image's own values do
// not depend on which other images share the call.
#pragma once
#include "lsr_wave.h"

namespace lsr {

constexpr int kFinishThreads = 1024;

// The N sums of one image's `count` slots of N doubles, in every lane of the calling wave.
// ORDER: lane l adds the slots l, l + 64, ... from the lowest up, starting from 0; then wave_all of every sum.
template <int N>
__device__ __forceinline__ void image_slot_sums(const double *__restrict__ slots, int count, double (&sum)[N]) {
    const int lane = threadIdx.x & (LSR_WAVE - 1);
#pragma unroll
    for (int k = 0; k < N; ++k) sum[k] = 0.0;
    for (int i = lane; i < count; i += LSR_WAVE)
#pragma unroll
        for (int k = 0; k < N; ++k) sum[k] += slots[(size_t)i * N + k];
#pragma unroll
    for (int k = 0; k < N; ++k) sum[k] = wave_all(sum[k], Add());
}

// The finish described above, for one workgroup of kFinishThreads.  per_image(v, lane, sum, part): the N sums of image v
// to its M contributions (called by whole waves); total(t): the M totals, called by thread 0 alone when `want_total`.
template <int N, int M, class PerImage, class Total>
__device__ __forceinline__ void image_finish(const double *__restrict__ slots, int V, int slots_per_image, bool want_total,
                                             PerImage per_image, Total total) {
    constexpr int kWaves = kFinishThreads / LSR_WAVE;
    __shared__ double s_tot[kWaves][M];
    const int wave = threadIdx.x / LSR_WAVE, lane = threadIdx.x & (LSR_WAVE - 1);
    double tot[M];
#pragma unroll
    for (int m = 0; m < M; ++m) tot[m] = 0.0;
    for (int v = wave; v < V; v += kWaves) {
        double sum[N], part[M];
        image_slot_sums<N>(slots + (size_t)v * slots_per_image * N, slots_per_image, sum);
        per_image(v, lane, sum, part);
#pragma unroll
        for (int m = 0; m < M; ++m) tot[m] += part[m];
    }
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) s_tot[wave][m] = tot[m];
    }
    __syncthreads();
    if (threadIdx.x == 0 && want_total) {
        double t[M];
#pragma unroll
        for (int m = 0; m < M; ++m) t[m] = 0.0;
        for (int w = 0; w < kWaves; ++w)
#pragma unroll
            for (int m = 0; m < M; ++m) t[m] += s_tot[w][m];
        total(t);
    }
}

// The finish of a loss that is the mean over images of (the image's one sum) * inv_pixels: per_view[v] and *loss, each
// optional.  Unit: a tag type of the including .hip file, so that every unit launches a kernel of its own.
template <class Unit>
__global__ __launch_bounds__(kFinishThreads) void k_image_mean_finish(const double *__restrict__ slots, int V, int slots_per_image,
                                                                       double inv_pixels, float *loss, float *per_view) {
    image_finish<1, 1>(slots, V, slots_per_image, loss != nullptr,
                       [=](int v, int lane, const double (&sum)[1], double (&part)[1]) {
                           part[0] = sum[0] * inv_pixels;
                           if (lane == 0 && per_view) per_view[v] = (float)part[0];
                       },
                       [=](const double (&t)[1]) { *loss = (float)(t[0] / V); });
}

// The tile of this workgroup in a grid of `tile` x `tile` pixel tiles, tiles_x * tiles_y per plane: the plane (an
// image, or a channel of one; in the caller's index type) and the tile's first pixel.
template <class Plane>
__device__ __forceinline__ void image_tile(int tiles_x, int tiles_y, int tile, Plane &plane, int &y0, int &x0) {
    const uint32_t b = blockIdx.x;
    const uint32_t per_plane = (uint32_t)(tiles_x * tiles_y);
    const uint32_t p = b / per_plane, t = b - p * per_plane;
    plane = (Plane)p;
    y0 = (int)(t / (uint32_t)tiles_x) * tile;
    x0 = (int)(t % (uint32_t)tiles_x) * tile;
}

}  // namespace lsr
