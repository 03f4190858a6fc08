// lsr_depth.h — the depth modes of the view record (include/lsr_rasterizer.h, slots [41..43]): what the projection
// kernels write into slot 6 of the screen record instead of the view-space z, and its derivatives for the geometry
// backward.  The compositing kernels blend slot 6 with the weights of every other channel and hand its gradient back
// (`gz`); nothing else reads it, so a mode costs no launch.
//
// The reference renders a per-Gaussian value u as a grey degree-0 SH colour on black and takes the channel mean
// (src/model/decoder/cuda_splatting.py:298-340), so the blended scalar is  d = max(0, C0 u + 0.5)  with
//   z = tz / s                 camera-space depth of the UNSCALED scene (tz: view-space z of the scaled one, s: slot [40])
//   depth               u = z
//   disparity           u = 1 / z
//   relative_disparity  u = 1 - (1 / (z + e) - 1 / (f + e)) / (1 / (n + e) - 1 / (f + e) + e),  e = 1e-10
//   log                 u = log(max(min(z, n), f))       (literally: log(far) whenever near < far)
// n / f: the caller's near / far (slots [42], [43]).  The mode is uniform per view: every branch below is a scalar one.
#pragma once
#include "lsr_internal.h"

namespace lsr {

constexpr float kDepthC0 = 0.28209479177387814f;
constexpr float kDepthEps = 1e-10f;

// u of a mode != LSR_DEPTH_NATIVE
__device__ __forceinline__ float depth_mode_value(int mode, float z, float n, float f) {
    if (mode == LSR_DEPTH_DEPTH) return z;
    if (mode == LSR_DEPTH_DISPARITY) return 1.0f / z;
    if (mode == LSR_DEPTH_RELATIVE_DISPARITY) {
        const float b = 1.0f / (f + kDepthEps);
        return 1.0f - (1.0f / (z + kDepthEps) - b) / (1.0f / (n + kDepthEps) - b + kDepthEps);
    }
    return logf(fmaxf(fminf(z, n), f));
}

// slot 6 of the screen record for a mode != LSR_DEPTH_NATIVE (never negative: the record staging of k_preprocess marks
// culled slots with a negative value)
__device__ __forceinline__ float depth_mode_payload(int mode, float tz, float s, float n, float f) {
    return fmaxf(0.0f, kDepthC0 * depth_mode_value(mode, tz / s, n, f) + 0.5f);
}

// dd/dz, dd/dn, dd/df at the unscaled depth z (all 0 where the colour clamp is active: C0 u + 0.5 < 0).  min / max hand
// their gradient to the selected argument.
struct DepthGrad { float dz, dn, df; };
__device__ __forceinline__ DepthGrad depth_mode_grad(int mode, float z, float n, float f) {
    DepthGrad g{0.0f, 0.0f, 0.0f};
    if (kDepthC0 * depth_mode_value(mode, z, n, f) + 0.5f < 0.0f) return g;
    if (mode == LSR_DEPTH_DEPTH) g.dz = kDepthC0;
    else if (mode == LSR_DEPTH_DISPARITY) g.dz = -kDepthC0 / (z * z);
    else if (mode == LSR_DEPTH_RELATIVE_DISPARITY) {
        const float a = 1.0f / (z + kDepthEps), b = 1.0f / (f + kDepthEps), c = 1.0f / (n + kDepthEps);
        const float D = c - b + kDepthEps, iD = 1.0f / D;
        g.dz = kDepthC0 * a * a * iD;                          // du/da = -1 / D, da/dz = -a^2
        g.dn = -kDepthC0 * (a - b) * c * c * iD * iD;          // du/dc = (a - b) / D^2, dc/dn = -c^2
        g.df = -kDepthC0 * (D - a + b) * b * b * iD * iD;      // du/db = (D - a + b) / D^2, db/df = -b^2
    } else {
        const float x = fminf(z, n), y = fmaxf(x, f), w = kDepthC0 / y;
        if (!(x > f)) g.df = w;
        else if (z < n) g.dz = w;
        else g.dn = w;
    }
    return g;
}

}  // namespace lsr
