// lsr_eig3.h — symmetric 3x3 covariance to log-scales and a unit quaternion (Sigma = R S^2 R^T), float32, for
// k_ply_pack_scene (ply.hip).  Host and device: tools/eig3_sweeps.cpp runs the same code on the CPU to choose the sweep
// count and to measure the reconstruction error.
//
// Cyclic Jacobi with a FIXED number of sweeps as straight-line code: no data-dependent trip count, everything in
// registers (6 + 9 floats), no divergence beyond the skipped rotation of an element that is already exactly 0.  The
// rotation angle is taken in the form that stays accurate for a tiny off-diagonal: theta = (a_qq - a_pp) / (2 a_pq),
// t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)); an overflowing theta gives t = 0, which is the right limit.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LSR_EIG3_FN __host__ __device__ __forceinline__
#else
#define LSR_EIG3_FN inline
#endif

namespace lsr {

// Sweeps of (0,1), (0,2), (1,2).  Chosen by tools/eig3_sweeps.cpp: the worst reconstruction error over the encoder's
// range and the degenerate set stops improving at 4 sweeps (it is float32 rounding from there on); one more is margin.
constexpr int kEig3Sweeps = 5;

// Annihilates a_pq.  arp / arq are the two remaining off-diagonal elements a_rp, a_rq (r the third index); (xp, xq),
// (yp, yq), (zp, zq) are the rows of the eigenvector matrix in columns p and q.
LSR_EIG3_FN void eig3_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, float &xp, float &xq, float &yp,
                             float &yq, float &zp, float &zq) {
    if (apq == 0.0f) return;
    const float theta = (aqq - app) / (2.0f * apq);
    const float t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
    const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0f;
    const float rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const float x = xp, y = yp, z = zp;
    xp = c * x - s * xq; xq = s * x + c * xq;
    yp = c * y - s * yq; yq = s * y + c * yq;
    zp = c * z - s * zq; zq = s * z + c * zq;
}

LSR_EIG3_FN void eig3_swap_columns(float &la, float &lb, float &xa, float &xb, float &ya, float &yb, float &za, float &zb) {
    if (la < lb) {
        float t;
        t = la; la = lb; lb = t;
        t = xa; xa = xb; xb = t;
        t = ya; ya = yb; yb = t;
        t = za; za = zb; zb = t;
    }
}

// Rotation matrix (rows r0*, r1*, r2*; det +1, orthonormal up to rounding) to the unit quaternion w,x,y,z with w >= 0.
// The largest of the four candidates 4w^2, 4x^2, 4y^2, 4z^2 is the pivot, so nothing is divided by a value near 0.
LSR_EIG3_FN void rotation_to_quaternion(float r00, float r01, float r02, float r10, float r11, float r12, float r20,
                                        float r21, float r22, float q[4]) {
    const float tw = 1.0f + r00 + r11 + r22, tx = 1.0f + r00 - r11 - r22, ty = 1.0f - r00 + r11 - r22,
                tz = 1.0f - r00 - r11 + r22;
    float w, x, y, z;
    if (tw >= tx && tw >= ty && tw >= tz) {
        w = tw; x = r21 - r12; y = r02 - r20; z = r10 - r01;
    } else if (tx >= ty && tx >= tz) {
        w = r21 - r12; x = tx; y = r01 + r10; z = r02 + r20;
    } else if (ty >= tz) {
        w = r02 - r20; x = r01 + r10; y = ty; z = r12 + r21;
    } else {
        w = r10 - r01; x = r02 + r20; y = r12 + r21; z = tz;
    }
    float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
    if (w < 0.0f) inv = -inv;
    q[0] = w * inv; q[1] = x * inv; q[2] = y * inv; q[3] = z * inv;
}

// c: xx, xy, xz, yy, yz, zz.  log_scale[k] = 0.5 log(max(lambda_k, 1e-12 lambda_max, 1e-37)), descending; q: the unit
// quaternion w,x,y,z (w >= 0) of the eigenvector matrix, its last column flipped where that makes det = +1.
template <int SWEEPS = kEig3Sweeps>
LSR_EIG3_FN void eig3_scale_rotation(const float c[6], float log_scale[3], float q[4]) {
    float a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
    float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        eig3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        eig3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        eig3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    eig3_swap_columns(a00, a11, v00, v01, v10, v11, v20, v21);
    eig3_swap_columns(a11, a22, v01, v02, v11, v12, v21, v22);
    eig3_swap_columns(a00, a11, v00, v01, v10, v11, v20, v21);
    const float det = v00 * (v11 * v22 - v12 * v21) - v01 * (v10 * v22 - v12 * v20) + v02 * (v10 * v21 - v11 * v20);
    if (det < 0.0f) { v02 = -v02; v12 = -v12; v22 = -v22; }
    const float floor_ = fmaxf(1e-12f * a00, 1e-37f);     // (a NaN lambda_max leaves 1e-37; the NaN then comes out of the logs)
    log_scale[0] = 0.5f * logf(a00 < floor_ ? floor_ : a00);
    log_scale[1] = 0.5f * logf(a11 < floor_ ? floor_ : a11);
    log_scale[2] = 0.5f * logf(a22 < floor_ ? floor_ : a22);
    rotation_to_quaternion(v00, v01, v02, v10, v11, v12, v20, v21, v22, q);
}

}  // namespace lsr
