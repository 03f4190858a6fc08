// lsr_sh_rotate_basis.h — the real SH basis Y of include/lsr_sh_rotate.h in double, homogeneous form (1 -> x.x): what
// the rotation-matrix kernels evaluate at rotated sample directions (sh_rotate.hip: D_l(R); scene_transform.hip: the
// same D_l(R) on the way to the "3dgs" matrices).
#pragma once
#include <hip/hip_runtime.h>

namespace lsr {

constexpr double kY0 = 0.28209479177387814, kY1 = 0.4886025119029199;
constexpr double kY2[5] = {1.0925484305920792, 1.0925484305920792, 0.31539156525252005, 1.0925484305920792,
                                         0.5462742152960396};
constexpr double kY3[7] = {0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154,
                                         0.4570457994644658, 1.445305721320277, 0.5900435899266435};
constexpr double kY4[9] = {2.5033429417967046, 1.7701307697799304, 0.9461746957575601, 0.6690465435572892,
                                         0.10578554691520431, 0.6690465435572892, 0.47308734787878004, 1.7701307697799304,
                                         0.6258357354491761};

// all 2l+1 components of band l at (x, y, z)
__device__ static void sh_band_all(int l, double x, double y, double z, double (&o)[9]) {
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z, rr = xx + yy + zz;
    switch (l) {
    case 0:
        o[0] = kY0;
        break;
    case 1:
        o[0] = kY1 * x; o[1] = kY1 * y; o[2] = kY1 * z;
        break;
    case 2:
        o[0] = kY2[0] * xz;
        o[1] = kY2[1] * xy;
        o[2] = kY2[2] * (2.0 * yy - zz - xx);
        o[3] = kY2[3] * yz;
        o[4] = kY2[4] * (zz - xx);
        break;
    case 3:
        o[0] = kY3[0] * x * (3.0 * zz - xx);
        o[1] = kY3[1] * xz * y;
        o[2] = kY3[2] * x * (4.0 * yy - zz - xx);
        o[3] = kY3[3] * y * (2.0 * yy - 3.0 * zz - 3.0 * xx);
        o[4] = kY3[4] * z * (4.0 * yy - zz - xx);
        o[5] = kY3[5] * y * (zz - xx);
        o[6] = kY3[6] * z * (zz - 3.0 * xx);
        break;
    default:
        o[0] = kY4[0] * xz * (zz - xx);
        o[1] = kY4[1] * xy * (3.0 * zz - xx);
        o[2] = kY4[2] * xz * (7.0 * yy - rr);
        o[3] = kY4[3] * xy * (7.0 * yy - 3.0 * rr);
        o[4] = kY4[4] * (yy * (35.0 * yy - 30.0 * rr) + 3.0 * rr * rr);
        o[5] = kY4[5] * yz * (7.0 * yy - 3.0 * rr);
        o[6] = kY4[6] * (zz - xx) * (7.0 * yy - rr);
        o[7] = kY4[7] * yz * (zz - 3.0 * xx);
        o[8] = kY4[8] * (zz * (zz - 3.0 * xx) - xx * (3.0 * zz - xx));
        break;
    }
}

}  // namespace lsr
