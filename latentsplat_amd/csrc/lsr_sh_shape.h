// lsr_sh_shape.h — the shapes of a scene's spherical harmonics, in one place: K coefficients per channel (K = (degree + 1)^2,
// degree 0..4), of which the K - 1 beyond the DC term make a Gaussian's f_rest row.  Plain C++ as well as HIP: the host-only
// scene writer includes it too.
#pragma once
#include <type_traits>

#ifdef __HIPCC__
#define LSR_SH_HD __host__ __device__
#else
#define LSR_SH_HD
#endif

namespace lsr {

LSR_SH_HD constexpr bool sh_valid_coeffs(int K) { return K == 1 || K == 4 || K == 9 || K == 16 || K == 25; }
LSR_SH_HD constexpr int sh_degree_of(int K) { return (K > 16) + (K > 9) + (K > 4) + (K > 1); }
LSR_SH_HD constexpr int sh_rest_floats(int K) { return 3 * (K - 1); }                  // floats of one f_rest row
LSR_SH_HD constexpr int sh_rest_stride(int K) { return sh_rest_floats(K) | 1; }        // its LDS stride; odd: no bank conflicts
LSR_SH_HD constexpr int sh_band_offset(int l) { return l * (4 * l * l - 1) / 3; }      // sum_{m<l} (2m+1)^2

// f(std::integral_constant<int, K>{}) for the K of a call whose sh_valid_coeffs(K) has been checked: the launchers are
// templates on K
template <class F>
void dispatch_sh_coeffs(int K, F &&f) {
    switch (K) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 9: f(std::integral_constant<int, 9>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        default: f(std::integral_constant<int, 25>{}); break;
    }
}

}  // namespace lsr

#undef LSR_SH_HD
