// eig3_sweeps.cpp — runs csrc/lsr_eig3.h (the covariance decomposition of k_ply_pack_scene) on the CPU for 1 ... 7 Jacobi
// sweeps and prints, per sweep count, the worst reconstruction error | R S^2 R^T - Sigma | / max |Sigma| (float64 rebuild
// from the float32 log-scales and quaternion) over (a) 200 000 covariances of the encoder's range — random rotations,
// overall scale log-uniform in [1e-3, 1], axis ratios down to 1/30 — and (b) the degenerate set: isotropic, two equal
// eigenvalues, exactly diagonal, rank 1, rank 2, zero, scale ratio 1e4, and (a) scaled by 1e-6 and by 1e3.
// This is where kEig3Sweeps comes from.   g++ -O2 -std=c++17 -Ilatentsplat_amd/csrc tools/eig3_sweeps.cpp -o eig3_sweeps
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "lsr_eig3.h"

namespace {

struct Cov { float c[6]; };

Cov build(const double q[4], const double s[3]) {
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    double S[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            S[3 * i + j] = 0;
            for (int k = 0; k < 3; ++k) S[3 * i + j] += R[3 * i + k] * s[k] * s[k] * R[3 * j + k];
        }
    return Cov{{(float)S[0], (float)S[1], (float)S[2], (float)S[4], (float)S[5], (float)S[8]}};
}

template <int SWEEPS>
double worst(const std::vector<Cov> &set, bool *finite) {
    double worst = 0;
    for (const Cov &cv : set) {
        float ls[3], qf[4];
        lsr::eig3_scale_rotation<SWEEPS>(cv.c, ls, qf);
        for (int k = 0; k < 3; ++k) *finite = *finite && std::isfinite(ls[k]);
        for (int k = 0; k < 4; ++k) *finite = *finite && std::isfinite(qf[k]);
        const double q[4] = {qf[0], qf[1], qf[2], qf[3]};
        const double s[3] = {std::exp((double)ls[0]), std::exp((double)ls[1]), std::exp((double)ls[2])};
        // (the rebuild rounds to float at the end, which is below the errors of interest)
        const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
        const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                             2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                             2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
        const int at[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
        double big = 0, err = 0;
        for (int e = 0; e < 6; ++e) big = std::max(big, std::fabs((double)cv.c[e]));
        for (int e = 0; e < 6; ++e) {
            double v = 0;
            for (int k = 0; k < 3; ++k) v += R[3 * at[e][0] + k] * s[k] * s[k] * R[3 * at[e][1] + k];
            err = std::max(err, std::fabs(v - (double)cv.c[e]));
        }
        if (big > 0) worst = std::max(worst, err / big);
    }
    return worst;
}

template <int SWEEPS>
void report(const std::vector<Cov> &range, const std::vector<Cov> &degenerate) {
    bool finite = true;
    const double a = worst<SWEEPS>(range, &finite), b = worst<SWEEPS>(degenerate, &finite);
    printf("sweeps %d: encoder range %.3e   degenerate set %.3e   %s\n", SWEEPS, a, b, finite ? "all finite" : "NON-FINITE");
}

}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    std::normal_distribution<double> normal;
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::vector<Cov> range, degenerate;
    const auto draw = [&](double scale) {
        const double q[4] = {normal(rng), normal(rng), normal(rng), normal(rng)};
        const double overall = scale * std::exp(std::log(1e-3) * uni(rng));
        const double s[3] = {overall, overall * std::exp(std::log(1.0 / 30) * uni(rng)), overall * std::exp(std::log(1.0 / 30) * uni(rng))};
        return build(q, s);
    };
    for (int i = 0; i < 200000; ++i) range.push_back(draw(1.0));
    for (int i = 0; i < 2000; ++i) {
        const double q[4] = {normal(rng), normal(rng), normal(rng), normal(rng)};
        const double a = 0.01 + uni(rng), b = 0.01 + uni(rng);
        const double sets[][3] = {{a, a, a}, {a, a, b}, {a, b, b}, {a, 0, 0}, {a, b, 0}, {0, 0, 0}, {a, 1e-4 * a, 1e-4 * a}, {a, b, 1e-4 * a}};
        for (const auto &s : sets) degenerate.push_back(build(q, s));
        const double id[4] = {1, 0, 0, 0};
        const double d[3] = {a, b, 0.5 * (a + b)};
        degenerate.push_back(build(id, d));                       // exactly diagonal, not sorted
        degenerate.push_back(draw(1e-6));
        degenerate.push_back(draw(1e3));
    }
    report<1>(range, degenerate);
    report<2>(range, degenerate);
    report<3>(range, degenerate);
    report<4>(range, degenerate);
    report<5>(range, degenerate);
    report<6>(range, degenerate);
    report<7>(range, degenerate);
    return 0;
}
