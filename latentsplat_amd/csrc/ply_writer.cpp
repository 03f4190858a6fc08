// ply_writer.cpp — host side of the scene export (include/lsr_ply.h, "scene export"): the file writer and the SH
// change-of-basis table.  Plain C++ with no HIP in it, like ply_reader.cpp, so that it builds into a stand-alone host
// program (and runs under the host sanitizers) on its own.
#include <stdint.h>
#include <stdio.h>

#include "lsr_ply.h"
#include "lsr_sh_axes_table.h"
#include "lsr_sh_shape.h"

extern "C" {

int lsr_ply_sh_axes_matrix(double *out) {
    if (!out) return LSR_ENULL;
    for (int i = 0; i < 25 * 25; ++i) out[i] = 0.0;
    int off = 0;
    for (int l = 0; l <= LSR_MAX_SH_DEGREE; ++l) {
        const int n = 2 * l + 1, at = l * l;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) out[25 * (at + i) + at + j] = kShAxesM[off + n * i + j];
        off += n * n;
    }
    return LSR_OK;
}

int lsr_ply_write_scene_host(const char *path, const float *rows_host, int64_t n, int32_t sh_coeffs) {
    if (!path || (n > 0 && !rows_host)) return LSR_ENULL;
    const int K = sh_coeffs;
    if (n < 0 || !lsr::sh_valid_coeffs(K)) return LSR_EINVAL;
    FILE *f = fopen(path, "wb");
    if (!f) return LSR_EINVAL;
    bool ok = fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %lld\n", (long long)n) > 0;
    static const char *const head[] = {"x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"};
    static const char *const tail[] = {"opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"};
    for (int k = 0; k < 9 && ok; ++k) ok = fprintf(f, "property float %s\n", head[k]) > 0;
    for (int k = 0; k < 3 * (K - 1) && ok; ++k) ok = fprintf(f, "property float f_rest_%d\n", k) > 0;
    for (int k = 0; k < 8 && ok; ++k) ok = fprintf(f, "property float %s\n", tail[k]) > 0;
    ok = ok && fprintf(f, "end_header\n") > 0;
    const size_t row_bytes = sizeof(float) * (size_t)LSR_PLY_SCENE_ROW_FLOATS(K);
    if (ok && n > 0) ok = fwrite(rows_host, row_bytes, (size_t)n, f) == (size_t)n;
    ok = (fclose(f) == 0) && ok;
    return ok ? LSR_OK : LSR_EINVAL;
}

}  // extern "C"
