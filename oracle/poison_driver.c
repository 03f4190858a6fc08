/*
 * poison_driver.c — stand-alone runner of raster_oracle.c for sanitizer builds (tests/test_poison_cpu.py).
 *
 * Reads the flat binary scene tests/poison_cases.write_flat_scene writes and runs, view by view, the oracle's
 * preprocess -> bin / sort -> render -> render backward -> preprocess backward with all-ones output gradients.  Built
 * together with raster_oracle.c under -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all, a scene of
 * non-finite and degenerate Gaussians must run to exit code 0: every float -> int conversion of the oracle is defined.
 * Prints one line per view (pairs, visible Gaussians, non-finite pixels).  Host code only; it never runs on a GPU machine.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int64_t oracle_preprocess(int G, int H, int W, const float *means3D, const float *cov3D, const float *opacities,
                          const float *shs, int sh_degree, int sh_coeffs, const float *colors_precomp,
                          const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx,
                          float tanfovy, int32_t *radii, int32_t *rect, uint32_t *tiles_touched, float *depth, float *xy,
                          float *conic_opacity, float *rgb, uint8_t *clamped);
void oracle_bin_sort(int G, int H, int W, const int32_t *rect, const uint32_t *tiles_touched, const float *depth, int64_t P,
                     uint64_t *keys, uint32_t *point_list, uint32_t *ranges);
void oracle_render(int H, int W, int C, const uint32_t *ranges, const uint32_t *point_list, const float *xy,
                   const float *conic_opacity, const float *depth, const float *rgb, const float *features, const float *bg,
                   float *out_color, float *out_feat, float *out_mask, float *out_depth, float *final_T, uint32_t *n_contrib,
                   uint32_t *n_considered, int32_t *fragile, int fragile_cap, int32_t *fragile_count);
void oracle_render_backward(int H, int W, int C, const uint32_t *ranges, const uint32_t *point_list, const float *xy,
                            const float *conic_opacity, const float *depth, const float *rgb, const float *features,
                            const float *bg, const float *final_T, const uint32_t *n_contrib, const float *dL_dcolor,
                            const float *dL_dfeat_out, const float *dL_dmask, const float *dL_ddepth, double *dL_dxy_ndc,
                            double *dL_dconic, double *dL_dopacity, double *dL_drgb, double *dL_dfeat, double *dL_dz);
void oracle_preprocess_backward(int G, int H, int W, const float *means3D, const float *cov3D, const float *shs, int sh_degree,
                                int sh_coeffs, int has_colors_precomp, const float *viewmatrix, const float *projmatrix,
                                const float *campos, float tanfovx, float tanfovy, const int32_t *radii, const uint8_t *clamped,
                                const double *dL_dxy_ndc, const double *dL_dconic, const double *dL_dopacity,
                                const double *dL_drgb, const double *dL_dz, float *dL_dmeans3D, float *dL_dcov3D,
                                float *dL_dopac_out, float *dL_dshs, float *dL_dcolors_precomp, float *dL_dmeans2D);

static void *zalloc(size_t n, size_t size) {
    void *p = calloc(n ? n : 1, size);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(3); }
    return p;
}

static float *read_floats(FILE *f, size_t n) {
    float *p = (float *)zalloc(n, sizeof(float));
    if (fread(p, sizeof(float), n, f) != n) { fprintf(stderr, "short scene file\n"); exit(3); }
    return p;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s scene.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hd[7];
    if (fread(hd, sizeof(int32_t), 7, f) != 7) { fprintf(stderr, "short header\n"); return 3; }
    const int V = hd[0], G = hd[1], H = hd[2], W = hd[3], deg = hd[4], K = hd[5], C = hd[6];
    if (V < 1 || G < 1 || H < 1 || W < 1 || K < 1 || C < 1 || C > 64 || (deg + 1) * (deg + 1) > K) { fprintf(stderr, "bad header\n"); return 3; }
    float *cam = read_floats(f, (size_t)V * 40);
    float *means = read_floats(f, (size_t)V * G * 3), *cov = read_floats(f, (size_t)V * G * 6);
    float *opac = read_floats(f, (size_t)G), *shs = read_floats(f, (size_t)G * K * 3);
    float *feat = read_floats(f, (size_t)V * G * C);
    fclose(f);
    const int T = ((W + 15) / 16) * ((H + 15) / 16), HW = H * W;
    for (int v = 0; v < V; ++v) {
        const float *cv = cam + (size_t)v * 40, *bg = cv + 2, *vm = cv + 5, *pm = cv + 21, *cp = cv + 37;
        const float *m = means + (size_t)v * G * 3, *c6 = cov + (size_t)v * G * 6, *ft = feat + (size_t)v * G * C;
        int32_t *radii = zalloc(G, 4), *rect = zalloc((size_t)G * 4, 4);
        uint32_t *tiles = zalloc(G, 4);
        float *depth = zalloc(G, 4), *xy = zalloc((size_t)G * 2, 4), *co = zalloc((size_t)G * 4, 4), *rgb = zalloc((size_t)G * 3, 4);
        uint8_t *clamped = zalloc((size_t)G * 3, 1);
        const int64_t P = oracle_preprocess(G, H, W, m, c6, opac, shs, deg, K, NULL, vm, pm, cp, cv[0], cv[1], radii, rect, tiles,
                                            depth, xy, co, rgb, clamped);
        uint64_t *keys = zalloc((size_t)P, 8);
        uint32_t *plist = zalloc((size_t)P, 4), *ranges = zalloc((size_t)T * 2, 4);
        oracle_bin_sort(G, H, W, rect, tiles, depth, P, keys, plist, ranges);
        float *oc = zalloc((size_t)3 * HW, 4), *of = zalloc((size_t)C * HW, 4), *om = zalloc(HW, 4), *od = zalloc(HW, 4), *fT = zalloc(HW, 4);
        uint32_t *nc = zalloc(HW, 4), *ncons = zalloc(HW, 4);
        int32_t *fragile = zalloc(2 * 4096, 4), nfrag = 0;
        oracle_render(H, W, C, ranges, plist, xy, co, depth, rgb, ft, bg, oc, of, om, od, fT, nc, ncons, fragile, 4096, &nfrag);
        long bad = 0, vis = 0;
        for (int i = 0; i < 3 * HW; ++i) bad += !isfinite(oc[i]);
        for (int i = 0; i < C * HW; ++i) bad += !isfinite(of[i]);
        for (int i = 0; i < G; ++i) vis += radii[i] > 0;
        float *gc = zalloc((size_t)3 * HW, 4), *gf = zalloc((size_t)C * HW, 4), *gm = zalloc(HW, 4), *gd = zalloc(HW, 4);
        for (int i = 0; i < 3 * HW; ++i) gc[i] = 1.0f;
        for (int i = 0; i < C * HW; ++i) gf[i] = 1.0f;
        for (int i = 0; i < HW; ++i) { gm[i] = 1.0f; gd[i] = 1.0f; }
        double *dxy = zalloc((size_t)G * 2, 8), *dcon = zalloc((size_t)G * 3, 8), *dop = zalloc(G, 8), *drgb = zalloc((size_t)G * 3, 8);
        double *dft = zalloc((size_t)G * C, 8), *dz = zalloc(G, 8);
        oracle_render_backward(H, W, C, ranges, plist, xy, co, depth, rgb, ft, bg, fT, nc, gc, gf, gm, gd, dxy, dcon, dop, drgb, dft, dz);
        float *g_m = zalloc((size_t)G * 3, 4), *g_c = zalloc((size_t)G * 6, 4), *g_o = zalloc(G, 4), *g_s = zalloc((size_t)G * K * 3, 4);
        float *g_2 = zalloc((size_t)G * 3, 4);
        oracle_preprocess_backward(G, H, W, m, c6, shs, deg, K, 0, vm, pm, cp, cv[0], cv[1], radii, clamped, dxy, dcon, dop, drgb, dz,
                                   g_m, g_c, g_o, g_s, NULL, g_2);
        printf("view %d: pairs %lld visible %ld non-finite pixels %ld\n", v, (long long)P, vis, bad);
        free(radii); free(rect); free(tiles); free(depth); free(xy); free(co); free(rgb); free(clamped); free(keys); free(plist);
        free(ranges); free(oc); free(of); free(om); free(od); free(fT); free(nc); free(ncons); free(fragile); free(gc); free(gf);
        free(gm); free(gd); free(dxy); free(dcon); free(dop); free(drgb); free(dft); free(dz); free(g_m); free(g_c); free(g_o);
        free(g_s); free(g_2);
    }
    free(cam); free(means); free(cov); free(opac); free(shs); free(feat);
    return 0;
}
