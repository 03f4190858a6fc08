// preprocess.hip — stage K1: per-(view, Gaussian) projection, EWA covariance, conic, radius,
// tile rectangle, colour from SH, plus the per-tile pair histogram (LDS-privatised).
// View-dependent payload channels (colour from SH, latent features from SH) are filled in
// afterwards by sh.hip for the Gaussians that survive culling.
//
// Build this file with -ffp-contract=off: radius / rectangle / depth bits feed the bit-exact
// tile lists, so every float operation must be the single IEEE operation written here (the CPU
// oracle performs the identical sequence).  Spec: SURVEY.md Appendix A.1-A.3.
#include <algorithm>

#include "lsr_blend.h"
#include "lsr_depth.h"
#include "lsr_key_emit.h"
#include "lsr_project.h"

namespace lsr {

typedef const float __attribute__((address_space(4))) *kfloat_ptr;   // constant address space: uniform loads become s_load

constexpr int kPreThreads = 256;
static_assert(kPreThreads == kPreThreadsScan, "the folded tile scan is sized for this workgroup");
constexpr int kPreItems = 8;  // (Gaussian, view) items per thread: 2048 per block, one histogram flush each

// VB = views per block.  Views that read the same input slice (a shared scene, or the views of one
// group) are processed by ONE block: a thread loads its Gaussian once and loops over the block's VB
// views, so a shared scene is read V / VB times instead of V times (269 of the kernel's
// 578 MB were per-view re-reads of the scene from L2/MALL).  Items per thread shrink by the same
// factor, so the grid keeps its size.
//
// SEG (round 5, single-pass binning: lsr_internal.h segment_capacity): the workgroup also EMITS the sort keys of its
// items.  When all its items are projected, the LDS histogram holds its pair count per (view, tile); the one global
// atomic per non-empty counter that used to add the count to the tile's total now RETURNS the old total — the
// workgroup's first slot in the tile's fixed-capacity key segment — and a second pass over the workgroup's own binning
// records (12 bytes each, written a few microseconds earlier by the same thread: L2 hits, and a thread only ever reads
// what it wrote itself) places `depth << 32 | index << 8 | sub-block code` at segment[base + LDS cursor++].  This is
// k_scatter's body without its launch, without the machine-wide re-read of the records from HBM and without the wait
// for the tile scan in front of it; the order of the keys inside a segment is whatever the atomics produce, as before
// (k_sort_tiles sorts distinct 64-bit keys).
// AA (LSR_FWD_ANTIALIAS): the opacity of the screen record and of the footprint is opacity * rho (lsr_project.h); instances
// of their own, so the ones without it keep their code and their 80 registers.
template <int COLOR_MODE, bool LDS_HIST, int VB, bool FMA, bool SEG, bool AA = false>
__global__ void __launch_bounds__(kPreThreads, 6)   // six waves per SIMD (80 VGPRs): the kernel streams, occupancy hides its latencies
k_preprocess(lsr_dims d, lsr_inputs in, float *__restrict__ rec, int RF, char *__restrict__ binrec, int narrow,
             int32_t *__restrict__ radii, uint32_t *__restrict__ tile_count, uint32_t *header, FoldedScan fs, int kItems, SegOut seg) {
    static_assert(!SEG || LDS_HIST, "the key emission reserves its slots from the LDS histogram");
    extern __shared__ uint32_t s_hist[];   // [VB][T] pair counts
    // 64-byte records are staged here and stored by the whole block as one contiguous run
    // (lane-contiguous 16-byte stores) instead of 4 strided partial-line stores per thread.
    // Layout [k][thread] with a row stride of kPreThreads + 4 float4: the per-thread stores (fixed k,
    // consecutive threads) and the run-order loads (4 consecutive lanes = the 4 words of one
    // record) are both bank-conflict free.
    constexpr int kRecRow = kPreThreads + 4;
    __shared__ float4 s_rec[kRecRow * 4];
    static_assert(sizeof(float4) * kRecRow * 4 >= sizeof(uint32_t) * kFoldTiles, "the folded tile scan stages its counts here");
    const bool staged = RF == 16;
    const int v0 = blockIdx.y * VB;
    const int G = d.num_gaussians;
    const int gx = (d.width + LSR_TILE - 1) / LSR_TILE, gy = (d.height + LSR_TILE - 1) / LSR_TILE;
    const int T = gx * gy;
    // per-view constants that cost an IEEE division each: once per block, not once per (Gaussian, view)
    __shared__ float2 s_focal[VB];
    if (threadIdx.x < VB && v0 + (int)threadIdx.x < d.num_views) {
        const float *vw = in.views + (size_t)(v0 + threadIdx.x) * LSR_VIEW_FLOATS;
        s_focal[threadIdx.x] = make_float2(d.width / (2.0f * vw[35]), d.height / (2.0f * vw[36]));
    }
    if (LDS_HIST)
        for (int t = threadIdx.x; t < VB * T; t += kPreThreads) s_hist[t] = 0;
    __syncthreads();
    const int ce = d.cov_elems;
    const size_t sl = (size_t)input_slice(d, v0);   // the input slice all views of this block read
    const float *means = in.means3D + sl * d.vs_means;
    const float *covs = in.cov3D + sl * d.vs_cov;
    const float *opac = in.opacities + sl * d.vs_opac;
    constexpr int coff = COLOR_MODE == LSR_COLOR_NONE ? 0 : 3;
    const bool direct_feat = d.feat_mode == LSR_FEAT_DIRECT;
    const bool skip_none = reached_only(d);

    // kItems Gaussians per thread (at most kPreItems / VB: 2048 (Gaussian, view) items per block and histogram flush;
    // fewer when the call is small, so that a single view still fills the machine: launch_preprocess)
    const int base = blockIdx.x * (kPreThreads * kItems);
#pragma unroll 1
    for (int it = 0; it < kItems; ++it) {
        const int chunk0 = base + it * kPreThreads;
        if (chunk0 >= G) break;   // block-uniform
        const int i = chunk0 + threadIdx.x;
        const bool in_range = i < G;
        const size_t ii = in_range ? (size_t)i : 0;
        // ---- the Gaussian, once for all views of the block ----
        const float q0 = means[3 * ii], q1 = means[3 * ii + 1], q2 = means[3 * ii + 2];
        const float *c6 = covs + (size_t)ce * ii;
        const float r0 = c6[0], r1 = c6[1], r2 = c6[2];
        const float r3 = c6[ce == 9 ? 4 : 3], r4 = c6[ce == 9 ? 5 : 4], r5 = c6[ce == 9 ? 8 : 5];
        const float opacity = opac[ii];
        float pay_in[3] = {0.0f, 0.0f, 0.0f};
        if (COLOR_MODE == LSR_COLOR_PRECOMP) {
            const float *cp = in.color + sl * d.vs_color + 3 * ii;
            pay_in[0] = cp[0]; pay_in[1] = cp[1]; pay_in[2] = cp[2];
        }
        const float *fp = in.features + sl * d.vs_feat + ii * d.feat_channels;
        // payload slots 8.. : rgb (if any; SH colour is filled in by sh.hip) then the feature channels,
        // zero padded.  View independent, so the two words of a 64-byte record are built once per Gaussian.
        auto payload = [&](int c4) {
            float w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 4 * c4 + k;
                w[k] = c < coff ? pay_in[c < 3 ? c : 0]
                                : ((direct_feat && c - coff < d.feat_channels) ? fp[c - coff] : 0.0f);
            }
            return make_float4(w[0], w[1], w[2], w[3]);
        };
        float4 pay0 = make_float4(0, 0, 0, 0), pay1 = make_float4(0, 0, 0, 0);
        if (staged) { pay0 = payload(0); pay1 = payload(1); }
        // The wait for these loads belongs HERE, once per Gaussian: left to the compiler it lands inside the
        // view loop as `s_waitcnt vmcnt(0)`, which on gfx9 also waits for the previous view's record stores.
        asm volatile("" :: "v"(q0), "v"(q1), "v"(q2), "v"(r0), "v"(r1), "v"(r2), "v"(r3), "v"(r4), "v"(r5), "v"(opacity),
                     "v"(pay0.x), "v"(pay0.y), "v"(pay0.z), "v"(pay0.w), "v"(pay1.x), "v"(pay1.y), "v"(pay1.z), "v"(pay1.w));

#pragma unroll 1
        for (int vb = 0; vb < VB; ++vb) {
            const int v = v0 + vb;
            if (v >= d.num_views) break;   // block-uniform
            // the camera goes through the scalar cache into SGPRs (constant address space: the table was
            // written by an earlier launch), not through 44 broadcast vector loads per lane
            const kfloat_ptr vw = (kfloat_ptr)(in.views + (size_t)v * LSR_VIEW_FLOATS);
            float vm[16], pm[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) { vm[k] = vw[k]; pm[k] = vw[16 + k]; }
            const float tanfovx = vw[35], tanfovy = vw[36];
            const float focal_x = s_focal[vb].x, focal_y = s_focal[vb].y;   // = width / (2 tan), height / (2 tan)
            const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
            const float scale = vw[40], scale2 = scale * scale;   // scene scale (1/near), applied like the reference does
            const size_t o = (size_t)v * G + ii;
            const float p0 = q0 * scale, p1 = q1 * scale, p2 = q2 * scale;
            const float s0 = r0 * scale2, s1 = r1 * scale2, s2 = r2 * scale2;
            const float s3 = r3 * scale2, s4 = r4 * scale2, s5 = r5 * scale2;
            const Projected pj = project_gaussian<FMA, AA>(vm, pm, limx, limy, focal_x, focal_y, p0, p1, p2, s0, s1, s2, s3, s4, s5,
                                                       d.width, d.height, gx, gy, in_range);
            const bool ok = pj.ok;
            const float px = pj.px, py = pj.py, conic_a = pj.conic_a, conic_b = pj.conic_b, conic_c = pj.conic_c, tz = pj.tz;
            const float my_radius = pj.radius;
            const float rec_opacity = AA ? opacity * pj.rho : opacity;   // what the compositing kernels and the footprint see
            const TileRect rect{pj.rminx, pj.rminy, pj.rmaxx, pj.rmaxy};

            // slot 6, what the compositing kernels blend into the depth image: the view z, or the view's depth mode applied
            // to it (lsr_depth.h; the mode is uniform: a scalar branch, not taken by tables without a mode).  The bin
            // record's depth word — sort key, visibility — stays tz.
            float zpay = tz;
            if (vw[41] != 0.0f) zpay = depth_mode_payload((int)vw[41], tz, scale, vw[42], vw[43]);
            const float4 rr0 = make_float4(px, py, conic_a, conic_b);
            const float4 rr1 = make_float4(conic_c, rec_opacity, ok ? zpay : -1.0f, 0.0f);   // a negative slot 6 marks a culled record (staging only)
            // footprint span for the half-tile render lists (k_scatter / k_sort_tiles); not part of the bit-exact contract
            const uint32_t span = ok ? footprint_cells(px, py, conic_a, conic_b, conic_c, rec_opacity, rect.x0, rect.y0) : kSpanNone;
            if (ok) {
                if (!staged) {
                    float4 *R = (float4 *)(rec + o * (size_t)RF);
                    R[0] = rr0; R[1] = rr1;
                    for (int c4 = 0; c4 < (RF - 8) / 4; ++c4) R[2 + c4] = payload(c4);
                }
                count_pairs(LDS_HIST ? s_hist + vb * T : tile_count + (size_t)v * T, gx, rect, span, skip_none);
            }
            if (in_range) {
                radii[o] = ok ? (int32_t)my_radius : 0;
                store_bin_record(binrec, narrow, o, ok, rect, tz, span);
            }
            if (staged) {
                s_rec[0 * kRecRow + threadIdx.x] = rr0;
                s_rec[1 * kRecRow + threadIdx.x] = rr1;
                s_rec[2 * kRecRow + threadIdx.x] = pay0;
                s_rec[3 * kRecRow + threadIdx.x] = pay1;
                __syncthreads();
                float4 *dst = (float4 *)(rec + ((size_t)v * G + chunk0) * 16);
                const int nrec = G - chunk0 < kPreThreads ? G - chunk0 : kPreThreads;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int idx = k * kPreThreads + threadIdx.x;      // float4 index inside the run
                    // culled Gaussians (slot 6 < 0 in their staged record; a visible one holds z > 0.2 or a mode's d >= 0) are
                    // never read: skip them
                    if (idx < nrec * 4 && s_rec[kRecRow + (idx >> 2)].z >= 0.0f) dst[idx] = s_rec[(idx & 3) * kRecRow + (idx >> 2)];
                }
                __syncthreads();
            }
        }
    }
    // ---- behind the projection: histogram flush or key emission, and the folded tile scan (lsr_key_emit.h, shared with
    // k_preprocess_sh) ----
    const int n_valid = min(VB, d.num_views - v0) * T;   // counters of the workgroup's views that exist
    if (LDS_HIST && !SEG) flush_counts<kPreThreads>(s_hist, tile_count + (size_t)v0 * T, n_valid);
    if (SEG) {
        uint32_t *s_first = s_hist + VB * T;      // (the dynamic allocation holds two arrays of VB * T words in this instance)
        reserve_segments<kPreThreads>(s_hist, s_first, tile_count + (size_t)v0 * T, n_valid);
        constexpr int KI = kPreItems / VB;        // most Gaussians per thread
        const KeyBuckets kb(s_rec, sizeof(s_rec), T);   // (the record staging array is idle by now)
#pragma unroll 1
        for (int vb = 0; vb < VB; ++vb) {
            const int v = v0 + vb;
            if (v >= d.num_views) break;             // block-uniform
            // this view's records of the thread's Gaussians: unconditional loads at clamped addresses, all in flight together
            uint3 br[KI];
            int index[KI];
            bool valid[KI];
#pragma unroll
            for (int it = 0; it < KI; ++it) {
                const int i = min(base + min(it, kItems - 1) * kPreThreads + (int)threadIdx.x, G - 1);
                br[it] = *(const uint3 *)(binrec + ((size_t)v * G + (size_t)i) * sizeof(BinRec));
                index[it] = base + it * kPreThreads + (int)threadIdx.x;
                valid[it] = it < kItems && index[it] < G;
            }
            emit_view_keys<kPreThreads, KI>(s_hist + vb * T, s_first + vb * T, kb, seg, (uint32_t)v, T, gx, skip_none, br, index, valid);
        }
    }
    if (fs.enabled) {
        __shared__ TileScanShared<kPreThreads> s_scan;
        folded_tile_scan<kPreThreads>(fs, header, tile_count, d.num_views * T, (uint32_t *)s_rec, s_scan);
    }
}

__global__ void __launch_bounds__(256) k_clear16(uint4 *p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
// Zero `bytes` (a multiple of 16) at a 16-byte aligned device address.
hipError_t launch_clear(void *ptr, size_t bytes, hipStream_t s) {
    const size_t n16 = bytes / 16;
    if (n16 == 0) return hipSuccess;
    const size_t blocks = (n16 + 255) / 256;
    hipLaunchKernelGGL(k_clear16, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, (uint4 *)ptr, n16);
    return hipGetLastError();
}

hipError_t launch_preprocess(const lsr_dims &d, const lsr_inputs &in, char *geom, int32_t *radii, const FoldedScan &fs_in,
                             bool seg_mode, hipStream_t s) {
    const GeomLayout L = geom_layout(d);
    const int T = (int)num_tiles(d);
    // zero header + tile_count + tile_cursor (adjacent).  A kernel rather than hipMemsetAsync: the
    // stage sequence is captured into hipGraphs (latency mode), where back-to-back replays of a
    // captured memset node were observed to leave the counters uncleared on ROCm 7.2.
    {
        hipError_t e = launch_clear(geom + L.header, L.tile_start - L.header, s);   // both offsets are 256-byte aligned
        if (e != hipSuccess) return e;
    }
    if (d.num_gaussians == 0) return hipSuccess;
    // views per block: 4 (or 2) when that many consecutive views read the same input slice
    const bool shared = d.vs_means == 0 && d.vs_cov == 0 && d.vs_opac == 0 && (d.color_mode != LSR_COLOR_PRECOMP || d.vs_color == 0) &&
                        (d.feat_channels == 0 || d.vs_feat == 0);
    const int span = shared ? d.num_views : (d.views_per_group > 1 ? d.views_per_group : 1);   // views per input slice
    int vb = (span % 4 == 0 || (shared && span >= 4)) ? 4 : ((span % 2 == 0 || (shared && span >= 2)) ? 2 : 1);
    if (const int forced_vb = env_int("LSR_PRE_VB", 0)) vb = std::min(vb, forced_vb >= 4 ? 4 : (forced_vb >= 2 ? 2 : 1));   // (development knob)
    // Gaussians per thread: kPreItems / vb (one LDS histogram flush per 2048 items) unless that leaves fewer than two
    // workgroups per CU — a single 300 k view was 147 workgroups of 8 sequential Gaussians per thread on 256 CUs
    const int64_t yblocks = (d.num_views + vb - 1) / vb;
    const int64_t fill = ((int64_t)d.num_gaussians * yblocks + (int64_t)kPreThreads * 2 * device_cus() - 1) / ((int64_t)kPreThreads * 2 * device_cus());
    // (development knob: (Gaussian, view) items per thread and histogram flush; the key emission of the single-pass binning
    // keeps a thread's binning records in registers: never more than kPreItems there)
    const int pre_items = seg_mode ? std::min(kPreItems, std::max(1, env_int("LSR_PRE_ITEMS", kPreItems))) : std::max(1, env_int("LSR_PRE_ITEMS", kPreItems));
    const int items = (int)std::max<int64_t>(1, std::min<int64_t>(std::max(1, pre_items / vb), fill));
    dim3 grid((d.num_gaussians + kPreThreads * items - 1) / (kPreThreads * items), (unsigned)yblocks);
    float *rec = (float *)(geom + L.rec);
    char *binrec = geom + L.bin;
    const int narrow = narrow_bins(d) ? 1 : 0;
    const int RF = L.rec_floats;
    uint32_t *tc = (uint32_t *)(geom + L.tile_count);
    FoldedScan fs = fs_in;
    fs.tile_start = (uint32_t *)(geom + L.tile_start); fs.tile_order = (uint32_t *)(geom + L.tile_order);
    const bool lds = (size_t)T * vb <= 4096;
    const size_t shm = lds ? (size_t)T * vb * 4 * (seg_mode ? 2 : 1) : 0;   // (single-pass binning: counts and first slots)
    const bool fma = projection_contraction();
    // single-pass binning: the caller asks for it only when segment_capacity(d) > 0, which implies byte tile coordinates
    // and T <= 1024 (the LDS histogram of up to 4 views)
    SegOut so{nullptr, 0u, index_packing(d).key_shift};
    if (seg_mode) {
        if (!lds || !narrow || L.seg_cap == 0) return hipErrorInvalidValue;
        so.keys = (uint64_t *)(geom + L.seg_keys); so.cap = L.seg_cap;
    }
    const bool aa = (d.forward_flags & LSR_FWD_ANTIALIAS) != 0;
#define LSR_PRE5(CM, LH, VBV, FM, SG, AAV) hipLaunchKernelGGL((k_preprocess<CM, LH, VBV, FM, SG, AAV>), grid, dim3(kPreThreads), shm, s, d, in, rec, RF, binrec, narrow, radii, tc, (uint32_t *)(geom + L.header), fs, items, so)
#define LSR_PRE4(CM, LH, VBV, FM, SG) do { if (aa) LSR_PRE5(CM, LH, VBV, FM, SG, true); else LSR_PRE5(CM, LH, VBV, FM, SG, false); } while (0)
#define LSR_PRE3(CM, LH, VBV, FM) do { if (LH && seg_mode) LSR_PRE4(CM, LH, VBV, FM, LH); else LSR_PRE4(CM, LH, VBV, FM, false); } while (0)
#define LSR_PRE2(CM, LH, VBV) do { if (fma) LSR_PRE3(CM, LH, VBV, true); else LSR_PRE3(CM, LH, VBV, false); } while (0)
#define LSR_PRE(CM)                                                                              \
    do {                                                                                         \
        if (lds) { if (vb == 4) LSR_PRE2(CM, true, 4); else if (vb == 2) LSR_PRE2(CM, true, 2); else LSR_PRE2(CM, true, 1); } \
        else { if (vb == 4) LSR_PRE2(CM, false, 4); else if (vb == 2) LSR_PRE2(CM, false, 2); else LSR_PRE2(CM, false, 1); } \
    } while (0)
    prof_begin(kStPreprocess, s);
    if (d.color_mode == LSR_COLOR_SH) LSR_PRE(LSR_COLOR_SH);
    else if (d.color_mode == LSR_COLOR_PRECOMP) LSR_PRE(LSR_COLOR_PRECOMP);
    else LSR_PRE(LSR_COLOR_NONE);
#undef LSR_PRE
#undef LSR_PRE2
#undef LSR_PRE3
#undef LSR_PRE4
#undef LSR_PRE5
    prof_end(kStPreprocess, s);
    return hipGetLastError();
}

}  // namespace lsr
