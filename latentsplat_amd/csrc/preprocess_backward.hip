// preprocess_backward.hip — stages K8+K9 fused: per Gaussian, push the screen-space gradients
// collected by the compositing backward through
//   conic -> 2D covariance -> 3D covariance (6 packed values) and -> view-space mean (via J),
//   NDC mean -> world mean (perspective divide),  view z -> world mean (depth output),
// and back through the in-kernel scene scale.  (SH colour / latent-SH gradients: sh.hip.)
// Also scatters the per-(view, Gaussian) opacity / feature / precomputed-colour gradients from the
// packed records to the caller's tensors.
// A block of 256 threads owns 256 / PARTS Gaussians; its PARTS wave groups split the views of those
// Gaussians between them (group p takes views p, p+PARTS, ...: PARTS x more waves in flight and shorter
// per-thread load chains than one thread per Gaussian).  The view is WAVE-UNIFORM, so the camera comes
// through the scalar cache into SGPRs (round 1 gave the PARTS lanes of a quad different views: 40
// broadcast vector loads per (view, Gaussian), which kept the texture addresser ~90 % busy).  Gradients
// of inputs shared between views (stride 0) are summed in registers and combined across the PARTS
// groups through LDS in a fixed order — no atomics, no read-modify-write.
// Divisions are v_rcp_f32 (1 ulp) here: unlike the forward's, these results feed no bit-exact list — except the clamp
// decision of the EWA Jacobian, which is the forward's bit for bit (lsr_project.h view_space<FMA>: the forward's t in the
// projection convention of the call; IEEE t.x / t.z against 1.3f * tanfov).  The cull decision is the forward's radii.
// Recomputed from the same inputs rather than stored by the forward: the geometry record keeps the layout the compositing
// kernels read, and the two IEEE divisions cost ~1-2 % of this kernel (profiles/r07_fuzz_edges.md; taking them only near
// the limit, behind a branch, measured slower).  (The convention is read again at launch: a call must not switch
// lsr_set_projection_contraction between its forward and its backward.)
// Spec: SURVEY.md Appendix A.6.
#include "lsr_depth.h"
#include "lsr_wave.h"
#include "lsr_project.h"

namespace lsr {

struct PreBwdParams {
    lsr_dims d;
    lsr_inputs in;
    const int32_t *radii;
    const float *geo;       // screen-space records; slot 7 = colour clamp bits (SH mode)
    int geo_floats;
    const float *rec;       // packed gradient records (lsr_internal.h GradLayout)
    const float *zero_rec;  // an all-zero record line: read in place of the (uncleared, unwritten) record of a culled slot
    int rec_floats;
    lsr_in_grads g;
    GroupStrides gs;        // view groups (blockIdx.y): element offsets of the next group's slices
    CamGrad cam;            // camera-gradient instances (CAM): the partial records of dL/d(view record)
    float *means2D_abs;     // ABS instances: [V][G][3] absolute view-space gradient (lsr_internal.h), else unused
};

constexpr int kPreBwdFeat = 8;   // shared direct-feature gradients kept in registers up to this many channels

typedef const float __attribute__((address_space(4))) *kfloat_ptr;   // constant address space: uniform loads become s_load
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }

constexpr int kPreBwdThreads = 256;
constexpr int kPreBwdShared = 3 + 6 + 1 + kPreBwdFeat + 3;   // register accumulators of the shared inputs

// CAM: the camera-gradient instance (lsr_backward_views), launched NEXT TO the plain one: per (view, Gaussian) the
// derivative of the loss w.r.t. the view record from the same quantities, summed over the wave (one view, 64 Gaussians) and
// stored as one partial record (lsr_internal.h kCam*); it stores nothing else.  (Folded into the plain instance, the extra
// uses changed how the compiler contracted the Gaussian gradients — no longer bit for bit those of lsr_backward — and the
// 32 live partial sums spilled inside the view loop.)  The plain instances are the code they were.
// AA (forwards run with LSR_FWD_ANTIALIAS): the record's opacity was o' = o rho, rho^2 = det0 / det (lsr_project.h), so the
// moment m0 = sum o' G dL/dalpha is also rho dL/drho, and rho's dependence on the 2D covariance joins dL/d(a, b, c) below.
// Instances of their own again: the ones without it are the code they were.
// ABS (lsr_backward_absgrad; plain instances only): next to means2D, store the absolute view-space gradient from slots 14 / 15
// of the record, whose line the thread has just read.  Instances of their own once more.
template <int PARTS, bool FMA, bool CAM = false, bool AA = false, bool ABS = false>
__global__ void __launch_bounds__(kPreBwdThreads, 4)
k_preprocess_bwd(PreBwdParams pk) {
    // view groups: blockIdx.y = group; its inputs, gradient outputs and workspace slices (uniform: scalar arithmetic)
    PreBwdParams p = pk;
    {
        const int64_t g = blockIdx.y;
        p.in.views += g * pk.gs.views; p.in.means3D += g * pk.gs.means; p.in.cov3D += g * pk.gs.cov; p.in.opacities += g * pk.gs.opac;
        p.radii += g * pk.gs.slots; p.geo += g * pk.gs.slots * pk.geo_floats; p.rec += g * pk.gs.slots * pk.rec_floats;
        p.g.means3D += g * pk.gs.means; p.g.cov3D += g * pk.gs.cov; p.g.opacities += g * pk.gs.opac;
        if (p.g.color) p.g.color += g * pk.gs.color;
        if (p.g.features) p.g.features += g * pk.gs.feat;
        if (p.g.means2D) p.g.means2D += g * pk.gs.slots * 3;
        if constexpr (ABS) p.means2D_abs += g * pk.gs.slots * 3;
    }
    constexpr int LPP = kPreBwdThreads / PARTS;               // Gaussians per block = lanes per part
    static_assert(!(CAM && ABS), "the camera-gradient instance stores nothing but its partial records");
    __shared__ float s_part[PARTS > 1 ? (PARTS - 1) * kPreBwdShared * LPP : 1];
    const int part = __builtin_amdgcn_readfirstlane((int)threadIdx.x / LPP);   // wave-uniform
    const int slot = (int)threadIdx.x % LPP;
    const lsr_dims &d = p.d;
    const int G = d.num_gaussians;
    const int gi = blockIdx.x * LPP + slot;
    const bool live = gi < G;
    const int i = live ? gi : G - 1;     // idle lanes shadow the last Gaussian and store nothing
    const int V = d.num_views;
    const int ce = d.cov_elems;
    float am[3] = {0, 0, 0}, ac[6] = {0, 0, 0, 0, 0, 0}, aop = 0.0f;  // accumulators for shared inputs
    float af[kPreBwdFeat], acol[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < kPreBwdFeat; ++c) af[c] = 0.0f;
    const int coff = d.color_mode != LSR_COLOR_NONE ? 3 : 0;
    const bool feat_direct = d.feat_channels > 0 && d.feat_mode == LSR_FEAT_DIRECT;
    const bool feat_reg = feat_direct && d.vs_feat == 0 && d.feat_channels <= kPreBwdFeat;
    const bool feat_rmw = feat_direct && d.vs_feat == 0 && !feat_reg;   // many shared channels: one group, memory accumulate
    // Occupancy, not prefetching, hides the memory latency here: holding the NEXT view's record in
    // registers (round 1) cost 175 VGPRs = 2 waves per SIMD (0.155 ms per 16 views; 0.137 without it).
    const bool pay16 = feat_reg && p.rec_floats == 16;
    // (all wave-uniform; the camera-gradient instance stores no features: its parts always split the views)
    const bool one_part = feat_rmw && !CAM;
    const int v_first = one_part ? 0 : part, v_step = one_part ? 1 : PARTS, v_end = (one_part && part != 0) ? 0 : V;
    for (int v = v_first; v < v_end; v += v_step) {
        const size_t o = (size_t)v * G + i;
        const bool vis = p.radii[o] > 0;
        // (the records of culled slots are not cleared: their lanes read the zero line — one cached line instead of 32 % of
        // the record array)
        const float *rc = vis ? p.rec + o * p.rec_floats : p.zero_rec;
        const float4 r0 = *(const float4 *)rc, r1 = *(const float4 *)(rc + 4);           // m1x m1y m2xx m2xy | m2yy m0 gz -
        float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0;
        if (pay16) { q0 = *(const float4 *)(rc + 8); q1 = *(const float4 *)(rc + 12); }
        if constexpr (ABS) {
            // slots 14 / 15: sums of magnitudes in the exponent's units (log2) and in pixels -> natural units, NDC (as m2x / m2y
            // below).  Every live row is written: culled slots read the zero line.  (Stored here, while little else is live: next
            // to the means2D store the two values and their address cost the instance a wave per SIMD.)
            const float2 ab = *(const float2 *)(rc + 14);
            if (live) {
                float *oa = p.means2D_abs + 3 * o;
                oa[0] = ab.x * (kLn2 * 0.5f * d.width); oa[1] = ab.y * (kLn2 * 0.5f * d.height); oa[2] = 0.0f;
            }
        }
        // opacity: the record holds m0 = sum opacity * G * dL/dalpha; dL/dopacity = m0 / opacity
        // (m0 != 0 implies opacity >= 1/255)
        // AA: m0 is taken with the record's o' = o rho, and dL/do = rho dL/do' = rho m0 / o' = m0 / o: the division by the
        // INPUT opacity below, and the shared-opacity sum, are right as they stand.
        if constexpr (!CAM) {   // (the camera-gradient instance stores nothing but its partial records)
        if (d.vs_opac != 0) {
            const float o_in = p.in.opacities[(size_t)v * d.vs_opac + i];
            if (live) p.g.opacities[(size_t)v * d.vs_opac + i] = r1.y != 0.0f ? r1.y * rcp(o_in) : 0.0f;
        } else aop += r1.y;   // shared opacity: one division after the sum over the views
        // features / precomputed colours: plain pass-through of the record
        if (feat_reg) {
            if (p.rec_floats == 16) {   // the whole payload half of the record as two 16-byte loads
                const float pay[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                if (coff == 0) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) af[c] += pay[c];        // slots past the last channel are zero
                } else {
#pragma unroll
                    for (int c = 0; c < 5; ++c) af[c] += pay[3 + c];
                }
            } else {
#pragma unroll
                for (int c = 0; c < kPreBwdFeat; ++c)
                    if (c < d.feat_channels) af[c] += rc[8 + coff + c];
            }
        } else if (feat_direct && live) {
            float *gf = p.g.features + (size_t)v * d.vs_feat + (size_t)i * d.feat_channels;
            const bool first = d.vs_feat != 0 || v == 0;
            for (int c = 0; c < d.feat_channels; ++c) gf[c] = first ? rc[8 + coff + c] : gf[c] + rc[8 + coff + c];
        }
        if (d.color_mode == LSR_COLOR_PRECOMP) {
            if (d.vs_color != 0) {
                float *gcp = p.g.color + (size_t)v * d.vs_color + 3 * (size_t)i;
                if (live) for (int c = 0; c < 3; ++c) gcp[c] = rc[8 + c];
            } else {
                for (int c = 0; c < 3; ++c) acol[c] += rc[8 + c];
            }
        }
        }
        // ---- geometry: every lane runs the arithmetic (culled lanes on whatever they hold; IEEE special
        // values are harmless), `vis` masks the results where they are accumulated or stored ----
        const kfloat_ptr vw = (kfloat_ptr)(p.in.views + (size_t)v * LSR_VIEW_FLOATS);
        float vm[16], pm[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { vm[k] = vw[k]; pm[k] = vw[16 + k]; }
        const float tanfovx = vw[35], tanfovy = vw[36];
        const float focal_x = d.width * rcp(2.0f * tanfovx), focal_y = d.height * rcp(2.0f * tanfovy);
        const float scale = vw[40], scale2 = scale * scale;
        const float *mp = p.in.means3D + (size_t)v * d.vs_means + 3 * (size_t)i;
        const float p0 = mp[0] * scale, p1 = mp[1] * scale, p2 = mp[2] * scale;
        // ---- covariance path ----
        const ViewSpace vt = view_space<FMA>(vm, p0, p1, p2);   // the forward's t, bit for bit
        const float tz = vt.t2;
        // ---- depth modes (view slots 41..43, uniform): the record's gz is dL/dd of the payload d(z), z = tz / s; what joins
        // dL/dt.z below is gz dd/dz / s.  A scalar branch in front of all the arithmetic of the native path: no product of that
        // path feeds a sum across it, so tables without a mode get the gradients they always got.
        float gz_t = r1.z;
        [[maybe_unused]] float gz_s = 0.0f, gz_n = 0.0f, gz_f = 0.0f;   // CAM: explicit scale term, dL/dnear, dL/dfar
        if (vw[41] != 0.0f) {
            const float is = rcp(scale), z = tz * is;
            const DepthGrad dg = depth_mode_grad((int)vw[41], z, vw[42], vw[43]);
            gz_t = r1.z * dg.dz * is;
            if constexpr (CAM) { gz_s = -(r1.z * dg.dz) * z * is; gz_n = r1.z * dg.dn; gz_f = r1.z * dg.df; }
        }
        const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
        const float itz = rcp(tz), itz2 = itz * itz, itz3 = itz2 * itz;
        const float txtz = vt.t0 / tz, tytz = vt.t1 / tz;   // IEEE, as the forward: these decide the clamp
        const float xm = (txtz < -limx || txtz > limx) ? 0.0f : 1.0f;
        const float ym = (tytz < -limy || tytz > limy) ? 0.0f : 1.0f;
        const float tx = fminf(limx, fmaxf(-limx, txtz)) * tz;
        const float ty = fminf(limy, fmaxf(-limy, tytz)) * tz;
        const float j00 = focal_x * itz, j02 = -(focal_x * tx) * itz2;
        const float j11 = focal_y * itz, j12 = -(focal_y * ty) * itz2;
        // Wr[r][c] = vm[4c + r]; M = J * Wr (2x3)
        float M[2][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            M[0][c] = j00 * vm[4 * c + 0] + j02 * vm[4 * c + 2];
            M[1][c] = j11 * vm[4 * c + 1] + j12 * vm[4 * c + 2];
        }
        const float *c6 = p.in.cov3D + (size_t)v * d.vs_cov + (size_t)ce * (size_t)i;
        const float sxx = c6[0] * scale2, sxy = c6[1] * scale2, sxz = c6[2] * scale2;
        const float syy = c6[ce == 9 ? 4 : 3] * scale2, syz = c6[ce == 9 ? 5 : 4] * scale2, szz = c6[ce == 9 ? 8 : 5] * scale2;
        const float S[3][3] = {{sxx, sxy, sxz}, {sxy, syy, syz}, {sxz, syz, szz}};
        float MS[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) MS[r][c] = M[r][0] * S[0][c] + M[r][1] * S[1][c] + M[r][2] * S[2][c];
        const float a = MS[0][0] * M[0][0] + MS[0][1] * M[0][1] + MS[0][2] * M[0][2] + LSR_LOWPASS;
        const float b = MS[0][0] * M[1][0] + MS[0][1] * M[1][1] + MS[0][2] * M[1][2];
        const float c = MS[1][0] * M[1][0] + MS[1][1] * M[1][1] + MS[1][2] * M[1][2] + LSR_LOWPASS;
        const float det = a * c - b * b;
        // The compositing backward leaves MOMENTS of u = opacity * G * dL/dalpha over the pixels:
        //   r0 = (sum u dx, sum u dy, sum u dx^2, sum u dx dy), r1.x = sum u dy^2   (d = mean - pixel).
        // With the conic (A, B, C) = (c, -b, a) / det constant over the pixels:
        //   dL/dmean_pix = -(A m1x + B m1y, B m1x + C m1y),  dL/d(A, B, C) = -(m2xx / 2, m2xy, m2yy / 2)
        const float4 gcon = make_float4(-0.5f * r0.z, -r0.w, -0.5f * r1.x, 0.0f);
        // one select covers both exits: a culled Gaussian or a singular covariance contributes nothing
        // (det_inv = 0 zeroes the conic, hence gpx / gpy and, through d2, dL/d(a, b, c))
        const float det_inv = (vis && det != 0.0f) ? rcp(det) : 0.0f;
        const float cA = c * det_inv, cB = -b * det_inv, cC = a * det_inv;
        const float gpx = -(cA * r0.x + cB * r0.y);
        const float gpy = -(cB * r0.x + cC * r0.y);
        const float d2 = det_inv * det_inv;
        // conic = (c, -b, a) / det
        float dL_da = d2 * (gcon.x * (-c * c) + gcon.y * (b * c) + gcon.z * (det - a * c));
        float dL_dc = d2 * (gcon.x * (det - a * c) + gcon.y * (a * b) + gcon.z * (-a * a));
        float dL_db = d2 * (gcon.x * (2.0f * b * c) - gcon.y * (det + 2.0f * b * b) + gcon.z * (2.0f * a * b));
        if constexpr (AA) {
            // rho^2 = det0 / det with det0 = a0 c0 - b^2 of the undilated diagonal (formed from it, as the forward does):
            // dL/drho = m0 / rho, so dL/d(ln rho) = m0 and d(ln rho) = (d det0 / det0 - d det / det) / 2; a0, c0 have the
            // derivatives of a, c.  Where the forward took the floor (det0 / det <= 0.000025, also det0 <= 0 or NaN) rho is a
            // constant: nothing is added, and nothing of 1 / det0 is formed.  The decision is RECOMPUTED here (this unit's
            // contracted det0, det0 * rcp(det)), not the forward's (its FMA convention, an IEEE division): within an ulp of the
            // threshold the two can differ — a floored forward gets a term of its finite size, or the reverse.  Unlike the clamp
            // of the Jacobian the term is continuous in the inputs there, only its derivative jumps, so no bits are kept for it.
            const float a0 = MS[0][0] * M[0][0] + MS[0][1] * M[0][1] + MS[0][2] * M[0][2];
            const float c0 = MS[1][0] * M[1][0] + MS[1][1] * M[1][1] + MS[1][2] * M[1][2];
            const float det0 = a0 * c0 - b * b;
            const bool rho_live = det_inv != 0.0f && det0 * det_inv > 0.000025f;   // (det_inv = 0: culled or singular)
            const float i0 = rcp(rho_live ? det0 : 1.0f), m0 = r1.y;
            dL_da += rho_live ? 0.5f * m0 * (c0 * i0 - c * det_inv) : 0.0f;
            dL_dc += rho_live ? 0.5f * m0 * (a0 * i0 - a * det_inv) : 0.0f;
            dL_db += rho_live ? m0 * b * (det_inv - i0) : 0.0f;
        }
        // packed Sigma gradient: diagonal once, off-diagonals twice (stored once)
        float gm[3], gc[6];
        gc[0] = dL_da * M[0][0] * M[0][0] + dL_db * M[0][0] * M[1][0] + dL_dc * M[1][0] * M[1][0];
        gc[3] = dL_da * M[0][1] * M[0][1] + dL_db * M[0][1] * M[1][1] + dL_dc * M[1][1] * M[1][1];
        gc[5] = dL_da * M[0][2] * M[0][2] + dL_db * M[0][2] * M[1][2] + dL_dc * M[1][2] * M[1][2];
        gc[1] = 2.0f * dL_da * M[0][0] * M[0][1] + dL_db * (M[0][0] * M[1][1] + M[0][1] * M[1][0]) + 2.0f * dL_dc * M[1][0] * M[1][1];
        gc[2] = 2.0f * dL_da * M[0][0] * M[0][2] + dL_db * (M[0][0] * M[1][2] + M[0][2] * M[1][0]) + 2.0f * dL_dc * M[1][0] * M[1][2];
        gc[4] = 2.0f * dL_da * M[0][1] * M[0][2] + dL_db * (M[0][1] * M[1][2] + M[0][2] * M[1][1]) + 2.0f * dL_dc * M[1][1] * M[1][2];
        // dL/dM, then dL/dJ = dM * Wr^T
        float dM[2][3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            dM[0][cc] = 2.0f * MS[0][cc] * dL_da + MS[1][cc] * dL_db;
            dM[1][cc] = 2.0f * MS[1][cc] * dL_dc + MS[0][cc] * dL_db;
        }
        // Wr[k][cc] = vm[4cc + k]
        const float dJ00 = dM[0][0] * vm[0] + dM[0][1] * vm[4] + dM[0][2] * vm[8];
        const float dJ02 = dM[0][0] * vm[2] + dM[0][1] * vm[6] + dM[0][2] * vm[10];
        const float dJ11 = dM[1][0] * vm[1] + dM[1][1] * vm[5] + dM[1][2] * vm[9];
        const float dJ12 = dM[1][0] * vm[2] + dM[1][1] * vm[6] + dM[1][2] * vm[10];
        const float dL_dtx = xm * (-focal_x * itz2) * dJ02;
        const float dL_dty = ym * (-focal_y * itz2) * dJ12;
        float dL_dtz = -focal_x * itz2 * dJ00 - focal_y * itz2 * dJ11 +
                       (2.0f * focal_x * tx) * itz3 * dJ02 + (2.0f * focal_y * ty) * itz3 * dJ12;
        dL_dtz += gz_t;
        // t = Wr p + trans  =>  dL/dp[cc] = sum_k Wr[k][cc] dt[k] = vm[4cc + k] dt[k]
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
            gm[cc] = vm[4 * cc + 0] * dL_dtx + vm[4 * cc + 1] * dL_dty + vm[4 * cc + 2] * dL_dtz;
        // ---- NDC mean path ----
        const float h0 = pm[0] * p0 + pm[4] * p1 + pm[8] * p2 + pm[12];
        const float h1 = pm[1] * p0 + pm[5] * p1 + pm[9] * p2 + pm[13];
        const float h3 = pm[3] * p0 + pm[7] * p1 + pm[11] * p2 + pm[15];
        const float m_w = rcp(h3 + 0.0000001f);
        const float mul1 = h0 * m_w * m_w, mul2 = h1 * m_w * m_w;
        const float m2x = gpx * (0.5f * d.width);   // d pixel / d ndc
        const float m2y = gpy * (0.5f * d.height);
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
            gm[cc] += (pm[4 * cc + 0] * m_w - pm[4 * cc + 3] * mul1) * m2x +
                      (pm[4 * cc + 1] * m_w - pm[4 * cc + 3] * mul2) * m2y;
        if constexpr (CAM) {
            // gm / gc are still the gradients w.r.t. the SCALED mean / covariance here
            float cg[kCamSlots];
            const float pp[3] = {p0, p1, p2};
            // t = Wr p + vm[12..14] and M = J Wr (Wr[k][c] = vm[4c + k]): dL/dWr = dt p^T + J^T dM
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                cg[kCamVm + 3 * cc + 0] = dL_dtx * pp[cc] + j00 * dM[0][cc];
                cg[kCamVm + 3 * cc + 1] = dL_dty * pp[cc] + j11 * dM[1][cc];
                cg[kCamVm + 3 * cc + 2] = dL_dtz * pp[cc] + j02 * dM[0][cc] + j12 * dM[1][cc];
            }
            cg[kCamVm + 9] = dL_dtx; cg[kCamVm + 10] = dL_dty; cg[kCamVm + 11] = dL_dtz;
            // (h0, h1, h3) = p^T pm[.., 0 / 1 / 3] + pm[12 + j]; ndc = (h0, h1) * m_w
            const float dh[3] = {m2x * m_w, m2y * m_w, -(m2x * mul1 + m2y * mul2)};
#pragma unroll
            for (int cc = 0; cc < 3; ++cc)
#pragma unroll
                for (int j = 0; j < 3; ++j) cg[kCamPm + 3 * cc + j] = dh[j] * pp[cc];
#pragma unroll
            for (int j = 0; j < 3; ++j) cg[kCamPm + 9 + j] = dh[j];
            // focal = size / (2 tanfov) enters J only; the clamped t.x / t.y are constants (no gradient through the limit)
            cg[kCamTanX] = -(dJ00 * itz - dJ02 * tx * itz2) * focal_x * rcp(tanfovx);
            cg[kCamTanY] = -(dJ11 * itz - dJ12 * ty * itz2) * focal_y * rcp(tanfovy);
            // scene scale s: p = s mean, Sigma = s^2 cov (packed off-diagonals: gc holds both halves)
            const float ci[6] = {c6[0], c6[1], c6[2], c6[ce == 9 ? 4 : 3], c6[ce == 9 ? 5 : 4], c6[ce == 9 ? 8 : 5]};
            float sc = 0.0f;
#pragma unroll
            for (int k = 0; k < 6; ++k) sc += gc[k] * ci[k];
            cg[kCamScaleGeo] = gm[0] * mp[0] + gm[1] * mp[1] + gm[2] * mp[2] + 2.0f * scale * sc + gz_s;
#pragma unroll
            for (int k = kCamScaleGeo + 1; k < kCamSlots; ++k) cg[k] = 0.0f;
            // culled slots and idle lanes contribute nothing (their arithmetic may have produced anything)
            const bool cv = live && vis;
#pragma unroll
            for (int k = 0; k <= kCamScaleGeo; ++k) cg[k] = cv ? cg[k] : 0.0f;
            const float r = wave_sum32(cg);
            const int lane = (int)threadIdx.x & (LSR_WAVE - 1);
            const int chunk = (int)blockIdx.x * (LPP / LSR_WAVE) + slot / LSR_WAVE;
            const size_t vg = (size_t)blockIdx.y * V + v;     // the view in the whole call
            if (lane <= kCamScaleGeo && chunk < p.cam.chunks)
                p.cam.part[(vg * p.cam.chunks + chunk) * kCamSlots + lane] = r;
            // near / far of the depth modes: a pair of their own per (view, chunk), zeros in the native mode
            float dn = cv ? gz_n : 0.0f, df = cv ? gz_f : 0.0f;
            wave_all_each(Add(), dn, df);
            if (lane == 0 && chunk < p.cam.chunks) *(float2 *)(p.cam.dpart + (vg * p.cam.chunks + chunk) * 2) = make_float2(dn, df);
        }
        if constexpr (CAM) continue;
        // gradients are w.r.t. the UNSCALED inputs: mean_scaled = s * mean, cov_scaled = s^2 * cov;
        // a culled Gaussian's values are discarded here (its arithmetic may have produced anything)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) gm[cc] = vis ? gm[cc] * scale : 0.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) gc[k] = vis ? gc[k] * scale2 : 0.0f;
        if (d.vs_means != 0) {
            float *o3 = p.g.means3D + (size_t)v * d.vs_means + 3 * (size_t)i;
            if (live) { o3[0] = gm[0]; o3[1] = gm[1]; o3[2] = gm[2]; }
        } else { am[0] += gm[0]; am[1] += gm[1]; am[2] += gm[2]; }
        if (d.vs_cov != 0) {
            float *o6 = p.g.cov3D + (size_t)v * d.vs_cov + (size_t)ce * (size_t)i;
            if (live) {
                if (ce == 9) {   // upper triangle carries the gradient (that is what the packing reads)
                    o6[0] = gc[0]; o6[1] = gc[1]; o6[2] = gc[2]; o6[3] = 0.0f; o6[4] = gc[3]; o6[5] = gc[4];
                    o6[6] = 0.0f; o6[7] = 0.0f; o6[8] = gc[5];
                } else {
#pragma unroll
                    for (int k = 0; k < 6; ++k) o6[k] = gc[k];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) ac[k] += gc[k];
        }
        if (p.g.means2D && live) {
            float *o2 = p.g.means2D + 3 * o;
            o2[0] = vis ? m2x : 0.0f; o2[1] = vis ? m2y : 0.0f; o2[2] = 0.0f;
        }
    }
    if constexpr (CAM) return;
    // ---- shared inputs: groups 1.. leave their partial sums in LDS, group 0 adds them in order and stores ----
    float *acc[kPreBwdShared];
    {
        int n = 0;
        for (int k = 0; k < 3; ++k) acc[n++] = &am[k];
        for (int k = 0; k < 6; ++k) acc[n++] = &ac[k];
        acc[n++] = &aop;
        for (int k = 0; k < kPreBwdFeat; ++k) acc[n++] = &af[k];
        for (int k = 0; k < 3; ++k) acc[n++] = &acol[k];
    }
    if (PARTS > 1) {
        if (part > 0) {
#pragma unroll
            for (int k = 0; k < kPreBwdShared; ++k) s_part[((part - 1) * kPreBwdShared + k) * LPP + slot] = *acc[k];
        }
        __syncthreads();
        if (part == 0) {
#pragma unroll
            for (int q = 1; q < PARTS; ++q)
#pragma unroll
                for (int k = 0; k < kPreBwdShared; ++k) *acc[k] += s_part[((q - 1) * kPreBwdShared + k) * LPP + slot];
        }
    }
    const bool writer = live && part == 0;
    if (d.vs_means == 0 && writer) {
        float *o3 = p.g.means3D + 3 * (size_t)i;
        o3[0] = am[0]; o3[1] = am[1]; o3[2] = am[2];
    }
    if (d.vs_cov == 0 && writer) {
        float *o6 = p.g.cov3D + (size_t)ce * (size_t)i;
        if (ce == 9) {
            o6[0] = ac[0]; o6[1] = ac[1]; o6[2] = ac[2]; o6[3] = 0.0f; o6[4] = ac[3]; o6[5] = ac[4];
            o6[6] = 0.0f; o6[7] = 0.0f; o6[8] = ac[5];
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) o6[k] = ac[k];
        }
    }
    if (d.vs_opac == 0 && writer) p.g.opacities[i] = aop != 0.0f ? aop * rcp(p.in.opacities[i]) : 0.0f;
    if (feat_reg && writer) {
        float *gf = p.g.features + (size_t)i * d.feat_channels;
#pragma unroll
        for (int c = 0; c < kPreBwdFeat; ++c)
            if (c < d.feat_channels) gf[c] = af[c];
    }
    if (d.color_mode == LSR_COLOR_PRECOMP && d.vs_color == 0 && writer) {
        float *gcp = p.g.color + 3 * (size_t)i;
        gcp[0] = acol[0]; gcp[1] = acol[1]; gcp[2] = acol[2];
    }
}

hipError_t launch_preprocess_backward(const lsr_dims &d_all, const lsr_inputs &in, const char *geom,
                                      const int32_t *radii, const char *grad,
                                      const lsr_in_grads &gin, hipStream_t s, const CamGrad &cam, float *means2D_abs) {
    if (d_all.num_gaussians == 0) return hipSuccess;
    const GeomLayout L = geom_layout(d_all);
    const GradLayout R = grad_layout(d_all);
    const lsr_dims d = group_dims(d_all);      // what one view group (blockIdx.y) looks like to the kernel
    PreBwdParams p;
    p.d = d; p.in = in; p.radii = radii;
    p.gs = group_strides(d_all);
    p.geo = (const float *)(geom + L.rec); p.geo_floats = L.rec_floats;
    p.rec = (const float *)(grad + R.rec); p.rec_floats = R.rec_floats;
    p.zero_rec = (const float *)(grad + R.fixed - 256);
    p.g = gin;
    p.cam = cam;
    p.means2D_abs = means2D_abs;
    prof_begin(kStPreprocessBwd, s);
    const int parts = d.num_views >= 4 ? 4 : (d.num_views >= 2 ? 2 : 1);
    const int per_block = kPreBwdThreads / parts;   // Gaussians per block
    const dim3 grid((unsigned)((d.num_gaussians + per_block - 1) / per_block), (unsigned)num_view_groups(d_all));
    // the projection convention of the forward (lsr_set_projection_contraction): the clamp decision must be its own
    const bool aa = (d.forward_flags & LSR_FWD_ANTIALIAS) != 0;   // the forward's flag word: its projection scaled the opacities
#define LSR_PREBWD3(PT, FM, CM, AAV, AB) hipLaunchKernelGGL((k_preprocess_bwd<PT, FM, CM, AAV, AB>), grid, dim3(kPreBwdThreads), 0, s, p)
#define LSR_PREBWD2(PT, FM, CM) do { \
        if (!CM && means2D_abs) { if (aa) LSR_PREBWD3(PT, FM, false, true, true); else LSR_PREBWD3(PT, FM, false, false, true); } \
        else if (aa) LSR_PREBWD3(PT, FM, CM, true, false); else LSR_PREBWD3(PT, FM, CM, false, false); } while (0)
#define LSR_PREBWD(FM, CM) do { \
        if (parts == 4) LSR_PREBWD2(4, FM, CM); else if (parts == 2) LSR_PREBWD2(2, FM, CM); else LSR_PREBWD2(1, FM, CM); } while (0)
    if (cam.part) {   // the camera gradient: a second launch over the same records (the plain instance follows below)
        if (projection_contraction()) LSR_PREBWD(true, true); else LSR_PREBWD(false, true);
    }
    if (projection_contraction()) LSR_PREBWD(true, false); else LSR_PREBWD(false, false);
#undef LSR_PREBWD
#undef LSR_PREBWD2
#undef LSR_PREBWD3
    prof_end(kStPreprocessBwd, s);
    return hipGetLastError();
}

}  // namespace lsr
