"""Which kernel instance and scheduling branch a rasterizer call reaches, restated in plain Python from the launchers, and
the case table of tests/test_grid_variants_{cpu,gpu}.py: the smallest shapes that flip each switch.

The kernels switch on two quantities: the tile grid (T tiles per view, N = V T (view, tile) counts) and the number of
half-tile work items 2 N measured against the launch's wave slots (CUs x resident waves).  `variants` restates every such
predicate (it never calls the library; sources named per line), the CPU test pins it for every case at 256 compute units
against the hand-written EXPECT table below — the "reaches" column — and the GPU test asserts the same for the device it
runs on, so that on a part with another CU count the cases fail by name instead of quietly testing another corner."""
from __future__ import annotations

FWD_WAVES = {4: 24, 8: 16, 12: 12, 36: 8}      # render_forward.hip launch_render_forward: resident waves per CU (LSR_RF / LSR_RFR)
MAX_REORDER_ITEMS = 16384                      # lsr_internal.h kMaxReorderItems
FOLD_TILES = 4096                              # lsr_internal.h kFoldTiles
SCAN_THREADS, SCAN_REGS = 1024, 8              # binning.hip kScanThreads, kScanRegs


def padded_channels(nch: int) -> int:
    """nchp of both compositing launchers: the payload width of the kernel instance."""
    return 4 if nch <= 4 else (8 if nch <= 8 else (12 if nch <= 12 else 36))


def variants(H, W, V, nch, depth_grad, record, shared, fused, cus, pairs=None, coef_words=4096):
    """H x W pixels, V views, nch payload channels (colour counts 3); depth_grad: the backward receives dL/ddepth; record: a
    backward follows the forward (LSR_FWD_FOR_BACKWARD); shared: all views read one input slice; fused: the projection and
    the SH payload run as one kernel (sh.hip fused_preprocess_sh); cus: compute units; pairs: the call's (Gaussian, tile)
    pairs (None: few enough for the per-SIMD-bin lists); coef_words: words of the fused kernel's coefficient rows
    (sh.hip coef_words_of: 64 x (3 K colour + C Kf latent coefficients))."""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    T = tx * ty
    N = V * T
    items = 2 * N
    nchp = padded_channels(nch)
    out = {}
    # lsr_internal.h narrow_bins: byte tile coordinates in 12-byte bin records, else 16-byte records
    out["narrow"] = tx <= 255 and ty <= 255
    # api.hip segment_capacity: single-pass binning (key segments) — byte coordinates, at most 1024 tiles per view, the
    # fused kernel's LDS (sh.hip fused_segments_fit), and segments of at least 1024 keys within 512 MB and 32-bit indices
    align4 = lambda x: (x + 3) & ~3
    fit = (max(align4(coef_words), 4096) + 2 * N) * 4 <= 65536
    cap = 8192
    while cap > 1024 and (N * cap * 8 > 512 << 20 or N * cap >= 1 << 32):
        cap = (cap // 2 + 63) // 64 * 64
    out["segments"] = (out["narrow"] and T <= 1024 and (not fused or fit)
                       and not (N * cap * 8 > 512 << 20 or N * cap >= 1 << 32))
    if fused:
        # sh.hip launch_preprocess_sh: lds_hist (always with segments)
        out["vb"] = None
        out["pre_lds"] = out["segments"] or (N <= 8192 and (align4(coef_words) + N) * 4 <= 65536)
    else:
        # preprocess.hip launch_preprocess: views per workgroup, LDS histogram of T vb counters
        span = V if shared else 1
        vb = 4 if (span % 4 == 0 or (shared and span >= 4)) else (2 if (span % 2 == 0 or (shared and span >= 2)) else 1)
        out["vb"] = vb
        out["pre_lds"] = T * vb <= 4096
    # lsr_internal.h fold_tile_scan: the projection kernel's last workgroup scans; else k_tile_scan is launched
    out["fold"] = N <= FOLD_TILES
    # lsr_tile_scan.h tile_scan_block in k_tile_scan: counts in registers while per <= kScanRegs (None: folded, counts in LDS)
    per = (N + SCAN_THREADS - 1) // SCAN_THREADS
    out["scan_in_regs"] = None if out["fold"] else per <= SCAN_REGS
    # binning.hip launch_binning: k_scatter<LDS_RESERVE> (what a scatter launch of these dims instantiates)
    out["scatter_lds"] = T <= 8192
    # render_forward.hip launch_render_forward: k_render_fwd_small (row items, or sub-block items for all) or the half-tile kernel
    small = nchp in (4, 8) and 2 * items <= 24 * cus
    out["fwd_kernel"] = ("quad" if 8 * items <= 24 * cus else "rows") if small else "half"
    # k_render_fwd: items beyond the static wave slots come from the queue (the small kernel's units always fit its slots)
    out["fwd_queue"] = out["fwd_kernel"] == "half" and items > cus * FWD_WAVES[nchp]
    # ... from the per-SIMD-bin lists instead of the global queue word (4-channel instances, short lists)
    out["bin_queue"] = out["fwd_queue"] and nchp == 4 and (pairs is None or pairs <= 3000 * N) and 4 * cus <= 4096
    # k_order_items: the RECORD half-tile forward writes tile_order2 for the backward
    out["reorder"] = (bool(record) and out["fwd_kernel"] == "half" and nchp in (4, 8)
                      and 16 * cus < items <= MAX_REORDER_ITEMS)
    # render_backward.hip launch_render_backward / launch_variant: wave slots, list splitting, queue branch
    wpb = {4: 16, 8: 12 if depth_grad else 16, 12: 8, 36: 4}[nchp]
    slots = cus * wpb
    pl = 0
    while pl < 3 and (items << (pl + 1)) <= slots:
        pl += 1
    out["bwd_parts_log2"] = pl
    out["bwd_queue"] = (items << pl) > slots
    return out


_SPLATS = dict(sigma_px=(1.0, 12.0), opacity_scale=1.0)
_STRIP = dict(color_sh_degree=1, feature_channels=4, sigma_px=(2.0, 40.0), opacity_scale=1.0)
_LARGE = dict(color_sh_degree=1, feature_channels=4, sigma_px=(2.0, 30.0), opacity_scale=1.0)

# per-view inputs: make_scene(G, image_size=max(H, W), views=V, seed=3, **scene); nch = 3 (colour) + feature channels
CASES = {
    "queue36": dict(H=272, W=256, V=4, G=3000, nch=35, scene=dict(color_sh_degree=1, feature_channels=32, **_SPLATS)),
    "static36": dict(H=272, W=256, V=1, G=3000, nch=35, scene=dict(color_sh_degree=1, feature_channels=32, **_SPLATS)),
    "queue12": dict(H=400, W=416, V=3, G=4000, nch=11, scene=dict(color_sh_degree=2, feature_channels=8, **_SPLATS)),
    "queue8": dict(H=520, W=528, V=2, G=4000, nch=7, scene=dict(color_sh_degree=2, feature_channels=4, **_SPLATS)),
    "queue4": dict(H=520, W=528, V=3, G=4000, nch=4, scene=dict(color_sh_degree=None, feature_channels=4, **_SPLATS)),
    "scan_regs": dict(H=496, W=512, V=5, G=4000, nch=4, scene=dict(color_sh_degree=None, feature_channels=4, **_SPLATS)),
    "scan_passes": dict(H=520, W=528, V=8, G=3000, nch=7, scene=dict(color_sh_degree=0, feature_channels=4, **_SPLATS)),
    "wide_x": dict(H=40, W=4090, V=2, G=30000, nch=7, scene=_STRIP),
    "tall_y": dict(H=4090, W=40, V=2, G=30000, nch=7, scene=_STRIP),
    "wide_global": dict(H=528, W=4112, V=1, G=12000, nch=7, scene=_LARGE),
    "narrow_global": dict(H=1040, W=2064, V=2, G=12000, nch=7, scene=_LARGE),
}
# shared scene through the scene-level inputs (test_parity_gpu._fused_scene_check, shared=True), LSR_FUSE_SH 1 and 0;
# coefficient rows: 64 x (3 x 16 + 4 x 4) = 4096 words
SHARED_CASES = {
    "shared_v3": dict(size=528, V=3, G=1500, nch=7, coef_words=4096,
                      scene=dict(color_sh_degree=3, feature_channels=4, feature_sh_degree=1, **_SPLATS)),
    "shared_v8": dict(size=528, V=8, G=1500, nch=7, coef_words=4096,
                      scene=dict(color_sh_degree=3, feature_channels=4, feature_sh_degree=1, **_SPLATS)),
}


def _row(narrow, segments, pre_lds, vb, fold, scan_in_regs, scatter_lds, fwd_kernel, fwd_queue, bin_queue, reorder,
         bwd_parts_log2, bwd_queue):
    return dict(narrow=narrow, segments=segments, pre_lds=pre_lds, vb=vb, fold=fold, scan_in_regs=scan_in_regs,
                scatter_lds=scatter_lds, fwd_kernel=fwd_kernel, fwd_queue=fwd_queue, bin_queue=bin_queue, reorder=reorder,
                bwd_parts_log2=bwd_parts_log2, bwd_queue=bwd_queue)


Y, n = True, False
# The "reaches" column at 256 compute units, worked out by hand from the sources (T, N, items in the comments), for a
# forward that a backward without a depth gradient follows.  A forward alone differs in `reorder` (False everywhere); a
# depth gradient changes nothing in this table at 256 CUs: the <8, depth gradient> instance has 3072 slots instead of 4096,
# and no case has between 3073 and 4096 items.
#                      narrow seg pre_lds vb fold regs scat_lds fwd    fwd_q bin_q reord pl bwd_q
EXPECT = {
    "queue36":       _row(Y, Y, Y, 1, Y, None, Y, "half", Y, n, n, 0, Y),   # T 272,  N 1088,  items 2176 > 2048 (fwd<36>), > 1024 (bwd<36>)
    "static36":      _row(Y, Y, Y, 1, Y, None, Y, "half", n, n, n, 0, n),   # T 272,  N 272,   items 544: 1088 > 1024, so unsplit, and static
    "queue12":       _row(Y, Y, Y, 1, Y, None, Y, "half", Y, n, n, 0, Y),   # T 650,  N 1950,  items 3900 > 3072, > 2048
    "queue8":        _row(Y, n, Y, 1, Y, None, Y, "half", Y, n, Y, 0, Y),   # T 1089, N 2178,  items 4356 > 4096 (and > 3072 with a depth gradient)
    "queue4":        _row(Y, n, Y, 1, Y, None, Y, "half", Y, Y, Y, 0, Y),   # T 1089, N 3267,  items 6534 > 6144, > 4096
    "scan_regs":     _row(Y, Y, Y, 1, n, Y,    Y, "half", Y, Y, Y, 0, Y),   # T 992,  N 4960 (5 counts per thread), items 9920
    "scan_passes":   _row(Y, n, Y, 1, n, n,    Y, "half", Y, n, n, 0, Y),   # T 1089, N 8712 (9 per thread), items 17424 > 16384
    "wide_x":        _row(n, n, Y, 1, Y, None, Y, "rows", n, n, n, 0, n),   # 3 x 256 tiles, N 1536, items 3072: 2 x 3072 = 6144 row units
    "tall_y":        _row(n, n, Y, 1, Y, None, Y, "rows", n, n, n, 0, n),   # 256 x 3 tiles
    "wide_global":   _row(n, n, n, 1, n, n,    n, "half", Y, n, n, 0, Y),   # 33 x 257 = 8481 tiles (9 per thread), items 16962 > 16384
    "narrow_global": _row(Y, n, n, 1, n, n,    n, "half", Y, n, n, 0, Y),   # 65 x 129 = 8385 tiles, N 16770 (17 per thread), items 33540
}
# (case, LSR_FUSE_SH) -> row
EXPECT_SHARED = {
    ("shared_v3", 1): _row(Y, n, Y, None, Y, None, Y, "half", Y, n, Y, 0, Y),   # T 1089, Vg T 3267 <= 8192 in 64 KB; items 6534
    ("shared_v3", 0): _row(Y, n, Y, 2,    Y, None, Y, "half", Y, n, Y, 0, Y),   # vb 2: 2178 counters
    ("shared_v8", 1): _row(Y, n, n, None, n, n,    Y, "half", Y, n, n, 0, Y),   # Vg T 8712 > 8192; items 17424 > 16384
    ("shared_v8", 0): _row(Y, n, n, 4,    n, n,    Y, "half", Y, n, n, 0, Y),   # vb 4: T vb 4356 > 4096
}
del Y, n


def expected(name, record=True, fuse=None):
    """The hand-written row of a case (of (case, fuse) for the shared scenes), for a forward with / without a backward."""
    row = dict(EXPECT[name] if fuse is None else EXPECT_SHARED[(name, fuse)])
    if not record:
        row["reorder"] = False
    return row


def variants_of(name, cus, depth_grad=False, record=True, fuse=None, pairs=None):
    """variants(...) of a case of the tables above."""
    if fuse is None:
        c = CASES[name]
        return variants(c["H"], c["W"], c["V"], c["nch"], depth_grad, record, False, False, cus, pairs)
    c = SHARED_CASES[name]
    return variants(c["size"], c["size"], c["V"], c["nch"], depth_grad, record, True, bool(fuse), cus, pairs, c["coef_words"])


def make_case_scene(name):
    """(scene, H, W) of a case: make_scene(G, image_size=max(H, W), views=V, seed=3, ...)."""
    from tests import util
    if name in CASES:
        c = CASES[name]
        return util.make_scene(c["G"], image_size=max(c["H"], c["W"]), views=c["V"], seed=3, **c["scene"]), c["H"], c["W"]
    c = SHARED_CASES[name]
    return util.make_scene(c["G"], image_size=c["size"], views=c["V"], seed=3, **c["scene"]), c["size"], c["size"]
