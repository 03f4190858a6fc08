"""The kernel instances and scheduling branches that only larger tile grids and more work items reach (tests/grid_variants.py:
two-phase binning, wide bin records, global-atomic tile counts, the stand-alone tile scan from registers and in passes, the
scatter without LDS reservation, the forward's queue / bin lists / item reordering, the backward's unsplit static and queue
branches for every payload width), forward AND backward against the oracle with the checks and bars of
tests/test_parity_gpu.py.  Every test first asserts that the case reaches what the table says on THIS device."""
import pytest
import torch

from tests import grid_variants as gv
from tests import util
from tests.test_parity_gpu import ABS_TOL, CLEAN_TOL, _check_forward, _fused_scene_check, _grad_scene

pytestmark = pytest.mark.gpu

RATIOS: dict = {}        # test id -> worst error / bar of its image and clean-gradient-row comparisons (printed: run with -s)


def _reaches(name, dev, **kw):
    """The case reaches its row of the table on this device — or fails naming the case to re-derive (never a skip)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    record = kw.get("record", True)
    got, want = gv.variants_of(name, cus, **kw), gv.expected(name, record=record, fuse=kw.get("fuse"))
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, (f"case {name!r} was derived for 256 compute units; with {cus} it reaches {diff} (got, table): "
                      f"re-derive its shape in tests/grid_variants.py")
    return want


class _one_oracle_per_view:
    """util.oracle_forward memoised per (case, view) while a case's tests run: the forward check and the two gradient
    checks of a case compare with the same, unchanged reference (same scene, same background)."""
    memo: dict = {}

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        memo = _one_oracle_per_view.memo
        for k in [k for k in memo if k[0] != self.name]:
            del memo[k]
        self.saved = util.oracle_forward

        def cached(bi, v):
            key = (self.name, v)
            if key not in memo:
                memo[key] = self.saved(bi, v)
            return memo[key]
        util.oracle_forward = cached
        return self

    def __exit__(self, *exc):
        util.oracle_forward = self.saved
        return False


class _ratios:
    """Records worst error / bar of the comparisons made inside (util.ACCOUNTING) under ``key`` and prints them."""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        self.n0 = len(util.ACCOUNTING)
        return self

    def __exit__(self, *exc):
        acc = util.ACCOUNTING[self.n0:]
        img = [a["worst_strict_err"] / (a["tol"] * a["scale"]) for a in acc if a["kind"] == "image"]
        grad = [a["worst_strict_err"] / (a["clean_tol"] * a["scale"]) for a in acc if a["kind"] == "grad"]
        RATIOS[self.key] = dict(image=max(img, default=None), clean_grad_rows=max(grad, default=None), passed=exc[0] is None)
        print(f"{self.key}: worst error / bar: images (bar {ABS_TOL:.0e}) {RATIOS[self.key]['image']}, "
              f"clean gradient rows (bar {CLEAN_TOL:.0e} of scale) {RATIOS[self.key]['clean_grad_rows']}")
        return False


def _bi(name):
    sc, H, W = gv.make_case_scene(name)
    return sc, H, W, util.boundary_inputs(sc, H, W, bg=(0.3, 0.1, 0.5))     # (the background of _grad_scene: one reference)


def _profiled(fn):
    """fn() and the set of stages it launched."""
    from latentsplat_amd import _lib
    _lib.profile_read(); _lib.profile_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return res, {k for k, (ms, n) in _lib.profile_read().items() if n}


def _forward_run(name, dev):
    """The synchronous forward of a case through the C ABI, with the structural assertions of the table."""
    want = _reaches(name, dev, record=False)
    sc, H, W, bi = _bi(name)
    run, launched = _profiled(lambda: util.HipRun(bi, dev))
    assert ("tile_scan" in launched) == (not want["fold"]), launched
    assert ("scatter" in launched) == (not want["segments"]), launched
    assert run.layout.geom_bin_stride == (12 if want["narrow"] else 16)
    assert run.header()[4] == 0, "overflow flag of the forward"
    return bi, run


@pytest.mark.parametrize("name", list(gv.CASES))
def test_forward_against_the_oracle(hip_device, name):
    with _one_oracle_per_view(name), _ratios(f"forward[{name}]"):
        bi, run = _forward_run(name, hip_device)
        _check_forward(bi, run)


@pytest.mark.parametrize("name", list(gv.CASES))
@pytest.mark.parametrize("with_aux", [False, True])
def test_gradients_against_the_oracle(hip_device, name, with_aux):
    from latentsplat_amd.rasterizer import last_forward_status
    _reaches(name, hip_device, record=True, depth_grad=with_aux)
    sc, H, W = gv.make_case_scene(name)
    with _one_oracle_per_view(name), _ratios(f"gradients[{name}, aux={with_aux}]"):
        _grad_scene(hip_device, sc, H, W, with_aux)
    assert not last_forward_status()["overflow"]


@pytest.mark.parametrize("name", ["queue4", "wide_global"])
def test_nosync_forward_gives_the_synchronous_bits(hip_device, name):
    """The no-sync forward (device-side pair count: the scatter and the later sort tiers always launched) on the bin lists
    (queue4) and on the wide scatter without LDS (wide_global): every output and the radii bit for bit."""
    from latentsplat_amd.rasterizer import last_forward_status, rasterize_views
    dev = hip_device
    _reaches(name, dev, record=False)
    sc, H, W, bi = _bi(name)
    t = {k: (None if bi[k] is None else bi[k].to(dev)) for k in ("means", "cov6", "opac", "shs", "features")}
    views = util.view_table(bi, dev)
    call = lambda **kw: rasterize_views(views, H, W, bi["sh_degree"], t["means"], t["cov6"], t["opac"], shs=t["shs"],
                                        features=t["features"], **kw)
    with torch.no_grad():
        ref = call()
        st = last_forward_status()
        assert not st["overflow"] and st["num_pairs"] > 0
        out = call(pair_capacity=2 * st["num_pairs"] + 64, max_tile_hint=int(st["max_tile_pairs"]))
        assert last_forward_status() == st, (last_forward_status(), st)
    for what, a, b in zip(("colour", "feature", "mask", "depth", "radii"), out, ref):
        assert (a is None) == (b is None), what
        assert a is None or torch.equal(a, b), f"{name}: {what} of the no-sync forward differs from the synchronous forward"


def test_queue4_through_the_global_queue(hip_device):
    """queue4 with LSR_FWD_BINQ = 0: the items beyond the static slots come from the one global queue word instead of the
    per-SIMD-bin lists; the same checks."""
    from latentsplat_amd import _lib
    name = "queue4"
    assert gv.expected(name)["bin_queue"]
    try:
        _lib.set_knob("LSR_FWD_BINQ", 0)
        with _one_oracle_per_view(name), _ratios("global_queue[queue4]"):
            bi, run = _forward_run(name, hip_device)
            _check_forward(bi, run)
            sc, H, W = gv.make_case_scene(name)
            for with_aux in (False, True):
                _grad_scene(hip_device, sc, H, W, with_aux)
    finally:
        _lib.set_knob("LSR_FWD_BINQ", -1)


@pytest.mark.parametrize("name,fuse", list(gv.EXPECT_SHARED))
def test_shared_scene_against_the_oracle(hip_device, name, fuse):
    """One scene shared by all views through the scene-level inputs: the fused projection + SH kernel (LSR_FUSE_SH = 1) and
    k_preprocess with two / four views per workgroup (0), each with and without its LDS tile histogram."""
    from latentsplat_amd import _lib
    from latentsplat_amd.rasterizer import last_forward_status
    want = _reaches(name, hip_device, fuse=fuse)
    sc, H, W = gv.make_case_scene(name)
    try:
        _lib.set_knob("LSR_FUSE_SH", fuse)
        with _ratios(f"shared[{name}, fuse={fuse}]"):
            _, launched = _profiled(lambda: _fused_scene_check(hip_device, sc, H, True))
    finally:
        _lib.set_knob("LSR_FUSE_SH", 1)
    assert ("tile_scan" in launched) == (not want["fold"]), launched
    assert "scatter" in launched and not want["segments"], launched
    assert {"render_forward", "render_backward"} <= launched
    assert not last_forward_status()["overflow"]
