"""Concurrent calls: whole forwards / training steps issued round-robin on two HIP streams (INTEGRATION.md "Threading /
streams", bench.py `pipelined_timing`), from two host threads, and inside captured graphs that contain the side-stream fork
and join.  The kernels' numerics are pinned elsewhere; what is pinned here is that no call's state leaks into another:
the per-thread host words / sequence numbers / side stream / pending front half of csrc/api.hip, the per-process knob table
and attribute guards, and the shape-keyed estimates of rasterizer.py.

Every result is compared with the SERIAL render of the same batch (alone on the current stream, device idle before and
after), in the same call form.  Scenes of one shape differ in every output tensor, so a swapped, mixed or stale result
cannot pass; with LSR_DETERMINISTIC=1 (child process) gradient sums are order-independent, so any difference at all is
cross-talk."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

# Shape A: colour (degree-1 SH) + 4 direct feature channels + depth = the 8-channel compositing instances.
# Shape B: no colour, 4 feature channels = the 4-channel and sub-block instances; 3 x 5 = 15 tiles.
SHAPES = {
    "A": dict(G=6000, V=2, H=64, W=64, color_sh_degree=1, seeds=(101, 102, 103, 104)),
    "B": dict(G=2500, V=3, H=48, W=80, color_sh_degree=None, seeds=(201, 202)),
}
# Chosen on the CPU with util.oracle_forward (check_guards_on_cpu below): every batch then has pairs in every view and a mask
# above 0.5 on at least a quarter of its pixels (make_scene's defaults leave shape B at 19-28 %); the longest tile lists of
# shape A (1000-1270 keys) straddle the first sort-tier boundary, so the scenes' hints select different sort variants.
SIGMA_PX = (1.0, 6.0)
OPACITY_SCALE = 0.6
ROUNDS = 3
GRAD_BAR = 1e-5          # of max(1, |serial|.max()): float-atomic order only (tests/test_latency_gpu.py)
OUT_NAMES = ("color", "feature", "mask", "depth", "radii")
IN_NAMES = ("means", "cov6", "opac", "shs", "features")


class _Batch:
    """One scene of one shape: boundary inputs on the host, view table and input tensors on the device."""

    def __init__(self, shape, seed, dev=None):
        s = SHAPES[shape]
        self.shape, self.seed, self.H, self.W, self.V = shape, seed, s["H"], s["W"], s["V"]
        sc = util.make_scene(s["G"], image_size=max(self.H, self.W), views=self.V, color_sh_degree=s["color_sh_degree"],
                             feature_channels=4, feature_sh_degree=0, seed=seed, sigma_px=SIGMA_PX, opacity_scale=OPACITY_SCALE)
        self.bi = util.boundary_inputs(sc, self.H, self.W, bg=(0.1, 0.2, 0.3))
        self.deg = int(self.bi["sh_degree"] or 0)
        self.name = f"{shape}{seed}"
        if dev is not None:
            self.views = util.view_table(self.bi, dev)
            self.t = {k: self.bi[k].to(dev) for k in IN_NAMES if self.bi[k] is not None}


def _all_batches(dev=None):
    return [_Batch(shape, seed, dev) for shape, s in SHAPES.items() for seed in s["seeds"]]


def check_guards_on_cpu(batch):
    """The guards of the comparison, on the oracle: pairs in every view, mask > 0.5 on at least a quarter of the pixels."""
    o = [util.oracle_forward(batch.bi, v) for v in range(batch.V)]
    covered = float(np.mean([(x["mask"] > 0.5).mean() for x in o]))
    assert all(x["P"] > 0 for x in o) and covered >= 0.25, (batch.name, [x["P"] for x in o], covered)
    return o


def _call(b, t=None, **kw):
    from latentsplat_amd.rasterizer import rasterize_views
    t = b.t if t is None else t
    return rasterize_views(b.views, b.H, b.W, b.deg, t["means"], t["cov6"], t["opac"], shs=t.get("shs"), features=t["features"], **kw)


def _step(b, cot, **kw):
    """Forward with grad + backward on the current stream: (outputs, input gradients)."""
    leaf = {k: v.clone().requires_grad_(True) for k, v in b.t.items()}
    out = _call(b, leaf, **kw)
    pairs = [(o, cot[n]) for o, n in zip(out[:4], OUT_NAMES) if o is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    return [None if o is None else o.detach() for o in out], {k: v.grad for k, v in leaf.items()}


class _Serial:
    """Every batch rendered alone on the current stream, once per call form; never written to afterwards."""

    def __init__(self, dev, oracle=True):
        from latentsplat_amd.rasterizer import last_forward_status
        self.dev = dev
        self.batches = _all_batches(dev)
        gen = torch.Generator().manual_seed(5)
        self.cot = {}
        for shape, s in SHAPES.items():
            V, H, W = s["V"], s["H"], s["W"]
            self.cot[shape] = {n: torch.randn(sh, generator=gen).to(dev) for n, sh in
                               (("color", (V, 3, H, W)), ("feature", (V, 4, H, W)), ("mask", (V, H, W)), ("depth", (V, H, W)))}
        self.default, self.status, self.nosync, self.train_out, self.grads, self.kw = {}, {}, {}, {}, {}, {}
        sync = lambda: torch.cuda.synchronize(dev)
        for b in self.batches:
            sync()
            with torch.no_grad():
                self.default[b.name] = _call(b)
            sync()
            st = self.status[b.name] = last_forward_status()
            assert st["num_pairs"] > 0 and not st["overflow"], (b.name, st)
            frac = float((self.default[b.name][2] > 0.5).float().mean())
            assert frac >= 0.25, f"{b.name}: mask above 0.5 on {frac:.0%} of the pixels only"
        for b in self.batches:
            cap = int(1.5 * max(self.status[o.name]["num_pairs"] for o in self.batches if o.shape == b.shape))
            self.kw[b.name] = dict(pair_capacity=cap, max_tile_hint=self.status[b.name]["max_tile_pairs"])
            sync()
            with torch.no_grad():
                self.nosync[b.name] = _call(b, **self.kw[b.name])
            sync()
            assert last_forward_status() == self.status[b.name], b.name
            self.train_out[b.name], self.grads[b.name] = _step(b, self.cot[b.shape])
            sync()
        for form in (self.default, self.nosync, self.train_out):
            for a in self.batches:
                for b in self.batches:
                    if a.shape == b.shape and a.seed < b.seed:
                        for n, x, y in zip(OUT_NAMES, form[a.name], form[b.name]):
                            assert x is None or not torch.equal(x, y), f"{a.name} and {b.name} render the same {n}"
        if oracle:
            for b in (self.batches[0], next(x for x in self.batches if x.shape == "B")):
                self._hold_to_oracle(b)

    def _hold_to_oracle(self, b):
        out = self.default[b.name]
        for v, o in enumerate(check_guards_on_cpu(b)):
            what = f"serial {b.name} view {v}"
            if o["color"] is not None:
                util.assert_close_except_fragile(out[0][v].cpu().numpy(), o["color"], o, 1e-4, what + " colour")
            util.assert_close_except_fragile(out[1][v].cpu().numpy(), o["feature"], o, 1e-4, what + " feature")
            util.assert_close_except_fragile(out[2][v].cpu().numpy(), o["mask"], o, 1e-4, what + " mask")
            dscale = max(1.0, float(np.abs(o["depth"]).max()))
            zmax = float(o["gdepth"][o["radii"] > 0].max(initial=1.0))
            util.assert_close_except_fragile(out[3][v].cpu().numpy(), o["depth"], o, 1e-4 * dscale, what + " depth (tol 1e-4 of the largest depth)",
                                             flip_bound=2e-2 * max(dscale, zmax), scale=dscale)
            assert np.array_equal(out[4][v].cpu().numpy(), o["radii"]), what + " radii"


@pytest.fixture(scope="module")
def ref(hip_device):
    return _Serial(hip_device)


def _same_outputs(got, want, what):
    for n, x, y in zip(OUT_NAMES, got, want):
        assert (x is None) == (y is None), (what, n)
        assert x is None or torch.equal(x, y), f"{what}: {n} differs from the serial render"


def _grad_error(got, want, what, bitwise=False):
    """Largest |got - serial| over the input gradients, in units of the bar's scale max(1, |serial|.max())."""
    worst = 0.0
    for k, w in want.items():
        err = float((got[k] - w).abs().max()) / max(1.0, float(w.abs().max()))
        assert torch.isfinite(got[k]).all(), (what, k)
        assert (torch.equal(got[k], w) if bitwise else err <= GRAD_BAR), f"{what}: d{k} off the serial gradient by {err:.3e} of scale"
        worst = max(worst, err)
    return worst


class _Marks:
    """Start / end events around each call; after the final synchronisation: how many pairs of calls on different streams
    overlapped in time.  Reported, never asserted on."""

    def __init__(self, dev):
        self.base = torch.cuda.Event(enable_timing=True)
        self.base.record(torch.cuda.current_stream(dev))
        self.calls = []

    def event(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def add(self, lane, e0, e1):
        self.calls.append((lane, e0, e1))

    def report(self, what):
        t = [(lane, self.base.elapsed_time(e0), self.base.elapsed_time(e1)) for lane, e0, e1 in self.calls]
        n = sum(1 for i, a in enumerate(t) for b in t[i + 1:] if a[0] != b[0] and max(a[1], b[1]) < min(a[2], b[2]))
        print(f"\n[concurrent] {what}: {n} pairs of calls on different streams overlapped in time ({len(t)} calls)")
        return n


def _round_robin(dev, batches, run, what):
    """Call i of ROUNDS rounds over all batches on streams[i % 2]; no host synchronisation of ours until the end."""
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize(dev)
    marks, got = _Marks(dev), []
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(dev))
    i = 0
    for _ in range(ROUNDS):
        for b in batches:
            with torch.cuda.stream(streams[i % 2]):
                e0 = marks.event()
                res = run(b)
                marks.add(i % 2, e0, marks.event())
            got.append((b, res))
            i += 1
    torch.cuda.synchronize(dev)
    marks.report(what)
    return got


def test_nosync_forwards_round_robin_on_two_streams(hip_device, ref):
    """bench.py's pipelined pattern: lsr_forward_nosync issued round-robin on two streams, the host never waiting."""
    with torch.no_grad():
        got = _round_robin(hip_device, ref.batches, lambda b: _call(b, **ref.kw[b.name]), "no-sync forwards")
    for i, (b, out) in enumerate(got):
        _same_outputs(out, ref.nosync[b.name], f"call {i} ({b.name})")


def test_default_forwards_round_robin_on_two_streams(hip_device, ref):
    """The synchronous forward on two streams: the first call of a shape takes the exact path (the host polls its mapped
    words while the other stream is busy), later ones the speculative path with the front half launched early — sized from
    ANOTHER scene's counts (a re-run through the exact path if that falls short)."""
    from latentsplat_amd import rasterizer as rz
    rz._ESTIMATES.clear()
    before = dict(rz.SPECULATION_STATS)
    with torch.no_grad():
        got = _round_robin(hip_device, ref.batches, _call, "default forwards")
    after = dict(rz.SPECULATION_STATS)
    print(f"[concurrent] default forwards: {({k: after[k] - before[k] for k in after})}")
    assert after["exact"] > before["exact"] and after["speculative"] > before["speculative"], (before, after)
    for i, (b, out) in enumerate(got):
        _same_outputs(out, ref.default[b.name], f"call {i} ({b.name})")


def _train_on_streams(dev, ref, beside, what, bitwise=False):
    from latentsplat_amd import _lib
    try:
        _lib.set_knob("LSR_CLEAR_BESIDE", beside)
        got = _round_robin(dev, ref.batches, lambda b: _step(b, ref.cot[b.shape]), what)
    finally:
        _lib.set_knob("LSR_CLEAR_BESIDE", -1)
    worst = 0.0
    for i, (b, (out, grads)) in enumerate(got):
        _same_outputs(out, ref.train_out[b.name], f"{what}, call {i} ({b.name})")
        worst = max(worst, _grad_error(grads, ref.grads[b.name], f"{what}, call {i} ({b.name})", bitwise))
    print(f"[concurrent] {what}: worst gradient difference from serial {worst:.3e} of scale (bar {GRAD_BAR:.0e})")
    return worst


@pytest.mark.parametrize("beside", [-1, 1], ids=["default_knobs", "clear_beside"])
def test_training_steps_on_two_streams(hip_device, ref, beside):
    """Forward with grad + backward per batch, on alternating streams.  The backward runs on autograd's worker thread (not the
    thread that made the forward), on the forward's stream.  With LSR_CLEAR_BESIDE=1 both caller streams fork into the calling
    thread's single side stream, so the clear of one call's gradient workspace runs beside the other stream's compositing."""
    _train_on_streams(hip_device, ref, beside, f"training steps (LSR_CLEAR_BESIDE={beside})")


def _train_on_threads(dev, ref, what, bitwise=False):
    barrier = threading.Barrier(2)
    results, errors = [[], []], []

    def work(k):
        try:
            stream = torch.cuda.Stream(dev)
            barrier.wait(timeout=60)
            with torch.cuda.stream(stream):
                for _ in range(ROUNDS):
                    for b in ref.batches[k::2]:
                        results[k].append((b, _step(b, ref.cot[b.shape])))
            stream.synchronize()
        except BaseException as e:      # re-raised by the test
            errors.append(e)
            barrier.abort()

    torch.cuda.synchronize(dev)
    threads = [threading.Thread(target=work, args=(k,), daemon=True) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)            # a cap: the serial work takes under a second; a stuck poll shows as a failure
    assert not any(th.is_alive() for th in threads), f"{what}: a thread is still running"
    if errors:
        raise errors[0]
    torch.cuda.synchronize(dev)
    worst = 0.0
    for k in range(2):
        assert len(results[k]) == ROUNDS * len(ref.batches[k::2])
        for i, (b, (out, grads)) in enumerate(results[k]):
            _same_outputs(out, ref.train_out[b.name], f"{what}, thread {k} call {i} ({b.name})")
            worst = max(worst, _grad_error(grads, ref.grads[b.name], f"{what}, thread {k} call {i} ({b.name})", bitwise))
    print(f"\n[concurrent] {what}: worst gradient difference from serial {worst:.3e} of scale (bar {GRAD_BAR:.0e})")
    return worst


def test_training_steps_on_two_host_threads(hip_device, ref):
    """Two new host threads, each with its own stream and half of the batches, released together: each thread's pinned host
    words, events (and the estimates it shares with the other) come into being while the other thread is inside a call."""
    _train_on_threads(hip_device, ref, "two host threads")


def _bitwise_child():
    """Body of the LSR_DETERMINISTIC=1 child process of test_bitwise_leg."""
    dev = torch.device("cuda:0")
    ref = _Serial(dev, oracle=False)
    ok, failure = True, ""
    try:
        for beside in (-1, 1):
            _train_on_streams(dev, ref, beside, f"training steps (LSR_CLEAR_BESIDE={beside})", bitwise=True)
        _train_on_threads(dev, ref, "two host threads", bitwise=True)
    except AssertionError as e:
        ok, failure = False, str(e).splitlines()[0]
    print("EQUAL", ok, failure)


def test_bitwise_leg(hip_device):
    """LSR_DETERMINISTIC=1 (read once per process: a child): the gradient sums are fixed-point, their order cannot explain a
    difference — the two-stream and two-thread training steps must give the serial gradients bit for bit."""
    code = "import sys; sys.path.insert(0, %r)\nfrom tests import test_concurrent_calls_gpu as m\nm._bitwise_child()\n" % util.ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LSR_DETERMINISTIC="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print("\n" + "\n".join(l for l in r.stdout.splitlines() if l.startswith(("[concurrent]", "EQUAL"))))
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("EQUAL True"), line


def _captured_training_step(dev, b, cot, kw, warm_beside):
    """Warm-up (LSR_CLEAR_BESIDE=`warm_beside`), capture and three replays (LSR_CLEAR_BESIDE=1) of forward + backward on
    the calling thread; the gradients the replays leave behind."""
    from latentsplat_amd import _lib
    leaf = {k: v.clone().requires_grad_(True) for k, v in b.t.items()}

    def step():
        out = _call(b, leaf, **kw)
        pairs = [(o, cot[n]) for o, n in zip(out[:4], OUT_NAMES) if o is not None]
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])

    try:
        _lib.set_knob("LSR_CLEAR_BESIDE", warm_beside)
        side = torch.cuda.Stream(dev)            # warm-up on a side stream, as torch.cuda.graph asks for
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(dev).wait_stream(side)
        for v in leaf.values():
            v.grad = None
        _lib.set_knob("LSR_CLEAR_BESIDE", 1)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize(dev)
    finally:
        _lib.set_knob("LSR_CLEAR_BESIDE", -1)
    return {k: v.grad.clone() for k, v in leaf.items()}


def _in_fresh_thread(fn):
    box = {}

    def work():
        try:
            box["value"] = fn()
        except BaseException as e:
            box["error"] = e

    th = threading.Thread(target=work, daemon=True)
    th.start()
    th.join(timeout=120)
    assert not th.is_alive(), "the thread is still running"
    if "error" in box:
        raise box["error"]
    return box["value"]


def test_captured_fork_and_join(hip_device, ref):
    """A hipGraph capture of forward + backward that DOES contain the fork into the library's side stream and the join back
    (LSR_CLEAR_BESIDE=1: the gradient-workspace clear beside the compositing kernel), replayed three times; then the same
    on a new host thread whose warm-up cleared in line, so that its side stream and events are first used inside the capture."""
    dev = hip_device
    b = ref.batches[0]
    want = ref.grads[b.name]
    got = _captured_training_step(dev, b, ref.cot[b.shape], ref.kw[b.name], warm_beside=1)
    worst = _grad_error(got, want, "captured fork / join")
    fresh = _in_fresh_thread(lambda: _captured_training_step(dev, b, ref.cot[b.shape], ref.kw[b.name], warm_beside=0))
    worst_fresh = _grad_error(fresh, want, "captured fork / join, side stream first used under capture")
    print(f"\n[concurrent] captured fork / join: worst gradient difference from eager {worst:.3e} of scale; "
          f"first use under capture {worst_fresh:.3e} (bar {GRAD_BAR:.0e})")


def test_front_half_under_capture(hip_device, ref):
    """lsr_forward_front + lsr_forward_nosync(LSR_FWD_FRONT_DONE) captured on a host thread that has never called the library
    (no pinned words, no events yet), replayed twice: the one-call lsr_forward_nosync bit for bit; and a synchronous forward
    made on that thread afterwards reads its own pair count, not what a replay left in the thread's host words."""
    from latentsplat_amd import _lib
    from latentsplat_amd._lib import Dims, Outputs
    dev = hip_device
    lib = _lib.load()
    b = ref.batches[0]
    other = ref.batches[1]
    run = util.HipRun(b.bi, dev)                    # workspaces, outputs and the counts of the scene
    run_other = util.HipRun(other.bi, dev)
    assert run.P != run_other.P
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    cap = int(1.5 * run.P)
    binws = torch.zeros(lib.lsr_binning_workspace_bytes(C.byref(run.d), cap, 2 ** 31 - 1), dtype=torch.uint8, device=dev)
    outs = Outputs(p(run.color_out), p(run.feat_out), p(run.mask_out), p(run.depth_out), p(run.radii))
    images = (run.color_out, run.feat_out, run.mask_out, run.depth_out)
    stream_of = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.lsr_forward_nosync(C.byref(run.d), C.byref(run.inp), p(run.geom), p(binws), p(run.img), cap, run.maxtile,
                                      C.byref(outs), stream_of()), "one-call no-sync")
    torch.cuda.synchronize(dev)
    want = [x.clone() for x in images] + [run.radii.clone()]
    d = Dims.from_buffer_copy(run.d)
    d.forward_flags |= _lib.FWD_FRONT_DONE

    def in_thread():
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _lib.check(lib.lsr_forward_front(C.byref(d), C.byref(run.inp), p(run.geom), p(run.radii), cap, stream_of()), "front")
            _lib.check(lib.lsr_forward_nosync(C.byref(d), C.byref(run.inp), p(run.geom), p(binws), p(run.img), cap, run.maxtile,
                                              C.byref(outs), stream_of()), "no-sync after front")
        for replay in range(2):
            for x in images:
                x.fill_(-7.0)
            run.radii.fill_(-7)
            graph.replay()
            torch.cuda.synchronize(dev)
            for n, x, y in zip(OUT_NAMES, images + (run.radii,), want):
                assert torch.equal(x, y), f"replay {replay}: {n} differs from the one-call no-sync forward"
        # the other scene, synchronously, on the thread whose graph wrote (or did not write) the host words
        npairs, maxtile = C.c_int64(0), C.c_int32(0)
        _lib.check(lib.lsr_forward_prepare(C.byref(run_other.d), C.byref(run_other.inp), p(run_other.geom), p(run_other.radii),
                                           C.byref(npairs), C.byref(maxtile), stream_of()), "prepare")
        torch.cuda.synchronize(dev)
        return npairs.value, maxtile.value

    assert _in_fresh_thread(in_thread) == (run_other.P, run_other.maxtile)
