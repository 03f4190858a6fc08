"""The fused Adam step without a GPU: the C ABI's export and argument checks (every documented LSR_EINVAL / LSR_ENULL
case of include/lsr_optim.h returns its code before any GPU work; nothing to do returns LSR_OK), the schedule, the
wrappers' refusals, the reference against itself, and the fitting tool's flags."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from latentsplat_amd import _lib
from tests import adam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENULL = 0, -1, -2
P = 0x1000       # a non-NULL pointer that is never dereferenced: every call below returns before any GPU work
VIS = C.c_void_p(0x2000)


def test_symbol_is_exported_and_listed():
    lib = _lib.load()
    assert hasattr(lib, "lsr_adam_step") and "lsr_adam_step" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "lsr_optim.h")).read()
    assert "lsr_adam_step" in header and "LSR_ADAM_MAX_TABLES 24" in header and "LSR_ADAM_MAX_WIDTH 4096" in header
    assert lib.lsr_abi_version() == 10 and _lib.ABI_VERSION == 10
    assert (_lib.ADAM_MAX_TABLES, _lib.ADAM_MAX_WIDTH, _lib.ADAM_MAX_ROWS) == (24, 4096, 1 << 40)
    import latentsplat_amd
    for name in ("adam_step", "SceneAdam", "expon_lr", "visible_from_radii"):
        assert callable(getattr(latentsplat_amd, name))
    assert issubclass(latentsplat_amd.SceneAdam, torch.optim.Adam)


def test_struct_layout_matches_the_header():
    """four pointers, an int64, two int32, eight floats, in the header's order: 80 bytes, no padding"""
    T = _lib.AdamTable
    assert C.sizeof(T) == 80
    names = [f[0] for f in T._fields_]
    assert names == ["param", "grad", "exp_avg", "exp_avg_sq", "rows", "width", "reserved", "beta1", "beta2", "one_minus_beta1",
                     "one_minus_beta2", "eps", "step_size", "inv_sqrt_bc2", "reserved_f"]
    assert [getattr(T, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76]
    header = open(os.path.join(ROOT, "include", "lsr_optim.h")).read()
    body = header[header.index("typedef struct lsr_adam_table {"):header.index("} lsr_adam_table;")]
    at = [body.index(n) for n in ("*param;", "*grad;", "*exp_avg;", "*exp_avg_sq;", "rows;", "width;", "reserved;", "beta1, beta2;",
                                  "one_minus_beta1, one_minus_beta2;", "eps;", "step_size;", "inv_sqrt_bc2;", "reserved_f;")]
    assert at == sorted(at)


def _table(**kw):
    base = dict(param=P, grad=P, exp_avg=P, exp_avg_sq=P, rows=100, width=3, reserved=0, beta1=0.9, beta2=0.999, one_minus_beta1=0.1,
                one_minus_beta2=0.001, eps=1e-15,
                step_size=1e-3, inv_sqrt_bc2=1.0, reserved_f=0.0)
    base.update(kw)
    return _lib.AdamTable(**base)


def _call(tables, visible=None, visible_rows=0, num_tables=None, null_tables=False):
    arr = (_lib.AdamTable * max(1, len(tables)))(*tables)
    return _lib.load().lsr_adam_step(None if null_tables else arr, len(tables) if num_tables is None else num_tables, visible,
                                     visible_rows, None)


INF, NAN = float("inf"), float("nan")


@pytest.mark.parametrize("bad", [dict(rows=-1), dict(rows=(1 << 40) + 1), dict(width=0), dict(width=-3), dict(width=4097),
                                 dict(reserved=1), dict(reserved_f=1.0), dict(reserved_f=NAN),
                                 dict(beta1=NAN), dict(beta2=INF), dict(eps=NAN), dict(eps=INF), dict(step_size=INF), dict(step_size=NAN),
                                 dict(inv_sqrt_bc2=INF), dict(inv_sqrt_bc2=NAN),
                                 dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=1.5), dict(beta2=-1e-3), dict(eps=-1e-8),
                                 dict(one_minus_beta1=NAN), dict(one_minus_beta2=INF), dict(one_minus_beta1=-0.1), dict(one_minus_beta2=1.5)])
def test_invalid_tables_are_rejected(bad):
    assert _call([_table(**bad)]) == EINVAL
    assert _call([_table(), _table(**bad)]) == EINVAL                       # in any position
    assert _call([_table(**dict(bad, rows=bad.get("rows", 0)))]) == EINVAL   # an empty table is checked too
    # LSR_EINVAL is reported before LSR_ENULL
    assert _call([_table(param=None), _table(**bad)]) == EINVAL


def test_count_and_sparse_checks():
    assert _call([_table()], num_tables=-1) == EINVAL and _call([_table()] * 2, num_tables=25) == EINVAL
    # sparse mode: every table with rows has visible_rows rows
    assert _call([_table(rows=100)], VIS, 99) == EINVAL and _call([_table(rows=100)], VIS, -1) == EINVAL
    assert _call([_table(rows=100), _table(rows=101)], VIS, 100) == EINVAL
    assert _call([_table(rows=100, param=None), _table(rows=0)], VIS, 100) == ENULL   # (a table without rows matches any mask)
    # dense mode: visible_rows is not read
    assert _call([_table(rows=0)], None, -7) == OK
    # a grid beyond one launch: 24 tables of 2^40 rows x 4096 floats
    assert _call([_table(rows=1 << 40, width=4096)] * 24) == EINVAL
    assert _call([_table(rows=1 << 40, width=4096, param=None)]) == EINVAL   # 2^40 workgroups of 4096 floats: one table is too much


def test_null_pointers_are_rejected():
    assert _call([_table()], null_tables=True) == ENULL
    for hole in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert _call([_table(**{hole: None})]) == ENULL, hole
        assert _call([_table(rows=0), _table(**{hole: None})]) == ENULL, hole
        assert _call([_table(**{hole: None})], VIS, 100) == ENULL, hole
        # a table without rows may have any pointers
        assert _call([_table(rows=0, **{hole: None})]) == OK, hole


def test_nothing_to_do_returns_ok():
    assert _call([], num_tables=0) == OK and _call([], num_tables=0, null_tables=True) == OK
    empty = _table(rows=0, param=None, grad=None, exp_avg=None, exp_avg_sq=None)
    assert _call([empty]) == OK and _call([empty] * 24) == OK
    assert _call([empty], VIS, 100) == OK and _call([empty], VIS, 0) == OK


def test_expon_lr():
    from latentsplat_amd import expon_lr
    a, b, S = 1.6e-4, 1.6e-6, 30_000
    assert expon_lr(0, a, b, S) == a and expon_lr(S, a, b, S) == b                     # the endpoints, exactly
    assert math.isclose(expon_lr(S // 2, a, b, S), math.sqrt(a * b), rel_tol=1e-12)    # the geometric mean
    assert expon_lr(S + 1, a, b, S) == b and expon_lr(10 * S, a, b, S) == b            # constant beyond
    assert expon_lr(-1, a, b, S) == 0.0 and expon_lr(5, 0.0, 0.0, S) == 0.0
    assert [expon_lr(s, a, b, S) for s in range(0, S + 1, 1000)] == sorted((expon_lr(s, a, b, S) for s in range(0, S + 1, 1000)), reverse=True)
    # the delay: delay_mult x lr_init at step 0, the plain schedule from delay_steps on, a quarter sine between
    assert expon_lr(0, a, b, S, delay_steps=100, delay_mult=0.01) == 0.01 * a
    assert expon_lr(100, a, b, S, 100, 0.01) == expon_lr(100, a, b, S) and expon_lr(5000, a, b, S, 100, 0.01) == expon_lr(5000, a, b, S)
    want = (0.01 + 0.99 * math.sin(0.5 * math.pi * 0.5)) * math.exp((1 - 50 / S) * math.log(a) + 50 / S * math.log(b))
    assert math.isclose(expon_lr(50, a, b, S, 100, 0.01), want, rel_tol=1e-12)


def test_adam_scalars_fold_the_step_count():
    from latentsplat_amd.optim import adam_scalars
    b1, b2 = 0.9, 0.999
    for t in (1, 2, 10, 1000):
        step_size, inv = adam_scalars(1e-3, (0.9, 0.999), t)
        assert math.isclose(step_size, 1e-3 / (1 - b1 ** t), rel_tol=1e-15) and math.isclose(inv, 1 / math.sqrt(1 - b2 ** t), rel_tol=1e-15)
        assert ref.scalars(1e-3, (0.9, 0.999), 1e-15, t)[5:] == (float(np.float32(step_size)), float(np.float32(inv)))
    assert ref.scalars(1e-3, (0.9, 0.999), 1e-15, 1)[2:4] == (float(np.float32(0.1)), float(np.float32(1 - 0.999)))
    assert float(np.float32(1 - 0.999)) != 1.0 - float(np.float32(0.999))          # why the table carries 1 - beta
    assert adam_scalars(1e-3, (0.9, 0.999), 7, bias_correction=False) == (1e-3, 1.0)
    with pytest.raises(_lib.LsrError, match="starts at 1"):
        adam_scalars(1e-3, (0.9, 0.999), 0)


def test_reference_is_adam():
    """tests/adam_ref.py against torch.optim.Adam in float64 on the CPU (betas that float32 holds exactly, so that the
    two mean the same recurrences), and its mask."""
    rng = np.random.default_rng(0)
    shape, T = (37, 5), 4
    hyper = dict(lr=0.01, betas=(0.5, 0.75), eps=1e-15)
    p0 = rng.normal(size=shape).astype(np.float32)
    grads = [ref.draw_grad(rng, shape) for _ in range(T)]
    r = ref.run(p0, grads, hyper)
    p = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.Adam([p], **hyper)
    for g in grads:
        p.grad = torch.from_numpy(g).double()
        opt.step()
    # (the reference's lr, eps and corrections are rounded to float32: 2^-24 of an update)
    assert np.allclose(r["p"], p.detach().numpy(), rtol=0, atol=2e-7 * hyper["lr"] * T)
    assert np.allclose(r["m"], opt.state[p]["exp_avg"].numpy(), rtol=1e-14) and np.allclose(r["v"], opt.state[p]["exp_avg_sq"].numpy(), rtol=1e-14)
    masks = [rng.uniform(size=shape[0]) < 0.5 for _ in range(T)]
    masks[0][3] = masks[1][3] = masks[2][3] = masks[3][3] = False
    s = ref.run(p0, grads, hyper, masks=masks)
    assert np.array_equal(s["p"][3], p0[3].astype(np.float64)) and not s["m"][3].any() and not s["v"][3].any()
    always = np.all(masks, axis=0)
    assert always.any() and np.array_equal(s["p"][always], r["p"][always]) and (r["bound_p"] > 0).all()


def _cpu_tables():
    z = lambda: torch.zeros(4, 3)
    return [dict(param=z(), grad=z(), exp_avg=z(), exp_avg_sq=z(), lr=1e-3, betas=(0.9, 0.999), eps=1e-15, step=1, bias_correction=True)]


def test_refuses_cpu_tensors():
    from latentsplat_amd import SceneAdam, adam_step
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        adam_step(_cpu_tables())
    p = torch.nn.Parameter(torch.zeros(4, 3))
    opt = SceneAdam([p], lr=1e-3)
    opt.step()                                       # no gradient: nothing to do
    assert len(opt.state) == 0
    p.grad = torch.ones(4, 3)
    with pytest.raises(_lib.LsrError, match="no CPU fallback"):
        opt.step()
    assert not p.detach().any()


def test_refuses_what_it_does_not_implement():
    from latentsplat_amd import SceneAdam
    p = torch.nn.Parameter(torch.zeros(4, 3))
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(_lib.LsrError, match=next(iter(kw))):
            SceneAdam([p], lr=1e-3, **kw)
    with pytest.raises(TypeError):
        SceneAdam([p], lr=1e-3, fused=True)
    opt = SceneAdam([dict(params=[p], lr=0.5, name="_xyz")], lr=0.0, bias_correction=False)
    g = opt.param_groups[0]
    assert g["eps"] == 1e-15 and g["betas"] == (0.9, 0.999) and g["bias_correction"] is False and g["lr"] == 0.5
    assert SceneAdam([p]).param_groups[0]["bias_correction"] is True
    opt.set_lr("_xyz", 0.25)
    assert g["lr"] == 0.25
    with pytest.raises(KeyError):
        opt.set_lr("_nope", 1.0)
    # a group that was switched on behind the constructor's back is refused at the step
    p.grad = torch.ones(4, 3)
    g["weight_decay"] = 0.1
    with pytest.raises(_lib.LsrError, match="weight_decay"):
        opt.step()
    # a stock Adam's state_dict loads (it has no bias_correction key) and the other way round
    stock = torch.optim.Adam([dict(params=[p], lr=0.5, name="_xyz")], lr=0.0, eps=1e-15)
    fused = SceneAdam([dict(params=[p], lr=0.1, name="_xyz")], lr=0.0)
    fused.load_state_dict(stock.state_dict())
    assert fused.param_groups[0]["lr"] == 0.5 and fused.param_groups[0]["bias_correction"] is True
    stock.load_state_dict(fused.state_dict())


def test_visible_from_radii():
    from latentsplat_amd import visible_from_radii
    radii = torch.tensor([[0, 3, 0, -1], [0, 0, 2, 0]], dtype=torch.int32)
    assert visible_from_radii(radii).tolist() == [False, True, True, False]
    with pytest.raises(_lib.LsrError):
        visible_from_radii(radii[0])


def test_fit_tool_lists_the_new_flags():
    tool = os.path.join(ROOT, "tools", "fit_ply.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--optimizer", "torch", "fused", "sparse", "--lr-position-final", "--lr-position-max-steps"):
        assert flag in out, flag
    bad = subprocess.run([sys.executable, tool, "scene.ply", "--out", "x", "--optimizer", "sgd"], capture_output=True, text=True)
    assert bad.returncode != 0 and "--optimizer" in bad.stderr
