"""Float64 restatement of the pose gradient of a 3DGS scene's rigid parts (latentsplat_amd.pose, csrc/scene_pose.hip) for
tests/test_pose_grad_*.py.  It shares nothing with the generated generator table: the "3dgs" basis is restated in torch
(asserted equal to scene_export_ref.basis to 1e-14), T_l(R) comes from its DEFINITION  B_l(R d) = T_l(R) . B_l(d)  by least
squares as transform_ref.band_matrix does (the pseudo-inverse of B_l at fixed directions is a constant outside the graph,
B_l(R d) is differentiable in R), R = R(p / |p|), s = exp(l), and the full map

    x' = s R x + t,   sigma' = sigma + l,   q' = (+-p / |p|) (x) q,   c'_l = T_l(R) c_l

is written out, so torch.autograd of :func:`forward` is the yardstick for every pose gradient.  (The sign of q_R is the
forward's choice; the tests read it off the forward's output with :func:`quaternion_signs`.)

:func:`abs_terms` returns, per output component, the same sums with absolute values: what a float32 evaluation's rounding
scales with.  The generators it needs are this file's own (the Jacobian of T_l(exp(eps [e_a]x)) at 0 by autograd of the
least-squares definition), and the moved quantities enter by their own absolute sums: |A| |x|, |L(q_R)| |q|, |T_l| |c_l|.

The bound.  With u = 2^-24, |kernel - reference| <= C u sum|terms| per component, C counted from the kernel's arithmetic
along the longest chain, a colour term of axis x or y at degree 4:
    11   the forward's c'_l (band 4: (2 l + 3) u |T_l| |c_l|, transform_ref's bound)
     8   T_l of the forward is that of the float32 matrix's polar factor, R(p) rounded: an angle of ~2 u, times |J^4| <= 4
     6   the six FMAs of the pair's dot over the channels
     2   the generator entry rounded to float32, and the FMA into the axis accumulator
    15   the further pair FMAs of that axis (16 pairs at degree 4)
     2   the quaternion term's FMA and the position term's add
     6   the wave sum (four exchanges within a row of 16 lanes, two levels over the four rows)
     1   the sums in double (2^-53 each) and the conversions, with room
     1   the float32 result
    -- 52.  Every other chain is shorter (translation: 8; log-scale: 19; quaternion and position terms of w: under 30).
The quaternion gradient is a double-precision combination of G_w rounded once more: C + 1 on its own absolute sums."""
from __future__ import annotations

from math import isqrt

import numpy as np
import torch

from tests import scene_export_ref as sref

U = 2.0 ** -24
C_TWIST = 52
C_QUATERNION = C_TWIST + 1
_DIRS = torch.from_numpy(sref.unit_directions(300, 777))


def basis(d: torch.Tensor) -> torch.Tensor:
    """The "3dgs" colour basis of csrc/lsr_sh.h at directions d (N, 3) -> (N, 25), differentiable."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    C1 = 0.4886025119029199
    b = [0.28209479177387814 * torch.ones_like(x),
         -C1 * y, C1 * z, -C1 * x,
         1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.31539156525252005 * (2 * zz - xx - yy),
         -1.0925484305920792 * xz, 0.5462742152960396 * (xx - yy),
         -0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * xy * z,
         -0.4570457994644658 * y * (4 * zz - xx - yy), 0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy),
         -0.4570457994644658 * x * (4 * zz - xx - yy), 1.445305721320277 * z * (xx - yy),
         -0.5900435899266435 * x * (xx - 3 * yy),
         2.5033429417967046 * xy * (xx - yy), -1.7701307697799304 * yz * (3 * xx - yy),
         0.9461746957575601 * xy * (7 * zz - 1), -0.6690465435572892 * yz * (7 * zz - 3),
         0.10578554691520431 * (zz * (35 * zz - 30) + 3), -0.6690465435572892 * xz * (7 * zz - 3),
         0.47308734787878004 * (xx - yy) * (7 * zz - 1), -1.7701307697799304 * xz * (xx - 3 * yy),
         0.6258357354491761 * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(b, dim=-1)


assert float((basis(_DIRS) - torch.from_numpy(sref.basis(_DIRS.numpy()))).abs().max()) < 1e-14
_PINV = [torch.linalg.pinv(basis(_DIRS)[:, l * l:(l + 1) ** 2]) for l in range(5)]        # (n, N) each: constants


def band_matrix(l: int, R: torch.Tensor) -> torch.Tensor:
    """T_l(R), differentiable in R:  B_l(d) T^T = B_l(R d)  solved with the fixed pseudo-inverse."""
    return (_PINV[l] @ basis(_DIRS @ R.T)[:, l * l:(l + 1) ** 2]).T


def rest_matrix(degree: int, R: torch.Tensor) -> torch.Tensor:
    return torch.block_diag(*[band_matrix(l, R) for l in range(1, degree + 1)]) if degree else torch.zeros(0, 0, dtype=R.dtype)


def rotation(p: torch.Tensor) -> torch.Tensor:
    w, x, y, z = (p / p.norm()).unbind()
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)


def left_matrix(q: torch.Tensor) -> torch.Tensor:
    w, x, y, z = q.unbind()
    return torch.stack([w, -x, -y, -z, x, w, -z, y, y, z, w, -x, z, -y, x, w]).reshape(4, 4)


def _rows(idx, n: int, T: int):
    if idx is None:
        return [torch.arange(n)] + [torch.zeros(0, dtype=torch.long)] * (T - 1)
    idx = torch.as_tensor(idx).to(torch.long).cpu()
    return [torch.nonzero(idx == k)[:, 0] for k in range(T)]


def forward(xyz, rest, scaling, rot, p, t, ls, idx=None, signs=None):
    """The map on float64 tensors (n, 3), (n, K - 1, 3), (n, 3), (n, 4) with poses p (T, 4), t (T, 3), ls (T,) or None;
    rows whose idx is out of range pass through.  Differentiable in everything."""
    n, T, degree = xyz.shape[0], p.shape[0], isqrt(rest.shape[1] + 1) - 1
    outs = [xyz.clone(), rest.clone(), scaling.clone(), rot.clone()]
    for k, rows in enumerate(_rows(idx, n, T)):
        if not rows.numel():
            continue
        R = rotation(p[k])
        l = ls[k] if ls is not None else torch.zeros((), dtype=xyz.dtype)
        sign = 1.0 if signs is None else float(signs[k])
        outs[0] = outs[0].index_copy(0, rows, l.exp() * (xyz[rows] @ R.T) + t[k])
        if degree:
            outs[1] = outs[1].index_copy(0, rows, torch.einsum("ij,njc->nic", rest_matrix(degree, R), rest[rows]))
        outs[2] = outs[2].index_copy(0, rows, scaling[rows] + l)
        outs[3] = outs[3].index_copy(0, rows, rot[rows] @ left_matrix(sign * p[k] / p[k].norm()).T)
    return tuple(outs)


def quaternion_signs(rot_in, rot_out, p, idx=None) -> torch.Tensor:
    """+-1 per transform: whether the forward that produced ``rot_out`` multiplied by +p/|p| or by -p/|p|."""
    rot_in, rot_out, p = (torch.as_tensor(v).detach().cpu().to(torch.float64) for v in (rot_in, rot_out, p))
    signs = torch.ones(p.shape[0], dtype=torch.float64)
    for k, rows in enumerate(_rows(idx, rot_in.shape[0], p.shape[0])):
        if rows.numel():
            plus = rot_in[rows] @ left_matrix(p[k] / p[k].norm()).T
            signs[k] = 1.0 if float((plus * rot_out[rows]).sum()) >= 0 else -1.0
    return signs


def pose_grads(scene64, p, t, ls, idx, grads64, signs=None):
    """autograd of :func:`forward`: (dL/dp (T, 4), dL/dt (T, 3), dL/dl (T,) or None) for L = sum of <g, output> over the
    outputs whose upstream gradient in ``grads64`` (four entries, None allowed) is given."""
    p, t = p.clone().requires_grad_(True), t.clone().requires_grad_(True)
    ls = None if ls is None else ls.clone().requires_grad_(True)
    outs = forward(*scene64, p, t, ls, idx, signs)
    loss = sum((o * g).sum() for o, g in zip(outs, grads64) if g is not None)
    wanted = [p, t] + ([ls] if ls is not None else [])
    if not torch.is_tensor(loss) or not loss.requires_grad:
        got = [torch.zeros_like(w) for w in wanted]
    else:
        got = [torch.zeros_like(w) if g is None else g for w, g in zip(wanted, torch.autograd.grad(loss, wanted, allow_unused=True))]
    return got[0], got[1], (got[2] if ls is not None else None)


_GENERATORS = None


def generators():
    """J[a][l]: this file's own generators, the Jacobian of eps -> T_l(exp(eps [e_a]x)) at 0 by autograd."""
    global _GENERATORS
    if _GENERATORS is None:
        out = []
        for a in range(3):
            i, j = (a + 1) % 3, (a + 2) % 3

            def rot(eps):        # the rotation by eps about axis a: I + (cos eps - 1) E + sin eps S
                E = torch.zeros(3, 3, dtype=torch.float64)
                E[i, i], E[j, j] = 1.0, 1.0
                S = torch.zeros(3, 3, dtype=torch.float64)
                S[i, j], S[j, i] = -1.0, 1.0
                return torch.eye(3, dtype=torch.float64) + (torch.cos(eps) - 1.0) * E + torch.sin(eps) * S
            blocks = [torch.zeros(1, 1, dtype=torch.float64)]
            for l in range(1, 5):
                blocks.append(torch.autograd.functional.jacobian(lambda e: band_matrix(l, rot(e)), torch.zeros((), dtype=torch.float64)))
            out.append(blocks)
        _GENERATORS = out
    return _GENERATORS


def abs_terms(scene64, p, t, ls, idx, grads64):
    """Per component of (dL/dp, dL/dt, dL/dl): the sums of the gradient with every term replaced by its absolute value and
    every moved quantity by its own absolute sum."""
    xyz, rest, scaling, rot = scene64
    n, T, degree = xyz.shape[0], p.shape[0], isqrt(rest.shape[1] + 1) - 1
    gx, gc, gs, gq = grads64
    J = generators()
    aw, at, al = torch.zeros(T, 3, dtype=torch.float64), torch.zeros(T, 3, dtype=torch.float64), torch.zeros(T, dtype=torch.float64)
    for k, rows in enumerate(_rows(idx, n, T)):
        if not rows.numel():
            continue
        R = rotation(p[k])
        s = float(ls[k].exp()) if ls is not None else 1.0
        if gx is not None:
            y, g = xyz[rows].abs() @ (s * R).abs().T, gx[rows].abs()
            for a in range(3):
                b, c = (a + 1) % 3, (a + 2) % 3
                aw[k, a] += (y[:, b] * g[:, c] + y[:, c] * g[:, b]).sum()
            at[k] += g.sum(0)
            al[k] += (g * y).sum()
        if gs is not None:
            al[k] += gs[rows].abs().sum()
        if gq is not None:
            q, g = rot[rows].abs() @ left_matrix(p[k] / p[k].norm()).abs().T, gq[rows].abs()
            for a in range(3):
                b, c = (a + 1) % 3, (a + 2) % 3
                aw[k, a] += 0.5 * (q[:, 0] * g[:, 1 + a] + g[:, 0] * q[:, 1 + a] + q[:, 1 + b] * g[:, 1 + c] + q[:, 1 + c] * g[:, 1 + b]).sum()
        if gc is not None and degree:
            for l in range(1, degree + 1):
                sl = slice(l * l - 1, (l + 1) ** 2 - 1)
                moved = torch.einsum("ij,njc->nic", band_matrix(l, R).abs(), rest[rows][:, sl].abs())
                for a in range(3):
                    aw[k, a] += torch.einsum("nic,ij,njc->", gc[rows][:, sl].abs(), J[a][l].abs(), moved)
    ph = (p / p.norm(dim=1, keepdim=True)).abs()
    w, v = ph[:, 0], ph[:, 1:]
    ap = torch.zeros(T, 4, dtype=torch.float64)
    ap[:, 0] = (aw * v).sum(1)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ap[:, 1 + a] = w * aw[:, a] + aw[:, b] * v[:, c] + aw[:, c] * v[:, b]
    ap *= 2.0 / p.norm(dim=1, keepdim=True)
    return ap, at, (al if ls is not None else None)


def random_poses(T: int, seed: int, t_max: float = 10.0, with_scale: bool = True):
    """Seeded float32 poses: quaternions of norm 0.5..2, |t| <= t_max, log-scales in +-0.5 (or None)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(T, 4, generator=g)
    p = p / p.norm(dim=1, keepdim=True) * (0.5 + 1.5 * torch.rand(T, 1, generator=g))
    t = torch.randn(T, 3, generator=g)
    t = t / t.norm(dim=1, keepdim=True) * t_max * torch.rand(T, 1, generator=g)
    ls = (torch.rand(T, generator=g) - 0.5) if with_scale else None
    return p.float(), t.float(), (ls.float() if ls is not None else None)


def twist_to_quaternion(Gw: np.ndarray, p: np.ndarray) -> np.ndarray:
    """dL/dp = (2 / |p|) (0, G_w) (x) p / |p|, numpy, one pose."""
    n2 = float(p @ p)
    w, v = p[0], p[1:]
    return 2.0 / n2 * np.concatenate([[-Gw @ v], w * Gw + np.cross(Gw, v)])
