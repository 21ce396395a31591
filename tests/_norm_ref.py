"""Plain references for the BatchNorm / GroupNorm / InstanceNorm kernels (csrc/norm_bn.hip).

Pure torch, written from the formulas (no ``F.batch_norm`` / ``F.group_norm``), differentiable
through autograd, and dtype-generic: called on float64 tensors it is the reference, called on
float32 tensors it is the "stock" evaluation (mean subtracted first) the f32 kernels are measured
against.  ``tests/test_norm_ref.py`` validates it against the stock functions in float64 on the CPU.

Layout: ``x`` is ``[N, C, *spatial]`` (or ``[M, C]``), channels at dim 1, any strides.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor

from torchbooster_amd.ops.norm import act_ref

U_BF16 = 2.0 ** -9   # unit roundoff of bf16 (8 significand bits)
U_F16 = 2.0 ** -12   # unit roundoff of f16 (11 significand bits)
U_F32 = 2.0 ** -24


class BNOut(NamedTuple):
    y: Tensor
    mean: Tensor             # [C] the mean the normalisation used (batch mean, or running mean in eval)
    var: Tensor              # [C] biased variance used (batch variance, or running variance in eval)
    running_mean: Optional[Tensor]  # new running mean (None without running stats / in eval: unchanged)
    running_var: Optional[Tensor]   # new running variance (unbiased batch variance mixed in)
    z: Tensor                # pre-activation
    scale: Tensor            # [C]  w * invstd
    shift: Tensor            # [C]  b - mean * scale
    invstd: Tensor           # [C]


class GNOut(NamedTuple):
    y: Tensor
    mean: Tensor    # [N, G]
    var: Tensor     # [N, G] biased
    z: Tensor
    scale: Tensor   # [N, C]
    shift: Tensor   # [N, C]
    invstd: Tensor  # [N, G]


def _bshape(x: Tensor):
    return [1, -1] + [1] * (x.dim() - 2)


def bn_ref(x: Tensor, w: Optional[Tensor], b: Optional[Tensor], res: Optional[Tensor], act: str, slope: float,
           eps: float, training: bool, rm: Optional[Tensor], rv: Optional[Tensor], momentum: float = 0.1) -> BNOut:
    """``act(batch_norm(x) + res)`` in the dtype of ``x``; every other tensor must have that dtype."""
    C = x.shape[1]
    dims = [0] + list(range(2, x.dim()))
    M = x.numel() // C
    bs = _bshape(x)
    new_rm = new_rv = None
    if training:
        mean = x.mean(dim=dims)
        xc = x - mean.view(bs)
        var = (xc * xc).mean(dim=dims)
        if rm is not None:
            unb = var * (M / (M - 1)) if M > 1 else var
            new_rm = ((1.0 - momentum) * rm + momentum * mean).detach()
            new_rv = ((1.0 - momentum) * rv + momentum * unb).detach()
    else:
        mean, var = rm, rv
        xc = x - mean.view(bs)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = invstd if w is None else w * invstd
    shift = -mean * scale if b is None else b - mean * scale
    z = xc * scale.view(bs)
    if b is not None:
        z = z + b.view(bs)
    if res is not None:
        z = z + res
    return BNOut(act_ref(z, act, slope), mean, var, new_rm, new_rv, z, scale, shift, invstd)


def gn_ref(x: Tensor, groups: int, w: Optional[Tensor], b: Optional[Tensor], res: Optional[Tensor], act: str,
           slope: float, eps: float) -> GNOut:
    """``act(group_norm(x) + res)``; InstanceNorm is ``groups == C``."""
    N, C = x.shape[0], x.shape[1]
    bs = _bshape(x)
    xg = x.reshape(N, groups, -1)
    mean = xg.mean(dim=2)
    xc = xg - mean.unsqueeze(2)
    var = (xc * xc).mean(dim=2)
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = (xc * invstd.unsqueeze(2)).reshape(x.shape)
    Cg = C // groups
    scale = invstd.repeat_interleave(Cg, dim=1)  # [N, C]
    mean_c = mean.repeat_interleave(Cg, dim=1)
    if w is not None:
        scale = scale * w.view(1, C)
    shift = -mean_c * scale if b is None else b.view(1, C) - mean_c * scale
    z = xh if w is None else xh * w.view(bs)
    if b is not None:
        z = z + b.view(bs)
    if res is not None:
        z = z + res
    return GNOut(act_ref(z, act, slope), mean, var, z, scale, shift, invstd)


# ------------------------------------------------------------------ block views and metrics
def chan_blocks(t: Tensor) -> Tensor:
    """[N, C, *] -> [C, M]: one block per channel (BatchNorm)."""
    C = t.shape[1]
    return t.movedim(1, 0).reshape(C, -1)


def group_blocks(t: Tensor, groups: int) -> Tensor:
    """[N, C, *] -> [N * G, Cg * HW]: one block per (sample, group) (GroupNorm)."""
    N = t.shape[0]
    return t.reshape(N * groups, -1)


def block_err(a: Tensor, ref: Tensor, blocks, keep: Optional[Tensor] = None) -> Tensor:
    """Relative L2 error of ``a`` against ``ref`` per block (f64); ``blocks`` maps a tensor to
    [blocks, elements].  ``keep`` (bool, like ``ref``) drops elements from both norms.  A block whose
    reference is exactly zero reports the absolute L2 error."""
    a, ref = a.detach().double(), ref.detach().double()
    d = a - ref
    if keep is not None:
        d, ref = d * keep, ref * keep
    dn, rn = blocks(d).norm(dim=1), blocks(ref).norm(dim=1)
    return torch.where(rn > 0, dn / rn.clamp_min(1e-300), dn)


def vec_err(a: Tensor, ref: Tensor):
    """(relative L2 over the vector, elementwise relative maximum) for per-channel vectors."""
    a, ref = a.detach().double().reshape(-1), ref.detach().double().reshape(-1)
    d = (a - ref).abs()
    l2 = (d.norm() / ref.norm().clamp_min(1e-300)).item()
    el = torch.where(ref != 0, d / ref.abs().clamp_min(1e-300), d).max().item()
    return l2, el


def _bcast(v: Tensor, x: Tensor) -> Tensor:
    """per-channel [C] or per-(sample, channel) [N, C] coefficients broadcast over ``x``"""
    if v.dim() == 1:
        return v.view(_bshape(x)).expand_as(x)
    return v.view(list(v.shape) + [1] * (x.dim() - 2)).expand_as(x)


def cond_terms(x: Tensor, scale: Tensor, shift: Tensor, res: Optional[Tensor]):
    """The three addends of the kernels' affine form  z = x * scale + shift (+ res), elementwise."""
    xs = x * _bcast(scale, x)
    sh = _bcast(shift, x)
    return xs, sh, res


def kappa(x: Tensor, scale: Tensor, shift: Tensor, res: Optional[Tensor], z: Tensor, blocks) -> Tensor:
    """Condition factor of the affine form per block:
    (||x * scale|| + ||shift|| + ||res||) / ||z||  (for a channel ||shift|| = |shift_c| sqrt(M))."""
    xs, sh, r = cond_terms(x.detach().double(), scale.detach().double(), shift.detach().double(),
                           None if res is None else res.detach().double())
    num = blocks(xs).norm(dim=1) + blocks(sh).norm(dim=1)
    if r is not None:
        num = num + blocks(r).norm(dim=1)
    return num / blocks(z.detach().double()).norm(dim=1).clamp_min(1e-300)


def kink_mask(x: Tensor, scale: Tensor, shift: Tensor, res: Optional[Tensor], z: Tensor, tol: float = 1e-4) -> Tensor:
    """Elements so close to the ReLU / leaky-ReLU kink that f32 arithmetic may land on the other
    side:  |z| < tol * (|x * scale| + |shift| + |res|)."""
    xs, sh, r = cond_terms(x.detach().double(), scale.detach().double(), shift.detach().double(),
                           None if res is None else res.detach().double())
    mag = xs.abs() + sh.abs()
    if r is not None:
        mag = mag + r.abs()
    return z.detach().double().abs() < tol * mag
