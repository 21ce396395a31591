"""Standalone activations on the native elementwise kernels (csrc/aux_ops.hip ``act_fwd_k`` /
``act_bwd_k``): the activations nothing upstream can absorb -- e.g. the LeakyReLU(0.2) after the
DCGAN discriminator's bias-only input conv, or a stock ``nn.LeakyReLU`` / ``nn.GELU`` that
:func:`~torchbooster_amd.nativize` finds after an op without an activation epilogue.  The
backward recomputes act'(x) from the saved input (the reference: ATen's ``leaky_relu`` /
``leaky_relu_backward`` kernels behind ``nn.LeakyReLU``, examples/img_gen/gan/gan.py:37-46).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from torchbooster_amd.ops._ext import native, use_native
from torchbooster_amd.ops.norm import ACT_CODES, act_ref

__all__ = ["activation", "leaky_relu", "LeakyReLU", "swiglu"]


class _ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, code, slope):
        ctx.save_for_backward(x)
        ctx.cfg = (code, slope)
        return native().act_fwd(x, code, slope)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        code, slope = ctx.cfg
        if torch.is_grad_enabled():  # double backward: differentiable recompute
            name = {v: k for k, v in ACT_CODES.items() if isinstance(k, str)}[code]
            with torch.enable_grad():
                xx = x.detach().requires_grad_(True)
                y = act_ref(xx, name, slope)
                (g,) = torch.autograd.grad(y, xx, dy, create_graph=True)
            return g, None, None
        return native().act_bwd(x, dy.to(x.dtype), code, slope), None, None


def activation(x: Tensor, act: str, slope: float = 0.01) -> Tensor:
    """``act`` in {"relu", "gelu", "silu", "leaky_relu"} on the native kernels (GPU, numel % 8 == 0)."""
    code = ACT_CODES[act]
    if use_native(x) and x.is_floating_point() and x.numel() % 8 == 0 and x.numel() > 0:
        return _ActFn.apply(x, code, float(slope))
    return act_ref(x, act, slope)


def leaky_relu(x: Tensor, negative_slope: float = 0.01) -> Tensor:
    return activation(x, "leaky_relu", negative_slope)


class LeakyReLU(nn.LeakyReLU):
    """``nn.LeakyReLU`` on the native kernels (``inplace`` is accepted and returns a new tensor)."""

    def forward(self, x: Tensor) -> Tensor:
        if use_native(x):
            return leaky_relu(x, self.negative_slope)
        return F.leaky_relu(x, self.negative_slope, self.inplace)


# --------------------------------------------------------------- SwiGLU gate
def _gate_rows(gu: Tensor) -> Tensor:
    """``gu`` ``[..., 2F]`` as the ``[M, 2F]`` rows csrc/swiglu.hip reads: unit column stride, 16-B aligned
    rows (a row-strided window of a wider tensor stays a view; anything else is copied, as in
    ``ops.attention.rope_packed``)."""
    rows = gu.reshape(-1, gu.shape[-1])
    es = rows.element_size()
    if (rows.stride(1) != 1 or rows.data_ptr() % 16
            or (rows.shape[0] > 1 and (rows.stride(0) < rows.shape[1] or rows.stride(0) * es % 16))):
        rows = rows.contiguous()
        if rows.data_ptr() % 16:
            rows = rows.clone()
    return rows


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        rows = _gate_rows(gu)
        ctx.save_for_backward(rows)  # the backward recomputes everything from gu
        ctx.shape = gu.shape
        return native().swiglu_fwd(rows).view(*gu.shape[:-1], gu.shape[-1] // 2)

    @staticmethod
    def backward(ctx, dy):
        (rows,) = ctx.saved_tensors
        if torch.is_grad_enabled():  # double backward: differentiable recompute
            with torch.enable_grad():
                xx = rows.detach().requires_grad_(True)
                F_ = xx.shape[-1] // 2
                y = F.silu(xx[..., :F_]) * xx[..., F_:]
                (g,) = torch.autograd.grad(y, xx, dy.reshape(y.shape).to(y.dtype), create_graph=True)
            return g.view(ctx.shape)
        d = dy.to(rows.dtype).reshape(rows.shape[0], rows.shape[1] // 2).contiguous()
        if d.data_ptr() % 16:
            d = d.clone()
        return native().swiglu_bwd(rows, d).view(ctx.shape)


def swiglu(gu: Tensor) -> Tensor:
    """``silu(gu[..., :F]) * gu[..., F:]`` for a packed ``gate | up`` tensor ``[..., 2F]`` -> ``[..., F]``: the
    gate of a Llama-style MLP whose two input projections are ONE ``Linear(dim, 2F)``.

    Native (csrc/swiglu.hip, one launch each way; the backward recomputes from ``gu``, the only thing
    saved) for CUDA bf16 / f32 with ``F % 8 == 0``; everything else is ``F.silu(a) * b`` under autograd."""
    if gu.shape[-1] % 2:
        raise ValueError(f"swiglu: the last dim must be even (gate | up), not {gu.shape[-1]}")
    Fh = gu.shape[-1] // 2
    if (use_native(gu) and gu.dtype in (torch.bfloat16, torch.float32) and Fh % 8 == 0 and gu.numel() > 0
            and not torch.is_autocast_enabled("cuda")):
        return _SwiGLUFn.apply(gu)
    return F.silu(gu[..., :Fh]) * gu[..., Fh:]
