"""Fused multi-head attention on the native flash-style MFMA kernels (csrc/attention.hip).

Not in the reference (no attention model): K26 of SURVEY.md
§2.3.1, for the ViT-B/16 north-star configuration.

* :func:`attention_packed` takes the packed ``[B, N, 3*H*D]`` output of a QKV
  projection and returns ``[B, N, H*D]`` — the layout the output projection
  reads — with no permute/contiguous copies in either direction: the kernels
  read q/k/v through strides and the backward writes dq/dk/dv straight into one
  packed ``dqkv`` buffer.
* :func:`attention` takes ``[B, H, N, D]`` q, k, v (any strides).

Native path: CUDA bf16 tensors with head dim 64.  Everything else (CPU, other
dtypes/head dims, ``TBAMD_FORCE_REFERENCE=1`` comparator runs) takes stock
``F.scaled_dot_product_attention``; :func:`attention_ref` is the explicit fp32
math the GPU tests compare against.

Masks (self-attention, both optional and combinable, the same on every path):

* ``causal=True``: query ``i`` attends to keys ``j <= i``;
* ``key_lengths``: an int32 ``[B]`` tensor on the inputs' device; in batch ``b`` keys
  ``j >= key_lengths[b]`` are hidden from every query (the ``key_padding_mask`` meaning).
  Queries at padded positions are computed like any other: the caller masks their loss.
  Each length is CLAMPED into ``[1, N]`` -- 0 behaves as 1 and anything above ``N`` as ``N`` --
  so no row is ever fully masked and no NaN path exists.  The native kernels read the lengths
  from device memory: no host sync, safe inside a graph capture, and a replay follows in-place
  changes of the tensor.

With both, query ``i`` of batch ``b`` sees keys ``j < min(key_lengths[b], i + 1)``.  The native
kernels skip the key tiles no query of a workgroup sees instead of masking them; gradients of
hidden keys are zeros.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd.function import once_differentiable

from torchbooster_amd.ops._ext import native, use_native

__all__ = ["attention", "attention_packed", "attention_ref", "native_supported"]


def _visible(N: int, device, causal: bool, key_lengths: Optional[Tensor]) -> Optional[Tensor]:
    """The boolean mask (True = attend) of the two masks, broadcastable to [B, H, N, N]; None = dense."""
    m = None
    if key_lengths is not None:
        kl = key_lengths.to(device=device, dtype=torch.int64).clamp(1, N)  # the kernels' clamp
        m = (torch.arange(N, device=device)[None, :] < kl[:, None])[:, None, None, :]
    if causal:
        c = torch.ones(N, N, dtype=torch.bool, device=device).tril()
        m = c if m is None else m & c
    return m


def attention_ref(q: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None, *, causal: bool = False,
                  key_lengths: Optional[Tensor] = None) -> Tensor:
    """softmax(q kᵀ · scale) v over [..., N, D] tensors (f32 softmax); with a mask, over
    [B, H, N, D] (the fp32 oracle of the masked kernels when given fp32 inputs)."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    m = _visible(q.shape[-2], q.device, causal, key_lengths)
    if m is not None:
        s = s.masked_fill(~m, float("-inf"))
    p = torch.softmax(s.float(), dim=-1).to(q.dtype)
    return torch.matmul(p, v)


def _check_lengths(key_lengths: Optional[Tensor], B: int, like: Tensor) -> None:
    if key_lengths is None:
        return
    if key_lengths.dtype != torch.int32 or key_lengths.shape != (B,) or key_lengths.device != like.device:
        raise ValueError("key_lengths must be an int32 tensor of shape [B] on the device of the inputs")


def _sdpa(q: Tensor, k: Tensor, v: Tensor, scale: float, causal: bool, key_lengths: Optional[Tensor]) -> Tensor:
    """Stock PyTorch (the comparator of --mode stock benchmarks; CPU path), same mask semantics."""
    m = _visible(q.shape[-2], q.device, causal, key_lengths)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=m, scale=scale)


def native_supported(q: Tensor) -> bool:
    return q.is_cuda and q.dtype == torch.bfloat16 and q.shape[-1] == 64 and use_native(q)


class _AttnFn(torch.autograd.Function):
    """q, k, v: [B, H, N, 64] views -> o [B, N, H, 64] (contiguous)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal=False, key_lengths=None):
        o, lse = native().attn_forward(q, k, v, scale, causal, key_lengths)
        ctx.save_for_backward(q, k, v, o, lse, key_lengths)
        ctx.scale, ctx.causal = scale, causal
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, do):
        q, k, v, o, lse, key_lengths = ctx.saved_tensors
        do = do.contiguous()
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        dk = torch.empty(k.shape, dtype=k.dtype, device=k.device)
        dv = torch.empty(v.shape, dtype=v.dtype, device=v.device)
        native().attn_backward(q, k, v, o.permute(0, 2, 1, 3), do.permute(0, 2, 1, 3), lse, ctx.scale, dq, dk, dv,
                               ctx.causal, key_lengths)
        return dq, dk, dv, None, None, None


class _AttnPackedFn(torch.autograd.Function):
    """qkv: [B, N, 3*H*64] -> [B, N, H*64]; the gradient is one packed buffer."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, causal=False, key_lengths=None):
        B, N, E3 = qkv.shape
        D = E3 // (3 * heads)
        t = qkv.view(B, N, 3, heads, D)
        q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
        o, lse = native().attn_forward(q, k, v, scale, causal, key_lengths)
        ctx.save_for_backward(qkv, o, lse, key_lengths)
        ctx.cfg = (heads, D, scale, causal)
        return o.view(B, N, heads * D)

    @staticmethod
    @once_differentiable
    def backward(ctx, do):
        qkv, o, lse, key_lengths = ctx.saved_tensors
        heads, D, scale, causal = ctx.cfg
        B, N, _ = qkv.shape
        t = qkv.view(B, N, 3, heads, D)
        dqkv = torch.empty_like(qkv)
        g = dqkv.view(B, N, 3, heads, D)
        do = do.contiguous().view(B, N, heads, D)
        native().attn_backward(t[:, :, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2), t[:, :, 2].transpose(1, 2),
                               o.permute(0, 2, 1, 3), do.permute(0, 2, 1, 3), lse, scale,
                               g[:, :, 0].transpose(1, 2), g[:, :, 1].transpose(1, 2), g[:, :, 2].transpose(1, 2),
                               causal, key_lengths)
        return dqkv, None, None, None, None


def _rows_ok(t: Tensor) -> bool:
    return t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0


def attention(q: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None, *, causal: bool = False,
              key_lengths: Optional[Tensor] = None) -> Tensor:
    """[B, H, N, D] -> [B, H, N, D].  ``causal`` / ``key_lengths``: the masks of the module docstring
    (self-attention: q, k, v of one shape; lengths clamped into [1, N])."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else float(scale)
    if (causal or key_lengths is not None) and not (q.dim() == 4 and q.shape == k.shape == v.shape):
        raise ValueError("attention masks need [B, H, N, D] self-attention inputs of one shape")
    _check_lengths(key_lengths, q.shape[0], q)
    if native_supported(q) and q.dim() == 4 and q.shape == k.shape == v.shape:
        q, k, v = (x if _rows_ok(x) else x.contiguous() for x in (q, k, v))
        return _AttnFn.apply(q, k, v, scale, bool(causal), key_lengths).permute(0, 2, 1, 3)
    return _sdpa(q, k, v, scale, causal, key_lengths)


def attention_packed(qkv: Tensor, heads: int, scale: Optional[float] = None, *, causal: bool = False,
                     key_lengths: Optional[Tensor] = None) -> Tensor:
    """[B, N, 3*H*D] packed q|k|v (head-major inside each) -> [B, N, H*D]; masks as :func:`attention`."""
    B, N, E3 = qkv.shape
    D = E3 // (3 * heads)
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    _check_lengths(key_lengths, B, qkv)
    if native_supported(qkv.view(B, N, 3, heads, D)) and _rows_ok(qkv):
        return _AttnPackedFn.apply(qkv, heads, scale, bool(causal), key_lengths)
    t = qkv.view(B, N, 3, heads, D).permute(2, 0, 3, 1, 4)
    o = _sdpa(t[0], t[1], t[2], scale, causal, key_lengths)
    return o.transpose(1, 2).reshape(B, N, heads * D)
