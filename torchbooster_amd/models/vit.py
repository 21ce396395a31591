"""Vision Transformer (ViT-B/16 and friends) — BASELINE.json config 5.

Not part of the reference (it has no attention model); built
for the north-star "ViT-B/16 224px bf16 DDP via torchbooster.lmdb + cosine
scheduler" configuration.  Pre-norm blocks; the residual add of each sub-block
is fused into the following LayerNorm kernel (``LayerNorm(x, residual)``
returns both the normalised tensor and the updated residual stream), patch
embedding is a 16x16/s16 conv (a GEMM over non-overlapping patches).
Attention is the native flash-style MFMA kernel (ops/attention.py,
csrc/attention.hip) reading the packed QKV projection output through strides
and writing the packed dQKV gradient; no Triton / aotriton kernels are used.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from torchbooster_amd.ops.attention import (attention_decode_packed, attention_extend_packed, attention_packed,
                                            kv_cache_append, rope_packed, rope_table)
from torchbooster_amd.ops.conv import Conv2d

from torchbooster_amd.ops.act import swiglu
from torchbooster_amd.ops.norm import LayerNorm, RMSNorm
from torchbooster_amd.ops.linear import GeluLink, Linear, LinearGELU, linear, linear_rows

__all__ = ["ViT", "vit_b_16", "vit_s_16", "vit_tiny", "Attention", "Block", "Rope", "SwiGLU"]


class Rope:
    """The rotary position embedding of one model: ``(max_len, head_dim, base)`` and the table of
    ``ops.attention.rope_table`` per (device, dtype), built on first use and shared by every
    :class:`Attention` that holds this object.

    Neither a parameter nor a buffer: ``model.to(torch.bfloat16)`` does not round it and ``.cuda()`` does
    not have to move it -- ``table(like)`` follows the device of ``like`` and is float32, or float64 for
    float64 activations.  A copy (``copy.deepcopy``, pickling) carries the three numbers and rebuilds its
    tables.  The device copy is a host-built tensor, so its first use must lie outside a graph capture
    (``TransformerLM.prefill`` and the eager step ahead of ``generate(graph=True)`` both see to that)."""

    def __init__(self, max_len: int, head_dim: int, base: float = 10000.0) -> None:
        if head_dim < 2 or head_dim % 2:
            raise ValueError(f"rotary embeddings need an even head dim, not {head_dim}")
        self.max_len, self.head_dim, self.base = int(max_len), int(head_dim), float(base)
        self._tables = {}

    def table(self, like: Tensor) -> Tensor:
        """``[max_len, 2, head_dim // 2]`` on the device of ``like``."""
        dtype = torch.float64 if like.dtype == torch.float64 else torch.float32
        key = (like.device, dtype)
        t = self._tables.get(key)
        if t is None:
            if like.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the rotary table must exist before a graph capture begins: run one eager "
                                   "step first")
            t = self._tables[key] = rope_table(self.max_len, self.head_dim, self.base, device=like.device,
                                               dtype=dtype)
        return t

    def __getstate__(self):
        return {"max_len": self.max_len, "head_dim": self.head_dim, "base": self.base}

    def __setstate__(self, state) -> None:
        self.__dict__.update(state)
        self._tables = {}


def ln_args(norm: LayerNorm):
    """The ``ln=(weight, bias, eps)`` prologue of ``ops.linear.linear_rows`` for a LayerNorm module."""
    return norm.weight, norm.bias, norm.eps


def norm_args(norm):
    """The norm prologue of ``ops.linear.linear_rows`` for a norm module, as keyword arguments:
    ``ln=(weight, bias, eps)`` for a LayerNorm, ``rms=(weight, eps)`` for an RMSNorm."""
    if isinstance(norm, RMSNorm):
        return {"rms": (norm.weight, norm.eps)}
    return {"ln": ln_args(norm)}


def make_norm(kind: str, dim: int):
    """The block norm ``kind`` names: ``"layer"`` (LayerNorm) or ``"rms"`` (RMSNorm), eps 1e-6."""
    if kind == "layer":
        return LayerNorm(dim, eps=1e-6)
    if kind == "rms":
        return RMSNorm(dim, eps=1e-6)
    raise ValueError(f"norm must be 'layer' or 'rms', not {kind!r}")


class Attention(nn.Module):
    """``causal``: query i attends to keys j <= i; ``key_lengths`` (int32 [B], clamped into [1, N]):
    the keys of batch b at or past its length are hidden (ops/attention.py).

    Incremental decoding (causal only, forward only; ``cached`` holds all of it): with ``cache=(k_cache, v_cache)``, each
    ``[B, H, cap, hd]``, and ``positions`` (int32 [B], the row each sequence writes next), an ``x`` of
    ``[B, 1, dim]`` is one decode step -- its k / v are appended at ``positions`` and the query attends to
    the cache rows ``j <= positions[b]`` -- and an ``x`` of ``[B, N > 1, dim]`` is a prefill: the masked
    self-attention as without a cache, plus one append of the same k / v at ``positions``.  With
    ``extend=True`` an ``x`` of any ``[B, T >= 1, dim]`` is T new tokens on top of what the cache holds:
    their k / v are appended at ``positions[b] + t`` and query ``t`` attends to the cache rows
    ``j <= positions[b] + t`` (``attention_extend_packed``; ``key_lengths`` is not used).

    ``kv_heads`` (grouped-query attention, ops/attention.py): ``heads`` query heads share ``kv_heads``
    key / value heads, query head ``h`` reading kv head ``h // (heads // kv_heads)``.  The projection is
    ``Linear(dim, (heads + 2 * kv_heads) * hd)`` and a cache ``[B, kv_heads, cap, hd]``.  ``None`` is
    ``heads``: plain multi-head attention, the same parameters and the same calls as without it.
    ``bias=False``: ``qkv`` and ``proj`` without biases.

    ``rope`` (a :class:`Rope`; ``None``: nothing changes): the q and k parts of the packed projection are
    rotated right behind ``self.qkv`` (``ops.attention.rope_packed``), so every path below reads rotated
    q / k and a cache holds rotated keys.  Token ``t`` is at position ``t`` without a cache and in a
    prefill, at ``positions[b] + t`` in a decode step and an extend; the cached paths rotate in place.

    ``window`` (an int >= 1, needs ``causal``; ``None``: nothing changes): sliding-window attention
    (ops/attention.py) -- a token sees itself and the ``window - 1`` tokens before it -- passed to every
    attention call below: training, prefill, decode step (``fused`` or not) and extend.

    ``rolling`` (an argument of ``forward`` / ``cached``, not of the layer: it belongs to the cache; needs
    ``window``): ``cache`` is a rolling pair ``[B, kv_heads, R, hd]`` (ops/attention.py) -- the decode step and
    the extend pass ``rolling=True`` on, and the prefill's append becomes the ring append with
    ``lengths=key_lengths``, which keeps the last ``R`` valid rows of each sequence.

    ``kv_scales`` (likewise an argument of ``forward`` / ``cached``: the ``(k_scale, v_scale)`` of an fp8 cache
    pair, ops/attention.py; ``None``: nothing is added to any call): passed to the append of a prefill and to
    the decode step and the extend.  A prefill's own attention reads its unquantised ``qkv``."""

    def __init__(self, dim: int, heads: int, causal: bool = False, kv_heads: Optional[int] = None,
                 rope: Optional[Rope] = None, bias: bool = True, window: Optional[int] = None) -> None:
        super().__init__()
        if window is not None:
            if isinstance(window, bool) or not isinstance(window, int) or window < 1:
                raise ValueError(f"window must be None or an int >= 1, not {window!r}")
            if not causal:
                raise ValueError("window needs causal attention")
        self.window = window
        if kv_heads is not None and (kv_heads < 1 or heads % kv_heads):
            raise ValueError(f"kv_heads {kv_heads} must divide heads {heads}")
        self.heads = heads
        self.kv_heads = heads if kv_heads is None else int(kv_heads)
        self.hd = dim // heads
        self.causal = causal
        if rope is not None and rope.head_dim != self.hd:
            raise ValueError(f"rope is for head dim {rope.head_dim}, this layer has {self.hd}")
        self.rope = rope
        self.qkv = Linear(dim, 3 * dim if kv_heads is None else (heads + 2 * self.kv_heads) * self.hd, bias=bias)
        self.proj = Linear(dim, dim, bias=bias)

    def _kw(self) -> dict:
        """``kv_heads`` / ``window`` where the layer has them: plain MHA without a window makes the calls it
        always made."""
        kw = {} if self.kv_heads == self.heads else {"kv_heads": self.kv_heads}
        if self.window is not None:
            kw["window"] = self.window
        return kw

    def rotate(self, qkv: Tensor, positions: Optional[Tensor] = None, inplace: bool = False) -> Tensor:
        """The packed projection with q and k rotated; ``qkv`` itself without ``rope``."""
        if self.rope is None:
            return qkv
        return rope_packed(qkv, self.heads, self.rope.table(qkv), positions, kv_heads=self.kv_heads, inplace=inplace)

    def forward(self, x: Tensor, key_lengths: Optional[Tensor] = None, *, cache=None,
                positions: Optional[Tensor] = None, extend: bool = False, rolling: bool = False,
                kv_scales=None) -> Tensor:
        if cache is not None:
            rkw = {"rolling": True} if rolling else {}  # a linear cache: the call it always made
            if kv_scales is not None:  # likewise a cache that is not fp8
                rkw["kv_scales"] = kv_scales
            return self.proj(self.cached(self.qkv(x), cache, positions, key_lengths, extend=extend, **rkw))
        kw = self._kw()
        return self.proj(attention_packed(self.rotate(self.qkv(x)), self.heads, 1.0 / math.sqrt(self.hd),
                                          causal=self.causal, key_lengths=key_lengths, **kw))

    def cached(self, qkv: Tensor, cache, positions: Optional[Tensor], key_lengths: Optional[Tensor] = None, *,
               extend: bool = False, fused: bool = False, rolling: bool = False, kv_scales=None) -> Tensor:
        """The cached paths of the class docstring on the packed projection ``qkv`` ``[B, T, (H + 2*Hkv)*hd]``
        (rotated here, in place) -> ``[B, T, H*hd]``, the input of ``proj``.  ``forward`` and
        ``Block.forward_rows`` both end here; ``fused`` folds the append of a decode step into its attention
        (``attention_decode_packed(fused=True)``)."""
        if not self.causal:
            raise ValueError("a KV cache needs causal attention")
        if positions is None:
            raise ValueError("a KV cache needs positions")
        if rolling and self.window is None:
            raise ValueError("a rolling cache needs a layer with a window")
        k_cache, v_cache = cache
        scale = 1.0 / math.sqrt(self.hd)
        kw = self._kw()
        skw = {} if kv_scales is None else {"kv_scales": kv_scales}  # not fp8: the calls it always made
        one = qkv.shape[1] == 1
        # a prefill's tokens sit at 0 .. N - 1 whatever row they are appended at, a step's at positions[b] + t
        qkv = self.rotate(qkv, positions if extend or one else None, inplace=True)
        if one or extend:
            if rolling:
                kw["rolling"] = True
            kw.update(skw)
            if one:  # attention_extend_packed would make this very call
                if fused:
                    return attention_decode_packed(qkv, self.heads, k_cache, v_cache, positions, scale, fused=True,
                                                   **kw)
                return attention_decode_packed(qkv, self.heads, k_cache, v_cache, positions, scale, **kw)
            return attention_extend_packed(qkv, self.heads, k_cache, v_cache, positions, scale, **kw)
        # a prefill: the masked self-attention never reads the cache; a ring keeps each sequence's last R valid rows
        kv_cache_append(k_cache, v_cache, qkv, self.heads, positions,
                        **({} if self.kv_heads == self.heads else {"kv_heads": self.kv_heads}),
                        **({"rolling": True, "lengths": key_lengths} if rolling else {}), **skw)
        return attention_packed(qkv, self.heads, scale, causal=True, key_lengths=key_lengths, **kw)

class MLP(nn.Module):
    def __init__(self, dim: int, hidden: int, bias: bool = True) -> None:
        super().__init__()
        self.fc1 = LinearGELU(dim, hidden, bias=bias)  # GELU fused into its backward / bias-grad pass
        self.fc2 = Linear(hidden, dim, bias=bias)

    def forward(self, x: Tensor) -> Tensor:
        # fc2 is the hidden activation's only consumer: its input gradient takes fc1's GELU
        # backward and bias gradient into the same GEMM epilogue (ops/linear.py GeluLink)
        link = GeluLink()
        return self.fc2(self.fc1(x, link), gelu_in=link)


class SwiGLU(nn.Module):
    """The gated SiLU MLP of Llama-style blocks: ``fc2(silu(gate) * up)`` with ``gate | up = fc1(x)``, the
    two input projections packed into ONE ``Linear(dim, 2 * hidden)`` (one GEMM; ``ops.act.swiglu``)."""

    def __init__(self, dim: int, hidden: int, bias: bool = True) -> None:
        super().__init__()
        self.fc1 = Linear(dim, 2 * hidden, bias=bias)
        self.fc2 = Linear(hidden, dim, bias=bias)

    def forward(self, x: Tensor) -> Tensor:
        return self.fc2(swiglu(self.fc1(x)))


class Block(nn.Module):
    """Pre-norm transformer block.  The defaults are the GPT-2 / ViT block: LayerNorm, a GELU MLP, biases.
    ``norm="rms"``: ``ln1`` / ``ln2`` are :class:`~torchbooster_amd.ops.norm.RMSNorm` (the attribute names
    stay: the ``(x, pending)`` protocol of ``forward`` is the same); ``mlp="swiglu"``: ``self.mlp`` is a
    :class:`SwiGLU` of hidden width ``int(dim * mlp_ratio)``; ``bias=False``: no bias in ``qkv``, ``proj`` and
    the MLP's linears -- together the Llama-style block.  ``window``: the sliding window of :class:`Attention`."""

    def __init__(self, dim: int, heads: int, mlp_ratio: float = 4.0, causal: bool = False,
                 kv_heads: Optional[int] = None, rope: Optional[Rope] = None, norm: str = "layer",
                 mlp: str = "gelu", bias: bool = True, window: Optional[int] = None) -> None:
        super().__init__()
        if mlp not in ("gelu", "swiglu"):
            raise ValueError(f"mlp must be 'gelu' or 'swiglu', not {mlp!r}")
        self.ln1 = make_norm(norm, dim)
        self.attn = Attention(dim, heads, causal, kv_heads, rope, bias=bias, window=window)
        self.ln2 = make_norm(norm, dim)
        hidden = int(dim * mlp_ratio)
        self.mlp = SwiGLU(dim, hidden, bias) if mlp == "swiglu" else MLP(dim, hidden, bias)

    def forward(self, x: Tensor, pending: Optional[Tensor] = None, key_lengths: Optional[Tensor] = None, *,
                cache=None, positions: Optional[Tensor] = None, extend: bool = False, rolling: bool = False,
                kv_scales=None):
        """``x``: residual stream; ``pending``: a sub-block output not yet added
        to it.  Returns (stream, pending) so adds fuse into the next LayerNorm.
        ``key_lengths``: per-batch key lengths for the attention (None: every key).
        ``cache`` / ``positions`` / ``extend`` / ``rolling`` / ``kv_scales``: this layer's KV cache, passed to
        :class:`Attention`."""
        if pending is None:
            h = self.ln1(x)
        else:
            h, x = self.ln1(x, pending)
        if kv_scales is not None:  # an fp8 cache
            a = self.attn(h, key_lengths, cache=cache, positions=positions, extend=extend,
                          **({"rolling": True} if rolling else {}), kv_scales=kv_scales)
        elif rolling:
            a = self.attn(h, key_lengths, cache=cache, positions=positions, extend=extend, rolling=True)
        else:
            a = self.attn(h, key_lengths, cache=cache, positions=positions, extend=extend)
        h, x = self.ln2(x, a)
        return x, self.mlp(h)

    def forward_rows(self, x: Tensor, *, cache, positions: Tensor, extend: bool = False,
                     rolling: bool = False, kv_scales=None) -> Tensor:
        """The decoding layer on the few-row kernels (ops/linear.py ``linear_rows``; causal, forward only):
        ``x`` ``[B, T, dim]`` is the residual stream itself -- there is no ``pending`` -- and so is the
        result.  Both norms (LayerNorm or RMSNorm) run as prologues of the product behind them, bias / GELU or
        SwiGLU / residual as epilogues, and the attention is ``Attention.cached(fused=True)``: with ``T == 1`` 5 launches with a
        single-chunk cache, 6 otherwise (one more with rotary positions: the rotation of ``qkv``).
        ``T > 1`` needs ``extend=True``.  Computes what ``forward`` computes with ``cache`` / ``positions`` /
        ``extend``, to rounding.  ``rolling``: ``cache`` is a rolling pair (:class:`Attention`);
        ``kv_scales``: it is an fp8 pair with these scales."""
        at = self.attn
        if x.shape[1] != 1 and not extend:
            raise ValueError("forward_rows: more than one token per sequence needs extend=True")
        qkv = linear_rows(x, at.qkv.weight, at.qkv.bias, **norm_args(self.ln1))
        a = at.cached(qkv, cache, positions, extend=extend, fused=True, **({"rolling": True} if rolling else {}),
                      **({} if kv_scales is None else {"kv_scales": kv_scales}))
        x = linear_rows(a, at.proj.weight, at.proj.bias, residual=x)
        act = "swiglu" if isinstance(self.mlp, SwiGLU) else "gelu"
        h = linear_rows(x, self.mlp.fc1.weight, self.mlp.fc1.bias, **norm_args(self.ln2), act=act)
        return linear_rows(h, self.mlp.fc2.weight, self.mlp.fc2.bias, residual=x)


class ViT(nn.Module):
    def __init__(self, image: int = 224, patch: int = 16, dim: int = 768, depth: int = 12, heads: int = 12,
                 mlp_ratio: float = 4.0, num_classes: int = 1000, in_ch: int = 3) -> None:
        super().__init__()
        self.patch = Conv2d(in_ch, dim, patch, patch)
        n = (image // patch) ** 2
        self.cls = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos = nn.Parameter(torch.zeros(1, n + 1, dim))
        self.blocks = nn.ModuleList([Block(dim, heads, mlp_ratio) for _ in range(depth)])
        self.norm = LayerNorm(dim, eps=1e-6)
        self.head = Linear(dim, num_classes)
        nn.init.trunc_normal_(self.pos, std=0.02)
        nn.init.trunc_normal_(self.cls, std=0.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def embed(self, x: Tensor) -> Tensor:
        """Patch embedding -> [B, N, D].  On the native path the non-overlapping
        16x16/s16 conv is one GEMM: a patchify copy ([B*N, C*p*p] rows in the
        conv weight's (c, kh, kw) order) and the native Linear (bias fused; its
        weight gradient is the split-K dW kernel)."""
        B, C, H, W = x.shape
        p = self.patch.kernel_size[0]
        w = self.patch.weight
        if x.is_cuda and x.dtype == torch.bfloat16 and (C * p * p) % 8 == 0 and H % p == 0 and W % p == 0:
            h, wn = H // p, W // p
            rows = x.reshape(B, C, h, p, wn, p).permute(0, 2, 4, 1, 3, 5).reshape(B * h * wn, C * p * p)
            y = linear(rows, w.reshape(w.shape[0], -1), self.patch.bias)
            return y.view(B, h * wn, -1)
        return self.patch(x).flatten(2).transpose(1, 2)

    def forward(self, x: Tensor) -> Tensor:
        x = self.embed(x)  # [B, N, D]
        x = torch.cat([self.cls.expand(x.shape[0], -1, -1).to(x.dtype), x], dim=1) + self.pos.to(x.dtype)
        pending = None
        for blk in self.blocks:
            x, pending = blk(x, pending)
        h, _ = self.norm(x, pending)
        return self.head(h[:, 0])


def vit_b_16(num_classes: int = 1000, image: int = 224) -> ViT:
    return ViT(image, 16, 768, 12, 12, 4.0, num_classes)


def vit_s_16(num_classes: int = 1000, image: int = 224) -> ViT:
    return ViT(image, 16, 384, 12, 6, 4.0, num_classes)


def vit_tiny(num_classes: int = 10, image: int = 32) -> ViT:
    return ViT(image, 4, 192, 4, 3, 4.0, num_classes)
