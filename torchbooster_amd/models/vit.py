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
                                            kv_cache_append, qk_norm_rope_packed, rope_packed, rope_table)
from torchbooster_amd.ops.conv import Conv2d

from torchbooster_amd.ops.act import swiglu
from torchbooster_amd.ops.gemm import grouped_linear
from torchbooster_amd.ops.norm import LayerNorm, RMSNorm
from torchbooster_amd.ops.linear import (MX_BLOCK, GeluLink, Linear, LinearGELU, linear, linear_mx, linear_rows,
                                         linear_rows_experts, moe_route_rows, mx_quantize)

__all__ = ["ViT", "vit_b_16", "vit_s_16", "vit_tiny", "Attention", "Block", "Rope", "SwiGLU", "MoE"]


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


def mx_snapshots(named, fmt: Optional[str]):
    """``{name: (codes, scales)}`` of the ``(name, linear)`` pairs whose ``in_features`` is a multiple of 32
    (``ops.linear.mx_quantize`` of the weight, on its device), or ``None`` for ``fmt=None``."""
    if fmt is None:
        return None
    if fmt != "mxfp4":
        raise ValueError(f"quantize_rows: fmt must be 'mxfp4' or None, not {fmt!r}")
    return {name: mx_quantize(lin.weight) for name, lin in named if lin.in_features % MX_BLOCK == 0}


def rows_weight(lin, mx):
    """The weight argument and the extra keywords of a ``linear_rows`` call on ``lin``: the parameter, or its
    MXFP4 snapshot ``mx = (codes, scales)``."""
    return (lin.weight, {}) if mx is None else (mx[0], {"mx_scales": mx[1]})


def snap_linear(lin, mx, name: str):
    """What multiplies by ``lin`` in a forward with the MXFP4 snapshots ``mx`` (``{name: (codes, scales)}`` or
    None): ``lin`` itself without a snapshot called ``name``, else ``ops.linear.linear_mx`` on the snapshot with
    ``lin``'s bias (keywords: its ``act=`` / ``residual=``)."""
    snap = (mx or {}).get(name)
    if snap is None:
        return lin
    return lambda x, **kw: linear_mx(x, snap[0], snap[1], lin.bias, **kw)


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
    the decode step and the extend.  A prefill's own attention reads its unquantised ``qkv``.

    ``qk_norm`` (``False``: nothing changes): an RMSNorm over every query and key head vector, with
    ``qk_eps``, ahead of the rotation -- ``q_norm`` / ``k_norm`` (:class:`~torchbooster_amd.ops.norm.RMSNorm`
    of the head dim) only hold the two weights, f32 under dtype casts and initialised to ones without an RNG
    draw.  It runs inside :meth:`rotate` (``ops.attention.qk_norm_rope_packed``: one launch for norm and
    rotation, the norm alone without ``rope``), hence on every path, and a cache holds normalised keys.

    ``sinks`` (``False``: nothing changes): attention sinks (ops/attention.py; gpt-oss) -- ``self.sinks`` is an f32
    ``[heads]`` parameter, one logit per query head that joins every row's softmax denominator and adds nothing
    to its output.  It is initialised to zeros without an RNG draw, stays f32 under dtype casts, and is passed
    to every attention call below: training, prefill, decode step (``fused`` or not) and extend.  A cache is
    unchanged."""

    def __init__(self, dim: int, heads: int, causal: bool = False, kv_heads: Optional[int] = None,
                 rope: Optional[Rope] = None, bias: bool = True, window: Optional[int] = None,
                 qk_norm: bool = False, qk_eps: float = 1e-6, sinks: bool = False) -> None:
        super().__init__()
        if not isinstance(qk_norm, bool):
            raise ValueError(f"qk_norm must be a bool, not {qk_norm!r}")
        if not isinstance(sinks, bool):
            raise ValueError(f"sinks must be a bool, not {sinks!r}")
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
        self.qk_norm = qk_norm
        if qk_norm:
            self.q_norm = RMSNorm(self.hd, float(qk_eps))
            self.k_norm = RMSNorm(self.hd, float(qk_eps))
        self.sinks = nn.Parameter(torch.zeros(heads)) if sinks else None

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        p = self.sinks  # the kernels read f32 sinks: as RMSNorm keeps its weight
        if p is not None and p.dtype != torch.float32:
            p.data = p.data.float()
        return self

    def _kw(self) -> dict:
        """``kv_heads`` / ``window`` / ``sinks`` where the layer has them: plain MHA without a window or sinks
        makes the calls it always made."""
        kw = {} if self.kv_heads == self.heads else {"kv_heads": self.kv_heads}
        if self.window is not None:
            kw["window"] = self.window
        if self.sinks is not None:
            kw["sinks"] = self.sinks
        return kw

    def rotate(self, qkv: Tensor, positions: Optional[Tensor] = None, inplace: bool = False) -> Tensor:
        """The packed projection with q and k normalised (``qk_norm``) and rotated (``rope``); ``qkv`` itself
        without either."""
        if self.qk_norm:
            return qk_norm_rope_packed(qkv, self.heads, self.q_norm.weight, self.k_norm.weight, self.q_norm.eps,
                                       None if self.rope is None else self.rope.table(qkv), positions,
                                       kv_heads=self.kv_heads, inplace=inplace)
        if self.rope is None:
            return qkv
        return rope_packed(qkv, self.heads, self.rope.table(qkv), positions, kv_heads=self.kv_heads, inplace=inplace)

    def forward(self, x: Tensor, key_lengths: Optional[Tensor] = None, *, cache=None,
                positions: Optional[Tensor] = None, extend: bool = False, rolling: bool = False,
                kv_scales=None, mx=None) -> Tensor:
        # mx: the block's MXFP4 snapshots (a quantised prefill); None: the parameters, the calls it always made
        qkv, proj = snap_linear(self.qkv, mx, "qkv"), snap_linear(self.proj, mx, "proj")
        if cache is not None:
            rkw = {"rolling": True} if rolling else {}  # a linear cache: the call it always made
            if kv_scales is not None:  # likewise a cache that is not fp8
                rkw["kv_scales"] = kv_scales
            return proj(self.cached(qkv(x), cache, positions, key_lengths, extend=extend, **rkw))
        kw = self._kw()
        return proj(attention_packed(self.rotate(qkv(x)), self.heads, 1.0 / math.sqrt(self.hd),
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

    def forward(self, x: Tensor, *, mx=None) -> Tensor:
        if mx:  # MXFP4 snapshots (forward only): GELU in fc1's epilogue
            fc1 = snap_linear(self.fc1, mx, "fc1")
            return snap_linear(self.fc2, mx, "fc2")(fc1(x) if fc1 is self.fc1 else fc1(x, act="gelu"))
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

    def forward(self, x: Tensor, *, mx=None) -> Tensor:
        return snap_linear(self.fc2, mx, "fc2")(swiglu(snap_linear(self.fc1, mx, "fc1")(x)))


class _Permute(torch.autograd.Function):
    """``rows[perm]`` for a permutation ``perm`` whose inverse is ``inv``: the backward is the gather
    ``d[inv]``, not the ``index_add`` autograd would record."""

    @staticmethod
    def forward(ctx, rows, perm, inv):
        ctx.save_for_backward(perm, inv)
        return rows.index_select(0, perm)

    @staticmethod
    def backward(ctx, d):
        perm, inv = ctx.saved_tensors
        return _Permute.apply(d, inv, perm), None, None


class _Dispatch(torch.autograd.Function):
    """Token rows ``h`` ``[T, dim]`` -> the ``T * top_k`` expert-sorted rows ``h[order // top_k]``.  The
    backward gathers the sorted gradients back by the inverse permutation and sums each token's ``top_k``
    rows in slot order: no ``index_add``, no atomics."""

    @staticmethod
    def forward(ctx, h, order, inv, top_k):
        ctx.save_for_backward(order, inv)
        ctx.top_k = top_k
        return h.index_select(0, torch.div(order, top_k, rounding_mode="floor"))

    @staticmethod
    def backward(ctx, d):
        order, inv = ctx.saved_tensors
        k = ctx.top_k
        dh = _Permute.apply(d, inv, order).view(-1, k, d.shape[-1])
        return (dh[:, 0] if k == 1 else dh.sum(1)), None, None, None


def _check_experts(experts, top_k) -> None:
    if isinstance(experts, bool) or not isinstance(experts, int) or experts < 1:
        raise ValueError(f"experts must be an int >= 1, not {experts!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= experts:
        raise ValueError(f"top_k must be an int in [1, experts = {experts}], not {top_k!r}")


class MoE(nn.Module):
    """Sparse mixture of ``experts`` SwiGLU MLPs with Mixtral's routing rule: ``logits = router(h)`` in f32
    (a bias-free ``Linear(dim, experts)``), the ``top_k`` largest logits of each token (ties to the lower
    index), gates = the f32 softmax over those ``top_k`` logits, ``y = sum_j gate_j * expert_{e_j}(h)``.  The
    experts' weights are stacked: ``fc1`` ``[experts, 2 * hidden, dim]`` (``gate | up``) and ``fc2``
    ``[experts, dim, hidden]``; they have no bias.

    Dispatch: a stable sort of the ``T * top_k`` (token, slot) pairs by expert, the group offsets from a
    ``searchsorted`` of the sorted expert ids (``bincount`` reads its bin count on the host), a gather of
    the rows, ``grouped_linear`` -> ``swiglu`` -> ``grouped_linear`` (ops/gemm.py; csrc/gemm_grouped.hip), and
    the combine by the inverse permutation: gather back to ``[T, top_k, dim]``, times the gates in f32, summed
    over ``top_k`` in slot order, one rounding.  No ``index_add``, no atomics, no host read: deterministic and
    hipGraph-capturable.  No capacity limit: no token is dropped.

    :meth:`aux_loss` is the Switch load-balancing loss of the last forward."""

    def __init__(self, dim: int, hidden: int, experts: int, top_k: int = 2, bias: bool = False) -> None:
        super().__init__()
        _check_experts(experts, top_k)
        if bias:
            raise ValueError("MoE experts have no bias")
        self.experts, self.top_k = experts, top_k
        self.router = nn.Linear(dim, experts, bias=False)
        self.fc1 = nn.Parameter(torch.empty(experts, 2 * hidden, dim))
        self.fc2 = nn.Parameter(torch.empty(experts, dim, hidden))
        for w in (self.fc1, self.fc2):  # each expert as nn.Linear initialises its weight
            nn.init.uniform_(w, -1.0 / math.sqrt(w.shape[2]), 1.0 / math.sqrt(w.shape[2]))
        self._aux: Optional[Tensor] = None

    def route(self, h: Tensor):
        """``h`` ``[T, dim]`` -> (f32 logits ``[T, experts]``, expert ids ``[T, top_k]``, f32 gates ``[T, top_k]``)."""
        logits = F.linear(h.float(), self.router.weight.float())
        top, idx = torch.sort(logits, dim=-1, descending=True, stable=True)  # stable: ties to the lower index
        return logits, idx[:, :self.top_k], torch.softmax(top[:, :self.top_k], dim=-1)

    def forward(self, x: Tensor) -> Tensor:
        E, k = self.experts, self.top_k
        h = x.reshape(-1, x.shape[-1])
        T = h.shape[0]
        logits, idx, gates = self.route(h)
        ids, order = torch.sort(idx.reshape(-1), stable=True)  # pair t * k + j, sorted by expert
        inv = torch.empty_like(order).scatter_(0, order, torch.arange(T * k, device=h.device))
        offsets = torch.searchsorted(ids, torch.arange(E + 1, device=h.device)).to(torch.int32)
        rows = _Dispatch.apply(h, order, inv, k)
        rows = grouped_linear(swiglu(grouped_linear(rows, self.fc1, offsets)), self.fc2, offsets)
        y = _Permute.apply(rows, inv, order).view(T, k, -1)
        y = y[:, 0].float() * gates[:, 0, None] if k == 1 else (y.float() * gates[:, :, None]).sum(1)
        # Switch: E * sum_e (share of the pairs routed to e) * (mean router probability of e)
        share = (offsets[1:] - offsets[:-1]).float() / float(max(T * k, 1))
        self._aux = E * (share * torch.softmax(logits, dim=-1).mean(0)).sum()
        return y.to(x.dtype).view(x.shape)

    def aux_loss(self) -> Tensor:
        """The load-balancing loss ``experts * sum_e f_e * p_e`` of the last forward, an f32 scalar (1 when the
        routing is uniform): ``f_e`` the share of the (token, slot) pairs sent to expert ``e``, ``p_e`` the
        mean router probability of ``e`` over the tokens.  Differentiable through ``p_e``."""
        if self._aux is None:
            raise RuntimeError("aux_loss: no forward has run")
        return self._aux


class Block(nn.Module):
    """Pre-norm transformer block.  The defaults are the GPT-2 / ViT block: LayerNorm, a GELU MLP, biases.
    ``norm="rms"``: ``ln1`` / ``ln2`` are :class:`~torchbooster_amd.ops.norm.RMSNorm` (the attribute names
    stay: the ``(x, pending)`` protocol of ``forward`` is the same); ``mlp="swiglu"``: ``self.mlp`` is a
    :class:`SwiGLU` of hidden width ``int(dim * mlp_ratio)``; ``bias=False``: no bias in ``qkv``, ``proj`` and
    the MLP's linears -- together the Llama-style block.  ``window``: the sliding window of :class:`Attention`; ``qk_norm``: its QK-norm;
    ``sinks``: its attention sinks.
    ``mlp="moe"``: ``self.mlp`` is a :class:`MoE` of ``experts`` SwiGLU experts of that hidden width, ``top_k`` per
    token (its router and experts never have a bias; ``bias`` then governs ``qkv`` and ``proj`` alone);
    ``forward_rows`` runs it on the few-row expert kernels (``ops.linear.moe_route_rows``, then
    ``linear_rows_experts`` twice: 3 launches) once ``quantize_rows()`` has snapshotted the experts as MXFP4,
    and raises ``ValueError`` before that; it does not update ``MoE.aux_loss``."""

    # the MXFP4 snapshots of quantize_rows, {name: (codes, scales)}: a plain attribute like the Rope tables
    mx_rows = None

    def __init__(self, dim: int, heads: int, mlp_ratio: float = 4.0, causal: bool = False,
                 kv_heads: Optional[int] = None, rope: Optional[Rope] = None, norm: str = "layer",
                 mlp: str = "gelu", bias: bool = True, window: Optional[int] = None,
                 qk_norm: bool = False, experts: int = 8, top_k: int = 2, sinks: bool = False) -> None:
        super().__init__()
        if mlp not in ("gelu", "swiglu", "moe"):
            raise ValueError(f"mlp must be 'gelu', 'swiglu' or 'moe', not {mlp!r}")
        if mlp == "moe":
            _check_experts(experts, top_k)
        self.ln1 = make_norm(norm, dim)
        self.attn = Attention(dim, heads, causal, kv_heads, rope, bias=bias, window=window,
                              **({"qk_norm": qk_norm} if qk_norm is not False else {}),
                              **({"sinks": sinks} if sinks is not False else {}))
        self.ln2 = make_norm(norm, dim)
        hidden = int(dim * mlp_ratio)
        if mlp == "moe":
            self.mlp = MoE(dim, hidden, experts, top_k)
        else:
            self.mlp = SwiGLU(dim, hidden, bias) if mlp == "swiglu" else MLP(dim, hidden, bias)

    def forward(self, x: Tensor, pending: Optional[Tensor] = None, key_lengths: Optional[Tensor] = None, *,
                cache=None, positions: Optional[Tensor] = None, extend: bool = False, rolling: bool = False,
                kv_scales=None, mx: bool = False):
        """``x``: residual stream; ``pending``: a sub-block output not yet added
        to it.  Returns (stream, pending) so adds fuse into the next LayerNorm.
        ``key_lengths``: per-batch key lengths for the attention (None: every key).
        ``cache`` / ``positions`` / ``extend`` / ``rolling`` / ``kv_scales``: this layer's KV cache, passed to
        :class:`Attention`.  ``mx``: ``qkv``, ``proj``, ``fc1`` and ``fc2`` multiply by their MXFP4 snapshots
        (``quantize_rows``) through ``ops.linear.linear_mx``; forward only, dense MLPs only (``ValueError``)."""
        mkw = {}  # mx=False: the calls it always made
        if mx:
            if isinstance(self.mlp, MoE) or self.mx_rows is None:
                raise ValueError("mx=True needs a dense MLP and the MXFP4 snapshots of quantize_rows()")
            mkw["mx"] = self.mx_rows
        if pending is None:
            h = self.ln1(x)
        else:
            h, x = self.ln1(x, pending)
        if kv_scales is not None:  # an fp8 cache
            a = self.attn(h, key_lengths, cache=cache, positions=positions, extend=extend,
                          **({"rolling": True} if rolling else {}), kv_scales=kv_scales, **mkw)
        elif rolling:
            a = self.attn(h, key_lengths, cache=cache, positions=positions, extend=extend, rolling=True, **mkw)
        else:
            a = self.attn(h, key_lengths, cache=cache, positions=positions, extend=extend, **mkw)
        h, x = self.ln2(x, a)
        return x, self.mlp(h, **mkw)

    def forward_rows(self, x: Tensor, *, cache, positions: Tensor, extend: bool = False,
                     rolling: bool = False, kv_scales=None) -> Tensor:
        """The decoding layer on the few-row kernels (ops/linear.py ``linear_rows``; causal, forward only):
        ``x`` ``[B, T, dim]`` is the residual stream itself -- there is no ``pending`` -- and so is the
        result.  Both norms (LayerNorm or RMSNorm) run as prologues of the product behind them, bias / GELU or
        SwiGLU / residual as epilogues, and the attention is ``Attention.cached(fused=True)``: with ``T == 1`` 5 launches with a
        single-chunk cache, 6 otherwise (one more with rotary positions or ``qk_norm`` or both: the one launch
        that normalises and rotates ``qkv``).
        ``T > 1`` needs ``extend=True``.  Computes what ``forward`` computes with ``cache`` / ``positions`` /
        ``extend``, to rounding.  ``rolling``: ``cache`` is a rolling pair (:class:`Attention`);
        ``kv_scales``: it is an fp8 pair with these scales."""
        at = self.attn
        if not self.has_rows_path():
            raise ValueError("forward_rows (fused=True): an MoE block decodes on the few-row kernels only with "
                             "MXFP4 expert snapshots: call quantize_rows() first")
        if x.shape[1] != 1 and not extend:
            raise ValueError("forward_rows: more than one token per sequence needs extend=True")
        mx = self.mx_rows or {}
        w, kw = rows_weight(at.qkv, mx.get("qkv"))
        qkv = linear_rows(x, w, at.qkv.bias, **norm_args(self.ln1), **kw)
        a = at.cached(qkv, cache, positions, extend=extend, fused=True, **({"rolling": True} if rolling else {}),
                      **({} if kv_scales is None else {"kv_scales": kv_scales}))
        w, kw = rows_weight(at.proj, mx.get("proj"))
        x = linear_rows(a, w, at.proj.bias, residual=x, **kw)
        if isinstance(self.mlp, MoE):
            return self.moe_rows(x)
        act = "swiglu" if isinstance(self.mlp, SwiGLU) else "gelu"
        w, kw = rows_weight(self.mlp.fc1, mx.get("fc1"))
        h = linear_rows(x, w, self.mlp.fc1.bias, **norm_args(self.ln2), act=act, **kw)
        w, kw = rows_weight(self.mlp.fc2, mx.get("fc2"))
        return linear_rows(h, w, self.mlp.fc2.bias, residual=x, **kw)

    def moe_rows(self, x: Tensor) -> Tensor:
        """The MoE half of ``forward_rows``, ``x + mlp(ln2(x))`` on the residual stream ``x`` ``[..., dim]``, in three
        launches (csrc/rows_experts_mx.hip): the router on the normed rows, the chosen experts' ``fc1`` with the norm
        prologue and the SwiGLU epilogue, their ``fc2`` with the gated combine and the residual.  Needs the MXFP4
        expert snapshots of ``quantize_rows``; forward only, and ``MoE.aux_loss`` is not updated."""
        mx = self.mx_rows
        rows = x.reshape(-1, x.shape[-1])
        ids, gates = moe_route_rows(rows, self.mlp.router.weight, self.mlp.top_k, **norm_args(self.ln2))
        h = linear_rows_experts(rows, *mx["fc1"], ids, **norm_args(self.ln2), act="swiglu")
        return linear_rows_experts(h, *mx["fc2"], ids, gates=gates, residual=rows).view(x.shape)

    def has_rows_path(self) -> bool:
        """Whether ``forward_rows`` can run: always, except for an MoE block without the MXFP4 expert snapshots
        of ``quantize_rows`` (there is no few-row kernel for bf16 experts)."""
        return not isinstance(self.mlp, MoE) or {"fc1", "fc2"} <= set(self.mx_rows or {})

    def quantize_rows(self, fmt: Optional[str] = "mxfp4") -> None:
        """Snapshot ``qkv``, ``proj``, ``fc1`` and ``fc2`` as MXFP4 for ``forward_rows`` (``fmt=None``: drop the
        snapshots); see ``TransformerLM.quantize_rows``.  An MoE MLP's stacked experts become ``fc1`` = (codes
        ``[E, 2 * hidden, dim / 2]``, scales ``[E, 2 * hidden, dim / 32]``) and ``fc2`` = (``[E, dim, hidden / 2]``,
        ``[E, dim, hidden / 32]``), ``mx_quantize`` of the ``[E * rows, K]`` view, when ``dim`` and ``hidden`` are
        both multiples of 32; its router stays bf16."""
        named = [("qkv", self.attn.qkv), ("proj", self.attn.proj)]
        moe = isinstance(self.mlp, MoE)
        if not moe:
            named += [("fc1", self.mlp.fc1), ("fc2", self.mlp.fc2)]
        self.mx_rows = mx_snapshots(named, fmt)
        if moe and fmt is not None and self.mlp.fc1.shape[2] % MX_BLOCK == 0 and self.mlp.fc2.shape[2] % MX_BLOCK == 0:
            for name, w in (("fc1", self.mlp.fc1), ("fc2", self.mlp.fc2)):
                E, rows, K = w.shape
                codes, scales = mx_quantize(w.reshape(E * rows, K))
                self.mx_rows[name] = (codes.view(E, rows, K // 2), scales.view(E, rows, K // MX_BLOCK))


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
