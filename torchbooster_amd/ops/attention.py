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

Sliding window (``window=``, a host ``int`` ``W >= 1``, never a device value; ``None``: no window), one
rule on every path: a row whose upper key limit is ``hi`` sees the keys ``max(0, hi - W) <= j < hi`` --
the window is counted back from the limit the row already has.  In :func:`attention` /
:func:`attention_packed` (which need ``causal=True`` for it) ``hi = min(clamp(key_lengths[b], 1, N),
i + 1)``: a valid token sees itself and the ``W - 1`` tokens before it (``i - W < j <= i``, the Hugging Face
``sliding_window``), a query at a padded position the last ``W`` valid keys, so still no row is fully
masked; ``W = 1`` is a row that sees only itself.  In the cache functions below ``hi`` is the limit they
state (``len`` of a decode, ``L(b, t)`` of an extend).  ``window < 1`` or a non-int raises ``ValueError``.
A window that can hide nothing -- ``W >= N``, or ``W >= cap`` for the cache functions, decided on the
host from shapes alone -- IS the call with ``window=None``: the same kernels, the same bits.  Natively a
windowed training call always runs the three 128-row kernels (a third instantiation, which also skips
the key tiles left of the window; there is no windowed whole-head kernel and ``attn_set_head_mask`` does
not apply), a windowed decode streams at most ``W`` rows per (batch, kv head) whatever the length, and a
windowed extend starts at its first query's lower limit.  Cache rows below ``max(0, hi - W)`` of a decode
NEVER enter arithmetic (not loaded, probability the constant 0; selected away before the multiply on the
PyTorch path); in an extend that holds for the rows below the smallest lower limit of a wave's 16
queries natively and of the call's first query on the PyTorch path, while rows between that bound and a
query's own lower limit are real, previously appended data that may meet an exact-zero probability.

KV-cache decoding (forward only; csrc/attention_decode.hip).  A cache is, per layer, a ``k_cache`` and
a ``v_cache`` of ``[B, H, cap, D]`` (``torch.empty`` is fine: see the guarantee below; ``[B, Hkv, cap, D]``
with ``kv_heads``, see the end of this docstring).

* :func:`kv_cache_append` copies the k and v rows of a packed ``qkv`` ``[B, T, 3*H*D]`` into the
  caches: token ``t`` of batch ``b`` goes to row ``positions[b] + t``; a row outside ``[0, cap)`` is
  DROPPED (the rest of that batch is still written).  ``T = 1`` is a decode step, ``T = N`` a prefill.
* :func:`attention_decode` attends one query per (batch, head), ``q`` ``[B, H, D]``, to the first
  ``len = clamp(lengths[b], 1, cap)`` cache rows -- 0 behaves as 1, anything above ``cap`` as ``cap``.
* :func:`attention_decode_packed` takes the ``[B, 1, 3*H*D]`` projection of one new token, appends
  its k/v at ``positions[b]`` and attends to keys ``j <= positions[b]``, returning ``[B, 1, H*D]``.

``lengths`` / ``positions`` are int32 ``[B]`` tensors on the inputs' device, read on the device like
``key_lengths``: no host sync on any path, safe inside a graph capture, a replay follows in-place
changes.  Cache rows at or past the length NEVER enter arithmetic -- the native kernels do not load
them, the PyTorch path selects them away before the multiply -- so junk there (NaN / Inf bit patterns
of an uninitialised cache, the pad rows of a ragged prefill) cannot reach the output.  The native path
(CUDA, bf16, D = 64) splits the keys over workgroups (``attn_decode_set_chunk`` keys each, grid fixed
from ``cap``) and merges the partials in a second launch in fixed order: deterministic, no atomics.
These functions do not build an autograd graph and raise if an input requires grad in grad mode.

Extend (forward only; csrc/attention_extend.hip): ``T >= 1`` new tokens per sequence against a cache
that already holds tokens -- continuing a conversation, chunked prefill, scoring several candidate
tokens in one pass.

* :func:`attention_extend` takes ``q`` ``[B, T, H, D]`` (any view with a contiguous last dim) whose
  k / v rows are already in the caches at rows ``positions[b] + t``: query ``t`` of batch ``b`` sees
  the cache rows ``j < L(b, t) = clamp(positions[b] + t + 1, 1, cap)`` -> ``[B, T, H, D]``.  A bad
  position never moves an address and no row is ever fully masked.
* :func:`attention_extend_packed` takes the packed ``[B, T, 3*H*D]`` projection of the new tokens:
  :func:`kv_cache_append`, then extend -> ``[B, T, H*D]``.  ``T == 1`` IS
  :func:`attention_decode_packed` (the same calls, bit-equal results).

What may enter arithmetic: cache rows at or past ``clamp(positions[b] + T, 1, cap)`` NEVER do (not
loaded by the native kernel, selected away before the multiply on the PyTorch path), which covers the
never-written part of a ``torch.empty`` cache.  Rows between a query's own limit ``L(b, t)`` and that
bound are the rows this call's tokens just appended: real finite data, which MAY be multiplied by an
exact-zero probability.  The native path (CUDA, bf16, D = 64) runs 16 queries per wave on the MFMA and
splits the keys over workgroups only when ``B * H * ceil(T / 16)`` cannot occupy the chip
(``attn_extend_set_split`` forces a split size, ``attn_extend_splits(B, H, T, cap)`` tells the count);
the partials are merged in fixed order, and ``positions`` are read on the device as above.

Grouped-query attention (``kv_heads=``): ``H`` query heads share ``Hkv`` key / value heads; ``Hkv``
must divide ``H``, ``G = H // Hkv``, and query head ``h`` reads kv head ``h // G`` (the
``repeat_interleave(G, dim=heads)`` convention; ``Hkv = 1`` is multi-query attention).  A packed
projection is then ``[B, T, (H + 2*Hkv)*D]``, still ``q | k | v`` and head-major inside each part, and
a cache is ``[B, Hkv, cap, D]``: ``G`` times smaller, and ``G`` times fewer bytes per decode step.
``kv_heads=None`` means ``Hkv = H``, which is everything above unchanged.  ``kv_heads`` is always
given explicitly, never inferred from a cache's shape: a cache with the wrong head count raises.  A
``kv_heads`` that does not divide ``heads`` raises ``ValueError``; a cache or a packed width that does
not match raises ``RuntimeError``.  The native decode kernel loads each cache row once for up to four
query heads of a group, and the decode / extend results have the bits of the same call on the caches
expanded to ``H`` heads.  Training and prefill (:func:`attention`, :func:`attention_packed` with
``Hkv < H``) expand k / v to ``H`` heads -- one materialised copy -- and run the existing kernels under
autograd, which sums dK / dV over each group; a group-aware training kernel is not part of this.

Rolling KV cache (``rolling=True`` on the five cache functions, a host ``bool`` that is never inferred from a
shape, like ``kv_heads``; csrc/attn_ring.h).  The caches are ``[B, Hkv, R, D]`` used as a RING: logical row
``j`` (the ``j``-th token of the sequence) lives in slot ``j mod R``, and ``positions`` / ``lengths`` keep
counting tokens, not slots -- the lower clamp to 1 stays, the upper clamp to the row count is gone.  With
an upper limit ``n`` -- ``max(lengths[b] + add, 1)`` of a decode, ``L(b, T - 1) = max(positions[b] + T, 1)`` of
an extend, for the whole call -- slot ``p`` holds logical row ``j(p)``, the largest ``j = p (mod R)`` with
``j < n``; ``j(p) < 0`` is a slot that was never written and is hidden.  A query with limit ``L`` and window
``W`` sees slot ``p`` iff ``max(0, L - W) <= j(p) < L``: over logical rows, exactly the window rule above, so
a rolling layer computes what the linear cache of all rows computes while it keeps ``R`` rows and streams
``R`` rows per step at any context length.  ``rolling=True`` needs a ``window`` with ``1 <= W <= R``
(``ValueError`` otherwise; ``W == R`` is a real window here and is not turned into ``window=None``).  An
extend appends its ``T`` rows before its first query reads, so it needs ``T <= R - W + 1``, decided on the
host from shapes (``ValueError``): the row written for token ``T - 1`` then replaces logical row
``positions[b] + T - 1 - R``, which lies below the first query's lower limit ``positions[b] + 1 - W``.  The
same inequality keeps "rows past the position" harmless in a ring -- the pad tokens of a ragged extend, the
rejected rows of a speculative round: such a stale slot is read as logical row ``pos + t - R``, which no
later query can see.  :func:`kv_cache_append` with ``rolling=True`` stores token ``t`` to slot
``(positions[b] + t) mod R`` iff ``positions[b] + t >= 0`` and ``n_b - R <= t < n_b``, ``n_b = clamp(lengths[b],
1, T)`` with its ``lengths=`` (int32 ``[B]``; a ragged prefill) and ``T`` without: the last ``R`` valid rows of
the call, no pad rows, at most one store per slot.  Hidden slots NEVER enter arithmetic on either path (not
loaded natively; selected away before either product on the PyTorch path, which is built from the same
``j(p)`` formula and is sync-free).  ``rolling=False``, the default, is everything above unchanged.

FP8 KV cache (``kv_scales=`` on the five cache functions; csrc/attn_fp8.h).  A cache pair whose two tensors are
``torch.float8_e4m3fn`` (OCP e4m3: 254 finite codes, maximum 448, no infinities) holds CODES, with two host floats
``(k_scale, v_scale)`` per layer -- never device values, like ``window``; ``None`` is ``(1.0, 1.0)``; each must be
finite and ``> 0`` and scales with any other pair raise ``ValueError``.  One rule on every path: a row is stored as
``code = rne_e4m3(clamp(f32(x) * inv, -448, 448))`` with ``inv = float32(1 / scale)`` formed on the host in double
-- the clamp is an explicit f32 min / max ahead of the conversion, so ±inf saturate to ±448 and nothing depends on
a conversion's overflow mode; NaN stays a NaN code -- and read as ``f32(code) * f32(scale)``.  :func:`kv_quantize`
and :func:`kv_dequantize` are that rule in PyTorch, for any device.  EVERY query that reads the cache sees the
dequantised codes, the step's own row included: a decode step or an extend quantises its new rows, stores the codes
and attends to them, so ``fused=True`` stays bit-equal to ``fused=False`` in output and cache bytes; only
:func:`attention_packed`, the prefill's attention, reads unquantised ``qkv``.  Everything else above holds as
stated -- which rows are visible, the clamps, positions read on the device, no host sync, capturability, the ring and
its ``T <= R - W + 1`` -- and hidden rows are never loaded and never dequantised: the NaN code ``0x7F`` in a hidden
row cannot reach an output.  Natively (CUDA, ``D == 64``, both caches e4m3 with 16-byte row conditions, bf16 ``q`` /
``qkv``) the kernels are the ``FP8`` instantiations of the append, decode and extend kernels: rows of 64 B, converted
by the packed hardware conversions; ``k_scale`` rides in the score factor (``scale * k_scale`` is one f32 product on
the host), ``P·V`` accumulates the unscaled codes and the f32 accumulator is multiplied by ``v_scale`` once, before
the partial or the output is written; the merge kernels, the workspaces and the grids are those of bf16.  The extend
kernel feeds the dequantised codes -- exact in bf16 -- to the bf16 MFMA.  Mixed dtypes, ``float8_e5m2``, CPU tensors,
other head dims and ``TBAMD_FORCE_REFERENCE=1`` take the PyTorch path, which dequantises the pair by the rule
(what stock PyTorch does with a pair that is not e4m3 / e4m3 is unchanged).  With bf16 caches every call is the call
it was.

Rotary position embeddings (csrc/rope.hip): :func:`rope_packed` rotates the q and k parts of a packed
projection by the angles :func:`rope_table` holds, before any of the functions above reads it -- so the
training path, the prefill, the append, the decode and the extend all see rotated q / k, a cache holds
rotated keys, and none of the attention kernels knows.  Positions follow the clamp rule of
``embed_rows`` and are read on the device.  Differentiable out of place (the gradient is the inverse
rotation), forward-only in place.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd.function import once_differentiable

from torchbooster_amd.ops._ext import native, use_native

__all__ = ["attention", "attention_packed", "attention_ref", "native_supported", "kv_cache_append",
           "attention_decode", "attention_decode_packed", "attention_extend", "attention_extend_packed",
           "rope_table", "rope_packed", "kv_quantize", "kv_dequantize"]


def _window(window, limit: Optional[int] = None) -> Optional[int]:
    """``window`` checked (``None`` or an int >= 1); ``None`` too when it can hide nothing (``>= limit``)."""
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise ValueError(f"window must be None or an int >= 1, not {window!r}")
    return None if limit is not None and window >= limit else window


def _visible(N: int, device, causal: bool, key_lengths: Optional[Tensor],
             window: Optional[int] = None) -> Optional[Tensor]:
    """The boolean mask (True = attend) of the masks, broadcastable to [B, H, N, N]; None = dense.
    ``window`` (with ``causal``): keys below ``max(0, hi - window)`` are hidden, ``hi`` the row's limit."""
    m = kl = None
    if key_lengths is not None:
        kl = key_lengths.to(device=device, dtype=torch.int64).clamp(1, N)  # the kernels' clamp
        m = (torch.arange(N, device=device)[None, :] < kl[:, None])[:, None, None, :]
    if causal:
        c = torch.ones(N, N, dtype=torch.bool, device=device).tril()
        m = c if m is None else m & c
    if window is not None:
        i = torch.arange(N, device=device)
        hi = i + 1 if kl is None else torch.minimum(kl[:, None], (i + 1)[None, :])  # [N] or [B, N]
        w = i >= (hi - window).clamp_min(0)[..., None]  # [N, N] or [B, N, N]: key j at or past the row's lower limit
        m = m & (w if kl is None else w[:, None])
    return m


def _check_window(window, causal: bool, N: int) -> Optional[int]:
    """The window of :func:`attention` / :func:`attention_packed`: it needs ``causal``; ``>= N`` is none."""
    window = _window(window, N)
    if window is not None and not causal:
        raise ValueError("window needs causal=True")
    return window


def attention_ref(q: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None, *, causal: bool = False,
                  key_lengths: Optional[Tensor] = None, window: Optional[int] = None) -> Tensor:
    """softmax(q kᵀ · scale) v over [..., N, D] tensors (f32 softmax); with a mask, over
    [B, H, N, D] (the fp32 oracle of the masked kernels when given fp32 inputs)."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    if window is not None and not causal:
        _window(window)
        raise ValueError("window needs causal=True")
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    m = _visible(q.shape[-2], q.device, causal, key_lengths, _window(window, q.shape[-2]))
    if m is not None:
        s = s.masked_fill(~m, float("-inf"))
    p = torch.softmax(s.float(), dim=-1).to(q.dtype)
    return torch.matmul(p, v)


def _check_lengths(key_lengths: Optional[Tensor], B: int, like: Tensor) -> None:
    if key_lengths is None:
        return
    if key_lengths.dtype != torch.int32 or key_lengths.shape != (B,) or key_lengths.device != like.device:
        raise ValueError("key_lengths must be an int32 tensor of shape [B] on the device of the inputs")


def _sdpa(q: Tensor, k: Tensor, v: Tensor, scale: float, causal: bool, key_lengths: Optional[Tensor],
          window: Optional[int] = None) -> Tensor:
    """Stock PyTorch (the comparator of --mode stock benchmarks; CPU path), same mask semantics."""
    m = _visible(q.shape[-2], q.device, causal, key_lengths, window)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=m, scale=scale)


def native_supported(q: Tensor) -> bool:
    return q.is_cuda and q.dtype == torch.bfloat16 and q.shape[-1] == 64 and use_native(q)


class _AttnFn(torch.autograd.Function):
    """q, k, v: [B, H, N, 64] views -> o [B, N, H, 64] (contiguous)."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal=False, key_lengths=None, window=None):
        kw = {} if window is None else {"window": window}  # no window: the call it always made
        o, lse = native().attn_forward(q, k, v, scale, causal, key_lengths, **kw)
        ctx.save_for_backward(q, k, v, o, lse, key_lengths)
        ctx.scale, ctx.causal, ctx.kw = scale, causal, kw
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
                               ctx.causal, key_lengths, **ctx.kw)
        return dq, dk, dv, None, None, None, None


class _AttnPackedFn(torch.autograd.Function):
    """qkv: [B, N, 3*H*64] -> [B, N, H*64]; the gradient is one packed buffer."""

    @staticmethod
    def forward(ctx, qkv, heads, scale, causal=False, key_lengths=None, window=None):
        B, N, E3 = qkv.shape
        D = E3 // (3 * heads)
        t = qkv.view(B, N, 3, heads, D)
        q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
        kw = {} if window is None else {"window": window}  # no window: the call it always made
        o, lse = native().attn_forward(q, k, v, scale, causal, key_lengths, **kw)
        ctx.save_for_backward(qkv, o, lse, key_lengths)
        ctx.cfg, ctx.kw = (heads, D, scale, causal), kw
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
                               causal, key_lengths, **ctx.kw)
        return dqkv, None, None, None, None, None


def _kv_heads(heads: int, kv_heads: Optional[int]) -> int:
    """``Hkv`` of a grouped-query layer: ``heads`` by default, otherwise a divisor of ``heads``."""
    hkv = heads if kv_heads is None else int(kv_heads)
    if hkv < 1 or heads % hkv:
        raise ValueError(f"kv_heads {kv_heads} must divide heads {heads}")
    return hkv


def _expand_kv(x: Tensor, G: int, dim: int) -> Tensor:
    """Repeat every head of ``x`` (heads at ``dim``) ``G`` times in place (``repeat_interleave``): an
    ``expand`` then a ``reshape``, one materialised copy whose gradient autograd sums over the group."""
    shape = list(x.shape)
    x = x.unsqueeze(dim + 1).expand(*shape[:dim + 1], G, *shape[dim + 1:])
    shape[dim] *= G
    return x.reshape(shape)


def _rows_ok(t: Tensor) -> bool:
    return t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0


def _rows(t: Tensor) -> Tensor:
    """``t`` as the native kernels read it: 16-B aligned rows of unit stride, through a copy if need be."""
    return t if _rows_ok(t) else t.contiguous()


def attention(q: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None, *, causal: bool = False,
              key_lengths: Optional[Tensor] = None, window: Optional[int] = None) -> Tensor:
    """[B, H, N, D] -> [B, H, N, D].  ``causal`` / ``key_lengths``: the masks of the module docstring
    (self-attention: q, k, v of one shape; lengths clamped into [1, N]).  ``window`` (needs ``causal``): the
    sliding window of the module docstring; ``window >= N`` is ``window=None``.

    Grouped-query attention: ``k`` / ``v`` may be ``[B, Hkv, N, D]`` with ``Hkv`` dividing ``H``; they are
    expanded to ``H`` heads (one copy) and dK / dV are summed over each group by autograd.  There is no
    group-aware training kernel."""
    scale = 1.0 / math.sqrt(q.shape[-1]) if scale is None else float(scale)
    if q.dim() == 4 and k.dim() == 4 and k.shape == v.shape and k.shape[1] != q.shape[1]:
        G = q.shape[1] // _kv_heads(q.shape[1], k.shape[1])
        k, v = _expand_kv(k, G, 1), _expand_kv(v, G, 1)
    window = _check_window(window, causal, q.shape[-2])
    if (causal or key_lengths is not None) and not (q.dim() == 4 and q.shape == k.shape == v.shape):
        raise ValueError("attention masks need [B, H, N, D] self-attention inputs of one shape")
    _check_lengths(key_lengths, q.shape[0], q)
    if native_supported(q) and q.dim() == 4 and q.shape == k.shape == v.shape:
        q, k, v = _rows(q), _rows(k), _rows(v)
        if window is None:  # the call it always made
            return _AttnFn.apply(q, k, v, scale, bool(causal), key_lengths).permute(0, 2, 1, 3)
        return _AttnFn.apply(q, k, v, scale, True, key_lengths, window).permute(0, 2, 1, 3)
    if window is None:
        return _sdpa(q, k, v, scale, causal, key_lengths)
    return _sdpa(q, k, v, scale, causal, key_lengths, window)


def attention_packed(qkv: Tensor, heads: int, scale: Optional[float] = None, *, causal: bool = False,
                     key_lengths: Optional[Tensor] = None, kv_heads: Optional[int] = None,
                     window: Optional[int] = None) -> Tensor:
    """[B, N, 3*H*D] packed q|k|v (head-major inside each) -> [B, N, H*D]; masks and ``window`` as
    :func:`attention`.

    ``kv_heads`` (grouped-query attention): ``qkv`` is ``[B, N, (H + 2*Hkv)*D]``.  With ``Hkv < H`` the
    packed tensor is split, k / v are expanded to ``H`` heads (one materialised copy) and
    :func:`attention` runs on that under autograd, which sums dK / dV over each group: a group-aware
    training kernel is out of scope."""
    hkv = _kv_heads(heads, kv_heads)
    window = _check_window(window, causal, qkv.shape[1])
    wkw = {} if window is None else {"window": window}  # no window: the calls it always made
    if hkv != heads:
        B, N, E = qkv.shape
        if E % (heads + 2 * hkv):
            raise RuntimeError("qkv must be [B, N, (H + 2*Hkv)*D]")
        D = E // (heads + 2 * hkv)
        q = qkv[..., :heads * D].view(B, N, heads, D).transpose(1, 2)
        k, v = (_expand_kv(qkv[..., o * D:(o + hkv) * D].view(B, N, hkv, D), heads // hkv, 2).transpose(1, 2)
                for o in (heads, heads + hkv))
        o = attention(q, k, v, 1.0 / math.sqrt(D) if scale is None else scale, causal=causal, key_lengths=key_lengths,
                      **wkw)
        return o.transpose(1, 2).reshape(B, N, heads * D)
    B, N, E3 = qkv.shape
    D = E3 // (3 * heads)
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    _check_lengths(key_lengths, B, qkv)
    if native_supported(qkv.view(B, N, 3, heads, D)) and _rows_ok(qkv):
        return _AttnPackedFn.apply(qkv, heads, scale, bool(causal), key_lengths, *wkw.values())
    t = qkv.view(B, N, 3, heads, D).permute(2, 0, 3, 1, 4)
    o = _sdpa(t[0], t[1], t[2], scale, causal, key_lengths, *wkw.values())
    return o.transpose(1, 2).reshape(B, N, heads * D)


# ---------------------------------------------------------------- KV-cache decoding (forward only)
def _forward_only(*tensors: Tensor) -> None:
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError("KV-cache decoding is forward-only: call it under torch.no_grad() or detach the inputs")


def _packed_dims(qkv: Tensor, heads: int, kv_heads: Optional[int], scale: Optional[float] = None, *,
                 T: str = "T", even: bool = False):
    """Validate a packed ``[B, T, (H + 2*Hkv)*D]`` projection -- ``T``: ``"T"`` (any), ``"1"`` or ``"T >= 1"`` --
    -> ``(hkv, B, T, D, scale)``, ``scale`` defaulting to ``1 / sqrt(D)``."""
    hkv = _kv_heads(heads, kv_heads)
    w = heads + 2 * hkv
    if qkv.dim() == 3:
        B, n, E = qkv.shape
        D = E // w
        if E == D * w and (T == "T" or n == 1 or (n > 1 and T != "1")) and not (even and D % 2):
            return hkv, B, n, D, 1.0 / math.sqrt(max(D, 1)) if scale is None else float(scale)
    raise RuntimeError(f"qkv must be [B, {T}, (H + 2*Hkv)*D]" + (" with an even D" if even else ""))


def _check_cache(k_cache: Tensor, v_cache: Tensor, B: int, H: int, D: int, pos: Tensor, name: str) -> None:
    """``H``: the cache's head count, i.e. ``Hkv`` of a grouped-query layer."""
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or tuple(k_cache.shape[:2]) != (B, H) \
            or k_cache.shape[3] != D or k_cache.shape[2] < 1:
        raise RuntimeError(f"k_cache / v_cache must be [B, Hkv, cap, D] = [{B}, {H}, cap, {D}]")
    if pos.dtype != torch.int32 or pos.shape != (B,) or pos.device != k_cache.device:
        raise RuntimeError(f"{name} must be an int32 tensor of shape [B] on the device of the cache")


_FP8 = torch.float8_e4m3fn
_FP8_MAX = 448.0


def _f32(x: float) -> float:
    """``x`` rounded to float32, as a Python float."""
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def _check_scale(scale) -> float:
    ok = isinstance(scale, (int, float)) and not isinstance(scale, bool) and math.isfinite(scale) and scale > 0
    if not ok:
        raise ValueError(f"an fp8 KV-cache scale must be a finite float > 0, not {scale!r}")
    return float(scale)


def kv_quantize(x: Tensor, scale: float = 1.0) -> Tensor:
    """The quantiser of an fp8 KV cache (module docstring): ``rne_e4m3(clamp(f32(x) * inv, -448, 448))`` with
    ``inv = float32(1 / scale)`` -> ``torch.float8_e4m3fn`` of ``x``'s shape.  ±inf saturate to ±448, NaN stays a
    NaN code.  Any device; the native append computes the same bytes."""
    inv = _f32(1.0 / _check_scale(scale))
    return (x.to(torch.float32) * inv).clamp(-_FP8_MAX, _FP8_MAX).to(_FP8)


def kv_dequantize(c: Tensor, scale: float = 1.0, dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """``f32(code) * f32(scale)`` of an fp8 KV cache (module docstring), one float32 product, -> ``dtype``
    (``torch.float64`` holds that float32 value exactly).  The NaN codes give NaN."""
    if c.dtype != _FP8:
        raise ValueError(f"kv_dequantize takes a torch.float8_e4m3fn tensor, not {c.dtype}")
    return (c.to(torch.float32) * _f32(_check_scale(scale))).to(dtype)


def _kv_scales(kv_scales, k_cache: Tensor, v_cache: Tensor) -> Optional[Tuple[float, float]]:
    """The ``(k_scale, v_scale)`` of an fp8 cache pair (``None`` given: ``(1.0, 1.0)``), checked; ``None`` for
    any other pair, with which scales raise ``ValueError``."""
    if k_cache.dtype != _FP8 or v_cache.dtype != _FP8:
        if kv_scales is not None:
            raise ValueError("kv_scales need float8_e4m3fn caches")
        return None
    if kv_scales is None:
        return (1.0, 1.0)
    try:
        ks, vs = kv_scales
    except (TypeError, ValueError):
        raise ValueError(f"kv_scales must be a (k_scale, v_scale) pair, not {kv_scales!r}") from None
    return (_check_scale(ks), _check_scale(vs))


def _scale_kw(sc: Optional[Tuple[float, float]]):
    """The trailing keywords of the native calls and of the PyTorch paths for the scales of :func:`_kv_scales`;
    a cache that is not fp8 adds nothing: the calls they always made."""
    if sc is None:
        return {}, {}
    return {"k_scale": sc[0], "v_scale": sc[1]}, {"kv_scales": sc}


def _rows_ok_bytes(t: Tensor) -> bool:
    """:func:`_rows_ok` for a one-byte element type: the same 16-B conditions, in bytes."""
    return t.stride(-1) == 1 and all(s % 16 == 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0


def _decode_native(x: Tensor, k_cache: Tensor, v_cache: Tensor) -> bool:
    if k_cache.dtype == _FP8:  # the fp8 instantiations: both caches e4m3, bf16 q / qkv
        return (v_cache.dtype == _FP8 and k_cache.is_cuda and v_cache.is_cuda and k_cache.shape[-1] == 64
                and use_native(k_cache) and x.is_cuda and x.dtype == torch.bfloat16
                and _rows_ok_bytes(k_cache) and _rows_ok_bytes(v_cache))
    return (native_supported(k_cache) and v_cache.dtype == torch.bfloat16 and v_cache.is_cuda and x.is_cuda
            and x.dtype == torch.bfloat16 and _rows_ok(k_cache) and _rows_ok(v_cache))


def _put_rows(cache: Tensor, take: Tensor, rows: Tensor, scale: Optional[float]) -> None:
    """``cache`` <- ``rows`` where ``take``, its own bits elsewhere; ``scale``: the cache is fp8 and the rows are
    quantised by the rule (selected as bytes, so untouched rows keep theirs)."""
    if scale is None:
        cache.copy_(torch.where(take, rows.to(cache.dtype), cache))
        return
    c8 = cache.view(torch.uint8)
    c8.copy_(torch.where(take, kv_quantize(rows, scale).view(torch.uint8), c8))


def _dequant_pair(k_cache: Tensor, v_cache: Tensor, kv_scales, ct: torch.dtype):
    """The caches as the PyTorch paths multiply them: dequantised (:func:`kv_dequantize`) to ``ct`` with
    ``kv_scales``, themselves without."""
    if kv_scales is None:
        return k_cache, v_cache
    return kv_dequantize(k_cache, kv_scales[0], ct), kv_dequantize(v_cache, kv_scales[1], ct)


def _ring_rows(n: Tensor, R: int) -> Tensor:
    """``j(p)`` of the module docstring for int64 limits ``n`` ``[B]`` (>= 1) -> int64 ``[B, R]``: the logical
    row slot ``p`` holds, the largest ``j = p (mod R)`` below ``n``; negative where none was written."""
    p = torch.arange(R, device=n.device)[None, :]
    return n[:, None] - 1 - torch.remainder(n[:, None] - 1 - p, R)


def _ring_kw(window, k_cache: Tensor, T: int = 1) -> dict:
    """The trailing keywords of a rolling call, checked on the host from shapes: a window ``1 <= W <= R``
    (kept as given: ``W == R`` is a window) and ``T <= R - W + 1`` rows appended ahead of the first query."""
    window = _window(window)
    if window is None:
        raise ValueError("rolling=True needs a window")
    if k_cache.dim() == 4:
        R = k_cache.shape[2]
        if window > R:
            raise ValueError(f"rolling=True needs window {window} <= the cache's {R} rows")
        if T > R - window + 1:
            raise ValueError(f"{T} new rows with window {window} need a ring of at least {window + T - 1} rows, "
                             f"not {R}")
    return {"window": window, "rolling": True}


def _append_ring_ref(k_cache: Tensor, v_cache: Tensor, qkv: Tensor, heads: int, positions: Tensor, hkv: int,
                     lengths: Optional[Tensor], kv_scales=None) -> None:
    """The PyTorch path of :func:`kv_cache_append` with ``rolling=True``, seen from the ring: slot ``p`` of
    batch ``b`` takes the one token ``t`` of ``[n_b - R, n_b)`` with ``positions[b] + t = p (mod R)`` if
    ``t >= 0`` and ``positions[b] + t >= 0``, and keeps its bits otherwise (no host sync, no scatter)."""
    B, T, E3 = qkv.shape
    D = E3 // (heads + 2 * hkv)
    R = k_cache.shape[2]
    if T == 0:
        return
    pos = positions.to(torch.int64)
    n = torch.full_like(pos, T) if lengths is None else lengths.to(torch.int64).clamp(1, T)
    t = _ring_rows(pos + n, R) - pos[:, None]  # [B, R]: the largest t = p - pos (mod R) below n_b
    take = ((t >= 0) & (t + pos[:, None] >= 0))[:, None, :, None]
    idx = t.clamp(0, T - 1)[:, :, None, None].expand(B, R, hkv, D)
    kv = qkv[..., heads * D:].reshape(B, T, 2, hkv, D)  # the k | v parts
    for cache, i in ((k_cache, 0), (v_cache, 1)):
        rows = kv[:, :, i].gather(1, idx).permute(0, 2, 1, 3)  # [B, Hkv, R, D]
        _put_rows(cache, take, rows, None if kv_scales is None else kv_scales[i])


def _append_ref(k_cache: Tensor, v_cache: Tensor, qkv: Tensor, heads: int, positions: Tensor,
                hkv: Optional[int] = None, kv_scales=None) -> None:
    """The PyTorch path of :func:`kv_cache_append`: seen from the cache, row j of batch b takes token
    j - positions[b] if that is one of the T tokens and keeps its bits otherwise (no host sync, no
    duplicate scatter indices, out-of-range rows simply have no cache row that asks for them)."""
    B, T, E3 = qkv.shape
    hkv = heads if hkv is None else hkv
    D = E3 // (heads + 2 * hkv)
    cap = k_cache.shape[2]
    t = torch.arange(cap, device=qkv.device)[None, :] - positions.to(torch.int64)[:, None]  # [B, cap]
    take = ((t >= 0) & (t < T))[:, None, :, None]
    idx = t.clamp(0, max(T - 1, 0))[:, :, None, None].expand(B, cap, hkv, D)
    kv = qkv[..., heads * D:].reshape(B, T, 2, hkv, D)  # the k | v parts
    for cache, i in ((k_cache, 0), (v_cache, 1)):
        rows = kv[:, :, i].gather(1, idx).permute(0, 2, 1, 3)  # [B, Hkv, cap, D]
        _put_rows(cache, take, rows, None if kv_scales is None else kv_scales[i])


def _decode_ref(q: Tensor, k_cache: Tensor, v_cache: Tensor, lengths: Tensor, scale: float,
                window: Optional[int] = None, rolling: bool = False, kv_scales=None) -> Tensor:
    """The PyTorch path of :func:`attention_decode` (softmax in fp32, or fp64 for fp64 inputs).  Hidden
    rows -- at or past the length, and below ``len - window`` -- are selected away before either product:
    a masked score is -inf whatever k held, and v is zeroed there because 0 * NaN is NaN.  A cache of
    ``Hkv < H`` heads is grouped-query attention.  ``rolling``: the same over the logical rows ``j(p)`` of the
    ring's slots (module docstring), with the length not clamped to the row count."""
    cap = k_cache.shape[2]
    if rolling:
        n = lengths.to(torch.int64).clamp_min(1)
        j = _ring_rows(n, cap)  # < n by construction
        vis = (j >= 0) & (j >= n[:, None] - window)
    else:
        n = lengths.to(torch.int64).clamp(1, cap)  # the kernels' clamp
        j = torch.arange(cap, device=q.device)[None, :]
        vis = j < n[:, None]
        if window is not None:
            vis = vis & (j >= n[:, None] - window)
    vis = vis[:, None, :]  # [B, 1, cap]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    k_cache, v_cache = _dequant_pair(k_cache, v_cache, kv_scales, ct)  # an fp8 pair: what the queries see
    v = torch.where(vis[..., None], v_cache, torch.zeros((), dtype=v_cache.dtype, device=q.device)).to(ct)
    B, H, D = q.shape
    if k_cache.shape[1] != H:  # query head h reads kv head h // G
        qg = q.to(ct).view(B, k_cache.shape[1], -1, D)
        s = torch.einsum("bkgd,bkjd->bkgj", qg, k_cache.to(ct)) * scale
        p = torch.softmax(s.masked_fill(~vis[:, :, None], float("-inf")), dim=-1)
        return torch.einsum("bkgj,bkjd->bkgd", p, v).reshape(B, H, D).to(q.dtype)
    s = torch.einsum("bhd,bhjd->bhj", q.to(ct), k_cache.to(ct)) * scale
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1)
    return torch.einsum("bhj,bhjd->bhd", p, v).to(q.dtype)


def kv_cache_append(k_cache: Tensor, v_cache: Tensor, qkv: Tensor, heads: int, positions: Tensor, *,
                    kv_heads: Optional[int] = None, rolling: bool = False,
                    lengths: Optional[Tensor] = None,
                    kv_scales: Optional[Tuple[float, float]] = None) -> None:
    """Write the k / v rows of the packed ``qkv`` ``[B, T, (H + 2*Hkv)*D]`` into ``k_cache`` / ``v_cache``
    ``[B, Hkv, cap, D]`` at rows ``positions[b] + t`` (int32 ``[B]``); rows outside ``[0, cap)`` are dropped.
    ``kv_heads``: ``Hkv`` of grouped-query attention (module docstring); ``None`` is ``H``.

    ``rolling=True``: the caches are a ring of ``R = cap`` slots (module docstring) and token ``t`` goes to
    slot ``(positions[b] + t) mod R`` iff ``positions[b] + t >= 0`` and ``n_b - R <= t < n_b``, where ``n_b =
    clamp(lengths[b], 1, T)`` with ``lengths`` (int32 ``[B]``: the valid tokens of a right-padded batch) and
    ``T`` without: the last ``R`` valid rows, no pad rows.  ``lengths`` without ``rolling`` raises
    ``ValueError``.

    ``kv_scales`` (``float8_e4m3fn`` caches only; ``None``: ``(1.0, 1.0)``): the rows are quantised by
    :func:`kv_quantize` with ``k_scale`` / ``v_scale`` as they are stored (module docstring)."""
    if lengths is not None and not rolling:
        raise ValueError("kv_cache_append: lengths needs rolling=True")
    _forward_only(qkv, k_cache, v_cache)
    hkv, B, _, D, _ = _packed_dims(qkv, heads, kv_heads)
    sc = _kv_scales(kv_scales, k_cache, v_cache)
    nkw, skw = _scale_kw(sc)
    if rolling and lengths is not None and (lengths.dtype != torch.int32 or lengths.shape != (B,)
                                            or lengths.device != k_cache.device):
        raise RuntimeError("lengths must be an int32 tensor of shape [B] on the device of the cache")
    with torch.no_grad():
        if _decode_native(qkv, k_cache, v_cache):
            if rolling:
                native().attn_kv_append(_rows(qkv), heads, k_cache, v_cache, positions, hkv, rolling=True,
                                        lengths=None if lengths is None else lengths.contiguous(), **nkw)
                return
            native().attn_kv_append(_rows(qkv), heads, k_cache, v_cache, positions, hkv, **nkw)
            return
        _check_cache(k_cache, v_cache, B, hkv, D, positions, "positions")
        if rolling:
            _append_ring_ref(k_cache, v_cache, qkv, heads, positions, hkv, lengths, **skw)
            return
        _append_ref(k_cache, v_cache, qkv, heads, positions, hkv, **skw)


def _cache_window(window, k_cache: Tensor) -> dict:
    """The ``window`` of a cache function as the trailing keyword of the native calls and of the PyTorch
    paths: ``{}`` -- the calls they always made -- without one or when it can hide nothing (``>= cap``)."""
    window = _window(window, k_cache.shape[2] if k_cache.dim() == 4 else None)
    return {} if window is None else {"window": window}


def attention_decode(q: Tensor, k_cache: Tensor, v_cache: Tensor, lengths: Tensor,
                     scale: Optional[float] = None, *, kv_heads: Optional[int] = None,
                     window: Optional[int] = None, rolling: bool = False,
                     kv_scales: Optional[Tuple[float, float]] = None) -> Tensor:
    """One query per (batch, head): ``q`` ``[B, H, D]`` against the first ``len = clamp(lengths[b], 1, cap)``
    rows of ``k_cache`` / ``v_cache`` ``[B, Hkv, cap, D]`` -> ``[B, H, D]``.  ``kv_heads``: ``Hkv`` of
    grouped-query attention (module docstring); ``None`` is ``H``.  ``window``: only the rows
    ``max(0, len - window) <= j < len`` (module docstring); ``window >= cap`` is ``window=None``.
    ``rolling=True`` (needs ``1 <= window <= cap``): the caches are a ring, ``len = max(lengths[b], 1)`` counts
    tokens and the query sees the slots whose logical row is in the window (module docstring).
    ``kv_scales`` (``float8_e4m3fn`` caches only; ``None``: ``(1.0, 1.0)``): the query sees the visible rows
    dequantised, ``f32(code) * scale`` (module docstring)."""
    _forward_only(q, k_cache, v_cache)
    if q.dim() != 3:
        raise RuntimeError("q must be [B, H, D]")
    B, H, D = q.shape
    hkv = _kv_heads(H, kv_heads)
    wkw = _ring_kw(window, k_cache) if rolling else _cache_window(window, k_cache)
    nkw, skw = _scale_kw(_kv_scales(kv_scales, k_cache, v_cache))
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    with torch.no_grad():
        if _decode_native(q, k_cache, v_cache):
            return native().attn_decode(_rows(q), H, k_cache, v_cache, lengths, 0, scale, None, hkv,
                                        **wkw, **nkw).view(B, H, D)
        _check_cache(k_cache, v_cache, B, hkv, D, lengths, "lengths")
        return _decode_ref(q, k_cache, v_cache, lengths, scale, **wkw, **skw)


def attention_decode_packed(qkv: Tensor, heads: int, k_cache: Tensor, v_cache: Tensor, positions: Tensor,
                            scale: Optional[float] = None, *, fused: bool = False,
                            kv_heads: Optional[int] = None, window: Optional[int] = None,
                            rolling: bool = False,
                            kv_scales: Optional[Tuple[float, float]] = None) -> Tensor:
    """One decode step on the packed ``[B, 1, (H + 2*Hkv)*D]`` projection of the new token: append its k / v
    at row ``positions[b]``, then attend to keys ``j <= positions[b]`` -> ``[B, 1, H*D]``.  ``kv_heads``:
    ``Hkv`` of grouped-query attention (module docstring); ``None`` is ``H``.  ``window``: as
    :func:`attention_decode`, with ``len = clamp(positions[b] + 1, 1, cap)``; the appended row is always
    inside it.

    ``fused=True`` (native path): the append is folded into the split kernel -- the wave whose chunk
    holds row ``positions[b]`` takes it from ``qkv`` and stores it to the cache -- and a cache of a single
    chunk is normalised there too, so a step is one or two launches instead of three.  Output and caches
    have the bits of ``fused=False``.

    ``rolling=True`` (needs ``1 <= window <= cap``): the caches are a ring -- the row goes to slot
    ``positions[b] mod cap`` (dropped when ``positions[b] < 0``) and ``len = max(positions[b] + 1, 1)``.

    ``kv_scales`` (``float8_e4m3fn`` caches only; ``None``: ``(1.0, 1.0)``): the new row is quantised as it is
    stored and the query sees it dequantised like every other row, ``fused`` or not (module docstring)."""
    _forward_only(qkv, k_cache, v_cache)
    hkv, B, _, D, scale = _packed_dims(qkv, heads, kv_heads, scale, T="1")
    wkw = _ring_kw(window, k_cache) if rolling else _cache_window(window, k_cache)
    akw = {"rolling": True} if rolling else {}  # the append's; no ring: the calls it always made
    nkw, skw = _scale_kw(_kv_scales(kv_scales, k_cache, v_cache))
    with torch.no_grad():
        if _decode_native(qkv, k_cache, v_cache):
            qkv, C = _rows(qkv), native()
            if fused:
                return C.attn_decode_append(qkv, heads, k_cache, v_cache, positions, scale,
                                            hkv, **wkw, **nkw).view(B, 1, heads * D)
            C.attn_kv_append(qkv, heads, k_cache, v_cache, positions, hkv, **akw, **nkw)
            return C.attn_decode(qkv, heads, k_cache, v_cache, positions, 1, scale, None,
                                 hkv, **wkw, **nkw).view(B, 1, heads * D)
        _check_cache(k_cache, v_cache, B, hkv, D, positions, "positions")
        if rolling:
            _append_ring_ref(k_cache, v_cache, qkv, heads, positions, hkv, None, **skw)
        else:
            _append_ref(k_cache, v_cache, qkv, heads, positions, hkv, **skw)
        q = qkv[:, 0, :heads * D].reshape(B, heads, D)
        return _decode_ref(q, k_cache, v_cache, positions.to(torch.int64) + 1, scale,
                           **wkw, **skw).reshape(B, 1, heads * D)


def _extend_ref(q: Tensor, k_cache: Tensor, v_cache: Tensor, positions: Tensor, scale: float,
                window: Optional[int] = None, rolling: bool = False, kv_scales=None) -> Tensor:
    """The PyTorch path of :func:`attention_extend` (softmax in fp32, or fp64 for fp64 inputs), sync-free.
    ``q`` ``[B, T, H, D]`` -> ``[B, T, H, D]``.  Scores are masked to -inf by ``L(b, t)``; v is zeroed at
    rows ``>= clamp(positions[b] + T, 1, cap)`` before the product because 0 * NaN is NaN.  Rows between
    a query's limit and that bound (this call's tokens) are multiplied by an exact-zero probability.
    A cache of ``Hkv < H`` heads is grouped-query attention.  ``window``: scores below ``L(b, t) - window``
    are masked as well, and v is also zeroed below the first query's lower limit ``L(b, 0) - window``.
    ``rolling``: the same over the logical rows ``j(p)`` of the ring's slots for the limit ``L(b, T - 1)``
    (module docstring), with no limit clamped to the row count; never-written slots are zeroed too."""
    B, T, H, D = q.shape
    cap = k_cache.shape[2]
    pos = positions.to(torch.int64)
    lim = pos[:, None] + torch.arange(1, T + 1, device=q.device)[None, :]  # L(b, t): [B, T]
    if rolling:
        lim = lim.clamp_min(1)
        j = _ring_rows(lim[:, -1], cap)  # [B, cap], < L(b, T - 1) by construction
        vis = (j[:, None, :] < lim[:, :, None]) & (j[:, None, :] >= lim[:, :, None] - window) & (j[:, None, :] >= 0)
        held = (j >= 0) & (j >= lim[:, :1] - window)
    else:
        lim = lim.clamp(1, cap)
        j = torch.arange(cap, device=q.device)
        vis = j[None, None, :] < lim[:, :, None]  # [B, T, cap]
        held = j[None, :] < (pos + T).clamp(1, cap)[:, None]  # [B, cap]
        if window is not None:
            vis = vis & (j[None, None, :] >= lim[:, :, None] - window)
            held = held & (j[None, :] >= lim[:, :1] - window)
    vis, held = vis[:, None], held[:, None, :, None]  # [B, 1, T, cap], [B, 1, cap, 1]
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    k_cache, v_cache = _dequant_pair(k_cache, v_cache, kv_scales, ct)  # an fp8 pair: what the queries see
    v = torch.where(held, v_cache, torch.zeros((), dtype=v_cache.dtype, device=q.device)).to(ct)
    if k_cache.shape[1] != H:  # query head h reads kv head h // G
        qg = q.to(ct).reshape(B, T, k_cache.shape[1], -1, D)
        s = torch.einsum("btkgd,bkjd->bkgtj", qg, k_cache.to(ct)) * scale
        p = torch.softmax(s.masked_fill(~vis[:, :, None], float("-inf")), dim=-1)
        return torch.einsum("bkgtj,bkjd->btkgd", p, v).reshape(B, T, H, D).to(q.dtype)
    s = torch.einsum("bthd,bhjd->bhtj", q.to(ct), k_cache.to(ct)) * scale
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), dim=-1)
    return torch.einsum("bhtj,bhjd->bthd", p, v).to(q.dtype)


def attention_extend(q: Tensor, k_cache: Tensor, v_cache: Tensor, positions: Tensor,
                     scale: Optional[float] = None, *, kv_heads: Optional[int] = None,
                     window: Optional[int] = None, rolling: bool = False,
                     kv_scales: Optional[Tuple[float, float]] = None) -> Tensor:
    """``T`` queries per (batch, head): ``q`` ``[B, T, H, D]`` (any view with a contiguous last dim), whose
    k / v rows are already in ``k_cache`` / ``v_cache`` ``[B, Hkv, cap, D]`` at rows ``positions[b] + t``.
    Query ``t`` sees rows ``j < clamp(positions[b] + t + 1, 1, cap)`` -> ``[B, T, H, D]``.  ``kv_heads``:
    ``Hkv`` of grouped-query attention (module docstring); ``None`` is ``H``.

    Cache rows at or past ``clamp(positions[b] + T, 1, cap)`` never enter arithmetic; rows between a
    query's own limit and that bound are this call's tokens (real finite data) and may be multiplied by
    an exact-zero probability.  ``window``: query ``t`` sees only the rows at or past ``L(b, t) - window``
    (module docstring, which also says what may enter arithmetic); ``window >= cap`` is ``window=None``.
    ``rolling=True`` (needs ``1 <= window <= cap`` and ``T <= cap - window + 1``): the caches are a ring, the
    rows sit in slots ``(positions[b] + t) mod cap`` and ``L(b, t) = max(positions[b] + t + 1, 1)`` counts
    tokens (module docstring).  ``kv_scales`` (``float8_e4m3fn`` caches only; ``None``: ``(1.0, 1.0)``): the
    queries see the rows dequantised (module docstring)."""
    _forward_only(q, k_cache, v_cache)
    if q.dim() != 4 or q.shape[1] < 1:
        raise RuntimeError("q must be [B, T >= 1, H, D]")
    B, T, H, D = q.shape
    hkv = _kv_heads(H, kv_heads)
    wkw = _ring_kw(window, k_cache, T) if rolling else _cache_window(window, k_cache)
    nkw, skw = _scale_kw(_kv_scales(kv_scales, k_cache, v_cache))
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    with torch.no_grad():
        if _decode_native(q, k_cache, v_cache):
            return native().attn_extend(_rows(q), k_cache, v_cache, positions, scale, None, hkv,
                                        **wkw, **nkw).view(B, T, H, D)
        _check_cache(k_cache, v_cache, B, hkv, D, positions, "positions")
        return _extend_ref(q, k_cache, v_cache, positions, scale, **wkw, **skw)


def attention_extend_packed(qkv: Tensor, heads: int, k_cache: Tensor, v_cache: Tensor, positions: Tensor,
                            scale: Optional[float] = None, *, kv_heads: Optional[int] = None,
                            window: Optional[int] = None, rolling: bool = False,
                            kv_scales: Optional[Tuple[float, float]] = None) -> Tensor:
    """``T`` new tokens on their packed ``[B, T, (H + 2*Hkv)*D]`` projection: append their k / v at rows
    ``positions[b] + t`` (rows outside ``[0, cap)`` are dropped), then query ``t`` attends to rows
    ``j < clamp(positions[b] + t + 1, 1, cap)`` -> ``[B, T, H*D]``.  ``T == 1`` is
    :func:`attention_decode_packed`.  What may enter arithmetic: see :func:`attention_extend`.
    ``kv_heads``: ``Hkv`` of grouped-query attention (module docstring); ``None`` is ``H``.  ``window``: as
    :func:`attention_extend` (``T == 1``: the same window in :func:`attention_decode_packed`).
    ``rolling=True``: the ring of :func:`kv_cache_append` and :func:`attention_extend` (``T <= cap - window +
    1``, or ``ValueError`` before anything is written).  ``kv_scales`` (``float8_e4m3fn`` caches only): as
    :func:`kv_cache_append` and :func:`attention_extend`; every query, a token's own included, sees quantised
    rows."""
    dims = _packed_dims(qkv, heads, kv_heads, scale, T="T >= 1")
    wkw = _ring_kw(window, k_cache, dims[2]) if rolling else _cache_window(window, k_cache)
    akw = {"rolling": True} if rolling else {}  # the append's; no ring: the calls it always made
    sc = _kv_scales(kv_scales, k_cache, v_cache)
    nkw, skw = _scale_kw(sc)
    if dims[2] == 1:
        return attention_decode_packed(qkv, heads, k_cache, v_cache, positions, scale, kv_heads=kv_heads, **wkw,
                                       **skw)
    _forward_only(qkv, k_cache, v_cache)
    hkv, B, T, D, scale = dims
    with torch.no_grad():
        if _decode_native(qkv, k_cache, v_cache):
            qkv, C = _rows(qkv), native()
            C.attn_kv_append(qkv, heads, k_cache, v_cache, positions, hkv, **akw, **nkw)
            q = qkv[..., :heads * D].view(B, T, heads, D)
            return C.attn_extend(q, k_cache, v_cache, positions, scale, None, hkv, **wkw, **nkw)
        _check_cache(k_cache, v_cache, B, hkv, D, positions, "positions")
        if rolling:
            _append_ring_ref(k_cache, v_cache, qkv, heads, positions, hkv, None, **skw)
        else:
            _append_ref(k_cache, v_cache, qkv, heads, positions, hkv, **skw)
        q = qkv[..., :heads * D].reshape(B, T, heads, D)
        return _extend_ref(q, k_cache, v_cache, positions, scale, **wkw, **skw).reshape(B, T, heads * D)


# ---------------------------------------------------------------- rotary position embedding
def rope_table(max_len: int, head_dim: int, base: float = 10000.0, *, device=None,
               dtype: torch.dtype = torch.float32) -> Tensor:
    """The angles of :func:`rope_packed`: ``[max_len, 2, head_dim // 2]``, row ``p`` holding
    ``cos(p * theta_i)`` and then ``sin(p * theta_i)`` with ``theta_i = base ** (-2 * i / head_dim)``.
    Built in float64 on the host and rounded once to ``dtype`` (float32 or float64), so the native
    kernel and the PyTorch path use the same numbers and no device math library's range reduction enters
    at large positions.  Another frequency schedule is another table of this shape."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"rope_table: dtype must be float32 or float64, not {dtype}")
    max_len, head_dim = int(max_len), int(head_dim)
    if max_len < 1 or head_dim < 2 or head_dim % 2:
        raise ValueError(f"rope_table: max_len {max_len} must be >= 1 and head_dim {head_dim} even and >= 2")
    i = torch.arange(head_dim // 2, dtype=torch.float64)
    theta = torch.pow(torch.tensor(float(base), dtype=torch.float64), -2.0 * i / head_dim)
    ang = torch.arange(max_len, dtype=torch.float64)[:, None] * theta[None, :]
    return torch.stack((ang.cos(), ang.sin()), dim=1).to(dtype).to(device)


def _rope_ref(qkv: Tensor, heads: int, hkv: int, table: Tensor, positions: Optional[Tensor], inverse: bool,
              inplace: bool) -> Tensor:
    """The PyTorch path of :func:`rope_packed`: the two formulas in fp32 (fp64 for fp64 inputs), one
    rounding, the kernel's clamp, no host sync."""
    B, T, E = qkv.shape
    hr = heads + hkv
    D = E // (hr + hkv)
    at = torch.arange(T, device=qkv.device)[None, :]
    if positions is not None:
        at = positions.to(torch.int64)[:, None] + at
    cs = table[at.clamp(0, table.shape[0] - 1)]  # [B | 1, T, 2, D / 2]
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    c, s = cs[:, :, 0, None, :].to(ct), cs[:, :, 1, None, :].to(ct)
    if inverse:
        s = -s
    x = qkv[..., :hr * D].reshape(B, T, hr, D).to(ct)
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    y = torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1).to(qkv.dtype).reshape(B, T, hr * D)
    if inplace:
        qkv[..., :hr * D].copy_(y)
        return qkv
    return torch.cat((y, qkv[..., hr * D:]), dim=-1)


def _rope_apply(qkv: Tensor, heads: int, hkv: int, table: Tensor, positions: Optional[Tensor], inverse: bool,
                inplace: bool) -> Tensor:
    D = qkv.shape[2] // (heads + 2 * hkv)
    if (qkv.is_cuda and qkv.dtype == torch.bfloat16 and D == 64 and table.dtype == torch.float32
            and use_native(qkv)):
        table = table.contiguous()
        pos = None if positions is None else positions.contiguous()
        if _rows_ok(qkv):
            return native().rope_packed(qkv, heads, table, pos, hkv, inverse, qkv if inplace else None)
        y = native().rope_packed(qkv.contiguous(), heads, table, pos, hkv, inverse, None)
        if inplace:  # the rotated part alone goes back: the value part is not touched
            w = (heads + hkv) * D
            qkv[..., :w].copy_(y[..., :w])
            return qkv
        return y
    return _rope_ref(qkv, heads, hkv, table, positions, inverse, inplace)


class _RopeFn(torch.autograd.Function):
    """The rotation is orthogonal: its gradient is the inverse rotation of the incoming gradient."""

    @staticmethod
    def forward(ctx, qkv, heads, hkv, table, positions, inverse):
        ctx.save_for_backward(table, positions)
        ctx.cfg = (heads, hkv, inverse)
        return _rope_apply(qkv, heads, hkv, table, positions, inverse, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        table, positions = ctx.saved_tensors
        heads, hkv, inverse = ctx.cfg
        return _rope_apply(g, heads, hkv, table, positions, not inverse, False), None, None, None, None, None


def rope_packed(qkv: Tensor, heads: int, table: Tensor, positions: Optional[Tensor] = None, *,
                kv_heads: Optional[int] = None, inverse: bool = False, inplace: bool = False) -> Tensor:
    """Rotary position embedding of a packed projection: ``qkv`` ``[B, T, (H + 2*Hkv)*D]`` -> the same shape,
    the ``H`` query heads and the ``Hkv`` key heads rotated, the value part copied bit for bit (with
    ``inplace=True`` the result is ``qkv`` itself and the value part is not touched at all).

    Rotate-half (GPT-NeoX / Llama) layout: for a head vector ``x`` of even length ``D`` at position ``p``,
    with ``c`` / ``s`` row ``p`` of ``table`` (``[max_len, 2, D // 2]``, :func:`rope_table`),
    ``y[i] = x[i] * c - x[i + D/2] * s`` and ``y[i + D/2] = x[i + D/2] * c + x[i] * s``; ``inverse=True``
    uses ``-s``, the transpose of the rotation and therefore its gradient.  Token ``t`` of batch ``b`` is at
    position ``clamp((positions[b] if given else 0) + t, 0, max_len - 1)`` -- the rule of
    ``ops.linear.embed_rows``: a bad position never becomes an address.  ``positions`` is an int32 ``[B]``
    tensor on the device of ``qkv``, read on the device: no host sync, safe inside a graph capture, a
    replay follows in-place changes.  ``kv_heads``: ``Hkv`` of grouped-query attention; ``None`` is ``H``.

    Native path (csrc/rope.hip, one launch): CUDA bf16, ``D == 64``, a float32 table on the same device; a
    view that is not 16-B aligned with row strides in multiples of 8 goes through ``.contiguous()``.
    Everything else -- CPU, other dtypes, another even ``D``, ``TBAMD_FORCE_REFERENCE=1`` -- is the PyTorch
    path: the same formulas in fp32 (fp64 for fp64 inputs) and the same clamp.

    Out of place it is differentiable w.r.t. ``qkv``: the gradient is ``rope_packed(grad, ...,
    inverse=not inverse)``, a new tensor; the table and the positions get none.  ``inplace=True`` is
    forward-only and raises if ``qkv`` requires grad in grad mode."""
    hkv, B, _, D, _ = _packed_dims(qkv, heads, kv_heads, even=True)
    if table.dim() != 3 or table.shape[1] != 2 or table.shape[2] != D // 2 or table.shape[0] < 1:
        raise RuntimeError(f"table must be [max_len, 2, D // 2 = {D // 2}], not {tuple(table.shape)}")
    if table.device != qkv.device:
        raise RuntimeError("table must be on the device of qkv")
    if positions is not None and (positions.dtype != torch.int32 or positions.shape != (B,)
                                  or positions.device != qkv.device):
        raise RuntimeError("positions must be an int32 tensor of shape [B] on the device of qkv")
    if inplace:
        if torch.is_grad_enabled() and qkv.requires_grad:
            raise RuntimeError("rope_packed(inplace=True) is forward-only: call it under torch.no_grad() or "
                               "detach the input")
        with torch.no_grad():
            return _rope_apply(qkv, heads, hkv, table, positions, bool(inverse), True)
    if torch.is_grad_enabled() and qkv.requires_grad:
        return _RopeFn.apply(qkv, heads, hkv, table, positions, bool(inverse))
    with torch.no_grad():
        return _rope_apply(qkv, heads, hkv, table, positions, bool(inverse), False)
