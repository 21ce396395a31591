"""Fused softmax cross-entropy (+ label smoothing) with batch accuracy.

Reference call sites: ``cross_entropy(logits, labels, label_smoothing=...)``
followed by ``metrics.accuracy(logits, labels)``
(/root/reference/examples/img_cls/resnet/resnet.py:61-62,
/root/reference/torchbooster/metrics.py:11-27).  One HIP kernel computes both
(csrc/loss.hip); SURVEY.md §2.3.1 K9/K10.

``linear_cross_entropy(x, weight, labels)`` is the language-model head: the vocabulary projection
``x weightᵀ`` and the cross entropy of its rows in one op that never holds the ``[tokens, vocab]``
logits.  Forward: a GEMM whose epilogue reduces each logits tile to (max, Σ exp) per row
(csrc/gemm.hip ``kEpiLse``) and a merge over the column tiles (csrc/loss.hip).  Backward: the same
GEMM over one vocabulary slice at a time, its epilogue writing the slice's logits gradient
(``kEpiDlogits``) into a reused chunk buffer that feeds the weight- and input-gradient GEMMs.  Any
vocabulary size runs without padding or copying the weight.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable
import torch.nn.functional as F
from torch import Tensor

from torchbooster_amd.ops import gemm as G
from torchbooster_amd.ops._ext import native, slot_alias, take_slot, use_native

__all__ = ["cross_entropy", "cross_entropy_accuracy", "linear_cross_entropy"]


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, smoothing, ignore_index):
        C = native()
        stats, lse = C.ce_forward(logits, labels, smoothing, ignore_index)
        ctx.save_for_backward(logits, labels, lse, stats)
        ctx.cfg = (smoothing, ignore_index)
        loss = stats[0]
        acc = stats[1]
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss, gacc):
        C = native()
        logits, labels, lse, stats = ctx.saved_tensors
        smoothing, ignore_index = ctx.cfg
        if gloss is None:
            return None, None, None, None
        dl = C.ce_backward(logits, labels, lse, gloss.reshape(1), stats, smoothing, ignore_index)
        return dl, None, None, None


def cross_entropy_accuracy(logits: Tensor, labels: Tensor, label_smoothing: float = 0.0,
                           ignore_index: int = -100) -> Tuple[Tensor, Tensor]:
    """Mean cross-entropy and batch accuracy (``(argmax == label).sum() / N``)."""
    if use_native(logits) and logits.dim() == 2 and labels.dim() == 1:
        return _CEFn.apply(logits, labels, float(label_smoothing), int(ignore_index))
    loss = F.cross_entropy(logits.float(), labels, ignore_index=ignore_index, label_smoothing=label_smoothing)
    with torch.no_grad():
        acc = (logits.argmax(dim=-1) == labels).sum() / logits.size(0)
    return loss, acc


def cross_entropy(logits: Tensor, labels: Tensor, label_smoothing: float = 0.0,
                  ignore_index: int = -100) -> Tensor:
    return cross_entropy_accuracy(logits, labels, label_smoothing, ignore_index)[0]


# Bytes of the backward's [M, chunk] bf16 logits-gradient buffer when ``chunk`` is not given.
# scripts/bench_lm_loss.py sweeps 64 / 256 / 1024 MiB (profiles/lm_loss/README.md): at 8192 rows 64 and
# 256 MiB are within 2 % of each other in time (each wins one vocabulary size), 1024 MiB is slower,
# and 64 MiB holds half the memory of 256.
_CHUNK_BUDGET = 64 << 20


def _default_chunk(M: int, tile_q: int, budget: int = _CHUNK_BUDGET) -> int:
    """The widest multiple of the column tile whose [M, chunk] bf16 buffer stays under ``budget``."""
    return max(tile_q, budget // (2 * max(M, 1)) // tile_q * tile_q)


class _LinearCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, w, labels, ignore_index, chunk):
        stats, lse = native().lm_loss_forward(x2, w, labels, ignore_index)
        ctx.save_for_backward(x2, w, labels, lse, stats)
        ctx.wparam = w
        ctx.cfg = (ignore_index, chunk)
        return stats[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss):
        C = native()
        x2, w, labels, lse, stats = ctx.saved_tensors
        ignore_index, chunk = ctx.cfg
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gloss is None or not (need_dx or need_dw):
            return None, None, None, None, None
        M, D = x2.shape
        V = w.shape[0]
        g = gloss.to(torch.float32).reshape(1)
        tq = int(C.lm_loss_tile_q())
        chunk = _default_chunk(M, tq) if chunk is None else max(tq, -(-int(chunk) // tq) * tq)
        chunk = min(chunk, -(-V // tq) * tq)
        flat = torch.empty(M * min(chunk, G._r8(V)), dtype=x2.dtype, device=x2.device)  # the one chunk buffer
        dw = slot = None
        if need_dw:
            slot = take_slot(ctx.wparam)
            if slot is not None and not (slot.dtype == w.dtype and slot.is_contiguous() and slot.shape == w.shape):
                slot = None
            dw = slot if slot is not None else torch.empty_like(w)
        dx = acc = None
        for v0 in range(0, V, chunk):
            v1 = min(V, v0 + chunk)
            ld = G._r8(v1 - v0)
            d = flat[:M * ld].view(M, ld)
            C.lm_loss_dlogits(x2, w, labels, lse, stats, g, v0, v1, ignore_index, d)
            # whole groups of 8 columns, then (last chunk of a vocabulary that is no multiple of 8) the
            # group holding the last < 8 columns and the buffer's zeroed pad columns: only those few
            # weight rows are ever padded
            a8 = v0 + (v1 - v0) // 8 * 8
            for c0, c1 in ((v0, a8), (a8, v1)):
                if c0 == c1:
                    continue
                dc = d[:, c0 - v0:c0 - v0 + G._r8(c1 - c0)]
                if need_dw:
                    # rows [c0, c1) of dW are a contiguous block of the [V, D] gradient, written exactly once
                    if c1 - c0 == dc.shape[1]:
                        G.mm_tn(dc, x2, out=dw[c0:c1])
                    else:
                        dw[c0:c1].copy_(G.mm_tn(dc, x2)[:c1 - c0])
                if need_dx:
                    part = G.mm_nn(dc, w[c0:c1])
                    if dx is None:
                        dx = part
                    elif acc is None:
                        acc = dx.float().add_(part)
                    else:
                        acc.add_(part)
        if acc is not None:  # several partial products: summed in f32, rounded once
            dx = acc.to(x2.dtype)
        if need_dw and slot is not None:
            dw = slot_alias(slot)
        return dx, dw, None, None, None


def linear_cross_entropy(x: Tensor, weight: Tensor, labels: Tensor, ignore_index: int = -100, *,
                         chunk: Optional[int] = None) -> Tensor:
    """Mean cross entropy of the rows of ``x weightᵀ`` (``x`` ``[..., D]``, ``weight`` ``[V, D]``, integer
    ``labels`` ``[...]``) over the valid rows, as an f32 scalar.  A row whose label is ``ignore_index`` or
    outside ``[0, V)`` is ignored; with no valid row the loss is NaN.  ``chunk``: vocabulary columns per
    backward pass (rounded up to the kernel's column tile; default: a 64 MiB buffer)."""
    D, V = x.shape[-1], weight.shape[0]
    ignore_index = int(ignore_index)
    if (use_native(x) and weight.is_cuda and labels.is_cuda and x.dtype == weight.dtype == torch.bfloat16
            and D % 8 == 0 and V > 0 and x.numel() > 0 and not torch.is_autocast_enabled("cuda")):
        x2 = G._rows(x)
        w = weight if weight.is_contiguous() and weight.data_ptr() % 16 == 0 else weight.contiguous()
        y = labels.reshape(-1).to(torch.int64).contiguous()
        return _LinearCEFn.apply(x2, w, y, ignore_index, chunk)
    y = labels.reshape(-1).to(torch.int64)
    y = torch.where((y < 0) | (y >= V), torch.full_like(y, ignore_index), y)
    logits = F.linear(x, weight).float()
    return F.cross_entropy(logits.reshape(-1, V), y, ignore_index=ignore_index)
