"""Decoder-only transformer language model (GPT-2 layout) on the ViT blocks.

Not part of the reference (it has no attention model): the text-side counterpart
of ``models/vit.py`` for the reference's torchtext / HF text loaders.  Token
embedding plus a learned position embedding, the pre-norm :class:`~torchbooster_amd.models.vit.Block`
with ``causal=True`` -- the fused residual LayerNorm, ``LinearGELU`` / ``GeluLink`` MLP and the native
causal attention kernels, which skip the key tiles above the diagonal (csrc/attention.hip) -- a final
LayerNorm and an untied, bias-free vocabulary projection.

``forward(tokens, lengths=None)``: ``tokens`` is an integer ``[B, N]`` tensor, ``lengths`` an optional
int32 ``[B]`` tensor of the valid tokens per sequence of a right-padded batch (clamped into ``[1, N]``
by the attention, ops/attention.py).  Logits are returned for every position, padded ones included:
the caller masks their loss.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from torchbooster_amd.models.vit import Block
from torchbooster_amd.ops.linear import Linear
from torchbooster_amd.ops.norm import LayerNorm

__all__ = ["TransformerLM", "gpt_tiny", "gpt2_small"]


class TransformerLM(nn.Module):
    def __init__(self, vocab: int, dim: int, depth: int, heads: int, max_len: int, mlp_ratio: float = 4.0) -> None:
        super().__init__()
        self.max_len = max_len
        self.tok = nn.Embedding(vocab, dim)
        self.pos = nn.Parameter(torch.zeros(1, max_len, dim))
        self.blocks = nn.ModuleList([Block(dim, heads, mlp_ratio, causal=True) for _ in range(depth)])
        self.norm = LayerNorm(dim, eps=1e-6)
        self.head = Linear(dim, vocab, bias=False)
        nn.init.normal_(self.tok.weight, std=0.02)
        nn.init.normal_(self.pos, std=0.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, tokens: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
        """[B, N] token ids -> [B, N, vocab] logits."""
        B, N = tokens.shape
        if N > self.max_len:
            raise ValueError(f"sequence length {N} exceeds max_len {self.max_len}")
        x = self.tok(tokens) + self.pos[:, :N].to(self.tok.weight.dtype)
        pending = None
        for blk in self.blocks:
            x, pending = blk(x, pending, lengths)
        h, _ = self.norm(x, pending)
        return self.head(h)


def gpt_tiny(vocab: int = 256, max_len: int = 128) -> TransformerLM:
    return TransformerLM(vocab, 128, 2, 2, max_len)


def gpt2_small(vocab: int = 50257, max_len: int = 1024) -> TransformerLM:
    return TransformerLM(vocab, 768, 12, 12, max_len)
