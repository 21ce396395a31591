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
the caller masks their loss.  ``features`` stops before the vocabulary projection, and ``loss`` trains
through the fused head (ops/loss.py ``linear_cross_entropy``), which masks the padded positions itself
and never stores the logits.

Generation (forward only, ``torch.no_grad()``): :class:`KVCache` holds the keys and values of every
layer and ``prefill`` runs the prompt once and fills it.  Every step after that is ONE body, ``_step``:
``extend`` runs T >= 1 new tokens per sequence on top of what the cache holds (csrc/attention_extend.hip;
one token: the split-KV decode kernels of csrc/attention_decode.hip), and ``decode_step(token, cache)`` is
``extend(token[:, None], cache, last_only=True)`` bit for bit.  Nothing in a step reads a device value on
the host -- positions and lengths live in device memory -- so a step can be captured into a graph and
replayed.  ``generate`` ties prefill and steps to greedy / temperature / top-k sampling
(``graph=True``: replayed steps), continues a conversation (``cache=...``) and decodes speculatively
(``draft=...``: the target scores a draft's proposals in one ``extend`` per round).

Fused decoding (``fused=True`` on ``decode_step`` / ``extend`` / ``generate``, off by default): the same
step on the few-row kernels -- ``embed_rows``, then per layer ``Block.forward_rows`` (LayerNorm, bias,
GELU and residual folded into four ``linear_rows`` products, the cache append folded into the decode
attention), then the final LayerNorm as the prologue of the vocabulary product.  ``embed_rows`` clamps a
token id outside ``[0, vocab)`` into range, the one difference from the default path.

Grouped-query attention (``TransformerLM(..., kv_heads=Hkv)``, ``Hkv`` dividing ``heads``): the
``heads`` query heads of every layer share ``Hkv`` key / value heads (``Hkv = 1`` is multi-query
attention), so a :class:`KVCache` layer is ``[B, Hkv, capacity, hd]`` -- ``heads // Hkv`` times smaller,
and as many times fewer bytes per decode step, which the decode kernel reads once for the heads that
share them (ops/attention.py).  Everything above works unchanged in meaning, including a
``generate(draft=)`` whose two models differ in ``kv_heads``.  ``kv_heads=None`` is ``heads``.

Rotary position embeddings (``TransformerLM(..., pos="rope", rope_base=10000.0)``): there is no learned
position table -- no ``pos`` parameter -- the token embedding alone feeds the first block, and every
layer rotates the q and k parts of its packed projection by the token's position (rotate-half layout,
``ops.attention.rope_packed``, csrc/rope.hip) before any attention path reads it.  A token is at position
``t`` in ``features`` / ``forward`` / ``loss`` / ``prefill`` and at ``cache.positions[b] + t`` in a step
(``decode_step`` / ``extend``), on the default and on the fused path, hence under
``generate`` with ``graph=True``, ``cache=`` and ``draft=`` (whose two models may differ in ``pos``).  A
:class:`KVCache` is unchanged and holds rotated keys; ``max_len`` stays the capacity limit and is the
length of the angle table, which one :class:`~torchbooster_amd.models.vit.Rope` per model owns outside
the parameters and buffers.  ``pos="learned"`` (the default) is everything above unchanged.

Llama-style blocks (``TransformerLM(..., norm="rms", mlp="swiglu", bias=False)``, each option on its own
too): ``norm="rms"`` makes every norm, the final one included, an RMSNorm (``ops.norm.RMSNorm``, the RMS
instantiation of the LayerNorm row kernels); ``mlp="swiglu"`` makes every MLP the gated SiLU
``fc2(silu(gate) * up)`` with ``gate | up`` from one ``Linear(dim, 2 * int(dim * mlp_ratio))``
(``ops.act.swiglu``, csrc/swiglu.hip; ``mlp_ratio=8/3`` has the parameters of a 4x GELU MLP); ``bias=False``
drops the biases of ``qkv``, ``proj`` and the MLP linears (``head`` never had one).  With ``pos="rope"`` and
``kv_heads`` that is the Llama / Mistral / Qwen decoder on every path above: the fused step runs the
RMSNorm as the ``rms=`` prologue and the gate as the ``act="swiglu"`` epilogue of ``linear_rows``, the same
number of launches per layer.  The defaults (``"layer"``, ``"gelu"``, ``True``) are everything above unchanged.

Sliding-window attention (``TransformerLM(..., window=W)``): a token sees itself and the ``W - 1`` tokens
before it (ops/attention.py states the rule for pad rows and the cache paths) in every layer, or, with a
sequence of ``depth`` entries, each ``None`` or an int, per layer -- alternating local / global layers
(Mistral, Gemma 2 / 3, gpt-oss).  Training skips the key tiles left of the window, a decode step streams
at most ``W`` cache rows per layer whatever the context, and ``prefill`` / ``decode_step`` / ``extend`` /
``generate`` (``graph=True``, ``cache=``, ``fused=True``, ``draft=`` -- whose two models may differ in
``window``) keep their meaning.  A :class:`KVCache` is by default unchanged: full capacity, rows never
recycled.  ``window=None`` (the default) is everything above unchanged.

Rolling KV cache (``KVCache(..., rolling=True, lookahead=16)``, ``generate(..., rolling=True)``): a layer with
a window ``W`` keeps ``R = roundup8(W + lookahead - 1)`` rows instead of ``capacity`` (when that is fewer) and
uses them as a ring -- logical row ``j`` lives in slot ``j mod R``, ``cache.positions`` keep counting tokens
(ops/attention.py states the rule) -- so a windowed layer costs ``O(W)`` memory and ``O(W)`` work per step at
any context length, and computes what the linear cache computes.  Layers without a window stay linear
(``cache.rolling[i]`` tells), so local / global alternation mixes both in one cache.  ``prefill`` of a prompt
longer than ``R`` keeps each sequence's last ``R`` valid rows; ``decode_step`` and ``generate`` (``graph=True``,
``fused=True``, ``cache=``, ``draft=``) run at any length up to ``capacity``; ``extend`` takes at most
``lookahead`` tokens per call on such a cache (``ValueError`` beyond: a ring has room for ``R - W + 1`` new
rows ahead of the first query; feeding more by chunking is left to the caller).  ``rolling=False`` (the
default) is everything above unchanged.

FP8 KV cache (``KVCache(..., dtype=torch.float8_e4m3fn, scales=None)``, ``generate(..., kv_dtype=, kv_scales=)``):
the cache holds e4m3 codes, half the bytes of bf16, with two host floats ``(k_scale, v_scale)`` per layer
(``cache.scales``; :func:`kv_scales` calibrates them on a prompt).  Rows are quantised as they are appended and
every query sees them dequantised -- a step's own row included, so ``fused=True`` keeps the bits of ``fused=False`` --
while ``prefill`` attends to its own unquantised projection (ops/attention.py states the rule).  It composes with
``kv_heads``, ``window`` and ``rolling`` and with every ``generate`` option above; any other cache dtype adds nothing
to any call.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from torchbooster_amd.models.vit import Block, Rope, make_norm, norm_args
from torchbooster_amd.ops.attention import _check_scale
from torchbooster_amd.ops.linear import Linear, embed_rows, linear_rows
from torchbooster_amd.ops.loss import linear_cross_entropy

__all__ = ["TransformerLM", "KVCache", "kv_scales", "gpt_tiny", "gpt2_small"]

_FP8 = torch.float8_e4m3fn


def _layer_scales(scales, depth: int) -> List[Tuple[float, float]]:
    """``scales`` of :class:`KVCache` as ``depth`` checked ``(k_scale, v_scale)`` pairs."""
    def pair(p) -> Tuple[float, float]:
        try:
            k, v = p
        except (TypeError, ValueError):
            raise ValueError(f"a KV-cache scale entry must be a (k_scale, v_scale) pair, not {p!r}") from None
        return (_check_scale(k), _check_scale(v))

    if scales is None:
        return [(1.0, 1.0)] * depth
    scales = list(scales)
    if len(scales) == 2 and all(isinstance(x, (int, float)) for x in scales):
        return [pair(scales)] * depth
    if len(scales) != depth:
        raise ValueError(f"scales has {len(scales)} entries, the model {depth} layers")
    return [pair(p) for p in scales]


class KVCache:
    """Per-layer keys and values of a :class:`TransformerLM` for ``batch`` sequences of up to ``capacity``
    tokens (default and upper limit: the model's ``max_len``).

    ``layers[i]`` is the ``(k, v)`` pair of block ``i``, each ``[B, kv_heads, capacity, hd]`` and uninitialised
    (``torch.empty``): rows at or past a sequence's position never enter arithmetic (ops/attention.py).
    ``positions`` (int32 ``[B]``) is the row each sequence writes next = the number of tokens it holds.

    ``rolling=True``: a layer whose window is ``W`` gets ``R = roundup8(W + lookahead - 1)`` rows if that is
    below ``capacity`` and is used as a ring (module docstring): ``rolling[i]`` is then ``True`` and
    ``layers[i]`` a ``[B, kv_heads, R, hd]`` pair.  A layer without a window, or with ``R >= capacity``, is
    exactly the linear layer it is without ``rolling`` (``rolling[i]`` ``False``).  ``capacity`` keeps its
    meaning -- logical tokens, ``<= max_len`` -- and ``lookahead`` (>= 1) is the most tokens one ``extend``
    may feed.  Bytes: ``sum_i 2 * B * kv_heads * rows_i * hd * itemsize``.

    ``dtype=torch.float8_e4m3fn``: an fp8 cache (ops/attention.py: rows are quantised as they are appended and
    every query sees them dequantised), half the bytes of bf16.  ``scales``: ``None`` (1.0 everywhere), one
    ``(k_scale, v_scale)`` pair for every layer or a sequence of ``depth`` pairs (:func:`kv_scales` calibrates
    them); host floats, finite and ``> 0``.  ``cache.scales`` is the list of ``depth`` pairs, or of ``depth``
    ``None`` for any other dtype, with which ``scales`` raise ``ValueError``."""

    def __init__(self, model: "TransformerLM", batch: int, capacity: Optional[int] = None, dtype=None,
                 device=None, *, rolling: bool = False, lookahead: int = 16, scales=None) -> None:
        capacity = model.max_len if capacity is None else int(capacity)
        if not 1 <= capacity <= model.max_len:
            raise ValueError(f"capacity {capacity} must be in [1, max_len = {model.max_len}]")
        lookahead = int(lookahead)
        if lookahead < 1:
            raise ValueError(f"lookahead {lookahead} must be at least 1")
        w = model.tok.weight
        dtype = w.dtype if dtype is None else dtype
        device = w.device if device is None else device
        if dtype == _FP8:
            self.scales: List[Optional[Tuple[float, float]]] = _layer_scales(scales, len(model.blocks))
        elif scales is not None:
            raise ValueError(f"scales need dtype=torch.float8_e4m3fn, not {dtype}")
        else:
            self.scales = [None] * len(model.blocks)
        attn = model.blocks[0].attn
        self.capacity = capacity
        self.lookahead = lookahead
        rows = [capacity] * len(model.blocks)
        if rolling:
            for i, blk in enumerate(model.blocks):
                if blk.attn.window is not None:
                    rows[i] = min(capacity, (blk.attn.window + lookahead - 1 + 7) // 8 * 8)
        self.rolling: List[bool] = [r < capacity for r in rows]
        self.layers: List[Tuple[Tensor, Tensor]] = [
            (torch.empty(batch, attn.kv_heads, r, attn.hd, dtype=dtype, device=device),
             torch.empty(batch, attn.kv_heads, r, attn.hd, dtype=dtype, device=device))
            for r in rows]
        self.positions = torch.zeros(batch, dtype=torch.int32, device=device)

    def reset(self) -> None:
        self.positions.zero_()


def _sample(logits: Tensor, temperature: float, top_k: Optional[int], generator) -> Tensor:
    """[B, vocab] logits -> [B] token ids: argmax at temperature 0, else a draw from
    softmax(logits / temperature) restricted to the top_k logits."""
    if temperature == 0:
        return logits.argmax(dim=-1)
    z = logits.float() / temperature
    if top_k is not None:
        kth = z.topk(min(int(top_k), z.shape[-1]), dim=-1).values[:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    return torch.multinomial(torch.softmax(z, dim=-1), 1, generator=generator)[:, 0]


class TransformerLM(nn.Module):
    def __init__(self, vocab: int, dim: int, depth: int, heads: int, max_len: int, mlp_ratio: float = 4.0,
                 kv_heads: Optional[int] = None, *, pos: str = "learned", rope_base: float = 10000.0,
                 norm: str = "layer", mlp: str = "gelu", bias: bool = True,
                 window: Union[None, int, Sequence[Optional[int]]] = None) -> None:
        super().__init__()
        if pos not in ("learned", "rope"):
            raise ValueError(f"pos must be 'learned' or 'rope', not {pos!r}")
        if window is None or isinstance(window, int):
            windows = [window] * depth
        elif isinstance(window, (str, bytes)) or not hasattr(window, "__iter__"):
            raise ValueError(f"window must be None, an int >= 1 or a sequence of {depth} such entries, not {window!r}")
        else:
            windows = list(window)
            if len(windows) != depth:
                raise ValueError(f"window has {len(windows)} entries, the model {depth} layers")
        self.max_len = max_len
        self.tok = nn.Embedding(vocab, dim)
        # learned: a [1, max_len, dim] table added to the token embedding; rope: none, the layers rotate q / k
        self.rope = Rope(max_len, dim // heads, rope_base) if pos == "rope" else None
        self.pos = nn.Parameter(torch.zeros(1, max_len, dim)) if self.rope is None else None
        kw = {} if self.rope is None else {"rope": self.rope}  # learned: the calls it always made
        if (norm, mlp, bias) != ("layer", "gelu", True):  # likewise the GPT-2 block
            kw.update(norm=norm, mlp=mlp, bias=bias)
        # (no window: the calls it always made)
        self.blocks = nn.ModuleList([Block(dim, heads, mlp_ratio, causal=True, kv_heads=kv_heads, **kw,
                                           **({} if w is None else {"window": w})) for w in windows])
        self.norm = make_norm(norm, dim)
        self.head = Linear(dim, vocab, bias=False)
        nn.init.normal_(self.tok.weight, std=0.02)
        if self.pos is not None:
            nn.init.normal_(self.pos, std=0.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def features(self, tokens: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
        """[B, N] token ids -> [B, N, dim], the output of the final norm (the input of ``head``)."""
        B, N = tokens.shape
        if N > self.max_len:
            raise ValueError(f"sequence length {N} exceeds max_len {self.max_len}")
        x, pending = self._embed(tokens), None
        for blk in self.blocks:
            x, pending = blk(x, pending, lengths)
        h, _ = self.norm(x, pending)
        return h

    def forward(self, tokens: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
        """[B, N] token ids -> [B, N, vocab] logits."""
        return self.head(self.features(tokens, lengths))

    def loss(self, tokens: Tensor, lengths: Optional[Tensor] = None, targets: Optional[Tensor] = None, *,
             ignore_index: int = -100) -> Tensor:
        """Mean next-token cross entropy of ``tokens`` ``[B, N]`` as an f32 scalar, through the fused head
        (ops/loss.py ``linear_cross_entropy``): no ``[B, N, vocab]`` logits are stored.

        ``targets`` ``[B, N]`` are used as given (``ignore_index`` entries do not count).  Without them
        ``targets[b, t] = tokens[b, t + 1]`` where ``t + 1 < clamp(lengths[b], 1, N)`` (``< N`` without
        ``lengths``) and ``ignore_index`` elsewhere, built on the device without a sync: the last position
        is always ignored, so all ``B * N`` rows go through the head without a slice copy."""
        B, N = tokens.shape
        if targets is None:
            if N < 2:
                raise ValueError("loss needs at least 2 tokens per sequence to form next-token targets")
            nxt = torch.roll(tokens, -1, dims=1).to(torch.int64)
            t1 = torch.arange(1, N + 1, device=tokens.device)
            end = N if lengths is None else lengths.to(torch.int64).clamp(1, N)[:, None]
            targets = torch.where(t1 < end, nxt, torch.full_like(nxt, ignore_index))
        elif targets.shape != tokens.shape:
            raise ValueError(f"targets {tuple(targets.shape)} must have the shape of tokens {tuple(tokens.shape)}")
        return linear_cross_entropy(self.features(tokens, lengths), self.head.weight, targets, ignore_index)

    # ---------------------------------------------------------------- generation (forward only)
    def prefill(self, tokens: Tensor, lengths: Optional[Tensor] = None,
                cache: Optional[KVCache] = None) -> Tuple[Tensor, KVCache]:
        """Run the prompt ``[B, N]`` once (causal, ``key_lengths=lengths``) and fill ``cache`` (a fresh
        full-size one by default) from row 0.  Returns the logits ``[B, vocab]`` of each sequence's last
        valid token -- position ``lengths[b] - 1``, or ``N - 1`` -- and the cache, whose ``positions`` are
        now the (clamped) lengths: the pad rows of a ragged batch are overwritten as each sequence grows."""
        B, N = tokens.shape
        if N > self.max_len:
            raise ValueError(f"sequence length {N} exceeds max_len {self.max_len}")
        with torch.no_grad():
            if cache is None:
                cache = KVCache(self, B)
            if N > cache.capacity:
                raise ValueError(f"prompt length {N} exceeds the cache capacity {cache.capacity}")
            cache.positions.zero_()
            x, pending = self._embed(tokens), None
            # the masked self-attention plus one append per layer
            for blk, kv, ring, sc in zip(self.blocks, cache.layers, cache.rolling, cache.scales):
                if sc is not None:  # an fp8 layer: the append quantises
                    x, pending = blk(x, pending, lengths, cache=kv, positions=cache.positions,
                                     **({"rolling": True} if ring else {}), kv_scales=sc)
                elif ring:  # the ring append: the last R valid rows of each sequence
                    x, pending = blk(x, pending, lengths, cache=kv, positions=cache.positions, rolling=True)
                else:
                    x, pending = blk(x, pending, lengths, cache=kv, positions=cache.positions)
            if lengths is None:
                cache.positions.fill_(N)
            else:
                cache.positions.copy_(lengths.clamp(1, N))
            x, pending = self._last_rows(x, pending, None if lengths is None else cache.positions, N)
            return self._logits(x, pending)[:, 0], cache

    def _embed(self, tokens: Tensor, positions: Optional[Tensor] = None) -> Tensor:
        """Token rows ``[B, T, dim]`` plus, with ``pos="learned"``, the learned position rows: ``0 .. T - 1``,
        or ``clamp(positions[b] + t, 0, max_len - 1)`` with ``positions`` (int32 ``[B]``)."""
        if self.pos is None:
            return self.tok(tokens)
        T, dtype = tokens.shape[1], self.tok.weight.dtype
        if positions is None:
            return self.tok(tokens) + self.pos[:, :T].to(dtype)
        at = positions.to(torch.int64)
        if T == 1:  # a decode step: one index_select, no arange and no advanced index
            at = at.clamp(0, self.max_len - 1)
            return self.tok(tokens) + self.pos[0].index_select(0, at).to(dtype)[:, None]
        at = at[:, None] + torch.arange(T, device=tokens.device)[None, :]
        return self.tok(tokens) + self.pos[0][at.clamp(0, self.max_len - 1)].to(dtype)

    @staticmethod
    def _last_rows(x: Tensor, pending: Optional[Tensor], valid: Optional[Tensor], T: int):
        """Each sequence's last valid row of ``x`` and of ``pending`` (when there is one), ``[B, T, dim]`` ->
        ``[B, 1, dim]``: row ``valid[b] - 1`` (``valid`` int32 ``[B]`` in ``[1, T]``), or ``T - 1`` without.
        With a ``pending`` the rows are contiguous, as the LayerNorm behind them reads them."""
        if valid is not None:
            last = (valid.to(torch.int64) - 1)[:, None, None].expand(x.shape[0], 1, x.shape[-1])
            return x.gather(1, last), None if pending is None else pending.gather(1, last)
        if T == 1:
            return x, pending
        if pending is None:
            return x[:, T - 1:], None
        return x[:, T - 1:].contiguous(), pending[:, T - 1:].contiguous()

    def _logits(self, x: Tensor, pending: Optional[Tensor], fused: bool = False) -> Tensor:
        """The final norm and the head on ``[B, T, dim]`` -> ``[B, T, vocab]``.  Default: ``x`` and its
        ``pending`` add; ``fused``: the residual stream alone, the norm as the product's prologue."""
        if fused:
            return linear_rows(x, self.head.weight, self.head.bias, **norm_args(self.norm))
        h, _ = self.norm(x, pending)
        return self.head(h)

    def _step(self, tokens: Tensor, cache: KVCache, lengths: Optional[Tensor], last_only: bool,
              fused: bool) -> Tensor:
        """``decode_step`` and ``extend``: ``tokens`` ``[B, T]`` at ``cache.positions[b] + t``, on the few-row
        kernels when ``fused``.  ``[B, T, vocab]``, or ``[B, vocab]`` with ``last_only``."""
        T = tokens.shape[1]
        with torch.no_grad():
            if fused:
                x = embed_rows(tokens, self.tok.weight, None if self.pos is None else self.pos[0], cache.positions)
            else:
                x = self._embed(tokens, cache.positions)
            pending = None
            for blk, kv, ring, sc in zip(self.blocks, cache.layers, cache.rolling, cache.scales):
                rkw = {"rolling": True} if ring else {}  # a linear layer: the calls it always made
                if sc is not None:  # an fp8 layer; any other: likewise
                    rkw["kv_scales"] = sc
                if fused:
                    x = blk.forward_rows(x, cache=kv, positions=cache.positions, extend=True, **rkw)
                else:
                    x, pending = blk(x, pending, cache=kv, positions=cache.positions, extend=True, **rkw)
            adv = None if lengths is None else lengths.clamp(1, T).to(torch.int32)
            if last_only:
                x, pending = self._last_rows(x, pending, adv, T)
            logits = self._logits(x, pending, fused)
            cache.positions.add_(T if adv is None else adv)
            return logits[:, 0] if last_only else logits

    def decode_step(self, token: Tensor, cache: KVCache, *, fused: bool = False) -> Tensor:
        """One new token per sequence, ``token`` ``[B]``, at ``cache.positions`` -> logits ``[B, vocab]``;
        ``cache.positions`` advance by one in place.  No device value is read on the host.
        ``fused=True``: the few-row kernels (module docstring); same result to rounding."""
        return self._step(token[:, None], cache, None, True, fused)

    def extend(self, tokens: Tensor, cache: KVCache, lengths: Optional[Tensor] = None, *,
               last_only: bool = False, fused: bool = False) -> Tensor:
        """``T`` new tokens per sequence, ``tokens`` ``[B, T]``, on top of what ``cache`` holds: token ``t``
        of sequence ``b`` runs at position ``cache.positions[b] + t`` and attends to the cache rows up to
        and including its own (the extend kernel of csrc/attention_extend.hip) -> logits ``[B, T, vocab]``.

        ``lengths`` (int32 ``[B]``): the valid tokens of each right-padded row, clamped into ``[1, T]``.
        ``cache.positions`` advance in place by them (by ``T`` without ``lengths``); the k / v rows of the
        pad tokens land past the new position and are overwritten as the sequence grows, the rule of the
        ragged prefill.  ``last_only=True`` returns ``[B, vocab]``, the logits of token
        ``clamp(lengths[b], 1, T) - 1`` alone (gathered before the final LayerNorm and the head).
        No device value is read on the host.  ``fused=True``: the few-row kernels (module docstring; native
        while ``B * T <= 16``, the PyTorch composition of ``linear_rows`` beyond); same result to rounding.
        On a cache with a rolling layer ``T`` may not exceed ``cache.lookahead`` (``ValueError``)."""
        B, T = tokens.shape
        if T < 1:
            raise ValueError("extend needs at least one token per sequence")
        if T > cache.capacity:
            raise ValueError(f"{T} new tokens exceed the cache capacity {cache.capacity}")
        if T > cache.lookahead and any(cache.rolling):
            raise ValueError(f"{T} new tokens exceed the lookahead {cache.lookahead} of a rolling cache")
        return self._step(tokens, cache, lengths, last_only, fused)

    def _speculative(self, tokens: Tensor, max_new_tokens: int, lengths: Optional[Tensor], eos: Optional[int],
                     draft: "TransformerLM", gamma: int, fused: bool = False,
                     rolling: bool = False, kv_dtype=None, kv_scales=None) -> Tuple[Tensor, Tensor]:
        """Greedy speculative decoding (``generate(draft=...)``)."""
        B, N = tokens.shape
        dev = tokens.device
        cap = N + max_new_tokens + gamma
        kw = {"fused": True} if fused else {}  # fused=False makes exactly the calls it always made
        rkw = {"rolling": True, "lookahead": max(16, gamma + 1)} if rolling else {}
        dkw = {} if kv_dtype is None else {"dtype": kv_dtype}  # the draft's cache: the dtype, scales of 1
        tkw = dict(dkw) if kv_scales is None else {**dkw, "scales": kv_scales}
        tc, dc = KVCache(self, B, capacity=cap, **rkw, **tkw), KVCache(draft, B, capacity=cap, **rkw, **dkw)
        logits, _ = self.prefill(tokens, lengths, tc)
        draft.prefill(tokens, lengths, dc)
        # invariant at the top of a round: both caches hold the history up to, but not including, `cur`
        cur = logits.argmax(dim=-1)
        out = torch.zeros(B, max_new_tokens + gamma + 1, dtype=torch.int64, device=dev)
        out[:, 0] = cur
        slot = torch.ones(B, dtype=torch.int64, device=dev)  # tokens emitted so far
        steps = torch.arange(gamma + 1, device=dev)[None, :]
        while int(slot.min()) < max_new_tokens:  # the one host read of a round
            base = tc.positions.clone()
            block = [cur]
            for _ in range(gamma):
                block.append(draft.decode_step(block[-1], dc, **kw).argmax(dim=-1))
            draft.decode_step(block[-1], dc, **kw)  # the last proposal's k / v: the caches stay in step
            block = torch.stack(block, dim=1)  # [B, gamma + 1]: cur, d_1 .. d_gamma
            tgt = self.extend(block, tc, **kw).argmax(dim=-1)  # tgt[:, i]: the target's token after block[:, :i + 1]
            agree = (block[:, 1:] == tgt[:, :-1]).to(torch.int64).cumprod(dim=1).sum(dim=1)
            n_emit = torch.minimum(agree + 1, (max_new_tokens - slot).clamp_min(0))  # 0: the sequence is done
            idx = slot[:, None] + steps
            out.scatter_(1, idx, torch.where(steps < n_emit[:, None], tgt, out.gather(1, idx)))
            cur = torch.where(n_emit > 0, tgt.gather(1, (n_emit - 1).clamp_min(0)[:, None])[:, 0], cur)
            slot = slot + n_emit
            # rejected rows are just rows past the position
            tc.positions.copy_(base + n_emit.to(torch.int32))
            dc.positions.copy_(tc.positions)
        out = out[:, :max_new_tokens]
        out_lengths = torch.full((B,), max_new_tokens, dtype=torch.int64, device=dev)
        if eos is not None:
            hit = out == eos
            first = hit.to(torch.int64).argmax(dim=1) + 1
            out_lengths = torch.where(hit.any(dim=1), first, out_lengths)
            past = torch.arange(max_new_tokens, device=dev)[None, :] >= out_lengths[:, None]
            out = torch.where(past, torch.full_like(out, eos), out)
        return out.contiguous(), out_lengths

    def generate(self, tokens: Tensor, max_new_tokens: int, lengths: Optional[Tensor] = None, *,
                 temperature: float = 0.0, top_k: Optional[int] = None, eos: Optional[int] = None,
                 generator=None, graph: bool = False, cache: Optional[KVCache] = None,
                 draft: Optional["TransformerLM"] = None, draft_tokens: int = 4,
                 fused: bool = False, rolling: bool = False, kv_dtype=None,
                 kv_scales=None) -> Tuple[Tensor, Tensor]:
        """Continue the prompts ``tokens`` ``[B, N]`` (``lengths``: valid tokens of each, right-padded) by
        ``max_new_tokens`` tokens -> ``(out [B, max_new_tokens], out_lengths [B])``.

        ``temperature == 0`` is greedy; otherwise tokens are drawn from ``softmax(logits / temperature)``
        restricted to the ``top_k`` logits with ``torch.multinomial(generator=generator)``.  With ``eos``, a
        sequence that has produced it emits ``eos`` from then on and ``out_lengths`` counts its tokens up
        to and including the first ``eos`` (the mask lives on the device: no per-step sync, no early exit).
        ``graph=True`` (CUDA): after the prefill and one eager decode step, ONE decode step plus the
        sampling is captured into a graph and replayed for the remaining tokens; greedy results equal
        ``graph=False`` bit for bit.

        ``cache`` (a :class:`KVCache` of batch ``B``): continue what it holds.  ``tokens`` are NEW tokens
        appended at ``cache.positions`` through ``extend(last_only=True)`` instead of a prefill; decoding
        then proceeds as above, ``graph=True`` included.  ``cache.positions.max()`` is read on the host
        once at entry (outside any capture): ``max + N + max_new_tokens`` must not exceed
        ``min(cache.capacity, max_len)``.  On return ``cache.positions[b] = start[b] + prompt_len[b] +
        out_lengths[b] - 1`` (set on the device): the cache holds the prompt and every emitted token BUT
        THE LAST, so the caller begins the next turn's ``tokens`` with ``out[b, out_lengths[b] - 1]``.

        ``draft`` (another :class:`TransformerLM` over the same vocabulary): greedy speculative decoding.
        Per round the draft proposes ``draft_tokens`` tokens with its own cache and ``decode_step``, the
        target scores ``[cur, d_1 .. d_γ]`` in ONE ``extend``, and the longest prefix on which the two
        argmaxes agree is accepted plus the target's own next token: 1 to γ + 1 tokens per sequence and
        round, equal to what greedy ``generate`` without a draft emits wherever the target's argmax is
        unambiguous.  Greedy only, eager only, own caches only (``temperature != 0``, ``top_k``,
        ``graph=True`` and ``cache`` raise), and ``N + max_new_tokens + draft_tokens`` must fit both
        models' ``max_len``.  Termination reads ONE device value (``slot.min()``) per round; ``eos`` is
        applied after the loop.

        ``fused=True``: every ``decode_step`` / ``extend`` made here runs on the few-row kernels (module
        docstring) -- with ``cache``, with ``graph=True`` and, with ``draft``, in both models.  ``prefill`` is
        unchanged.

        ``rolling=True``: the caches made here are rolling (:class:`KVCache`; with ``draft`` both, with
        ``lookahead=max(16, draft_tokens + 1)``).  A caller's ``cache`` is what it was built as -- a rolling one
        works with every option above; its ``tokens`` are fed through ``extend``, so at most
        ``cache.lookahead`` of them per call.  The ``max_len`` checks stay as they are.

        ``kv_dtype`` / ``kv_scales``: the ``dtype`` and ``scales`` of the caches made here (:class:`KVCache`;
        ``torch.float8_e4m3fn`` is the fp8 cache, ``kv_scales`` as its ``scales``).  With ``draft`` the draft's
        cache gets ``kv_dtype`` and scales of 1.  A caller's ``cache`` brings its own and takes neither
        (``ValueError``).  Works with ``graph=True``, ``fused=True`` and ``rolling=True``."""
        B, N = tokens.shape
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        if N + max_new_tokens > self.max_len:
            raise ValueError(f"prompt {N} + max_new_tokens {max_new_tokens} exceeds max_len {self.max_len}")
        if graph and not tokens.is_cuda:
            raise ValueError("graph=True needs CUDA tensors")
        if draft is not None:
            gamma = int(draft_tokens)
            if temperature != 0 or top_k is not None or graph or cache is not None:
                raise ValueError("speculative decoding is greedy and eager with its own caches: no temperature, "
                                 "top_k, graph=True or cache")
            if gamma < 1:
                raise ValueError("draft_tokens must be at least 1")
            if draft.tok.num_embeddings != self.tok.num_embeddings:
                raise ValueError("the draft model must share the target's vocabulary")
            if N + max_new_tokens + gamma > min(self.max_len, draft.max_len):
                raise ValueError(f"prompt {N} + max_new_tokens {max_new_tokens} + draft_tokens {gamma} exceeds "
                                 f"max_len {min(self.max_len, draft.max_len)}")
            with torch.no_grad():
                if kv_dtype is not None or kv_scales is not None:
                    return self._speculative(tokens, max_new_tokens, lengths, eos, draft, gamma, fused, bool(rolling),
                                             kv_dtype, kv_scales)
                if rolling:
                    return self._speculative(tokens, max_new_tokens, lengths, eos, draft, gamma, fused, True)
                return self._speculative(tokens, max_new_tokens, lengths, eos, draft, gamma, fused)
        start = None
        kw = {"fused": True} if fused else {}  # fused=False makes exactly the calls it always made
        if cache is not None:
            if kv_dtype is not None or kv_scales is not None:
                raise ValueError("kv_dtype / kv_scales are for the caches generate makes: a cache brings its own")
            if cache.positions.shape[0] != B:
                raise ValueError(f"the cache holds {cache.positions.shape[0]} sequences, tokens {B}")
            held = int(cache.positions.max())
            room = min(cache.capacity, self.max_len)
            if held + N + max_new_tokens > room:
                raise ValueError(f"cache position {held} + prompt {N} + max_new_tokens {max_new_tokens} exceeds {room}")
        with torch.no_grad():
            dev = tokens.device
            if cache is None:
                ckw = {"rolling": True} if rolling else {}
                if kv_dtype is not None:
                    ckw["dtype"] = kv_dtype
                if kv_scales is not None:
                    ckw["scales"] = kv_scales
                cache = KVCache(self, B, capacity=N + max_new_tokens, **ckw)
                logits, _ = self.prefill(tokens, lengths, cache)
            else:
                logits = self.extend(tokens, cache, lengths, last_only=True, **kw)
                start = cache.positions.clone()  # start[b] + prompt_len[b]
            out = torch.zeros(B, max_new_tokens, dtype=torch.int64, device=dev)
            out_lengths = torch.zeros(B, dtype=torch.int64, device=dev)
            finished = torch.zeros(B, dtype=torch.bool, device=dev)
            slot = torch.zeros(B, 1, dtype=torch.int64, device=dev)  # the column of `out` written next
            cur = torch.zeros(B, dtype=torch.int64, device=dev)  # the token fed to the next decode step

            def emit(logits: Tensor) -> None:
                tok = _sample(logits, temperature, top_k, generator)
                if eos is not None:
                    tok = torch.where(finished, torch.full_like(tok, eos), tok)
                out.scatter_(1, slot, tok[:, None])
                out_lengths.add_((~finished).to(torch.int64))
                if eos is not None:
                    finished.logical_or_(tok == eos)
                slot.add_(1)
                cur.copy_(tok)

            def step() -> None:
                emit(self.decode_step(cur, cache, **kw))

            emit(logits)
            eager = max_new_tokens - 1
            if graph and eager > 1:
                step()  # warm-up: first-use work of the decode path happens outside the capture
                eager = 0
                g = torch.cuda.CUDAGraph()
                if generator is not None and temperature != 0:
                    g.register_generator_state(generator)
                torch.cuda.synchronize()
                with torch.cuda.graph(g):
                    step()
                for _ in range(max_new_tokens - 2):
                    g.replay()
            for _ in range(eager):
                step()
            if start is not None:  # a caller's cache: keep every emitted token but the last
                cache.positions.copy_(start + (out_lengths - 1).to(torch.int32))
            return out, out_lengths


def kv_scales(model: TransformerLM, tokens: Tensor, lengths: Optional[Tensor] = None, *,
              margin: float = 1.0) -> List[Tuple[float, float]]:
    """Calibrate the scales of an fp8 :class:`KVCache` on a prompt: one ``prefill`` of ``tokens`` ``[B, N]``
    (``lengths``: the valid tokens of a right-padded batch) into a temporary cache of the model's dtype, then
    per layer ``(amax_k / 448 * margin, amax_v / 448 * margin)`` with ``amax`` the largest magnitude over the
    VALID cached rows -- pad rows do not count -- so those rows quantise without saturating (``margin > 1``
    leaves headroom for later tokens).  A layer whose rows are all zero gets 1.0.  Reads the device once."""
    margin = float(margin)
    if not (margin > 0 and margin < float("inf")):
        raise ValueError(f"margin must be a finite float > 0, not {margin!r}")
    B, N = tokens.shape
    with torch.no_grad():
        _, cache = model.prefill(tokens, lengths, KVCache(model, B, capacity=N))
        n = cache.positions.to(torch.int64)  # the clamped lengths
        valid = torch.arange(N, device=n.device)[None, :] < n[:, None]  # [B, N]
        amax = torch.stack([torch.stack([c.float().abs().amax(dim=(1, 3)).masked_fill(~valid, 0).max() for c in kv])
                            for kv in cache.layers]).to(torch.float64)
    out = []
    for k, v in amax.tolist():  # the one host read
        out.append(tuple(a / 448.0 * margin if a > 0 else 1.0 for a in (k, v)))
    return out


def gpt_tiny(vocab: int = 256, max_len: int = 128, pos: str = "learned", *, norm: str = "layer", mlp: str = "gelu",
             bias: bool = True, kv_heads: Optional[int] = None, mlp_ratio: float = 4.0, window=None) -> TransformerLM:
    return TransformerLM(vocab, 128, 2, 2, max_len, mlp_ratio, kv_heads, pos=pos, norm=norm, mlp=mlp, bias=bias,
                         window=window)


def gpt2_small(vocab: int = 50257, max_len: int = 1024, pos: str = "learned", *, norm: str = "layer",
               mlp: str = "gelu", bias: bool = True, kv_heads: Optional[int] = None,
               mlp_ratio: float = 4.0, window=None) -> TransformerLM:
    return TransformerLM(vocab, 768, 12, 12, max_len, mlp_ratio, kv_heads, pos=pos, norm=norm, mlp=mlp, bias=bias,
                         window=window)
