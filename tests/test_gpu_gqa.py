"""Grouped-query attention on the native kernels: ``kv_heads`` in ``attn_kv_append``, the split-KV decode
(csrc/attention_decode.hip: one wave serves a head block of 1 .. 4 query heads from one load of each
K / V row), its fused append, the extend kernel (csrc/attention_extend.hip) and ``TransformerLM``.

Two bars.  Bits: per query head the decode / extend kernels do the arithmetic of the one-head-per-wave
kernel in its order, so every result is ``torch.equal`` to the same call without ``kv_heads`` on the
caches expanded with ``repeat_interleave`` (query head ``h`` reads kv head ``h // G``).  Accuracy: the
forward bar of test_gpu_attention.py / test_gpu_decode.py, relative Frobenius error < 1e-2 against fp32
math on the bf16 inputs (``randn * 1.5``).  Kernel checks run with 64 keys per workgroup and with the
default.  The default head block shares loads only when the grid can spare the waves, which no test-sized
shape can, so every decode check runs twice: ``shared`` forces the largest block of 4, 3, 2, 1 that divides
``G`` -- the decode cases then give head blocks of 2, 3, 4, 2 x 4, 5 x 1 and 2 x 3 -- and ``default`` leaves
the policy alone (one head per wave, ``G`` waves per kv head).  Lengths sit on both sides of a 64-key chunk
edge, inside the last partial chunk and in caches whose later chunks are empty.
"""
import contextlib
import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.models.gpt import KVCache, TransformerLM  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops import attention as A  # noqa: E402
from torchbooster_amd.ops.attention import (attention_decode, attention_decode_packed, attention_extend,  # noqa: E402
                                            attention_extend_packed, kv_cache_append)

DEV = "cuda"
BF = torch.bfloat16
SCALE = 1.0 / math.sqrt(64)


@pytest.fixture(params=[64, None], ids=["chunk64", "default"])
def chunk(request):
    nat = _ext.native()
    old = nat.attn_decode_set_chunk(-1)
    if request.param is not None:
        nat.attn_decode_set_chunk(request.param)
    try:
        yield nat.attn_decode_set_chunk(-1)
    finally:
        nat.attn_decode_set_chunk(old)


@pytest.fixture(params=["shared", "default"])
def blocks(request):
    """A context manager, given G.  ``shared``: it forces the head block to the largest of 4, 3, 2, 1 that
    divides G; ``default``: it leaves the policy alone."""
    @contextlib.contextmanager
    def forced(G):
        nat = _ext.native()
        old = nat.attn_decode_set_head_block(-1)
        if request.param == "shared":
            nat.attn_decode_set_head_block(next(gb for gb in (4, 3, 2, 1) if G % gb == 0))
        try:
            yield
        finally:
            nat.attn_decode_set_head_block(old)
    return forced


@pytest.fixture(params=[64, 0], ids=["split64", "default_split"])
def split(request):
    nat = _ext.native()
    old = nat.attn_extend_set_split(-1)
    nat.attn_extend_set_split(request.param)
    try:
        yield request.param
    finally:
        nat.attn_extend_set_split(old)


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _expand(c, G):
    return c.repeat_interleave(G, dim=1)


def _oracle(q, kc, vc, limits, scale=SCALE):
    """fp32 softmax over the visible keys only.  q [B, T, H, 64], FULL-head caches [B, H, cap, 64];
    limits[b][t] (host ints, clamped) rows are visible."""
    q, kc, vc = q.float(), kc.float(), vc.float()
    out = torch.zeros_like(q)
    for b in range(q.shape[0]):
        for t in range(q.shape[1]):
            n = min(max(limits[b][t], 1), kc.shape[2])
            s = torch.einsum("hd,hjd->hj", q[b, t], kc[b, :, :n]) * scale
            out[b, t] = torch.einsum("hj,hjd->hd", torch.softmax(s, -1), vc[b, :, :n])
    return out


@functools.lru_cache(maxsize=None)
def _case(B, H, Hkv, T, cap):
    """A packed projection [B, T, (H + 2*Hkv)*64], caches [B, Hkv, cap, 64] and their expansion to H
    heads: made once per shape, shared by every test and setting, never modified."""
    g = torch.Generator(device=DEV).manual_seed(1000 * cap + 100 * T + 10 * H + Hkv)
    packed = torch.randn(B, T, (H + 2 * Hkv) * 64, device=DEV, generator=g).mul(1.5).to(BF)
    kc, vc = (torch.randn(B, Hkv, cap, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    return packed, kc, vc, _expand(kc, H // Hkv), _expand(vc, H // Hkv)


def _q(packed, H):
    B, T, _ = packed.shape
    return packed[..., :H * 64].view(B, T, H, 64)  # a strided view into the packed rows


def _kv(packed, H, Hkv):
    B, T, _ = packed.shape
    return (packed[..., H * 64:(H + Hkv) * 64].view(B, T, Hkv, 64), packed[..., (H + Hkv) * 64:].view(B, T, Hkv, 64))


# ---------------------------------------------------------------- decode
DECODE_CASES = [(2, 4, 2, 70, (1, 70)), (4, 6, 2, 200, (63, 64, 65, 129)), (4, 8, 2, 200, (7, 8, 9, 200)),
                (2, 8, 1, 520, (128, 520)), (2, 5, 1, 70, (1, 70)), (2, 12, 2, 200, (65, 200))]


@functools.lru_cache(maxsize=None)
def _decode_oracle(B, H, Hkv, cap, lengths):
    packed, _, _, ke, ve = _case(B, H, Hkv, 1, cap)
    return _oracle(_q(packed, H), ke, ve, [[n] for n in lengths])[:, 0]


def test_head_block_choice():
    """The default: the largest block of 4, 3, 2 that divides G and leaves B * H * nchunks / block >= 3072
    waves, else 1 (128 keys per chunk); a forced block is taken where it divides G."""
    nat = _ext.native()
    hb = nat.attn_decode_head_block
    assert nat.attn_decode_set_chunk(-1) == 128 and nat.attn_decode_set_head_block(-1) == 0
    assert hb(8, 12, 1, 4096) == 1 and hb(8, 12, 12, 4096) == 1  # 3072 one-head waves: none to spare
    assert hb(64, 12, 1, 1024) == 2 and hb(64, 12, 4, 1024) == 1  # 6144
    assert hb(32, 12, 1, 4096) == 4 and hb(32, 12, 4, 4096) == 3 and hb(32, 12, 6, 4096) == 2  # 12288
    assert hb(128, 12, 2, 4096) == 3 and hb(128, 10, 2, 4096) == 1 and hb(128, 12, 0, 4096) == 1  # G = 6, 5, 1
    old = nat.attn_decode_set_head_block(4)
    try:
        assert hb(2, 8, 1, 520) == 4 and hb(2, 8, 2, 520) == 4 and hb(2, 12, 2, 200) == 1  # 4 does not divide 6
        with pytest.raises(RuntimeError):
            nat.attn_decode_set_head_block(5)
        with pytest.raises(RuntimeError):
            hb(2, 8, 3, 520)
        assert nat.attn_decode_set_head_block(-1) == 4
    finally:
        nat.attn_decode_set_head_block(old)


@pytest.mark.parametrize("B,H,Hkv,cap,lengths", DECODE_CASES)
def test_decode_bit_equal_to_expanded_and_matches_fp32(chunk, blocks, monkeypatch, B, H, Hkv, cap, lengths):
    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    monkeypatch.setattr(A, "_decode_ref", boom)
    packed, kc, vc, ke, ve = _case(B, H, Hkv, 1, cap)
    q = _q(packed, H)[:, 0]
    assert not q.is_contiguous()
    kl = _i32(lengths)
    with blocks(H // Hkv):
        got = attention_decode(q, kc, vc, kl, kv_heads=Hkv)
        again = attention_decode(q, kc, vc, kl, kv_heads=Hkv)
    assert got.shape == (B, H, 64) and got.dtype == BF and torch.isfinite(got).all()
    assert torch.equal(got, attention_decode(q, ke, ve, kl))
    assert torch.equal(got, again)  # deterministic
    e = _err(got, _decode_oracle(B, H, Hkv, cap, lengths))
    print(f"B,H,Hkv,cap={B},{H},{Hkv},{cap} lengths={lengths} chunk={chunk}: o {e:.2e}")
    assert e < 1e-2, e


@pytest.mark.parametrize("gb", [1, 2, 4])
def test_forced_head_block_has_the_same_bits(chunk, gb):
    """The head block only decides which wave computes a head: 1 (head mapping alone), 2 and 4 give the
    same bits, and the workspace is fully written whatever the block."""
    B, H, Hkv, cap, lengths = 4, 8, 2, 200, (7, 8, 9, 200)
    packed, kc, vc, _, _ = _case(B, H, Hkv, 1, cap)
    q = _q(packed, H)[:, 0]
    nat = _ext.native()
    want = attention_decode(q, kc, vc, _i32(lengths), kv_heads=Hkv)
    old = nat.attn_decode_set_head_block(gb)
    try:
        ws = torch.full((nat.attn_decode_workspace(B, H, cap),), float("nan"), device=DEV)
        got = nat.attn_decode(q, H, kc, vc, _i32(lengths), 0, SCALE, ws, Hkv).view(B, H, 64)
    finally:
        nat.attn_decode_set_head_block(old)
    assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("fill", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("H,Hkv", [(6, 2), (8, 1)])
def test_junk_past_the_length_never_enters(chunk, blocks, fill, H, Hkv):
    B, cap, lengths = 4, 200, (63, 64, 65, 1)
    packed, kc, vc, _, ve = _case(B, H, Hkv, 1, cap)
    q = _q(packed, H)[:, 0]
    hidden = torch.arange(cap, device=DEV)[None, None, :, None] >= _i32(lengths)[:, None, None, None]

    def run(value):
        k2 = torch.where(hidden, torch.full_like(kc, value), kc)
        v2 = torch.where(hidden, torch.full_like(vc, value), vc)
        with blocks(H // Hkv):
            return attention_decode(q, k2, v2, _i32(lengths), kv_heads=Hkv)

    got = run(fill)
    assert torch.isfinite(got).all()
    assert torch.equal(got, run(0.0))
    assert torch.equal(got[3], ve[3, :, 0])  # one visible key: exactly its value row, for every head of the group


def test_argument_checks_on_the_native_path():
    """kv_heads is never inferred: a non-dividing value is a ValueError, a cache or a packed width that
    does not match it a RuntimeError from the binding's checks."""
    B, H, Hkv, cap = 2, 4, 2, 70
    packed, kc, vc, ke, ve = _case(B, H, Hkv, 1, cap)
    q = _q(packed, H)[:, 0]
    kl = _i32((1, 70))
    nat = _ext.native()
    with pytest.raises(ValueError):
        attention_decode(q, kc, vc, kl, kv_heads=3)
    with pytest.raises(RuntimeError):
        nat.attn_decode(q, H, kc, vc, kl, 0, SCALE, None, 3)
    for call in (lambda: attention_decode(q, ke, ve, kl, kv_heads=Hkv),  # a cache with H heads
                 lambda: attention_decode(q, kc, vc, kl),  # Hkv heads, no keyword
                 lambda: attention_extend(_q(packed, H), ke, ve, kl, kv_heads=Hkv),
                 lambda: attention_extend(_q(packed, H), kc, vc, kl),
                 lambda: kv_cache_append(ke.clone(), ve.clone(), packed, H, kl, kv_heads=Hkv),
                 lambda: attention_decode_packed(packed, H, ke.clone(), ve.clone(), kl, fused=True, kv_heads=Hkv)):
        with pytest.raises(RuntimeError):
            call()
    wide = torch.zeros(B, 1, 3 * H * 64, device=DEV, dtype=BF)  # the width of plain multi-head attention
    for call in (lambda: kv_cache_append(kc.clone(), vc.clone(), wide, H, kl, kv_heads=Hkv),
                 lambda: attention_decode_packed(wide, H, kc.clone(), vc.clone(), kl, kv_heads=Hkv),
                 lambda: attention_decode_packed(wide, H, kc.clone(), vc.clone(), kl, fused=True, kv_heads=Hkv)):
        with pytest.raises(RuntimeError):
            call()


# ---------------------------------------------------------------- append and the fused step
SENTINEL = -7.25


@pytest.mark.parametrize("H,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("T,positions", [(1, (0, 3)), (5, (0, 3)), (5, (-2, 6)), (5, (9, 0))])
def test_append(monkeypatch, H, Hkv, T, positions):
    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    monkeypatch.setattr(A, "_append_ref", boom)
    B, cap = 2, 9
    g = torch.Generator(device=DEV).manual_seed(T)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * 64, device=DEV, generator=g).to(BF)
    kc = torch.full((B, Hkv, cap, 64), SENTINEL, device=DEV, dtype=BF)
    vc = torch.full_like(kc, SENTINEL)
    kv_cache_append(kc, vc, qkv, H, _i32(positions), kv_heads=Hkv)
    for cache, src in zip((kc, vc), _kv(qkv, H, Hkv)):
        want = torch.full_like(cache, SENTINEL)
        for b in range(B):
            for t in range(T):
                if 0 <= positions[b] + t < cap:
                    want[b, :, positions[b] + t] = src[b, t]
        assert torch.equal(cache, want)


def _both(blocks, packed, H, Hkv, kc, vc, pos):
    """(output, k cache, v cache) of the unfused and of the fused step on copies of the caches."""
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    with blocks(H // Hkv):
        o1 = attention_decode_packed(packed, H, k1, v1, pos, kv_heads=Hkv)
        o2 = attention_decode_packed(packed, H, k2, v2, pos, fused=True, kv_heads=Hkv)
    return (o1, k1, v1), (o2, k2, v2)


@pytest.mark.parametrize("H,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("cap,positions", [(200, (0, 63, 64, 127, 128, 199)), (40, (0, 39, 17, 1, 38, 20))],
                         ids=["cap200", "single_chunk"])
def test_fused_is_bit_equal(chunk, blocks, H, Hkv, cap, positions):
    B = len(positions)
    packed, kc, vc, ke, ve = _case(B, H, Hkv, 1, cap)
    pos = _i32(positions)
    (o1, k1, v1), (o2, k2, v2) = _both(blocks, packed, H, Hkv, kc, vc, pos)
    assert o2.shape == (B, 1, H * 64) and o2.dtype == BF and torch.isfinite(o2).all()
    assert torch.equal(o1, o2) and torch.equal(k1, k2) and torch.equal(v1, v2)
    k, v = _kv(packed, H, Hkv)
    hit = torch.arange(cap, device=DEV)[None, None, :, None] == pos[:, None, None, None]
    assert torch.equal(k2, torch.where(hit, k[:, 0, :, None], kc))  # the row stored, every other bit unchanged
    assert torch.equal(v2, torch.where(hit, v[:, 0, :, None], vc))
    # and the step is the step on expanded caches without kv_heads, given the expanded packed row
    full = torch.cat([packed[..., :H * 64], _expand(k[:, 0], H // Hkv).reshape(B, 1, -1),
                      _expand(v[:, 0], H // Hkv).reshape(B, 1, -1)], dim=-1)
    assert torch.equal(o2, attention_decode_packed(full, H, ke.clone(), ve.clone(), pos, fused=True))
    e = _err(o2.view(B, H, 64), _oracle(_q(packed, H), _expand(k2, H // Hkv), _expand(v2, H // Hkv),
                                         [[p + 1] for p in positions])[:, 0])
    assert e < 1e-2, e


@pytest.mark.parametrize("H,Hkv", [(4, 2), (8, 1)])
def test_positions_outside_the_cache_are_dropped(chunk, blocks, H, Hkv):
    B, cap = 2, 200
    packed, kc, vc, _, ve = _case(B, H, Hkv, 1, cap)
    (o1, k1, v1), (o2, k2, v2) = _both(blocks, packed, H, Hkv, kc, vc, _i32((-1, cap)))
    assert torch.equal(k2, kc) and torch.equal(v2, vc) and torch.equal(k1, kc) and torch.equal(v1, vc)
    assert torch.equal(o1, o2) and torch.isfinite(o2).all()
    assert torch.equal(o2[0, 0].view(H, 64), ve[0, :, 0])  # length clamped to 1: exactly the first value row


def test_graph_replay_follows_positions(blocks):
    B, H, Hkv, cap = 2, 8, 2, 200
    packed, kc0, vc0, _, _ = _case(B, H, Hkv, 1, cap)
    pos = _i32((150, 20))
    kc, vc = kc0.clone(), vc0.clone()
    kw = {"fused": True, "kv_heads": Hkv}
    attention_decode_packed(packed, H, kc0.clone(), vc0.clone(), pos, **kw)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with blocks(H // Hkv), torch.cuda.graph(graph):  # the block is part of the captured grid
        out = attention_decode_packed(packed, H, kc, vc, pos, **kw)
    graph.replay()
    first = out.clone()
    pos.copy_(_i32((7, 199)))
    graph.replay()
    torch.cuda.synchronize()
    ke, ve = kc0.clone(), vc0.clone()
    assert torch.equal(first, attention_decode_packed(packed, H, ke, ve, _i32((150, 20)), kv_heads=Hkv))
    assert torch.equal(out, attention_decode_packed(packed, H, ke, ve, _i32((7, 199)), kv_heads=Hkv))
    assert not torch.equal(out, first)
    assert torch.equal(kc, ke) and torch.equal(vc, ve)


# ---------------------------------------------------------------- extend
@pytest.mark.parametrize("H,Hkv", [(4, 2), (8, 2)])
@pytest.mark.parametrize("T", [2, 5, 16, 17])
def test_extend_bit_equal_to_expanded_and_matches_fp32(split, monkeypatch, T, H, Hkv):
    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    monkeypatch.setattr(A, "_extend_ref", boom)
    monkeypatch.setattr(A, "_append_ref", boom)
    B, cap, positions = 2, 200, (7, 150)
    packed, kc, vc, _, _ = _case(B, H, Hkv, T, cap)
    pos = _i32(positions)
    k2, v2 = kc.clone(), vc.clone()
    got = attention_extend_packed(packed, H, k2, v2, pos, kv_heads=Hkv)  # the append, then the extend
    assert got.shape == (B, T, H * 64) and got.dtype == BF and torch.isfinite(got).all()
    ke, ve = _expand(k2, H // Hkv), _expand(v2, H // Hkv)
    q = _q(packed, H)
    assert torch.equal(got.view(B, T, H, 64), attention_extend(q, k2, v2, pos, kv_heads=Hkv))
    assert torch.equal(got.view(B, T, H, 64), attention_extend(q, ke, ve, pos))
    e = _err(got.view(B, T, H, 64), _oracle(q, ke, ve, [[p + t + 1 for t in range(T)] for p in positions]))
    print(f"T,H,Hkv={T},{H},{Hkv} split={split} nsplit={_ext.native().attn_extend_splits(B, H, T, cap)}: o {e:.2e}")
    assert e < 1e-2, e


def test_extend_packed_with_one_token_is_the_decode_step(monkeypatch):
    B, H, Hkv, cap = 2, 8, 2, 200
    packed, kc, vc, _, _ = _case(B, H, Hkv, 1, cap)
    pos = _i32((7, 150))
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    want = attention_decode_packed(packed, H, k1, v1, pos, kv_heads=Hkv)
    calls = []
    real = A.attention_decode_packed
    monkeypatch.setattr(A, "attention_decode_packed", lambda *a, **k: calls.append(k) or real(*a, **k))
    got = attention_extend_packed(packed, H, k2, v2, pos, kv_heads=Hkv)
    assert calls == [{"kv_heads": Hkv}]
    assert torch.equal(got, want) and torch.equal(k1, k2) and torch.equal(v1, v2)


# ---------------------------------------------------------------- model
@pytest.fixture(scope="module", params=[2, 1], ids=["kv2", "kv1"])
def lm(request):
    """The fp32 model, its bf16 copy, tokens, and the teacher-forced logits of both full forwards
    (fp32 on the stock path, bf16 native) at positions j .. N - 2: computed once per kv_heads."""
    torch.manual_seed(0)
    B, N, j = 2, 70, 33
    base = TransformerLM(256, 256, 2, 4, 128, kv_heads=request.param).cuda()
    tokens = torch.randint(0, 256, (B, N), device=DEV)
    lengths = _i32((70, 41))
    mnat = copy.deepcopy(base).to(BF)
    mp = pytest.MonkeyPatch()
    with torch.no_grad():
        full = mnat(tokens, lengths)[:, j:N - 1].float()
        try:
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")  # the stock run: every op on its PyTorch path
            ref = copy.deepcopy(base)(tokens, lengths)[:, j:N - 1].float()
        finally:
            mp.undo()
    keep = torch.arange(j, N - 1, device=DEV)[None, :] < lengths[:, None]
    return base, mnat, tokens, lengths, j, ref, full, keep


@pytest.mark.parametrize("how", ["decode_step", "decode_step_fused", "extend4"])
def test_incremental_logits_vs_reference(lm, how):
    """The rule of test_gpu_decode.py test_gpt_tiny_incremental_vs_reference: against the fp32 stock full
    forward, the incremental native logits are at most 1.5x as far off as the full-forward native ones
    (pad positions of the second sequence excluded on both sides)."""
    base, mnat, tokens, lengths, j, ref, full, keep = lm
    N = tokens.shape[1]
    hkv = mnat.blocks[0].attn.kv_heads
    _, cache = mnat.prefill(tokens[:, :j], lengths.clamp(max=j))
    assert all(c.shape == (2, hkv, 128, 64) for kv in cache.layers for c in kv)
    if how == "extend4":
        inc = torch.cat([mnat.extend(tokens[:, t:t + 4], cache) for t in range(j, N - 1, 4)], dim=1).float()
    else:
        kw = {"fused": True} if how == "decode_step_fused" else {}
        inc = torch.stack([mnat.decode_step(tokens[:, t], cache, **kw) for t in range(j, N - 1)], dim=1).float()
    assert cache.positions.tolist() == [N - 1, N - 1]
    e_inc, e_full = _err(inc[keep], ref[keep]), _err(full[keep], ref[keep])
    print(f"kv_heads={hkv} {how}: incremental {e_inc:.5f} full forward {e_full:.5f} ({e_inc / e_full:.2f}x)")
    assert torch.isfinite(inc).all()
    assert e_inc <= 1.5 * e_full, (e_inc, e_full)


def test_generate_graph_equals_eager_and_speculative_runs(lm):
    _, mnat, tokens, _, _, _, _, _ = lm
    prompt = tokens[:, :9]
    for kw in ({}, {"fused": True}):
        a, a_len = mnat.generate(prompt, 24, graph=False, **kw)
        b, b_len = mnat.generate(prompt, 24, graph=True, **kw)
        assert torch.equal(a, b) and torch.equal(a_len, b_len)
        assert a.shape == (2, 24) and int(a.min()) >= 0 and int(a.max()) < 256
    torch.manual_seed(1)
    draft = TransformerLM(256, 128, 1, 2, 128, kv_heads=1).cuda().to(BF)
    assert KVCache(draft, 2).layers[0][0].shape == (2, 1, 128, 64)
    out, out_len = mnat.generate(prompt, 12, draft=draft, draft_tokens=4)
    assert out.shape == (2, 12) and out_len.tolist() == [12, 12]
    assert int(out.min()) >= 0 and int(out.max()) < 256


def test_training_step_qkv_gradient_vs_reference(lm, monkeypatch):
    """One ``loss().backward()``: the gradient of every block's ``qkv.weight`` -- through the expanded
    k / v, so dK / dV are summed over each group -- against the same weights on the fp32 stock path, at
    the model-level gradient bar of test_gpu_lm_loss.py: at most 1.5x the error of stock bf16 autocast."""
    base, _, tokens, lengths, _, _, _, _ = lm

    def run(model, autocast=False):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF, enabled=autocast):
            loss = model.loss(tokens, lengths)
        loss.backward()
        return loss.detach().float(), torch.cat([b.attn.qkv.weight.grad.float().reshape(-1) for b in model.blocks])

    lnat, gnat = run(copy.deepcopy(base).to(BF))
    with monkeypatch.context() as mp:  # the stock runs: every op on its PyTorch path
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        l32, g32 = run(copy.deepcopy(base))
        lamp, gamp = run(copy.deepcopy(base), autocast=True)
    e_nat, e_amp = _err(gnat, g32), _err(gamp, g32)
    print(f"loss fp32 {float(l32):.5f} native {float(lnat):.5f} autocast {float(lamp):.5f}; qkv.weight gradient "
          f"error vs fp32: native {e_nat:.5f} autocast {e_amp:.5f} ({e_nat / e_amp:.2f}x)")
    assert torch.isfinite(lnat) and torch.isfinite(gnat).all()
    assert e_nat <= 1.5 * e_amp, (e_nat, e_amp)
