"""Sliding-window attention on the PyTorch paths (CPU; fp64 where it is the oracle).

The rule (ops/attention.py): a row whose upper key limit is ``hi`` sees keys ``max(0, hi - W) <= j < hi``.
Here it is written out a second time, as loops over an explicit boolean mask, and everything the
package computes with ``window=`` is compared against a softmax through that mask.
"""
import math

import pytest
import torch

from torchbooster_amd.models import gpt_tiny
from torchbooster_amd.models.gpt import KVCache, TransformerLM
from torchbooster_amd.models.vit import Attention, Block
from torchbooster_amd.ops.attention import (_decode_ref, _extend_ref, attention, attention_decode,
                                            attention_decode_packed, attention_extend, attention_extend_packed,
                                            attention_packed, attention_ref)

D = 8
SCALE = 1.0 / math.sqrt(D)


def _mask(N, W, lengths=None, B=1):
    """[B, N, N] bool, True = attend, built from the rule one element at a time."""
    m = torch.zeros(B, N, N, dtype=torch.bool)
    for b in range(B):
        n = N if lengths is None else min(max(int(lengths[b]), 1), N)
        for i in range(N):
            hi = min(n, i + 1)
            lo = hi if W is None else max(0, hi - W)
            m[b, i, (0 if W is None else lo):hi] = True
    return m


def _explicit(q, k, v, m):
    s = (q @ k.transpose(-1, -2)) * SCALE
    s = s.masked_fill(~m[:, None], float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def _windows(N):
    return sorted({w for w in (1, 2, 64, N - 1, N, N + 3) if w >= 1})


def _lengths_for(N):
    return [None] if N == 1 else [None, (N, 1, max(1, N // 2), N - 1)]


@pytest.mark.parametrize("N", [1, 5, 70])
def test_formula_and_gradients(N):
    torch.manual_seed(N)
    for lengths in _lengths_for(N):
        B = 1 if lengths is None else len(lengths)
        kl = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
        q, k, v, g = (torch.randn(B, 2, N, D, dtype=torch.float64) for _ in range(4))
        for W in _windows(N):
            m = _mask(N, W, lengths, B)
            # a valid token sees itself and the W - 1 tokens before it
            if lengths is None:
                i = torch.arange(N)
                assert torch.equal(m[0], (i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - W))
            assert m.any(dim=-1).all()  # no row is fully masked
            want_in = [t.clone().requires_grad_() for t in (q, k, v)]
            want = _explicit(*want_in, m)
            want.backward(g)
            # attention_ref takes its softmax in fp32 whatever the inputs are (its docstring): 1e-5, the fp32
            # bar of tests/test_extend.py; the SDPA path stays in fp64
            for fn, atol in ((attention_ref, 1e-5), (attention, 1e-12)):
                got_in = [t.clone().requires_grad_() for t in (q, k, v)]
                got = fn(*got_in, SCALE, causal=True, key_lengths=kl, window=W)
                got.backward(g)
                assert torch.allclose(got, want, atol=atol, rtol=0), (fn.__name__, N, W, lengths)
                for a, b in zip(got_in, want_in):
                    assert torch.allclose(a.grad, b.grad, atol=atol, rtol=0), (fn.__name__, N, W, lengths)
            if W == 1 and lengths is None:
                assert torch.equal(attention(q, k, v, SCALE, causal=True, window=1), v)


@pytest.mark.parametrize("hkv", [2, 1])
def test_packed_and_grouped(hkv):
    torch.manual_seed(1)
    B, N, H, W = 2, 9, 2, 3
    qkv = torch.randn(B, N, (H + 2 * hkv) * D, dtype=torch.float64)
    kl = torch.tensor((9, 4), dtype=torch.int32)
    got = attention_packed(qkv, H, causal=True, key_lengths=kl, kv_heads=hkv, window=W)
    q = qkv[..., :H * D].view(B, N, H, D).transpose(1, 2)
    k, v = (qkv[..., o * D:(o + hkv) * D].view(B, N, hkv, D).transpose(1, 2).repeat_interleave(H // hkv, dim=1)
            for o in (H, H + hkv))
    want = _explicit(q, k, v, _mask(N, W, (9, 4), B)).transpose(1, 2).reshape(B, N, H * D)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)


def test_window_at_least_N_is_no_window():
    torch.manual_seed(2)
    N = 7
    q, k, v = (torch.randn(2, 2, N, D) for _ in range(3))
    kl = torch.tensor((7, 3), dtype=torch.int32)
    for W in (N, N + 3):
        assert torch.equal(attention(q, k, v, causal=True, window=W), attention(q, k, v, causal=True))
        assert torch.equal(attention(q, k, v, causal=True, key_lengths=kl, window=W),
                           attention(q, k, v, causal=True, key_lengths=kl))
        assert torch.equal(attention_ref(q, k, v, causal=True, window=W), attention_ref(q, k, v, causal=True))
    assert not torch.equal(attention(q, k, v, causal=True, window=N - 1), attention(q, k, v, causal=True))


# ---------------------------------------------------------------- cache paths
def _cache_oracle(q, kc, vc, lim, W):
    """q [B, T, H, D]; query (b, t) over its visible rows max(0, lim - W) .. lim - 1 only (host ints)."""
    out = torch.zeros_like(q)
    G = q.shape[2] // kc.shape[1]
    for b in range(q.shape[0]):
        for t in range(q.shape[1]):
            hi = lim[b][t]
            lo = 0 if W is None else max(0, hi - W)
            kk, vv = (c[b, :, lo:hi].repeat_interleave(G, dim=0) for c in (kc, vc))
            s = torch.einsum("hd,hjd->hj", q[b, t], kk) * SCALE
            out[b, t] = torch.einsum("hj,hjd->hd", torch.softmax(s, -1), vv)
    return out


@pytest.mark.parametrize("hkv", [2, 1])
@pytest.mark.parametrize("W", [1, 3, 8, 19, 20, 25])
def test_decode_reference_and_poison(W, hkv):
    torch.manual_seed(W)
    B, H, cap = 3, 2, 20
    lengths = (20, 9, 0)  # 0 behaves as 1
    q = torch.randn(B, H, D, dtype=torch.float64)
    kc, vc = (torch.randn(B, hkv, cap, D, dtype=torch.float64) for _ in range(2))
    lens = torch.tensor(lengths, dtype=torch.int32)
    lim = [[min(max(n, 1), cap)] for n in lengths]
    want = _cache_oracle(q[:, None], kc, vc, lim, W)[:, 0]
    got = attention_decode(q, kc, vc, lens, SCALE, kv_heads=hkv, window=W)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)
    assert torch.equal(got, _decode_ref(q, kc, vc, lens, SCALE, **({} if W >= cap else {"window": W})))
    if W >= cap:
        assert torch.equal(got, attention_decode(q, kc, vc, lens, SCALE, kv_heads=hkv))
    k2, v2 = kc.clone(), vc.clone()
    for b in range(B):  # NaN below the window and at or past the length
        k2[b, :, :max(0, lim[b][0] - W)] = float("nan")
        v2[b, :, :max(0, lim[b][0] - W)] = float("nan")
        k2[b, :, lim[b][0]:] = float("nan")
        v2[b, :, lim[b][0]:] = float("inf")
    assert torch.equal(attention_decode(q, k2, v2, lens, SCALE, kv_heads=hkv, window=W), got)


@pytest.mark.parametrize("hkv", [2, 1])
@pytest.mark.parametrize("T,W", [(1, 4), (5, 1), (5, 3), (5, 7), (5, 30), (12, 2)])
def test_extend_reference_and_poison(T, W, hkv):
    torch.manual_seed(10 * T + W)
    B, H, cap = 2, 2, 30
    pos = (11, 0)
    q = torch.randn(B, T, H, D, dtype=torch.float64)
    kc, vc = (torch.randn(B, hkv, cap, D, dtype=torch.float64) for _ in range(2))
    p = torch.tensor(pos, dtype=torch.int32)
    lim = [[min(max(pos[b] + t + 1, 1), cap) for t in range(T)] for b in range(B)]
    want = _cache_oracle(q, kc, vc, lim, W)
    got = attention_extend(q, kc, vc, p, SCALE, kv_heads=hkv, window=W)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)
    if W >= cap:
        assert torch.equal(got, attention_extend(q, kc, vc, p, SCALE, kv_heads=hkv))
    k2, v2 = kc.clone(), vc.clone()
    for b in range(B):  # NaN below the call's smallest lower limit and at or past pos + T
        k2[b, :, :max(0, lim[b][0] - W)] = float("nan")
        v2[b, :, :max(0, lim[b][0] - W)] = float("nan")
        k2[b, :, lim[b][-1]:] = float("nan")
        v2[b, :, lim[b][-1]:] = float("nan")
    assert torch.equal(attention_extend(q, k2, v2, p, SCALE, kv_heads=hkv, window=W), got)
    assert torch.equal(_extend_ref(q, k2, v2, p, SCALE, **({} if W >= cap else {"window": W})), got)


def test_packed_cache_functions():
    torch.manual_seed(5)
    B, H, cap, W = 2, 2, 16, 3
    p = torch.tensor((6, 2), dtype=torch.int32)
    kc, vc = (torch.randn(B, H, cap, D, dtype=torch.float64) for _ in range(2))
    one = torch.randn(B, 1, 3 * H * D, dtype=torch.float64)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    a = attention_decode_packed(one, H, k1, v1, p, window=W)
    b = attention_extend_packed(one, H, k2, v2, p, window=W)  # T == 1 IS the decode call
    assert torch.equal(a, b) and torch.equal(k1, k2) and torch.equal(v1, v2)
    assert torch.equal(a.view(B, H, D), attention_decode(one[:, 0, :H * D].reshape(B, H, D), k1, v1, p + 1, window=W))
    assert not torch.equal(a, attention_decode_packed(one, H, kc.clone(), vc.clone(), p))
    many = torch.randn(B, 4, 3 * H * D, dtype=torch.float64)
    got = attention_extend_packed(many, H, k1, v1, p, window=W)
    want = attention_extend(many[..., :H * D].reshape(B, 4, H, D), k1, v1, p, window=W)
    assert torch.equal(got.view(B, 4, H, D), want)


# ---------------------------------------------------------------- models/gpt.py, fp64
def _lm(window, **kw):
    torch.manual_seed(0)
    return TransformerLM(256, 32, 2, 2, 64, window=window, **kw).double()


LLAMA = dict(kv_heads=2, pos="rope", norm="rms", mlp="swiglu", bias=False, mlp_ratio=2.0)


@pytest.mark.parametrize("window,kw", [(4, {}), ((4, None), {}), (4, LLAMA), ((None, 3), LLAMA)],
                         ids=["w4", "w4-global", "llama-w4", "llama-global-w3"])
def test_incremental_matches_full_forward(window, kw):
    if "kv_heads" in kw:
        kw = dict(kw, kv_heads=1 if window == (None, 3) else 2)
    model = _lm(window, **kw)
    torch.manual_seed(1)
    tokens = torch.randint(0, 256, (2, 14))
    N = tokens.shape[1]
    with torch.no_grad():
        full = model(tokens)
        assert not torch.allclose(full, _lm(None, **kw)(tokens), atol=1e-6)  # the window is smaller than N
    # prefill + decode steps
    j = 6
    logits, cache = model.prefill(tokens[:, :j])
    assert torch.allclose(logits, full[:, j - 1], atol=1e-9, rtol=0)
    for t in range(j, N):
        step = model.decode_step(tokens[:, t], cache)
        assert torch.allclose(step, full[:, t], atol=1e-9, rtol=0), t
    # chunked extend from an empty cache
    cache = KVCache(model, 2, capacity=20)
    parts = torch.cat([model.extend(tokens[:, a:b], cache) for a, b in ((0, 5), (5, 6), (6, 14))], dim=1)
    assert torch.allclose(parts, full, atol=1e-9, rtol=0), (parts - full).abs().max()
    # generate(cache=) over two turns equals one shot
    p, turn2 = tokens[:, :5], tokens[:, 7:10]
    cache = KVCache(model, 2, capacity=40)
    out1, _ = model.generate(p, 4, cache=cache)
    assert torch.equal(out1, model.generate(p, 4)[0])
    out2, _ = model.generate(torch.cat([out1[:, -1:], turn2], dim=1), 5, cache=cache)
    assert torch.equal(out2, model.generate(torch.cat([p, out1, turn2], dim=1), 5)[0])
    with torch.no_grad():  # greedy generation is the argmax of the full forward
        seq = torch.cat([p, out1], dim=1)
        assert torch.equal(model(seq)[:, 4:-1].argmax(-1), out1)


def test_draft_and_target_may_differ_in_window():
    target, draft = _lm(4), _lm((2, None))
    tokens = torch.randint(0, 256, (2, 6), generator=torch.Generator().manual_seed(3))
    want, _ = target.generate(tokens, 7)
    got, _ = target.generate(tokens, 7, draft=draft, draft_tokens=3)
    assert torch.equal(got, want)


@pytest.mark.parametrize("W", [1, 3])
def test_receptive_field(W):
    torch.manual_seed(0)
    model = TransformerLM(256, 32, 1, 2, 32, window=W).double()
    tokens = torch.randint(0, 256, (2, 10), generator=torch.Generator().manual_seed(4))
    other = tokens.clone()
    other[:, 0] = (other[:, 0] + 1) % 256
    with torch.no_grad():
        a, b = model(tokens), model(other)
    assert torch.equal(a[:, W:], b[:, W:])
    for i in range(W):
        assert not torch.equal(a[:, i], b[:, i]), i


def test_default_model_is_unchanged():
    torch.manual_seed(0)
    a = gpt_tiny()
    torch.manual_seed(0)
    b = gpt_tiny(window=None)
    torch.manual_seed(0)
    c = TransformerLM(256, 128, 2, 2, 128, window=(None, None))
    torch.manual_seed(0)
    w = gpt_tiny(window=5)  # a window adds no parameter and draws nothing from the RNG
    tokens = torch.randint(0, 256, (2, 9))
    with torch.no_grad():
        want = a(tokens)
        for m in (b, c):
            assert list(m.state_dict()) == list(a.state_dict())
            assert torch.equal(m(tokens), want)
        assert list(w.state_dict()) == list(a.state_dict())
        assert all(torch.equal(x, y) for x, y in zip(w.state_dict().values(), a.state_dict().values()))
        assert torch.equal(w(tokens)[:, :5], want[:, :5]) and not torch.equal(w(tokens), want)
        wide = gpt_tiny(window=9)  # window >= N
        wide.load_state_dict(a.state_dict())
        assert torch.equal(wide(tokens), want)


def test_block_and_attention_keyword():
    torch.manual_seed(0)
    blk = Block(32, 2, causal=True, window=3).double()
    assert blk.attn.window == 3 and Block(32, 2, causal=True).attn.window is None
    x = torch.randn(2, 7, 32, dtype=torch.float64)
    with torch.no_grad():
        full = blk.attn(x)
        cache = tuple(torch.empty(2, 2, 10, 16, dtype=torch.float64) for _ in range(2))
        pos = torch.zeros(2, dtype=torch.int32)
        pre = blk.attn(x[:, :4], cache=cache, positions=pos)  # prefill
        assert torch.allclose(pre, full[:, :4], atol=1e-12, rtol=0)
        ext = blk.attn(x[:, 4:6], cache=cache, positions=pos + 4, extend=True)
        one = blk.attn(x[:, 6:], cache=cache, positions=pos + 6)
        assert torch.allclose(torch.cat([ext, one], dim=1), full[:, 4:], atol=1e-12, rtol=0)


def test_errors():
    q = torch.randn(1, 1, 4, D)
    kc = torch.randn(1, 1, 6, D)
    pos = torch.zeros(1, dtype=torch.int32)
    qkv = torch.randn(1, 4, 3 * D)
    for fn in (attention, attention_ref):
        with pytest.raises(ValueError):
            fn(q, q, q, window=2)  # needs causal
        for bad in (0, -1, 2.0, "2", True):
            with pytest.raises(ValueError):
                fn(q, q, q, causal=True, window=bad)
    with pytest.raises(ValueError):
        attention_packed(qkv, 1, window=2)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError):
            attention_packed(qkv, 1, causal=True, window=bad)
        with pytest.raises(ValueError):
            attention_decode(q[:, :, 0], kc, kc, pos, window=bad)
        with pytest.raises(ValueError):
            attention_decode_packed(qkv[:, :1], 1, kc.clone(), kc.clone(), pos, window=bad)
        with pytest.raises(ValueError):
            attention_extend(q.transpose(1, 2), kc, kc, pos, window=bad)
        with pytest.raises(ValueError):
            attention_extend_packed(qkv, 1, kc.clone(), kc.clone(), pos, window=bad)
        with pytest.raises(ValueError):
            Attention(32, 2, causal=True, window=bad)
        with pytest.raises(ValueError):
            TransformerLM(16, 32, 2, 2, 8, window=bad)
    with pytest.raises(ValueError):
        Attention(32, 2, window=2)  # needs causal
    with pytest.raises(ValueError):
        TransformerLM(16, 32, 2, 2, 8, window=(2,))  # one entry, two layers
    with pytest.raises(ValueError):
        TransformerLM(16, 32, 2, 2, 8, window=(2, None, 2))
