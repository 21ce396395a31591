"""Attention sinks on the PyTorch paths (CPU, fp64): the rule of ops/attention.py written out a second time -- an
explicit extra column over the rows a query sees, picked with host ints -- against everything the package computes
with ``sinks=``.  ``H = 3``, one sink per regime: +6 (takes most of the mass), 0 (near the scores), -4 (small)."""
import math

import pytest
import torch

from torchbooster_amd.models import gpt_tiny
from torchbooster_amd.models.gpt import TransformerLM
from torchbooster_amd.models.vit import Attention, Block
from torchbooster_amd.ops.attention import (attention, attention_decode, attention_decode_packed, attention_extend,
                                            attention_extend_packed, attention_packed, attention_ref)

D, H = 8, 3
SCALE = 1.0 / math.sqrt(D)
SINKS = torch.tensor([6.0, 0.0, -4.0])


def _rows(q, k, v, lim, W, sinks=SINKS):
    """q [B, T, H, D]; k, v [B, Hkv, n, D] logical rows.  Query (b, t) over its visible rows
    max(0, lim - W) .. lim - 1 (host ints) plus the sink column -> (o, lse [B, T, H])."""
    out, lse = torch.zeros_like(q), torch.zeros(q.shape[:3], dtype=q.dtype)
    G = q.shape[2] // k.shape[1]
    for b in range(q.shape[0]):
        for t in range(q.shape[1]):
            hi = lim[b][t]
            lo = 0 if W is None else max(0, hi - W)
            kk, vv = (c[b, :, lo:hi].repeat_interleave(G, dim=0) for c in (k, v))
            s = torch.cat((torch.einsum("hd,hjd->hj", q[b, t], kk) * SCALE, sinks.to(q.dtype)[:, None]), dim=-1)
            out[b, t] = torch.einsum("hj,hjd->hd", torch.softmax(s, -1)[:, :-1], vv)
            lse[b, t] = torch.logsumexp(s, -1)
    return out, lse


MODES = {"dense": {}, "causal": {"causal": True}, "ragged": {"causal": True, "lengths": (7, 3)},
         "window": {"causal": True, "window": 3}, "ragged-window": {"causal": True, "lengths": (7, 1), "window": 2}}


@pytest.mark.parametrize("mode", list(MODES))
def test_formula_and_gradients(mode):
    torch.manual_seed(0)
    B, N = 2, 7
    kw = dict(MODES[mode])
    lengths, W = kw.pop("lengths", (N, N)), kw.get("window")
    if "lengths" in MODES[mode]:
        kw["key_lengths"] = torch.tensor(lengths, dtype=torch.int32)
    q, k, v, g = (torch.randn(B, H, N, D, dtype=torch.float64) for _ in range(4))
    lim = [[min(lengths[b], i + 1) if kw.get("causal") else lengths[b] for i in range(N)] for b in range(B)]
    want, lse = (t.transpose(1, 2) for t in _rows(q.transpose(1, 2), k, v, lim, W))
    # the closed form of the issue: dsinks[h] = -sum_{b, i} exp(sinks[h] - lse) * rowsum(dO * O)
    dsinks = -(torch.exp(SINKS.double()[None, :, None] - lse) * (g * want).sum(-1)).sum((0, 2))
    for fn in (attention_ref, attention):
        s = SINKS.clone().requires_grad_()
        got = fn(q, k, v, SCALE, sinks=s, **kw)
        assert torch.allclose(got, want, atol=1e-12, rtol=0), fn.__name__
        got.backward(g)
        assert s.grad.dtype == torch.float32
        assert torch.allclose(s.grad.double(), dsinks, atol=0, rtol=1e-6), (s.grad, dsinks)  # one f32 rounding
        assert not torch.allclose(fn(q, k, v, SCALE, **kw), want, atol=1e-3)  # the sinks matter
    qkv = torch.cat([t.transpose(1, 2).reshape(B, N, H * D) for t in (q, k, v)], dim=-1)
    got = attention_packed(qkv, H, SCALE, sinks=SINKS, **kw).view(B, N, H, D).transpose(1, 2)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)
    # gradcheck: q, k, v at the default step; sinks are f32 by contract, so their step is 2^-7 -- exact in f32
    # at +6, 0 and -4 -- and the bar the central difference's own error, eps^2 / 6 * |f'''| < 1e-5 (|f'''| < 1)
    ins = [t[:1, :, :4].clone().requires_grad_() for t in (q, k, v)]
    kl = {} if "key_lengths" not in kw else {"key_lengths": torch.tensor([3], dtype=torch.int32)}
    flags = {x: kw[x] for x in ("causal", "window") if x in kw}
    assert torch.autograd.gradcheck(lambda *a: attention(*a, SCALE, sinks=SINKS, **flags, **kl), ins)
    assert torch.autograd.gradcheck(lambda s: attention(*ins, SCALE, sinks=s.float(), **flags, **kl),
                                    [SINKS.double().requires_grad_()], eps=2.0 ** -7, atol=1e-5, rtol=0)


@pytest.mark.parametrize("hkv", [3, 1])
@pytest.mark.parametrize("W,R", [(None, None), (5, None), (5, 8)], ids=["linear", "window", "rolling"])
def test_decode_and_extend_references(W, R, hkv):
    """Linear and rolling caches against the explicit form over the visible rows; hidden rows hold NaN."""
    torch.manual_seed(1)
    B, n, T = 2, (13, 4), 3  # tokens each sequence holds after the call; the extend feeds the last T
    kl, vl = (torch.randn(B, hkv, 16, D, dtype=torch.float64) for _ in range(2))
    q = torch.randn(B, T, H, D, dtype=torch.float64)
    lim = [[n[b] - T + t + 1 for t in range(T)] for b in range(B)]
    want = _rows(q, kl, vl, lim, W)[0]
    kc, vc = (torch.full((B, hkv, R or 16, D), float("nan"), dtype=torch.float64) for _ in range(2))
    for b in range(B):  # only the rows some query of the extend sees; a ring holds row j in slot j mod R
        for j in range(0 if W is None else max(0, lim[b][0] - W), n[b]):
            kc[b, :, j % (R or 16)], vc[b, :, j % (R or 16)] = kl[b, :, j], vl[b, :, j]
    kw = {"kv_heads": hkv, "sinks": SINKS, **({} if W is None else {"window": W}), **({"rolling": True} if R else {})}
    pos = torch.tensor([x - T for x in n], dtype=torch.int32)
    got = attention_extend(q, kc, vc, pos, SCALE, **kw)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)
    assert not torch.allclose(attention_extend(q, kc, vc, pos, SCALE, **{**kw, "sinks": None}), want, atol=1e-3)
    # the decode of the last query sees the rows of lim[b][-1]; the rows below its window may be NaN too
    one = attention_decode(q[:, -1], kc, vc, torch.tensor(n, dtype=torch.int32), SCALE, **kw)
    assert torch.allclose(one, want[:, -1], atol=1e-12, rtol=0)
    # the packed step appends its row and is the same on both functions
    qkv, at = torch.randn(B, 1, (H + 2 * hkv) * D, dtype=torch.float64), torch.tensor(n, dtype=torch.int32)
    c1, c2 = (kc.clone(), vc.clone()), (kc.clone(), vc.clone())
    a = attention_decode_packed(qkv, H, *c1, at, SCALE, **kw)
    assert torch.equal(a, attention_extend_packed(qkv, H, *c2, at, SCALE, **kw))
    assert torch.equal(a.view(B, H, D), attention_decode(qkv[:, 0, :H * D].reshape(B, H, D), *c1, at + 1, SCALE, **kw))


CONF = dict(sinks=True, norm="rms", mlp="swiglu", pos="rope", kv_heads=2, window=[4, None])


def _lm(**kw):
    torch.manual_seed(0)
    model = gpt_tiny(**{**CONF, **kw}).double()
    for i, blk in enumerate(model.blocks):
        if blk.attn.sinks is not None:
            blk.attn.sinks.data.copy_(torch.tensor([2.0 - i, -1.0]))
    return model


def test_incremental_matches_full_forward():
    model = _lm()
    assert all(b.attn.sinks.dtype == torch.float32 and b.attn.sinks.shape == (2,) for b in model.blocks)
    tokens = torch.randint(0, 256, (2, 14), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        full = model(tokens)
        assert not torch.allclose(full, _lm(sinks=False)(tokens), atol=1e-6)
    for fused in (False, True):
        logits, cache = model.prefill(tokens[:, :6])
        assert torch.allclose(logits, full[:, 5], atol=1e-9, rtol=0)
        for t in range(6, 9):
            assert torch.allclose(model.decode_step(tokens[:, t], cache, fused=fused), full[:, t], atol=1e-9, rtol=0)
        ext = model.extend(tokens[:, 9:], cache, fused=fused)
        assert torch.allclose(ext, full[:, 9:], atol=1e-9, rtol=0), fused
    out, _ = model.generate(tokens[:, :5], 6)  # a rolling cache and a draft without sinks change no token
    assert torch.equal(model.generate(tokens[:, :5], 6, rolling=True)[0], out)
    assert torch.equal(model.generate(tokens[:, :5], 6, draft=_lm(sinks=False), draft_tokens=3)[0], out)
    model.loss(tokens).backward()
    assert all(b.attn.sinks.grad.abs().min() > 0 for b in model.blocks)


def test_default_model_is_unchanged():
    torch.manual_seed(0)
    a = gpt_tiny(**{**CONF, "sinks": False})
    torch.manual_seed(0)
    b = gpt_tiny(**{k: v for k, v in CONF.items() if k != "sinks"})
    torch.manual_seed(0)
    c = gpt_tiny(**CONF)  # sinks draw nothing from the RNG and start at zero
    assert list(a.state_dict()) == list(b.state_dict())
    assert [k for k in c.state_dict() if k not in a.state_dict()] == ["blocks.0.attn.sinks", "blocks.1.attn.sinks"]
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]) and torch.equal(v, c.state_dict()[k]), k
    assert all(not blk.attn.sinks.any() for blk in c.blocks)
    assert c.to(torch.bfloat16).blocks[0].attn.sinks.dtype == torch.float32
    assert Block(32, 2, causal=True).attn.sinks is None and Block(32, 2, causal=True, sinks=True).attn.sinks.shape == (2,)


def test_errors():
    q, kc, qkv = torch.randn(1, H, 4, D), torch.randn(1, H, 6, D), torch.randn(1, 4, 3 * H * D)
    pos = torch.zeros(1, dtype=torch.int32)
    for bad in (SINKS.double(), SINKS[:2], SINKS[None], SINKS.tolist()):
        for call in (lambda: attention(q, q, q, sinks=bad), lambda: attention_ref(q, q, q, sinks=bad),
                     lambda: attention_packed(qkv, H, sinks=bad),
                     lambda: attention_decode(q[:, :, 0], kc, kc, pos, sinks=bad),
                     lambda: attention_decode_packed(qkv[:, :1], H, kc.clone(), kc.clone(), pos, sinks=bad),
                     lambda: attention_extend(q.transpose(1, 2), kc, kc, pos, sinks=bad),
                     lambda: attention_extend_packed(qkv, H, kc.clone(), kc.clone(), pos, sinks=bad)):
            with pytest.raises(ValueError):
                call()
    for bad in (1, None, "yes"):
        for make in (lambda: Attention(32, 2, causal=True, sinks=bad), lambda: TransformerLM(16, 32, 2, 2, 8, sinks=bad)):
            with pytest.raises(ValueError):
                make()
