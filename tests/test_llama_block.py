"""RMSNorm, SwiGLU and the Llama-style ``TransformerLM`` on the CPU, in fp64 where it matters.

``rms_norm`` and ``swiglu`` are checked against their formulas written out element by element and with
``gradcheck``; ``linear_rows(rms=, act="swiglu")`` against the composition it stands for; the model
(``norm="rms", mlp="swiglu", bias=False, pos="rope", kv_heads=2``) by the incremental paths against the full
forward, as tests/test_rope.py does for the rotary model; and the default model against itself with the new
keywords spelled out: the same parameters from the same RNG draws, the same logits bit for bit.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from torchbooster_amd.models.gpt import KVCache, TransformerLM, gpt2_small, gpt_tiny
from torchbooster_amd.models.vit import Block, SwiGLU
from torchbooster_amd.ops.act import swiglu
from torchbooster_amd.ops.linear import linear_rows
from torchbooster_amd.ops.norm import LayerNorm, RMSNorm, rms_norm

F64 = torch.float64


def _randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


# ---------------------------------------------------------------- the two ops
@pytest.mark.parametrize("with_res", [False, True])
def test_rms_norm_is_the_formula(with_res):
    M, C, eps = 3, 10, 1e-6
    x, r, w = _randn(M, C, seed=1), _randn(M, C, seed=2), 1.0 + 0.2 * _randn(C, seed=3)
    if with_res:
        y, xs = rms_norm(x, w, eps, residual=r)
        assert torch.equal(xs, x + r)
    else:
        y, xs = rms_norm(x, w, eps), x
    assert y.dtype == F64 and y.shape == x.shape
    for m in range(M):
        ms = sum(float(xs[m, c]) ** 2 for c in range(C)) / C
        for c in range(C):
            want = float(xs[m, c]) / math.sqrt(ms + eps) * float(w[c])
            assert abs(float(y[m, c]) - want) < 1e-12, (m, c)
    # leading dims are kept, no weight is a weight of ones
    y3 = rms_norm(x.view(1, M, C), None, eps)
    assert y3.shape == (1, M, C) and torch.allclose(y3[0], rms_norm(x, torch.ones(C, dtype=F64), eps), atol=1e-15)


def test_swiglu_is_the_formula():
    M, Fh = 3, 5
    gu = _randn(M, 2 * Fh, seed=4, scale=3.0)
    y = swiglu(gu)
    assert y.shape == (M, Fh) and y.dtype == F64
    for m in range(M):
        for c in range(Fh):
            g, u = float(gu[m, c]), float(gu[m, Fh + c])
            assert abs(float(y[m, c]) - g / (1.0 + math.exp(-g)) * u) < 1e-12, (m, c)
    assert swiglu(gu.view(1, M, 2 * Fh)).shape == (1, M, Fh)
    with pytest.raises(ValueError):
        swiglu(gu[:, :9])


def test_gradcheck():
    x = _randn(4, 8, seed=5).requires_grad_()
    r = _randn(4, 8, seed=6).requires_grad_()
    w = (1.0 + 0.2 * _randn(8, seed=7)).requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: rms_norm(a, b, 1e-6), (x, w))
    assert torch.autograd.gradcheck(lambda a, c, b: rms_norm(a, b, 1e-6, residual=c), (x, r, w))
    gu = _randn(4, 12, seed=8, scale=2.0).requires_grad_()
    assert torch.autograd.gradcheck(swiglu, (gu,))


def test_rms_norm_module_keeps_an_f32_weight():
    m = RMSNorm(16)
    assert list(m.state_dict()) == ["weight"] and torch.equal(m.weight, torch.ones(16)) and m.eps == 1e-6
    m = m.to(torch.bfloat16)
    assert m.weight.dtype == torch.float32
    x = torch.randn(2, 3, 16, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    y = m(x)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    y2, xs = m(x, x)
    assert y2.dtype == torch.bfloat16 and torch.equal(xs, x + x)


# ---------------------------------------------------------------- linear_rows
def test_linear_rows_argument_checks():
    x, w, b = _randn(2, 8, seed=10), _randn(6, 8, seed=11), _randn(6, seed=12)
    g = torch.ones(8, dtype=F64)
    with pytest.raises(ValueError):
        linear_rows(x, w, b, ln=(g, g, 1e-6), rms=(g, 1e-6))
    with pytest.raises(ValueError):
        linear_rows(x, w, b, act="swiglu", residual=_randn(2, 3, seed=13))
    with pytest.raises(ValueError):
        linear_rows(x, w[:5], b[:5], act="swiglu")
    with pytest.raises(ValueError):
        linear_rows(x, w, b, act="relu")


@pytest.mark.parametrize("with_bias", [False, True])
def test_linear_rows_equals_the_composition(with_bias):
    x, w = _randn(2, 3, 8, seed=14), _randn(6, 8, seed=15)
    b = _randn(6, seed=16) if with_bias else None
    g = 1.0 + 0.2 * _randn(8, seed=17)
    want = swiglu(F.linear(rms_norm(x, g, 1e-6), w, b))
    got = linear_rows(x, w, b, rms=(g, 1e-6), act="swiglu")
    assert got.shape == (2, 3, 3) and torch.allclose(got, want, atol=1e-14, rtol=0)
    # each on its own, with the other prologue / epilogues
    assert torch.allclose(linear_rows(x, w, b, rms=(g, 1e-6)), F.linear(rms_norm(x, g, 1e-6), w, b), atol=1e-14)
    assert torch.allclose(linear_rows(x, w, b, rms=(g, 1e-6), act="gelu"),
                          F.gelu(F.linear(rms_norm(x, g, 1e-6), w, b)), atol=1e-14)
    beta = 0.1 * _randn(8, seed=18)
    assert torch.allclose(linear_rows(x, w, b, ln=(g, beta, 1e-6), act="swiglu"),
                          swiglu(F.linear(F.layer_norm(x, (8,), g, beta, 1e-6), w, b)), atol=1e-14)
    # ln=(gamma, None, eps) keeps meaning LayerNorm without a bias
    assert torch.allclose(linear_rows(x, w, b, ln=(g, None, 1e-6)), F.linear(F.layer_norm(x, (8,), g, None, 1e-6), w, b),
                          atol=1e-14)
    with pytest.raises(RuntimeError):
        linear_rows(x, w, b, rms=(g.clone().requires_grad_(), 1e-6))


# ---------------------------------------------------------------- model
@pytest.fixture(scope="module")
def lm():
    torch.manual_seed(0)
    model = TransformerLM(64, 128, 2, 4, 32, kv_heads=2, pos="rope", norm="rms", mlp="swiglu", bias=False).double()
    with torch.no_grad():
        for blk in model.blocks:
            blk.attn.qkv.weight.mul_(8)
            blk.mlp.fc1.weight.mul_(8)
            blk.ln1.weight.add_(0.1 * torch.randn(128, dtype=F64))
            blk.ln2.weight.add_(0.1 * torch.randn(128, dtype=F64))
        model.norm.weight.add_(0.1 * torch.randn(128, dtype=F64))
    tokens = torch.randint(0, 64, (2, 14))
    with torch.no_grad():
        full = model(tokens)
    return model, tokens, full


def test_the_model_is_built_of_the_new_parts(lm):
    model, _, _ = lm
    keys = list(model.state_dict())
    assert not any(k.endswith(".bias") for k in keys), keys
    assert isinstance(model.norm, RMSNorm)
    for blk in model.blocks:
        assert isinstance(blk.ln1, RMSNorm) and isinstance(blk.ln2, RMSNorm) and isinstance(blk.mlp, SwiGLU)
        assert blk.mlp.fc1.weight.shape == (2 * 512, 128) and blk.mlp.fc2.weight.shape == (128, 512)
        assert blk.attn.qkv.bias is None and blk.attn.proj.bias is None
    assert model.head.bias is None and model.pos is None


def test_the_gate_matters(lm, monkeypatch):
    """The setup is sensitive: with the gate's SiLU taken out the logits move by a good part of their size."""
    import torchbooster_amd.models.vit as vit

    model, tokens, full = lm
    monkeypatch.setattr(vit, "swiglu", lambda gu: gu[..., :gu.shape[-1] // 2] * gu[..., gu.shape[-1] // 2:])
    with torch.no_grad():
        flat = model(tokens)
    assert (flat - full).abs().max() > 0.1, (flat - full).abs().max()


@pytest.mark.parametrize("fused", [False, True])
def test_decode_step_matches_full_forward(lm, fused):
    model, tokens, full = lm
    j = 5
    logits, cache = model.prefill(tokens[:, :j])
    assert torch.allclose(logits, full[:, j - 1], atol=1e-10, rtol=0)
    got = torch.stack([model.decode_step(tokens[:, t], cache, fused=fused) for t in range(j, 14)], dim=1)
    assert cache.positions.tolist() == [14, 14]
    assert torch.allclose(got, full[:, j:], atol=1e-10, rtol=0), (got - full[:, j:]).abs().max()


@pytest.mark.parametrize("fused", [False, True])
def test_extend_matches_full_forward(lm, fused):
    model, tokens, full = lm
    j = 5
    _, cache = model.prefill(tokens[:, :j])
    got = torch.cat([model.extend(tokens[:, t:t + 3], cache, fused=fused) for t in range(j, 14, 3)], dim=1)  # T = 3
    assert cache.positions.tolist() == [14, 14]
    assert torch.allclose(got, full[:, j:], atol=1e-10, rtol=0), (got - full[:, j:]).abs().max()


@pytest.mark.parametrize("fused", [False, True])
def test_generate_greedy_equals_the_recompute_loop(lm, fused):
    model, tokens, _ = lm
    out, out_len = model.generate(tokens[:, :4], 8, fused=fused)
    cur = tokens[:, :4]
    with torch.no_grad():
        for _ in range(8):
            cur = torch.cat([cur, model(cur)[:, -1].argmax(-1, keepdim=True)], dim=1)
    assert torch.equal(out, cur[:, 4:]) and out_len.tolist() == [8, 8]
    # continuing a cache, and a default-block draft under the Llama-style target
    cache = KVCache(model, 2)
    model.prefill(tokens[:, :2], cache=cache)
    assert torch.equal(model.generate(tokens[:, 2:4], 8, cache=cache, fused=fused)[0], out)
    torch.manual_seed(1)
    draft = TransformerLM(64, 64, 1, 2, 32).double()
    assert torch.equal(model.generate(tokens[:, :4], 8, draft=draft, draft_tokens=3, fused=fused)[0], out)


def test_loss_backward_reaches_every_parameter(lm):
    model, tokens, _ = lm
    model.zero_grad(set_to_none=True)
    loss = model.loss(tokens, _i32((14, 9)))
    loss.backward()
    assert torch.isfinite(loss)
    for name, p in model.named_parameters():
        assert not name.endswith("bias"), name
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert p.grad.abs().sum() > 0, name
    model.zero_grad(set_to_none=True)


def test_each_option_on_its_own():
    tokens = torch.randint(0, 64, (2, 6), generator=torch.Generator().manual_seed(2))
    for kw in ({"norm": "rms"}, {"mlp": "swiglu"}, {"bias": False}):
        torch.manual_seed(4)
        model = TransformerLM(64, 64, 1, 2, 16, **kw).double()
        keys = list(model.state_dict())
        assert any(k.endswith("ln1.bias") for k in keys) == ("norm" not in kw)
        assert any(k.endswith("fc1.bias") for k in keys) == ("bias" not in kw)
        with torch.no_grad():
            full = model(tokens)
            _, cache = model.prefill(tokens[:, :3])
            got = model.extend(tokens[:, 3:], cache, fused=True)
        assert torch.allclose(got, full[:, 3:], atol=1e-10, rtol=0), kw


def test_unknown_options_raise():
    with pytest.raises(ValueError):
        TransformerLM(64, 128, 1, 4, 32, norm="batch")
    with pytest.raises(ValueError):
        TransformerLM(64, 128, 1, 4, 32, mlp="relu")
    with pytest.raises(ValueError):
        Block(64, 2, norm="group")
    with pytest.raises(ValueError):
        Block(64, 2, mlp="glu")


def test_factories_take_the_options():
    m = gpt_tiny(norm="rms", mlp="swiglu", bias=False, kv_heads=1, mlp_ratio=2.0, pos="rope")
    blk = m.blocks[0]
    assert isinstance(blk.ln1, RMSNorm) and blk.mlp.fc1.weight.shape == (2 * 256, 128) and blk.attn.kv_heads == 1
    assert blk.attn.qkv.bias is None and m.pos is None
    assert isinstance(gpt_tiny().blocks[0].ln1, LayerNorm)
    # mlp_ratio = 8/3 at dim 768: a SwiGLU MLP with the parameters of the 4x GELU MLP
    assert int(768 * 8 / 3) == 2048 and 3 * 768 * 2048 == 2 * 768 * 3072
    assert callable(gpt2_small)


# ---------------------------------------------------------------- the default is unchanged
def test_the_default_is_the_model_it_always_was():
    torch.manual_seed(3)
    a = TransformerLM(64, 128, 2, 4, 32)
    after_a = torch.rand(1)
    torch.manual_seed(3)
    b = TransformerLM(64, 128, 2, 4, 32, norm="layer", mlp="gelu", bias=True)
    assert torch.equal(after_a, torch.rand(1))  # the same RNG draws: the stream stands where it stood
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert any(k.endswith("ln1.bias") for k in sa) and any(k.endswith("fc1.bias") for k in sa)
    assert type(a.norm) is LayerNorm and all(type(blk.ln1) is LayerNorm for blk in a.blocks)
    tokens = torch.randint(0, 64, (2, 9), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        assert torch.equal(a(tokens), b(tokens))
        la, ca = a.prefill(tokens[:, :4])
        lb, cb = b.prefill(tokens[:, :4])
        assert torch.equal(la, lb)
        for fused in (False, True):
            assert torch.equal(a.decode_step(tokens[:, 4], ca, fused=fused), b.decode_step(tokens[:, 4], cb, fused=fused))
