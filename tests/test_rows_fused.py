"""Fused decoding on the PyTorch (CPU) path: ops/linear.py ``linear_rows`` / ``embed_rows`` and the
``fused=True`` control flow of models/gpt.py ``decode_step`` / ``extend`` / ``generate``.

On CPU tensors the few-row ops are their PyTorch composition, so the fused step must compute what the
default step computes: the model checks run in fp64 with the seed and setup of tests/test_decode.py and
tests/test_extend.py, where the two paths differ by ~1e-15 and the top-2 logit gaps those files state
(>= 1e-3) make token equality safe.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from torchbooster_amd.models import gpt_tiny
from torchbooster_amd.models.gpt import KVCache
from torchbooster_amd.ops.linear import embed_rows, linear_rows

K, Q = 24, 10


def _written_out(x, w, b, ln, act, res):
    h = x
    if ln is not None:
        g, be, eps = ln
        mu = h.mean(-1, keepdim=True)
        var = ((h - mu) ** 2).mean(-1, keepdim=True)
        h = (h - mu) / torch.sqrt(var + eps) * g + be
    y = h @ w.t()
    if b is not None:
        y = y + b
    if act == "gelu":
        y = 0.5 * y * (1.0 + torch.erf(y / 2.0 ** 0.5))
    if res is not None:
        y = y + res
    return y


@pytest.mark.parametrize("shape", [(1,), (17,), (2, 3)])
@pytest.mark.parametrize("with_ln,epi,with_bias",
                         list(itertools.product([False, True], [None, "gelu", "residual"], [False, True])))
def test_linear_rows_is_the_composition_fp64(shape, with_ln, epi, with_bias):
    g = torch.Generator().manual_seed(len(shape) + 7 * with_ln)
    x = torch.randn(*shape, K, generator=g, dtype=torch.float64)
    w = torch.randn(Q, K, generator=g, dtype=torch.float64)
    b = torch.randn(Q, generator=g, dtype=torch.float64) if with_bias else None
    ln = (torch.randn(K, generator=g, dtype=torch.float64), torch.randn(K, generator=g, dtype=torch.float64),
          1e-6) if with_ln else None
    res = torch.randn(*shape, Q, generator=g, dtype=torch.float64) if epi == "residual" else None
    got = linear_rows(x, w, b, ln=ln, act="gelu" if epi == "gelu" else None, residual=res)
    want = _written_out(x, w, b, ln, epi, res)
    assert got.shape == (*shape, Q) and got.dtype == torch.float64
    assert torch.allclose(got, want, atol=1e-12, rtol=0), (got - want).abs().max()


def test_linear_rows_f32_affine_on_fp64_rows_and_argument_checks():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, K, generator=g, dtype=torch.float64)
    w = torch.randn(Q, K, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(K, generator=g), torch.randn(K, generator=g)  # LayerNorm keeps its affine in f32
    got = linear_rows(x, w, ln=(gamma, beta, 1e-6))
    want = _written_out(x, w, None, (gamma.double(), beta.double(), 1e-6), None, None)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)
    with pytest.raises(ValueError):
        linear_rows(x, w, act="relu")
    with pytest.raises(ValueError):
        linear_rows(x, w, act="gelu", residual=torch.zeros(3, Q, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        linear_rows(x, w.clone().requires_grad_())
    with torch.no_grad():
        linear_rows(x, w.clone().requires_grad_())


def test_embed_rows_equals_embedding_plus_positions():
    g = torch.Generator().manual_seed(1)
    vocab, max_len, dim = 11, 9, 8
    tok = torch.randn(vocab, dim, generator=g, dtype=torch.float64)
    pos = torch.randn(max_len, dim, generator=g, dtype=torch.float64)
    tokens = torch.randint(0, vocab, (3, 4), generator=g)
    positions = torch.tensor((0, 3, 7), dtype=torch.int32)  # 7 + t runs past max_len - 1 = 8: clamped
    got = embed_rows(tokens, tok, pos, positions)
    at = (positions.long()[:, None] + torch.arange(4)[None]).clamp(0, max_len - 1)
    assert at[2].tolist() == [7, 8, 8, 8]
    assert torch.equal(got, tok[tokens] + pos[at])
    assert torch.equal(embed_rows(tokens, tok, pos), tok[tokens] + pos[:4][None])
    below = embed_rows(tokens, tok, pos, torch.tensor((-5, 0, 0), dtype=torch.int32))
    assert torch.equal(below[0], tok[tokens[0]] + pos[torch.tensor([0, 0, 0, 0])])
    # the one difference from nn.Embedding: an id outside [0, vocab) is clamped into range
    bad = torch.tensor([[-1, vocab, 3, vocab + 100]])
    got = embed_rows(bad, tok, pos, torch.zeros(1, dtype=torch.int32))
    assert torch.equal(got, tok[torch.tensor([[0, vocab - 1, 3, vocab - 1]])] + pos[:4][None])


# ---------------------------------------------------------------- models/gpt.py, fp64
@pytest.fixture(scope="module")
def lm():
    torch.manual_seed(0)
    model = gpt_tiny().double()
    tokens = torch.randint(0, 256, (2, 12))
    return model, tokens


def test_decode_step_fused_agrees_teacher_forced(lm):
    model, tokens = lm
    _, c1 = model.prefill(tokens[:, :3])
    _, c2 = model.prefill(tokens[:, :3])
    for j in range(3, 12):
        want = model.decode_step(tokens[:, j], c1)
        got = model.decode_step(tokens[:, j], c2, fused=True)
        assert got.shape == want.shape == (2, 256)
        assert torch.allclose(got, want, atol=1e-12, rtol=0), (j, (got - want).abs().max())
        assert torch.equal(c1.positions, c2.positions)
    for (k1, v1), (k2, v2) in zip(c1.layers, c2.layers):
        assert torch.allclose(k1[:, :, :12], k2[:, :, :12], atol=1e-12, rtol=0)
        assert torch.allclose(v1[:, :, :12], v2[:, :, :12], atol=1e-12, rtol=0)


def test_extend_fused_agrees_ragged_and_last_only(lm):
    model, tokens = lm
    j = 4
    for lens, last_only in itertools.product((None, torch.tensor((8, 3), dtype=torch.int32)), (False, True)):
        _, c1 = model.prefill(tokens[:, :j])
        _, c2 = model.prefill(tokens[:, :j])
        want = model.extend(tokens[:, j:], c1, lens, last_only=last_only)
        got = model.extend(tokens[:, j:], c2, lens, last_only=last_only, fused=True)
        assert got.shape == want.shape == ((2, 256) if last_only else (2, 8, 256))
        assert torch.allclose(got, want, atol=1e-12, rtol=0), (got - want).abs().max()
        assert torch.equal(c1.positions, c2.positions)
        assert c2.positions.tolist() == ([12, 12] if lens is None else [j + 8, j + 3])
    # one token per sequence goes through the decode attention
    _, c1 = model.prefill(tokens[:, :j])
    _, c2 = model.prefill(tokens[:, :j])
    want = model.extend(tokens[:, j:j + 1], c1)
    got = model.extend(tokens[:, j:j + 1], c2, fused=True)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)
    with pytest.raises(ValueError):
        model.extend(tokens, KVCache(model, 2, capacity=11), fused=True)


def test_generate_fused_is_token_equal(lm):
    model, tokens = lm
    want, want_len = model.generate(tokens[:, :4], 8)
    out, out_len = model.generate(tokens[:, :4], 8, fused=True)
    assert torch.equal(out, want) and torch.equal(out_len, want_len)
    lengths = torch.tensor((4, 7), dtype=torch.int32)
    assert torch.equal(model.generate(tokens[:, :7], 8, lengths, fused=True)[0],
                       model.generate(tokens[:, :7], 8, lengths)[0])
    eos = int(want[0, 2])
    want, want_len = model.generate(tokens[:, :4], 8, eos=eos)
    out, out_len = model.generate(tokens[:, :4], 8, eos=eos, fused=True)
    assert torch.equal(out, want) and torch.equal(out_len, want_len) and int(out_len[0]) <= 3


def test_generate_fused_two_turns_with_a_cache(lm):
    model, tokens = lm
    p, turn2 = tokens[:, :4], tokens[:, 6:9]
    n1, n2 = 5, 6
    caches = [KVCache(model, 2, capacity=40) for _ in range(2)]
    outs = []
    for cache, kw in zip(caches, ({}, {"fused": True})):
        out1, _ = model.generate(p, n1, cache=cache, **kw)
        out2, len2 = model.generate(torch.cat([out1[:, -1:], turn2], dim=1), n2, cache=cache, **kw)
        outs.append((out1, out2, len2))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert torch.equal(caches[0].positions, caches[1].positions)
    assert caches[1].positions.tolist() == [4 + n1 - 1 + 1 + 3 + n2 - 1] * 2


@pytest.mark.parametrize("which", ["self", "other"])
def test_generate_fused_speculative(lm, which):
    model, tokens = lm
    if which == "self":
        draft = model
    else:
        torch.manual_seed(1)
        draft = gpt_tiny().double()
    want, want_len = model.generate(tokens[:, :4], 9)
    out, out_len = model.generate(tokens[:, :4], 9, draft=draft, draft_tokens=4, fused=True)
    assert torch.equal(out, want) and torch.equal(out_len, want_len)


def test_fused_step_passes_the_flag_to_both_models(lm, monkeypatch):
    """``generate(fused=True, draft=...)`` makes every decode_step and extend of both models fused."""
    from torchbooster_amd.models.gpt import TransformerLM

    model, tokens = lm
    seen = []
    real_step, real_extend = TransformerLM.decode_step, TransformerLM.extend

    def step(self, *a, **k):
        seen.append(("step", k.get("fused", False)))
        return real_step(self, *a, **k)

    def extend(self, *a, **k):
        seen.append(("extend", k.get("fused", False)))
        return real_extend(self, *a, **k)

    monkeypatch.setattr(TransformerLM, "decode_step", step)
    monkeypatch.setattr(TransformerLM, "extend", extend)
    model.generate(tokens[:, :4], 6, draft=model, draft_tokens=2, fused=True)
    assert {s[0] for s in seen} == {"step", "extend"} and all(s[1] for s in seen)
    seen.clear()
    model.generate(tokens[:, :4], 3, cache=KVCache(model, 2), fused=True)
    assert {s[0] for s in seen} == {"step", "extend"} and all(s[1] for s in seen)
