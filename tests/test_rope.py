"""Rotary position embeddings on the PyTorch (CPU) path, in fp64: ``rope_table`` / ``rope_packed`` of
ops/attention.py, ``embed_rows`` without a position table, and ``TransformerLM(pos="rope")``.

Convention under test (rotate-half, the GPT-NeoX / Llama layout): a head vector ``x`` of even length ``D``
at position ``p``, ``theta_i = base ** (-2 * i / D)``, ``c = cos(p * theta_i)``, ``s = sin(p * theta_i)``:
``y[i] = x[i] * c - x[i + D/2] * s`` and ``y[i + D/2] = x[i + D/2] * c + x[i] * s``; token ``t`` of batch ``b``
is at ``clamp(positions[b] + t, 0, max_len - 1)``.  The op oracle is an explicit loop over (batch, token,
head, i) with ``math.cos`` / ``math.sin`` of the formula: it shares no code with ``rope_packed``.
Tolerances mirror tests/test_gqa.py: ``atol=1e-9, rtol=0`` for model logits against the full forward;
the op comparisons are ``1e-12`` (a handful of fp64 roundings on values of order one).

The model tests multiply every ``attn.qkv.weight`` by 8 so that positions matter to the logits: at the
default init scale the scores are so small that dropping the rotation moves the logits by ~0.02, at this
scale by 0.6 - 0.7 at a logit scale of 0.85, eight orders of magnitude above the ``1e-9`` bars.
"""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from torchbooster_amd.models.gpt import KVCache, TransformerLM, gpt_tiny
from torchbooster_amd.ops.attention import rope_packed, rope_table
from torchbooster_amd.ops.linear import embed_rows

B, H, D, MAXLEN = 2, 4, 16, 24
BASE = 10000.0
F64 = torch.float64
POSITIONS = [None, (0, 7), (-3, MAXLEN + 5)]


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32)


def _data(hkv, T, seed=0):
    g = torch.Generator().manual_seed(100 * hkv + T + seed)
    return torch.randn(B, T, (H + 2 * hkv) * D, generator=g, dtype=F64)


def _oracle(x, hkv, positions, inverse=False, max_len=MAXLEN, base=BASE):
    """the formula, one element at a time"""
    out = x.clone()
    T = x.shape[1]
    for b in range(B):
        for t in range(T):
            p = min(max((0 if positions is None else positions[b]) + t, 0), max_len - 1)
            for h in range(H + hkv):  # q heads, then k heads; the value part stays
                o = h * D
                for i in range(D // 2):
                    ang = p * base ** (-2.0 * i / D)
                    c, s = math.cos(ang), (-math.sin(ang) if inverse else math.sin(ang))
                    a, z = float(x[b, t, o + i]), float(x[b, t, o + i + D // 2])
                    out[b, t, o + i] = a * c - z * s
                    out[b, t, o + i + D // 2] = z * c + a * s
    return out


@pytest.fixture(scope="module")
def table():
    return rope_table(MAXLEN, D, BASE, dtype=F64)


# ---------------------------------------------------------------- the op
@pytest.mark.parametrize("hkv", [4, 2, 1])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("inverse", [False, True])
def test_rope_packed_matches_the_formula(table, hkv, T, positions, inverse):
    x = _data(hkv, T)
    keep = x.clone()
    got = rope_packed(x, H, table, _i32(positions), kv_heads=hkv, inverse=inverse)
    want = _oracle(x, hkv, positions, inverse)
    assert got.shape == x.shape and torch.equal(x, keep)
    assert torch.allclose(got, want, atol=1e-12, rtol=0), (got - want).abs().max()
    assert torch.equal(got[..., (H + hkv) * D:], x[..., (H + hkv) * D:])  # the value part, bit for bit
    # in place: the same numbers in the same storage
    y = x.clone()
    ret = rope_packed(y, H, table, _i32(positions), kv_heads=hkv, inverse=inverse, inplace=True)
    assert ret.data_ptr() == y.data_ptr() and torch.equal(y, got)
    # the inverse undoes it
    back = rope_packed(got, H, table, _i32(positions), kv_heads=hkv, inverse=not inverse)
    assert torch.allclose(back, x, atol=1e-12, rtol=0)


def test_default_kv_heads_is_heads(table):
    x = _data(H, 3)
    assert torch.equal(rope_packed(x, H, table), rope_packed(x, H, table, kv_heads=H))


def test_strided_view(table):
    wide = torch.randn(B, 5, (H + 4) * D + 8, generator=torch.Generator().manual_seed(2), dtype=F64)
    view = wide[..., 8:]
    got = rope_packed(view, H, table, _i32((0, 7)), kv_heads=2)
    assert torch.equal(got, rope_packed(view.contiguous(), H, table, _i32((0, 7)), kv_heads=2))


def test_gradient_is_the_inverse_rotation(table):
    hkv, pos = 2, _i32((0, 7))
    x = _data(hkv, 3).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: rope_packed(t, H, table, pos, kv_heads=hkv), (x,))
    assert torch.autograd.gradcheck(lambda t: rope_packed(t, H, table, pos, kv_heads=hkv, inverse=True), (x,))
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(9), dtype=F64)
    y = rope_packed(x, H, table, pos, kv_heads=hkv)
    (dx,) = torch.autograd.grad(y, x, g)
    assert torch.equal(dx, rope_packed(g, H, table, pos, kv_heads=hkv, inverse=True))
    assert dx.data_ptr() != g.data_ptr()
    assert torch.equal(dx[..., (H + hkv) * D:], g[..., (H + hkv) * D:])


@pytest.mark.parametrize("shift", [1, 6])
def test_scores_depend_on_relative_positions_only(table, shift):
    """q at positions m, k at positions n: q . k is unchanged when both move by ``shift`` (inside the table)."""
    T = 5
    x = _data(H, T, seed=3)
    m = (2, 9)
    assert max(m) + T - 1 + shift < MAXLEN

    def scores(pos):
        y = rope_packed(x, H, table, _i32(pos))
        q = y[..., :H * D].reshape(B, T, H, D)
        k = y[..., H * D:2 * H * D].reshape(B, T, H, D)
        return torch.einsum("bthd,buhd->bhtu", q, k)

    a, b = scores(m), scores(tuple(p + shift for p in m))
    assert torch.allclose(a, b, atol=1e-10, rtol=0), (a - b).abs().max()
    assert (a - scores(None)[..., :, :]).abs().max() < 1e-10  # positions 0 .. T - 1 are a shift as well
    assert (a - torch.einsum("bthd,buhd->bhtu", x[..., :H * D].reshape(B, T, H, D),
                             x[..., H * D:2 * H * D].reshape(B, T, H, D))).abs().max() > 1e-2  # and it rotates


# ---------------------------------------------------------------- the table
def test_rope_table():
    t64 = rope_table(MAXLEN, D, BASE, dtype=F64)
    t32 = rope_table(MAXLEN, D, BASE)
    assert t64.shape == t32.shape == (MAXLEN, 2, D // 2)
    assert t32.dtype == torch.float32 and t64.dtype == F64
    assert torch.equal(t32, t64.to(torch.float32))  # rounded once
    for p in (0, 1, MAXLEN - 1):
        for i in (0, 3, D // 2 - 1):
            ang = p * BASE ** (-2.0 * i / D)
            assert abs(float(t64[p, 0, i]) - math.cos(ang)) < 1e-13 and abs(float(t64[p, 1, i]) - math.sin(ang)) < 1e-13
    assert torch.equal(t64[0, 0], torch.ones(D // 2, dtype=F64)) and torch.equal(t64[0, 1], torch.zeros(D // 2, dtype=F64))
    with pytest.raises(ValueError):
        rope_table(MAXLEN, D, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        rope_table(MAXLEN, 15)


def test_model_table_survives_dtype_changes():
    want64 = rope_table(32, 32, BASE, dtype=F64)
    model = TransformerLM(64, 128, 2, 4, 32, kv_heads=2, pos="rope")
    assert all(blk.attn.rope is model.rope for blk in model.blocks)  # one shared object
    assert not any("rope" in k for k in model.state_dict()) and not list(model.buffers())
    model = model.to(torch.bfloat16)
    t = model.rope.table(model.tok.weight)
    assert t.dtype == torch.float32 and torch.equal(t, want64.to(torch.float32))
    model = model.double()
    t = model.rope.table(model.tok.weight)
    assert t.dtype == F64 and torch.equal(t, want64)
    clone = copy.deepcopy(model)
    assert clone.rope is not model.rope and all(blk.attn.rope is clone.rope for blk in clone.blocks)
    assert torch.equal(clone.rope.table(clone.tok.weight), want64)
    tokens = torch.randint(0, 64, (2, 6), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert torch.equal(clone(tokens), model(tokens))


# ---------------------------------------------------------------- errors
def test_errors(table):
    x = _data(2, 3)
    with pytest.raises(ValueError):
        rope_packed(x, H, table, kv_heads=3)
    with pytest.raises(RuntimeError):
        rope_packed(x, H, table)  # the width of kv_heads = 2 is not 3 * H * D
    with pytest.raises(RuntimeError):
        rope_packed(x, H, rope_table(MAXLEN, 2 * D, dtype=F64), kv_heads=2)  # table of another head dim
    with pytest.raises(RuntimeError):
        rope_packed(x, H, table, torch.zeros(B, dtype=torch.int64), kv_heads=2)  # positions are int32
    with pytest.raises(RuntimeError):
        rope_packed(x.clone().requires_grad_(), H, table, kv_heads=2, inplace=True)
    with torch.no_grad():  # forward-only use is fine
        rope_packed(x.clone().requires_grad_(), H, table, kv_heads=2, inplace=True)
    with pytest.raises(ValueError):
        TransformerLM(64, 128, 1, 4, 32, pos="sinusoid")


# ---------------------------------------------------------------- model
@pytest.fixture(scope="module")
def lm():
    torch.manual_seed(0)
    model = TransformerLM(64, 128, 2, 4, 32, kv_heads=2, pos="rope").double()
    with torch.no_grad():
        for blk in model.blocks:
            blk.attn.qkv.weight.mul_(8)
    tokens = torch.randint(0, 64, (2, 14))
    with torch.no_grad():
        full = model(tokens)
    return model, tokens, full


def test_positions_matter(lm, monkeypatch):
    """The setup is sensitive: without the rotation the logits move by a good part of their own size."""
    import torchbooster_amd.models.vit as vit

    model, tokens, full = lm
    monkeypatch.setattr(vit, "rope_packed", lambda qkv, *a, **k: qkv)
    with torch.no_grad():
        flat = model(tokens)
    assert (flat - full).abs().max() > 0.1, (flat - full).abs().max()


@pytest.mark.parametrize("fused", [False, True])
def test_decode_step_matches_full_forward(lm, fused):
    model, tokens, full = lm
    j = 5
    logits, cache = model.prefill(tokens[:, :j])
    assert torch.allclose(logits, full[:, j - 1], atol=1e-9, rtol=0)
    got = torch.stack([model.decode_step(tokens[:, t], cache, fused=fused) for t in range(j, 14)], dim=1)
    assert cache.positions.tolist() == [14, 14]
    assert torch.allclose(got, full[:, j:], atol=1e-9, rtol=0), (got - full[:, j:]).abs().max()


@pytest.mark.parametrize("fused", [False, True])
def test_extend_matches_full_forward(lm, fused):
    model, tokens, full = lm
    j = 5
    _, cache = model.prefill(tokens[:, :j])
    got = torch.cat([model.extend(tokens[:, j:j + 4], cache, fused=fused),
                     model.extend(tokens[:, j + 4:], cache, fused=fused)], dim=1)
    assert cache.positions.tolist() == [14, 14]
    assert torch.allclose(got, full[:, j:], atol=1e-9, rtol=0), (got - full[:, j:]).abs().max()


@pytest.mark.parametrize("fused", [False, True])
def test_ragged_prefill_then_decode(lm, fused):
    """Sequences of 6 and 3 prompt tokens in one right-padded prefill, then decoding: each against the full
    forward of that sequence alone."""
    model, tokens, _ = lm
    lens = (6, 3)
    n_new = 5
    prompt = tokens[:, :6].clone()
    prompt[1, 3:] = 0  # padding
    logits, cache = model.prefill(prompt, _i32(lens))
    assert cache.positions.tolist() == list(lens)
    steps = [logits]
    feed = torch.stack([tokens[b, lens[b]:lens[b] + n_new] for b in range(2)])
    for t in range(n_new):
        steps.append(model.decode_step(feed[:, t], cache, fused=fused))
    got = torch.stack(steps, dim=1)  # [2, 1 + n_new, vocab]
    for b in range(2):
        with torch.no_grad():
            alone = model(tokens[b:b + 1, :lens[b] + n_new])[0]
        want = alone[lens[b] - 1:]
        assert torch.allclose(got[b], want, atol=1e-9, rtol=0), (b, (got[b] - want).abs().max())


def test_speculative_with_a_learned_multi_query_draft_equals_greedy(lm):
    model, tokens, _ = lm
    torch.manual_seed(1)
    draft = TransformerLM(64, 64, 1, 2, 32, kv_heads=1, pos="learned").double()
    plain, plain_len = model.generate(tokens[:, :4], 8)
    cur = tokens[:, :4]
    with torch.no_grad():
        for _ in range(8):
            cur = torch.cat([cur, model(cur)[:, -1].argmax(-1, keepdim=True)], dim=1)
    assert torch.equal(plain, cur[:, 4:])
    for fused in (False, True):
        out, out_len = model.generate(tokens[:, :4], 8, draft=draft, draft_tokens=3, fused=fused)
        assert torch.equal(out, plain) and torch.equal(out_len, plain_len)
    # and the other way round: a rope draft under a learned target
    torch.manual_seed(2)
    target = TransformerLM(64, 64, 1, 2, 32).double()
    plain, plain_len = target.generate(tokens[:, :4], 8)
    out, out_len = target.generate(tokens[:, :4], 8, draft=model, draft_tokens=3)
    assert torch.equal(out, plain) and torch.equal(out_len, plain_len)


def test_generate_continues_a_cache(lm):
    model, tokens, _ = lm
    plain, _ = model.generate(tokens[:, :6], 6)
    cache = KVCache(model, 2)
    model.prefill(tokens[:, :2], cache=cache)
    out, _ = model.generate(tokens[:, 2:6], 6, cache=cache)
    assert torch.equal(out, plain)


def test_loss_backward_reaches_every_parameter(lm):
    model, tokens, _ = lm
    model.zero_grad(set_to_none=True)
    loss = model.loss(tokens, _i32((14, 9)))
    loss.backward()
    assert torch.isfinite(loss)
    names = [n for n, _ in model.named_parameters()]
    assert "pos" not in names and "pos" not in model.state_dict() and model.pos is None
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert p.grad.abs().sum() > 0, name
    model.zero_grad(set_to_none=True)


# ---------------------------------------------------------------- the default is unchanged
def test_learned_is_the_model_it_always_was():
    torch.manual_seed(3)
    a = TransformerLM(64, 128, 1, 4, 32)
    torch.manual_seed(3)
    b = TransformerLM(64, 128, 1, 4, 32, pos="learned")
    na, nb = list(a.named_parameters()), list(b.named_parameters())
    assert [n for n, _ in na] == [n for n, _ in nb] and "pos" in dict(na)
    assert all(torch.equal(p, q) for (_, p), (_, q) in zip(na, nb))
    assert list(a.state_dict()) == list(b.state_dict())
    assert a.rope is None and all(blk.attn.rope is None for blk in a.blocks)
    # the same RNG draws: the stream stands where it stood
    torch.manual_seed(3)
    TransformerLM(64, 128, 1, 4, 32)
    after_a = torch.rand(1)
    torch.manual_seed(3)
    TransformerLM(64, 128, 1, 4, 32, pos="learned")
    assert torch.equal(after_a, torch.rand(1))
    # a rope model has the same parameters but the table
    torch.manual_seed(3)
    c = TransformerLM(64, 128, 1, 4, 32, pos="rope")
    assert [n for n, _ in c.named_parameters()] == [n for n, _ in na if n != "pos"]
    assert gpt_tiny(pos="rope").pos is None and gpt_tiny().pos is not None


def test_embed_rows_without_a_position_table():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(10, 8, generator=g, dtype=F64)
    tokens = torch.tensor([[0, 9, 3], [12, -1, 5]])  # two ids out of range
    want = F.embedding(tokens.clamp(0, 9), w)
    assert torch.equal(embed_rows(tokens, w, None), want)
    assert torch.equal(embed_rows(tokens, w), want)
    assert torch.equal(embed_rows(tokens, w, None, _i32((3, 100))), want)  # positions have nothing to select
