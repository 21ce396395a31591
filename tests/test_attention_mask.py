"""Causal and key-length masks of ops/attention.py on the stock (CPU) path, and models/gpt.py.

The oracle is an explicit masked softmax in fp64 written out here; the clamp of ``key_lengths`` into
[1, N] (0 behaves as 1, N + 3 as N) is part of the contract on every path.
"""
import pytest
import torch

from torchbooster_amd.ops.attention import attention, attention_packed, attention_ref

B, H, N, D = 2, 2, 9, 16
SCALE = D ** -0.5


def _oracle(q, k, v, causal, lengths):
    """softmax over the visible keys only, in fp64, one (batch, head, query) row at a time."""
    q, k, v = q.double(), k.double(), v.double()
    out = torch.zeros_like(q)
    for b in range(q.shape[0]):
        lim_b = N if lengths is None else min(max(int(lengths[b]), 1), N)
        for h in range(q.shape[1]):
            for i in range(N):
                lim = min(lim_b, i + 1) if causal else lim_b
                s = (k[b, h, :lim] @ q[b, h, i]) * SCALE
                out[b, h, i] = torch.softmax(s, 0) @ v[b, h, :lim]
    return out


@pytest.fixture(scope="module")
def qkv():
    g = torch.Generator().manual_seed(0)
    return tuple(torch.randn(B, H, N, D, generator=g) for _ in range(3))


CASES = [(True, None), (False, [4, 9]), (True, [4, 9]), (False, [1, 6]), (True, [7, 2])]


@pytest.mark.parametrize("causal,lengths", CASES)
def test_masked_attention_matches_fp64(qkv, causal, lengths):
    q, k, v = qkv
    kl = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    want = _oracle(q, k, v, causal, lengths)
    got = attention(q, k, v, causal=causal, key_lengths=kl)
    ref = attention_ref(q, k, v, causal=causal, key_lengths=kl)
    assert got.shape == ref.shape == (B, H, N, D)
    assert torch.allclose(got.double(), want, atol=1e-5), (got.double() - want).abs().max()
    assert torch.allclose(ref.double(), want, atol=1e-5), (ref.double() - want).abs().max()
    packed = torch.stack([t.transpose(1, 2) for t in (q, k, v)], dim=2).reshape(B, N, 3 * H * D)
    got_p = attention_packed(packed, H, causal=causal, key_lengths=kl)
    assert torch.allclose(got_p.double(), want.transpose(1, 2).reshape(B, N, H * D), atol=1e-5)


def test_masked_attention_backward_cpu(qkv):
    q, k, v = (t.clone().requires_grad_() for t in qkv)
    kl = torch.tensor([4, 9], dtype=torch.int32)
    attention(q, k, v, causal=True, key_lengths=kl).sum().backward()
    # a key at or past the length of its batch gets no gradient; the last key only from the last query
    assert torch.count_nonzero(k.grad[0, :, 4:]) == 0 and torch.count_nonzero(v.grad[0, :, 4:]) == 0
    assert torch.count_nonzero(v.grad[1, :, 8]) > 0
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v))


@pytest.mark.parametrize("causal", [False, True])
def test_key_lengths_clamp(qkv, causal):
    """Lengths 0 and N + 3 behave as 1 and N."""
    q, k, v = qkv
    bad = torch.tensor([0, N + 3], dtype=torch.int32)
    good = torch.tensor([1, N], dtype=torch.int32)
    for fn in (attention, attention_ref):
        a = fn(q, k, v, causal=causal, key_lengths=bad)
        b = fn(q, k, v, causal=causal, key_lengths=good)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
    assert torch.allclose(attention(q, k, v, causal=causal, key_lengths=bad).double(),
                          _oracle(q, k, v, causal, [1, N]), atol=1e-5)


def test_unmasked_defaults_unchanged(qkv):
    q, k, v = qkv
    assert torch.equal(attention(q, k, v), attention(q, k, v, causal=False, key_lengths=None))
    assert torch.allclose(attention(q, k, v), attention_ref(q, k, v), atol=1e-6)


def test_key_lengths_validation(qkv):
    q, k, v = qkv
    with pytest.raises(ValueError):
        attention(q, k, v, key_lengths=torch.tensor([4, 9]))  # int64
    with pytest.raises(ValueError):
        attention(q, k, v, key_lengths=torch.tensor([4, 9, 9], dtype=torch.int32))  # not [B]


def test_transformer_lm_is_causal():
    from torchbooster_amd.models import gpt_tiny

    torch.manual_seed(0)
    n, j = 12, 7
    model = gpt_tiny().eval()
    tokens = torch.randint(0, 256, (2, n))
    other = tokens.clone()
    other[:, j:] = (other[:, j:] + 1 + torch.randint(0, 200, (2, n - j))) % 256
    with torch.no_grad():
        a, b = model(tokens), model(other)
    assert a.shape == (2, n, 256) and a.dtype == torch.float32
    assert torch.allclose(a[:, :j], b[:, :j], atol=1e-6)
    assert not torch.allclose(a[:, j:], b[:, j:], atol=1e-3)


def test_transformer_lm_lengths_hide_padding():
    """With lengths, the tokens at or past a sequence's length do not reach its valid positions
    (they would anyway not under the causal mask; the check is on a non-causal read of the same
    blocks) and the model trains through the masked path."""
    from torchbooster_amd.models import gpt_tiny
    from torchbooster_amd.models.vit import Block

    torch.manual_seed(1)
    blk = Block(32, 2).eval()
    x = torch.randn(2, 10, 32)
    y = x.clone()
    y[0, 6:] = torch.randn(4, 32)
    kl = torch.tensor([6, 10], dtype=torch.int32)
    with torch.no_grad():
        (sa, pa), (sb, pb) = blk(x, None, kl), blk(y, None, kl)
    assert torch.allclose((sa + pa)[0, :6], (sb + pb)[0, :6], atol=1e-6)
    assert torch.allclose((sa + pa)[1], (sb + pb)[1], atol=1e-6)
    model = gpt_tiny()
    logits = model(torch.randint(0, 256, (2, 10)), kl)
    logits.float().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_gpt2_small_param_count():
    from torchbooster_amd.models import gpt2_small

    V, d, L, P = 50257, 768, 12, 1024
    block = (2 * d) + (d * 3 * d + 3 * d) + (d * d + d) + (2 * d) + (d * 4 * d + 4 * d) + (4 * d * d + d)
    closed = V * d + P * d + L * block + 2 * d + d * V  # embeddings, blocks, final norm, untied bias-free head
    assert closed == 163_037_184
    model = gpt2_small()
    assert sum(p.numel() for p in model.parameters()) == closed
    assert model.head.weight is not model.tok.weight and model.head.bias is None
    assert model.blocks[0].attn.hd == 64 and model.blocks[0].attn.causal
