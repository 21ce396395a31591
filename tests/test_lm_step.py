"""``TransformerLM.decode_step`` IS ``extend`` of one token with ``last_only=True``: models/gpt.py runs
both through one step body, and this pins the identity that body rests on -- logits, positions and every
held cache row ``torch.equal``, on the PyTorch (CPU) path, default and fused.
"""
import pytest
import torch

from torchbooster_amd.models.gpt import KVCache, TransformerLM

VOCAB, B, STEPS = 97, 3, 5
PREFILL = (5, 3, 1)


def _held(cache):
    """The cache rows below each sequence's position, layer by layer."""
    pos = cache.positions.tolist()
    return [t[b, :, :pos[b]] for kv in cache.layers for t in kv for b in range(len(pos))]


@pytest.mark.parametrize("fused", [False, True], ids=["default", "fused"])
@pytest.mark.parametrize("pos", ["learned", "rope"])
@pytest.mark.parametrize("kv_heads", [None, 1], ids=["mha", "mqa"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16], ids=["fp64", "bf16"])
def test_decode_step_is_extend_of_one_token(dtype, kv_heads, pos, fused):
    torch.manual_seed(0)
    model = TransformerLM(VOCAB, 128, 2, 2, 32, kv_heads=kv_heads, pos=pos).to(dtype).eval()
    prompt = torch.randint(0, VOCAB, (B, max(PREFILL)))
    tok = torch.randint(0, VOCAB, (B, STEPS))
    lengths = torch.tensor(PREFILL, dtype=torch.int32)
    kw = {"fused": True} if fused else {}
    c1, c2 = KVCache(model, B), KVCache(model, B)
    first, _ = model.prefill(prompt, lengths, c1)
    again, _ = model.prefill(prompt, lengths, c2)
    assert torch.equal(first, again)
    for j in range(STEPS):
        a = model.decode_step(tok[:, j], c1, **kw)
        b = model.extend(tok[:, j:j + 1], c2, last_only=True, **kw)
        assert a.shape == (B, VOCAB) and torch.isfinite(a.float()).all()
        assert torch.equal(a, b), (j, (a.float() - b.float()).abs().max())
        assert torch.equal(c1.positions, c2.positions)
        assert c1.positions.tolist() == [n + j + 1 for n in PREFILL]
        for r1, r2 in zip(_held(c1), _held(c2)):
            assert torch.equal(r1, r2)
