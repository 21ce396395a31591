"""tests/test_lm_step.py on the native path: ``decode_step`` is ``extend`` of one token with
``last_only=True`` bit for bit -- logits, positions, held cache rows -- on bf16 ``gpt_tiny``-sized models
(head dim 64), default and fused, with a cache of one decode chunk and of two (the merge kernel runs).
The kernels are deterministic and the two calls launch the same ones, so every comparison is ``torch.equal``.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.models.gpt import KVCache, TransformerLM  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402

DEV = "cuda"
B, STEPS = 2, 3
PREFILL = (5, 3)


@pytest.fixture(scope="module", params=[(None, "learned"), (None, "rope"), (1, "learned"), (1, "rope")],
                ids=["mha-learned", "mha-rope", "mqa-learned", "mqa-rope"])
def setup(request):
    kv_heads, pos = request.param
    torch.manual_seed(0)
    model = TransformerLM(256, 128, 2, 2, 256, kv_heads=kv_heads, pos=pos).to(DEV).to(torch.bfloat16).eval()
    prompt = torch.randint(0, 256, (B, max(PREFILL)), device=DEV)
    tok = torch.randint(0, 256, (B, STEPS), device=DEV)
    return model, prompt, tok, torch.tensor(PREFILL, dtype=torch.int32, device=DEV)


def _held(cache):
    pos = cache.positions.tolist()
    return [t[b, :, :pos[b]] for kv in cache.layers for t in kv for b in range(len(pos))]


@pytest.mark.parametrize("capacity", [64, 200], ids=["one-chunk", "two-chunks"])
@pytest.mark.parametrize("fused", [False, True], ids=["default", "fused"])
def test_decode_step_is_extend_of_one_token(setup, fused, capacity):
    model, prompt, tok, lengths = setup
    chunk = _ext.native().attn_decode_set_chunk(-1)
    assert (capacity > chunk) == (capacity == 200), chunk  # 200 rows: split and merge; 64: the split alone
    kw = {"fused": True} if fused else {}
    c1, c2 = KVCache(model, B, capacity=capacity), KVCache(model, B, capacity=capacity)
    first, _ = model.prefill(prompt, lengths, c1)
    again, _ = model.prefill(prompt, lengths, c2)
    assert torch.equal(first, again)
    for j in range(STEPS):
        a = model.decode_step(tok[:, j], c1, **kw)
        b = model.extend(tok[:, j:j + 1], c2, last_only=True, **kw)
        assert a.shape == (B, 256) and torch.isfinite(a).all()
        assert torch.equal(a, b), (j, (a.float() - b.float()).abs().max().item())
        assert torch.equal(c1.positions, c2.positions)
        assert c1.positions.tolist() == [n + j + 1 for n in PREFILL]
        for r1, r2 in zip(_held(c1), _held(c2)):
            assert torch.equal(r1, r2)
