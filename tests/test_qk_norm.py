"""QK-norm on the PyTorch (CPU) path: ``qk_norm_rope_packed`` of ops/attention.py in fp64 against the formula
written out independently, its gradients by ``gradcheck``, and ``TransformerLM(qk_norm=True)``: which
parameters it adds, what it rejects, and prefill + decode against the full forward."""
import pytest
import torch

from torchbooster_amd.models.gpt import TransformerLM, gpt_tiny
from torchbooster_amd.ops.attention import qk_norm_rope_packed, rope_packed, rope_table

F64 = torch.float64
B, T, H, HKV, D = 1, 3, 2, 1, 8


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, (H + 2 * HKV) * D, generator=g, dtype=F64)
    qw, kw = (1 + 0.5 * torch.randn(D, generator=g, dtype=F64) for _ in range(2))
    return qkv, qw, kw, rope_table(16, D, dtype=F64), torch.tensor([5], dtype=torch.int32)


@pytest.mark.parametrize("rotate", [True, False])
def test_formula_and_gradcheck(rotate):
    qkv, qw, kw, table, pos = _inputs()
    table = table if rotate else None
    got = qk_norm_rope_packed(qkv, H, qw, kw, 1e-6, table, pos, kv_heads=HKV)
    x = qkv[..., :(H + HKV) * D].reshape(B, T, H + HKV, D)
    n = x / (x.pow(2).sum(-1, keepdim=True) / D + 1e-6).sqrt() * torch.stack([qw] * H + [kw] * HKV)
    ref = torch.cat((n.reshape(B, T, -1), qkv[..., (H + HKV) * D:]), dim=-1)
    if rotate:  # the rotation has its own tests (tests/test_rope.py)
        ref = rope_packed(ref, H, table, pos, kv_heads=HKV)
    torch.testing.assert_close(got, ref, atol=1e-12, rtol=0)
    args = [t.clone().requires_grad_() for t in (qkv, qw, kw)]
    assert torch.autograd.gradcheck(lambda a, b, c: qk_norm_rope_packed(a, H, b, c, 1e-6, table, pos, kv_heads=HKV), args)


def test_parameters_with_and_without():
    torch.manual_seed(0)
    plain = gpt_tiny(pos="rope")
    torch.manual_seed(0)
    off = gpt_tiny(pos="rope", qk_norm=False)
    torch.manual_seed(0)
    on = gpt_tiny(pos="rope", qk_norm=True).to(torch.bfloat16)
    sd_plain, sd_off, sd_on = plain.state_dict(), off.state_dict(), on.state_dict()
    assert list(sd_plain) == list(sd_off) and all(torch.equal(sd_plain[k], sd_off[k]) for k in sd_plain)
    added = sorted(set(sd_on) - set(sd_plain))
    assert added == sorted(f"blocks.{i}.attn.{n}_norm.weight" for i in range(2) for n in "qk")
    assert set(sd_plain) <= set(sd_on)
    for k in added:
        assert sd_on[k].dtype == torch.float32 and sd_on[k].shape == (64,) and bool((sd_on[k] == 1).all())
    # no RNG draw: the other parameters are what the seed gives without the option
    assert all(torch.equal(sd_on[k], sd_plain[k].to(sd_on[k].dtype)) for k in sd_plain)


def test_raises():
    qkv, qw, kw, table, pos = _inputs()
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            TransformerLM(64, 32, 1, 2, 16, qk_norm=bad)
    with pytest.raises(RuntimeError):
        qk_norm_rope_packed(qkv, H, qw[:-1], kw, kv_heads=HKV)
    with pytest.raises(RuntimeError):
        qk_norm_rope_packed(qkv, H, qw, kw.to(torch.bfloat16), kv_heads=HKV)
    with pytest.raises(RuntimeError):
        qk_norm_rope_packed(qkv.float(), H, qw.float(), kw, kv_heads=HKV)  # f64 weights go with f64 inputs only
    with pytest.raises(RuntimeError):
        qk_norm_rope_packed(qkv, H, qw.requires_grad_(), kw, kv_heads=HKV, inplace=True)
    with torch.no_grad():
        keep = qkv.clone()
        out = qk_norm_rope_packed(qkv, H, qw, kw, 1e-6, table, pos, kv_heads=HKV, inplace=True)
        assert out is qkv
        assert torch.equal(out, qk_norm_rope_packed(keep, H, qw, kw, 1e-6, table, pos, kv_heads=HKV))


@pytest.mark.parametrize("pos", ["rope", "learned"])
def test_prefill_and_decode_equal_the_full_forward(pos):
    torch.manual_seed(1)
    model = gpt_tiny(pos=pos, norm="rms", kv_heads=1, qk_norm=True)
    with torch.no_grad():
        for blk in model.blocks:
            blk.attn.q_norm.weight.copy_(1 + 0.5 * torch.randn(64))
            blk.attn.k_norm.weight.copy_(1 + 0.5 * torch.randn(64))
    tokens = torch.randint(0, 256, (2, 12))
    with torch.no_grad():
        full = model(tokens)
        _, cache = model.prefill(tokens[:, :8])
        for t in range(8, 12):
            step = model.decode_step(tokens[:, t], cache)
        off = gpt_tiny(pos=pos, norm="rms", kv_heads=1)
        off.load_state_dict(model.state_dict(), strict=False)
        assert (off(tokens) - full).abs().max() > 1e-3  # the norm matters to the logits
    assert (step - full[:, -1]).norm() <= 1e-5 * full[:, -1].norm()
