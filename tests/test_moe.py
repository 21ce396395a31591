"""Mixture-of-experts on the CPU: the PyTorch path of ``ops.gemm.grouped_linear`` against the per-expert float64
product, and ``TransformerLM(mlp="moe")`` -- parameters, gradients, generation, validation."""
import pytest
import torch

from torchbooster_amd.models.gpt import KVCache, TransformerLM, gpt_tiny
from torchbooster_amd.models.vit import Block, MoE
from torchbooster_amd.ops.gemm import grouped_linear


def _lm(**kw):
    torch.manual_seed(0)
    return TransformerLM(97, 32, 2, 2, 24, 2.0, mlp="moe", experts=4, top_k=2, norm="rms", pos="rope", bias=False, **kw)


@pytest.mark.parametrize("offsets,bounds", [([0, 0, 1, 13, 30], [0, 0, 1, 13, 30]), ([0, 30, 30, 30, 30], None),
                                            ([3, 3, 3, 3, 3], [0, 3, 3, 3, 3]),
                                            ([0, 20, 10, 99, -4], [0, 20, 20, 34, 34])])
def test_grouped_linear_reference_path(offsets, bounds):
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(34, 24, generator=g).requires_grad_(), torch.randn(4, 16, 24, generator=g).requires_grad_()
    dy = torch.randn(34, 16, generator=g)
    y = grouped_linear(x, w, torch.tensor(offsets, dtype=torch.int32))
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    b = bounds or offsets
    ry, rdx, rdw = torch.zeros(34, 16, dtype=torch.float64), torch.zeros(34, 24, dtype=torch.float64), []
    for e in range(4):
        rows = slice(b[e], b[e + 1])
        ry[rows] = x[rows].double() @ w[e].double().t()
        rdx[rows] = dy[rows].double() @ w[e].double()
        rdw.append(dy[rows].double().t() @ x[rows].double())
    for got, ref in ((y, ry), (dx, rdx), (dw, torch.stack(rdw))):
        assert torch.allclose(got.double(), ref, atol=1e-4, rtol=0)
    assert not y[b[4]:].any() and not dx[b[4]:].any()  # rows of no expert


def test_lm_parameters_and_gradients():
    model = _lm()
    keys = set(model.state_dict())
    for i in range(2):
        assert {f"blocks.{i}.mlp.router.weight", f"blocks.{i}.mlp.fc1", f"blocks.{i}.mlp.fc2"} <= keys
    mlp = model.blocks[0].mlp
    assert mlp.router.weight.shape == (4, 32) and mlp.fc1.shape == (4, 128, 32) and mlp.fc2.shape == (4, 32, 64)
    tokens = torch.randint(0, 97, (2, 20))
    (model.loss(tokens) + 0.01 * sum(b.mlp.aux_loss() for b in model.blocks)).backward()
    for b in model.blocks:
        for p in (b.mlp.router.weight, b.mlp.fc1, b.mlp.fc2):
            assert p.grad is not None and p.grad.abs().amax(tuple(range(1, p.dim()))).min() > 0  # every expert


def test_lm_generate_and_decode():
    model = _lm().double()
    tokens = torch.randint(0, 97, (2, 12))
    out, n = model.generate(tokens, 4)
    assert out.shape == (2, 4) and n.tolist() == [4, 4]
    with torch.no_grad():
        full = model(tokens)
        _, cache = model.prefill(tokens[:, :11], cache=KVCache(model, 2))
        assert torch.allclose(model.decode_step(tokens[:, 11], cache), full[:, 11], atol=1e-9, rtol=0)
        with pytest.raises(ValueError, match="MoE"):
            model.decode_step(tokens[:, 11], cache, fused=True)
        with pytest.raises(ValueError, match="MoE"):
            model.generate(tokens, 4, fused=True)


def test_aux_loss_is_one_for_uniform_routing():
    moe = MoE(16, 24, experts=4, top_k=2)
    torch.nn.init.zeros_(moe.router.weight)  # all logits tie: every token takes experts 0 and 1, p_e = 1 / 4
    moe(torch.randn(6, 16))
    assert moe.aux_loss().item() == pytest.approx(4 * 2 * 0.5 * 0.25)


@pytest.mark.parametrize("kw", [{"experts": 0}, {"experts": 2.0}, {"experts": True}, {"top_k": 0}, {"top_k": 5},
                                {"top_k": 1.0}])
def test_validation(kw):
    for build in (lambda: MoE(16, 24, **{"experts": 4, **kw}), lambda: Block(16, 2, mlp="moe", **{"experts": 4, **kw}),
                  lambda: gpt_tiny(mlp="moe", **{"experts": 4, **kw})):
        with pytest.raises(ValueError):
            build()


def test_other_models_keep_their_parameters():
    torch.manual_seed(3)
    a = gpt_tiny().state_dict()
    torch.manual_seed(3)
    b = gpt_tiny(mlp="gelu").state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not any("router" in k for k in a)
