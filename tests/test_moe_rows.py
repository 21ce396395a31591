"""The PyTorch paths of the few-row MoE calls (``linear_rows_experts``, ``moe_route_rows``) against their formulas
written out in f64, ``quantize_rows`` on an MoE model, and fused MoE decoding on the CPU."""
import copy

import pytest
import torch
import torch.nn.functional as F

from torchbooster_amd.models.gpt import KVCache, gpt_tiny
from torchbooster_amd.ops.linear import linear_rows_experts, moe_route_rows, mx_dequantize, mx_quantize

F64 = torch.float64
E, K, FH, M, TOP = 4, 64, 96, 3, 2


def _stack(rows, k, seed):
    w = torch.randn(E * rows, k, generator=torch.Generator().manual_seed(seed), dtype=F64) / k ** 0.5
    codes, scales = mx_quantize(w)
    return codes.view(E, rows, k // 2), scales.view(E, rows, k // 32), mx_dequantize(codes, scales, F64).view(E, rows, k)


IDS = torch.tensor([[0, 3], [-2, 1], [9, 2]], dtype=torch.int32)  # two of them out of range: clamped
IDC = IDS.long().clamp(0, E - 1)


@pytest.mark.parametrize("pro", [None, "ln", "rms"])
@pytest.mark.parametrize("act", [None, "swiglu"])
def test_pair_mode_fallback(pro, act):
    codes, scales, wd = _stack(2 * FH, K, 1)
    g = torch.Generator().manual_seed(2)
    x, gamma, beta = torch.randn(M, K, generator=g, dtype=F64), torch.rand(K, generator=g, dtype=F64) + 0.5, \
        torch.randn(K, generator=g, dtype=F64)
    kw, h = {}, x
    if pro == "ln":
        kw, h = {"ln": (gamma, beta, 1e-6)}, F.layer_norm(x, (K,), gamma, beta, 1e-6)
    if pro == "rms":
        kw, h = {"rms": (gamma, 1e-6)}, x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * gamma
    want = torch.einsum("mk,mjqk->mjq", h, wd[IDC])
    if act:
        want = F.silu(want[..., :FH]) * want[..., FH:]
    got = linear_rows_experts(x, codes, scales, IDS, act=act, **kw)
    assert got.dtype == F64 and torch.allclose(got, want, atol=1e-12, rtol=1e-12)


@pytest.mark.parametrize("residual", [False, True])
def test_combine_mode_fallback(residual):
    codes, scales, wd = _stack(K, FH, 3)
    g = torch.Generator().manual_seed(4)
    x, res = torch.randn(M, TOP, FH, generator=g, dtype=F64), torch.randn(M, K, generator=g, dtype=F64)
    gates = torch.softmax(torch.randn(M, TOP, generator=g), -1)
    want = (gates.double()[:, :, None] * torch.einsum("mjk,mjqk->mjq", x, wd[IDC])).sum(1) + (res if residual else 0)
    got = linear_rows_experts(x, codes, scales, IDS, gates=gates, residual=res if residual else None)
    assert got.shape == (M, K) and torch.allclose(got, want, atol=1e-12, rtol=1e-12)


@pytest.mark.parametrize("pro", [None, "rms"])
def test_route_fallback(pro):
    g = torch.Generator().manual_seed(5)
    x, w, gamma = torch.randn(M, K, generator=g), torch.randn(8, K, generator=g), torch.rand(K, generator=g) + 0.5
    w[6] = w[1]  # a tie: the lower index first
    h = x if pro is None else x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * gamma
    logits = h.double() @ w.double().t()
    top, idx = torch.sort(logits, dim=-1, descending=True, stable=True)
    ids, gates = moe_route_rows(x, w, 3, **({} if pro is None else {"rms": (gamma, 1e-6)}))
    assert ids.dtype == torch.int32 and gates.dtype == torch.float32
    assert torch.equal(ids.long(), idx[:, :3])
    assert torch.allclose(gates.double(), torch.softmax(top[:, :3], -1), atol=1e-6, rtol=0)


def test_value_errors():
    codes, scales, _ = _stack(K, FH, 3)
    x, x3, gates = torch.randn(M, FH, dtype=F64), torch.randn(M, TOP, FH, dtype=F64), torch.rand(M, TOP)
    bad = [
        lambda: linear_rows_experts(x, codes[0], scales[0], IDS),  # not a stack
        lambda: linear_rows_experts(x, codes, scales[:, :, :2], IDS),  # scales do not fit the codes
        lambda: linear_rows_experts(x, codes.float(), scales, IDS),
        lambda: linear_rows_experts(x, codes, scales, IDS.long()),
        lambda: linear_rows_experts(x[:2], codes, scales, IDS),
        lambda: linear_rows_experts(x, codes, scales, IDS, gates=gates),  # combine mode wants [M, top_k, K]
        lambda: linear_rows_experts(x3, codes, scales, IDS, gates=gates.double()),
        lambda: linear_rows_experts(x3, codes, scales, IDS, gates=gates, act="swiglu"),
        lambda: linear_rows_experts(x3, codes, scales, IDS, gates=gates, residual=torch.zeros(M, K + 1, dtype=F64)),
        lambda: linear_rows_experts(x, codes, scales, IDS, residual=torch.zeros(M, K, dtype=F64)),
        lambda: linear_rows_experts(x, codes[:, :63], scales[:, :63], IDS, act="swiglu"),
        lambda: moe_route_rows(x, torch.randn(8, FH + 1, dtype=F64), 2),
        lambda: moe_route_rows(x, torch.randn(8, FH, dtype=F64), 9),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()


def _moe_model():
    torch.manual_seed(11)
    m = gpt_tiny(mlp="moe", experts=4, top_k=2, norm="rms", pos="rope", bias=False).double().eval()
    for blk in m.blocks:
        blk.mlp.router.weight.data *= 16.0  # wide routing margins
    return m


def test_quantize_rows_snapshots_the_experts():
    m = _moe_model()
    keys = set(m.state_dict())
    m.quantize_rows()
    mx = m.blocks[1].mx_rows
    assert set(mx) == {"qkv", "proj", "fc1", "fc2"} and set(m.state_dict()) == keys
    assert [tuple(t.shape) for t in mx["fc1"] + mx["fc2"]] == [(4, 1024, 64), (4, 1024, 4), (4, 128, 256), (4, 128, 16)]
    assert all(t.dtype == torch.uint8 for t in mx["fc1"] + mx["fc2"])
    m.quantize_rows(None)
    assert m.blocks[1].mx_rows is None and m.mx_rows is None and set(m.state_dict()) == keys
    with pytest.raises(ValueError, match="quantize_rows"):
        m.decode_step(torch.zeros(2, dtype=torch.long), KVCache(m, 2), fused=True)


def test_fused_decode_equals_unfused_decode_of_the_dequantised_model():
    m = _moe_model()
    m.quantize_rows()
    ref = copy.deepcopy(m)
    ref.quantize_rows(None)
    lins = [ref.head] + [lin for b in ref.blocks for lin in (b.attn.qkv, b.attn.proj)]
    for w in [lin.weight for lin in lins] + [w for b in ref.blocks for w in (b.mlp.fc1, b.mlp.fc2)]:
        w.data = mx_dequantize(*mx_quantize(w.reshape(-1, w.shape[-1])), F64).view(w.shape)
    tokens = torch.randint(0, 256, (2, 5), generator=torch.Generator().manual_seed(12))
    ca, cb = KVCache(m, 2), KVCache(ref, 2)
    # the unfused MoE multiplies by the gates and sums in f32 whatever the dtype: 2^-24 relative per layer on
    # logits of order 1, against f64 sums here
    for t in (tokens[:, :4], tokens[:, 4:]):  # 16 pairs, then 4
        got, want = m.extend(t, ca, fused=True), ref.extend(t, cb)
        assert torch.allclose(got, want, atol=1e-6, rtol=0), (got - want).abs().max().item()
    got, want = m.decode_step(tokens[:, 0], ca, fused=True), ref.decode_step(tokens[:, 0], cb)
    assert torch.allclose(got, want, atol=1e-6, rtol=0)
    # with a cache the prompt goes through extend (a prefill would read m's unquantised parameters)
    assert torch.equal(m.generate(tokens, 5, fused=True, cache=KVCache(m, 2))[0],
                       ref.generate(tokens, 5, cache=KVCache(ref, 2))[0])
