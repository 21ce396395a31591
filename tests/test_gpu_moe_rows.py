"""The few-row MoE kernels on the GPU (csrc/rows_experts_mx.hip): ``linear_rows_experts`` in pair and combine mode,
``moe_route_rows``, and a quantised MoE model on ``fused=True``.

Pair mode is checked bit for bit against the one-weight kernel (``linear_rows(mx_scales=)``); combine mode against
fp64 on the dequantised experts, with the bars of tests/test_gpu_rows_mx.py: relative Frobenius error below 1e-2,
and at most 1.5x the error of the composition of bf16-rounded pair products combined in f32 (more roundings).
The router is checked where the fp64 rule is unambiguous: every gap among the reference's first ``top_k + 1``
logits exceeds ``K * 2^-22 * max_e sum_k |h_k w_ek|``, four times the worst-case f32 summation error of two logits.
"""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.models.gpt import KVCache, gpt_tiny  # noqa: E402
from torchbooster_amd.models.vit import Block  # noqa: E402
from torchbooster_amd.ops.linear import (linear_rows, linear_rows_experts, moe_route_rows, mx_dequantize,  # noqa: E402
                                         mx_quantize)

DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
EPS = 1e-6
PROS = [None, "ln", "rms"]


def _experts(g, E, Qw, K):
    """Random codes under scales that vary by 2^+-6 from block to block, weights of about K^-0.5."""
    codes = torch.randint(0, 256, (E, Qw, K // 2), generator=g, dtype=torch.uint8).to(DEV)
    mid = 127 - 1 - round(0.5 * torch.log2(torch.tensor(float(K))).item())
    return codes, (mid + torch.randint(-6, 7, (E, Qw, K // 32), generator=g)).to(torch.uint8).to(DEV)


def _prologue(g, K, pro):
    gamma, beta = (1.0 + 0.2 * torch.randn(K, generator=g)).to(DEV), (0.1 * torch.randn(K, generator=g)).to(DEV)
    return {"ln": (gamma, beta, EPS)} if pro == "ln" else {"rms": (gamma, EPS)} if pro == "rms" else {}


def _normed(x, kw):
    """fp64 prologue, rounded to bf16 as the kernels round it."""
    h = x.double()
    if "ln" in kw:
        h = F.layer_norm(h, h.shape[-1:], kw["ln"][0].double(), kw["ln"][1].double(), EPS).to(BF).double()
    if "rms" in kw:
        h = (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS) * kw["rms"][0].double()).to(BF).double()
    return h


def _id_patterns(g, M, top_k, E):
    P = M * top_k
    rnd = torch.randint(0, E, (P,), generator=g)
    rnd[0], rnd[P - 1] = -3, E + 5  # (one id when P == 1): must equal the clamped call
    return [torch.full((P,), E - 1), torch.arange(P) % E, rnd]


# every (K, Q, (M, top_k)) of the list; the expert count, the prologue and the activation rotate through it
SHAPES = list(itertools.product([32, 96, 768, 2080, 4096], [7, 67], [(1, 1), (1, 4), (3, 2), (5, 3), (8, 2), (16, 1)]))
CASES = [(K, Q, M, k, [1, 4, 33][i % 3], PROS[i // 3 % 3], [None, "swiglu"][i // 2 % 2])
         for i, (K, Q, (M, k)) in enumerate(SHAPES)]


@pytest.mark.parametrize("K,Q,M,top_k,E,pro,act", CASES)
def test_pair_mode_has_the_bits_of_the_one_weight_kernel(K, Q, M, top_k, E, pro, act):
    g = torch.Generator().manual_seed(7919 * M + 31 * K + Q + top_k)
    codes, scales = _experts(g, E, 2 * Q if act else Q, K)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(BF).to(DEV)
    kw = dict(_prologue(g, K, pro), act=act)
    for ids in _id_patterns(g, M, top_k, E):
        out = linear_rows_experts(x, codes, scales, ids.view(M, top_k).int().to(DEV), **kw)
        assert out.shape == (M, top_k, Q) and out.dtype == BF
        for m, j in itertools.product(range(M), range(top_k)):
            e = int(ids[m * top_k + j].clamp(0, E - 1))
            assert torch.equal(out[m, j], linear_rows(x[m:m + 1], codes[e], mx_scales=scales[e], **kw)[0]), (m, j, e)


@pytest.mark.parametrize("K,Q,M,top_k,E", [c[:5] for c in CASES])
def test_combine_mode_against_f64(K, Q, M, top_k, E):
    g = torch.Generator().manual_seed(104729 + 7919 * M + 31 * K + Q + top_k)
    codes, scales = _experts(g, E, Q, K)
    x = (torch.randn(M, top_k, K, generator=g) * 1.5 + 0.3).to(BF).to(DEV)
    gates = torch.softmax(torch.randn(M, top_k, generator=g), -1).to(DEV)
    res = torch.randn(M, Q, generator=g).to(BF).to(DEV)
    ids = _id_patterns(g, M, top_k, E)[2].view(M, top_k).int().to(DEV)
    idc = ids.long().clamp(0, E - 1)
    wd = mx_dequantize(codes.view(E * Q, -1), scales.view(E * Q, -1), F64).view(E, Q, K)
    ref = res.double() + (gates.double()[:, :, None] * torch.einsum("mjk,mjqk->mjq", x.double(), wd[idc])).sum(1)
    got = linear_rows_experts(x, codes, scales, ids, gates=gates, residual=res)
    pairs = torch.stack([linear_rows(x[m, j:j + 1], codes[idc[m, j]], mx_scales=scales[idc[m, j]])[0]
                         for m in range(M) for j in range(top_k)]).view(M, top_k, Q)
    base = (res.float() + (gates[:, :, None] * pairs.float()).sum(1)).to(BF)
    assert got.shape == (M, Q) and got.dtype == BF and torch.isfinite(got).all()
    for name, v in [("all", lambda t: t.reshape(1, -1)), ("last 8 columns", lambda t: t[:, -8:].reshape(1, -1)),
                    ("rows", lambda t: t)]:
        den = v(ref).norm(dim=1).clamp_min(1e-300)
        e = (v(got).double() - v(ref)).norm(dim=1) / den
        e0 = (v(base).double() - v(ref)).norm(dim=1) / den
        print(f"K,Q,M,top_k,E={K},{Q},{M},{top_k},{E} {name}: fused {e.max().item():.2e} composed {e0.max().item():.2e}")
        assert (e < 1e-2).all(), (name, e.max().item())
        assert (e <= 1.5 * e0).all(), (name, e.tolist(), e0.tolist())
    assert torch.equal(got, linear_rows_experts(x, codes, scales, ids, gates=gates, residual=res))
    for m in (0, M - 1):  # a token alone has the bits it has among the others
        s = slice(m, m + 1)
        assert torch.equal(linear_rows_experts(x[s], codes, scales, ids[s], gates=gates[s], residual=res[s])[0], got[m]), m
    none = linear_rows_experts(x, codes, scales, ids, gates=gates)
    want = (gates.double()[:, :, None] * torch.einsum("mjk,mjqk->mjq", x.double(), wd[idc])).sum(1)
    assert ((none.double() - want).norm() / want.norm()).item() < 1e-2


def _router_inputs(E, K, M, pro, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(BF)
    w = (torch.randn(E, K, generator=g) * 4.0 / K ** 0.5).to(BF)
    return x.to(DEV), w.to(DEV), _prologue(g, K, pro)


def _route_ref(x, w, top_k, kw):
    """(ids, gates, logits) of the fp64 rule on the bf16-rounded normed row, after asserting that it is unambiguous."""
    h = _normed(x, kw)
    logits = h @ w.double().t()
    top, idx = torch.sort(logits, dim=-1, descending=True, stable=True)
    bound = x.shape[1] * 2.0 ** -22 * (h.abs() @ w.double().abs().t()).amax(dim=1, keepdim=True)
    if w.shape[0] > top_k:
        gaps = top[:, :top_k] - top[:, 1:top_k + 1]
        assert (gaps > bound).all(), (gaps.min().item(), bound.max().item())
    return idx[:, :top_k], torch.softmax(top[:, :top_k], dim=-1), logits


ROUTES = [(2, 1, 32, "rms", 0), (2, 2, 768, "ln", 0), (8, 2, 768, "rms", 0), (8, 4, 4096, "ln", 1), (33, 1, 32, "ln", 0),
          (33, 4, 768, "rms", 0), (256, 2, 4096, "rms", 5), (256, 4, 32, "ln", 0), (256, 1, 768, "ln", 0)]


@pytest.mark.parametrize("E,top_k,K,pro,seed", ROUTES)
def test_router_against_f64(E, top_k, K, pro, seed):
    x, w, kw = _router_inputs(E, K, 5, pro, seed)
    want_ids, want_gates, _ = _route_ref(x, w, top_k, kw)
    ids, gates = moe_route_rows(x, w, top_k, **kw)
    assert ids.dtype == torch.int32 and gates.dtype == torch.float32 and ids.shape == gates.shape == (5, top_k)
    assert torch.equal(ids.long(), want_ids)
    assert (gates.double() - want_gates).abs().max().item() <= 1e-5


def test_router_tie_goes_to_the_lower_index():
    x, w, _ = _router_inputs(8, 768, 3, None, 1)
    w[5] = w[2]
    x[:] = w[2] * 8.0  # rows 2 and 5 are the two largest logits, and equal
    ids, gates = moe_route_rows(x, w, 2)
    assert ids.tolist() == [[2, 5]] * 3 and torch.equal(gates, torch.full_like(gates, 0.5))


def _moe_calls(x, rw, fc1, fc2, top_k, kw):
    ids, gates = moe_route_rows(x, rw, top_k, **kw)
    h = linear_rows_experts(x, *fc1, ids, act="swiglu", **kw)
    return linear_rows_experts(h, *fc2, ids, gates=gates, residual=x)


def test_graph_capture_follows_the_routing():
    g = torch.Generator().manual_seed(5)
    E, K, Fh, M, top_k = 8, 768, 96, 4, 2
    fc1, fc2 = _experts(g, E, 2 * Fh, K), _experts(g, E, K, Fh)
    xs = [(torch.randn(M, K, generator=g) * 1.5).to(BF).to(DEV) for _ in range(3)]
    rw, kw = (torch.randn(E, K, generator=g) * 4.0 / K ** 0.5).to(BF).to(DEV), _prologue(g, K, "rms")
    want = [_moe_calls(t, rw, fc1, fc2, top_k, kw) for t in xs]  # also the warm-up
    routes = [moe_route_rows(t, rw, top_k, **kw)[0] for t in xs]
    assert not torch.equal(routes[0], routes[1]) and not torch.equal(routes[1], routes[2])
    buf = xs[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _moe_calls(buf, rw, fc1, fc2, top_k, kw)
    for i in (0, 1, 2, 1):
        buf.copy_(xs[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[i]), i


def test_block_moe_half_against_the_unfused_moe():
    torch.manual_seed(3)
    blk = Block(128, 2, causal=True, norm="rms", mlp="moe", experts=8, top_k=2, bias=False).to(DEV).to(BF).eval()
    blk.mlp.router.weight.data *= 16.0  # wide routing margins
    blk.quantize_rows()
    ref = copy.deepcopy(blk)
    for w in (ref.mlp.fc1, ref.mlp.fc2):
        w.data = mx_dequantize(*mx_quantize(w.reshape(-1, w.shape[2])), BF).view(w.shape)
    x = torch.randn(2, 3, 128).to(BF).to(DEV)
    with torch.no_grad():
        _route_ref(x.view(-1, 128), blk.mlp.router.weight, 2, {"rms": (blk.ln2.weight, blk.ln2.eps)})
        want = (x + ref.mlp(ref.ln2(x))).double()
        got = blk.moe_rows(x).double()
    e = ((got - want).norm() / want.norm()).item()
    print(f"block MoE half: fused against unfused on the dequantised experts {e:.2e}")
    assert e < 1e-2, e


def test_model_decodes_fused_after_quantize_rows():
    torch.manual_seed(21)
    m = gpt_tiny(mlp="moe", experts=4, top_k=2, norm="rms", pos="rope", bias=False).to(DEV).to(BF).eval()
    tokens = torch.randint(0, 256, (2, 4), device=DEV)
    with pytest.raises(ValueError, match="MoE"):
        m.decode_step(tokens[:, 0], KVCache(m, 2), fused=True)
    m.quantize_rows()
    assert m.blocks[0].mx_rows["fc1"][0].shape == (4, 1024, 64) and m.blocks[0].mx_rows["fc2"][1].shape == (4, 128, 16)
    cache = KVCache(m, 2)
    ext = m.extend(tokens, cache, fused=True)
    step = m.decode_step(tokens[:, 0], cache, fused=True)
    assert ext.shape == (2, 4, 256) and step.shape == (2, 256) and torch.isfinite(ext).all() and torch.isfinite(step).all()
    a, la = m.generate(tokens, 6, fused=True, graph=True)
    c, lc = m.generate(tokens, 6, fused=True, graph=False)
    assert torch.equal(a, c) and torch.equal(la, lc)
    win = gpt_tiny(mlp="moe", experts=4, top_k=2, norm="rms", pos="rope", bias=False, window=8).to(DEV).to(BF).eval()
    win.quantize_rows()
    out, _ = win.generate(tokens, 12, fused=True, rolling=True, kv_dtype=torch.float8_e4m3fn)
    assert out.shape[0] == 2
