"""Fused decoding on the GPU: the append folded into the decode attention (csrc/attention_decode.hip
``attn_decode_append``), ``embed_rows`` and the ``fused=True`` step of models/gpt.py.

``attention_decode_packed(fused=True)`` reorders no arithmetic: output and both caches are compared with
``torch.equal`` against append -> split -> merge, on the shapes of tests/test_gpu_decode.py.  The model
checks follow the protocol of test_gpt_tiny_incremental_vs_reference: against the stock fp32 model the
fused logits may be at most 1.5x as far off as the full native forward.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.models import gpt_tiny  # noqa: E402
from torchbooster_amd.models.gpt import KVCache  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops.attention import attention_decode_packed  # noqa: E402
from torchbooster_amd.ops.linear import embed_rows  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(params=[64, None], ids=["chunk64", "default"])
def chunk(request):
    nat = _ext.native()
    old = nat.attn_decode_set_chunk(-1)
    if request.param is not None:
        nat.attn_decode_set_chunk(request.param)
    try:
        yield nat.attn_decode_set_chunk(-1)
    finally:
        nat.attn_decode_set_chunk(old)


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _pos(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _case(B, H, cap):
    g = torch.Generator(device=DEV).manual_seed(1000 * cap + 10 * B + H)
    packed = torch.randn(B, 1, 3 * H * 64, device=DEV, generator=g).mul(1.5).to(BF)
    kc, vc = (torch.randn(B, H, cap, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    return packed, kc, vc


def _both(packed, H, kc, vc, pos):
    """(output, k cache, v cache) of the unfused and of the fused step on copies of the caches."""
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    o1 = attention_decode_packed(packed, H, k1, v1, pos)
    o2 = attention_decode_packed(packed, H, k2, v2, pos, fused=True)
    return (o1, k1, v1), (o2, k2, v2)


# the shapes of tests/test_gpu_decode.py CASES; the lengths there are positions + 1 here
CASES = [(1, 1, 1, (1,)), (2, 2, 70, (1, 70)), (4, 2, 200, (7, 8, 9, 200)), (4, 3, 200, (63, 64, 65, 129)),
         (2, 2, 520, (128, 520))]


@pytest.mark.parametrize("B,H,cap,lengths", CASES)
def test_fused_is_bit_equal(chunk, B, H, cap, lengths):
    packed, kc, vc = _case(B, H, cap)
    pos = _pos([n - 1 for n in lengths])
    (o1, k1, v1), (o2, k2, v2) = _both(packed, H, kc, vc, pos)
    assert o2.shape == (B, 1, H * 64) and o2.dtype == BF and torch.isfinite(o2).all()
    assert torch.equal(o1, o2) and torch.equal(k1, k2) and torch.equal(v1, v2)
    assert not torch.equal(k2, kc)  # the row was stored
    for b, n in enumerate(lengths):
        assert torch.equal(k2[b, :, n - 1], packed[b, 0].view(3, H, 64)[1])
        assert torch.equal(v2[b, :, n - 1], packed[b, 0].view(3, H, 64)[2])


@pytest.mark.parametrize("cap", [1, 64, 65, 128, 129])
def test_single_chunk_and_chunk_edges(chunk, cap):
    """cap <= chunk: the split kernel writes the output itself (no merge); one past it: two chunks."""
    B, H = 3, 2
    packed, kc, vc = _case(B, H, cap)
    for pos in ((0, 0, 0), (cap - 1, cap // 2, 0), (62, 63, 64), (63, 64, 65)):
        p = _pos([min(v, cap - 1) for v in pos])
        (o1, k1, v1), (o2, k2, v2) = _both(packed, H, kc, vc, p)
        assert torch.equal(o1, o2) and torch.equal(k1, k2) and torch.equal(v1, v2), (cap, pos)


def test_positions_outside_the_cache_are_dropped(chunk):
    B, H, cap = 4, 2, 200
    packed, kc, vc = _case(B, H, cap)
    pos = _pos((-1, cap, cap + 7, -(2 ** 31)))
    (o1, k1, v1), (o2, k2, v2) = _both(packed, H, kc, vc, pos)
    assert torch.equal(k2, kc) and torch.equal(v2, vc)  # nothing stored
    assert torch.equal(o1, o2) and torch.isfinite(o2).all()
    assert torch.equal(o2[0, 0].view(H, 64), vc[0, :, 0])  # length clamped to 1: exactly the first value row
    top = _pos((2 ** 31 - 1,) * B)
    (o1, k1, v1), (o2, k2, v2) = _both(packed, H, kc, vc, top)
    assert torch.equal(k2, kc) and torch.equal(o1, o2)


@pytest.mark.parametrize("fill", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_junk_at_or_past_the_position_never_enters(chunk, fill):
    """Every cache row at or past the position holds junk -- the position's own row too, which the step
    overwrites: the output is finite and equal to the zero-filled run."""
    B, H, cap = 4, 3, 200
    packed, kc, vc = _case(B, H, cap)
    positions = (62, 63, 64, 0)
    pos = _pos(positions)
    hidden = torch.arange(cap, device=DEV)[None, None, :, None] >= pos[:, None, None, None]

    def run(value):
        k2 = torch.where(hidden, torch.full_like(kc, value), kc)
        v2 = torch.where(hidden, torch.full_like(vc, value), vc)
        return attention_decode_packed(packed, H, k2, v2, pos, fused=True), k2, v2

    got, k2, v2 = run(fill)
    zero, _, _ = run(0.0)
    assert torch.isfinite(got).all() and torch.equal(got, zero)
    assert torch.equal(got[3, 0].view(H, 64), packed[3, 0].view(3, H, 64)[2])  # one visible key: its own v
    for b, p in enumerate(positions):
        assert torch.isfinite(k2[b, :, :p + 1]).all() and torch.isfinite(v2[b, :, :p + 1]).all()


def test_graph_replay_follows_positions():
    B, H, cap = 2, 2, 200
    packed, kc0, vc0 = _case(B, H, cap)
    pos = _pos((150, 20))
    kc, vc = kc0.clone(), vc0.clone()
    attention_decode_packed(packed, H, kc0.clone(), vc0.clone(), pos, fused=True)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = attention_decode_packed(packed, H, kc, vc, pos, fused=True)
    graph.replay()
    first = out.clone()
    pos.copy_(_pos((7, 199)))
    graph.replay()
    torch.cuda.synchronize()
    ke, ve = kc0.clone(), vc0.clone()
    assert torch.equal(first, attention_decode_packed(packed, H, ke, ve, _pos((150, 20))))
    assert torch.equal(out, attention_decode_packed(packed, H, ke, ve, _pos((7, 199))))
    assert not torch.equal(out, first)
    assert torch.equal(kc, ke) and torch.equal(vc, ve)


# ---------------------------------------------------------------- embed_rows
@torch.no_grad()
def test_embed_rows_is_bit_equal_and_clamps():
    torch.manual_seed(0)
    model = gpt_tiny().cuda().to(BF)
    B, T = 3, 5
    tokens = torch.randint(0, 256, (B, T), device=DEV)
    positions = _pos((0, 60, 125))  # 125 + t runs past max_len - 1 = 127
    at = positions.to(torch.int64)[:, None] + torch.arange(T, device=DEV)[None, :]
    want = model.tok(tokens) + model.pos[0][at.clamp(0, model.max_len - 1)].to(BF)  # extend's expression
    got = embed_rows(tokens, model.tok.weight, model.pos[0], positions)
    assert got.dtype == BF and torch.equal(got, want)
    at1 = positions.to(torch.int64).clamp(0, model.max_len - 1)
    want1 = (model.tok(tokens[:, 0]) + model.pos[0].index_select(0, at1).to(BF))[:, None]  # decode_step's
    assert torch.equal(embed_rows(tokens[:, :1], model.tok.weight, model.pos[0], positions), want1)
    assert torch.equal(embed_rows(tokens, model.tok.weight, model.pos[0]),
                       model.tok(tokens) + model.pos[:, :T].to(BF))
    bad = torch.tensor([[-1, 256, 2 ** 40, -(2 ** 40), 7]] * B, device=DEV)
    got = embed_rows(bad, model.tok.weight, model.pos[0], positions)
    ids = torch.tensor([[0, 255, 255, 0, 7]] * B, device=DEV)
    assert torch.isfinite(got).all() and torch.equal(got, embed_rows(ids, model.tok.weight, model.pos[0], positions))


# ---------------------------------------------------------------- gpt_tiny, bf16
@pytest.fixture(scope="module")
def tiny(request):
    """The models, tokens and the two full-forward logit sets of test_gpt_tiny_incremental_vs_reference:
    computed once, never modified."""
    import copy
    import os

    torch.manual_seed(0)
    B, N = 3, 70
    base = gpt_tiny().cuda()
    tokens = torch.randint(0, 256, (B, N), device=DEV)
    mnat = copy.deepcopy(base).to(BF)
    with torch.no_grad():
        full = mnat(tokens).float()
        old = os.environ.get("TBAMD_FORCE_REFERENCE")
        os.environ["TBAMD_FORCE_REFERENCE"] = "1"  # the stock run: every op on its PyTorch path
        try:
            ref = copy.deepcopy(base)(tokens).float()
        finally:
            if old is None:
                del os.environ["TBAMD_FORCE_REFERENCE"]
            else:
                os.environ["TBAMD_FORCE_REFERENCE"] = old
    return mnat, tokens, full, ref


def test_decode_step_fused_vs_reference(tiny):
    mnat, tokens, full, ref = tiny
    B, j, N = 2, 33, 70
    _, cache = mnat.prefill(tokens[:B, :j])
    steps = [mnat.decode_step(tokens[:B, t], cache, fused=True) for t in range(j, N - 1)]
    inc = torch.stack(steps, dim=1).float()
    assert cache.positions.tolist() == [N - 1] * B
    e_inc, e_full = _err(inc, ref[:B, j:N - 1]), _err(full[:B, j:N - 1], ref[:B, j:N - 1])
    print(f"gpt_tiny teacher-forced logits vs fp32: fused decode_step {e_inc:.5f} full forward {e_full:.5f} "
          f"({e_inc / e_full:.2f}x)")
    assert torch.isfinite(inc).all()
    assert e_inc <= 1.5 * e_full, (e_inc, e_full)


@pytest.mark.parametrize("B,T", [(2, 5), (3, 5), (2, 9)], ids=["10rows", "15rows", "18rows-fallback"])
def test_extend_fused_vs_reference(tiny, B, T):
    mnat, tokens, full, ref = tiny
    j = 33
    n = (70 - 1 - j) // T * T
    _, cache = mnat.prefill(tokens[:B, :j])
    parts = [mnat.extend(tokens[:B, t:t + T], cache, fused=True) for t in range(j, j + n, T)]
    inc = torch.cat(parts, dim=1).float()
    assert cache.positions.tolist() == [j + n] * B
    e_inc, e_full = _err(inc, ref[:B, j:j + n]), _err(full[:B, j:j + n], ref[:B, j:j + n])
    print(f"gpt_tiny extend(fused) B={B} T={T} vs fp32: {e_inc:.5f} full forward {e_full:.5f} "
          f"({e_inc / e_full:.2f}x)")
    assert torch.isfinite(inc).all()
    assert e_inc <= 1.5 * e_full, (e_inc, e_full)
    # last_only with ragged lengths picks those rows
    _, c2 = mnat.prefill(tokens[:B, :j])
    lens = _pos([T, 2, 1][:B])
    last = mnat.extend(tokens[:B, j:j + T], c2, lens, last_only=True, fused=True)
    assert last.shape == (B, 256) and c2.positions.tolist() == [j + v for v in [T, 2, 1][:B]]
    # the same logits from another launch shape (the 18-row case: from the other path): the project's bar
    assert _err(last, torch.stack([parts[0][b, v - 1] for b, v in enumerate([T, 2, 1][:B])])) < 1e-2


def test_nan_filled_cache_yields_finite_logits(tiny):
    mnat, tokens, _, _ = tiny
    cache = KVCache(mnat, 2, capacity=100)
    for k, v in cache.layers:
        k.fill_(float("nan"))
        v.fill_(float("nan"))
    logits, _ = mnat.prefill(tokens[:2, :9], cache=cache)
    assert torch.isfinite(logits).all()
    for t in range(9, 14):
        assert torch.isfinite(mnat.decode_step(tokens[:2, t], cache, fused=True)).all()
    assert torch.isfinite(mnat.extend(tokens[:2, 14:18], cache, fused=True)).all()
    assert cache.positions.tolist() == [18, 18]


def test_generate_fused_graph_equals_eager_and_speculative_runs(tiny):
    mnat, tokens, _, _ = tiny
    prompt = tokens[:2, :9]
    a, a_len = mnat.generate(prompt, 24, fused=True, graph=False)
    b, b_len = mnat.generate(prompt, 24, fused=True, graph=True)
    assert torch.equal(a, b) and torch.equal(a_len, b_len)
    assert a.shape == (2, 24) and int(a.min()) >= 0 and int(a.max()) < 256
    out, out_len = mnat.generate(prompt, 12, fused=True, draft=mnat, draft_tokens=4)
    assert out.shape == (2, 12) and out.dtype == torch.int64 and out_len.tolist() == [12, 12]
    assert int(out.min()) >= 0 and int(out.max()) < 256


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type.name == "CUDA"]


@pytest.mark.parametrize("capacity,per_layer", [(200, 6), (64, 5)])
def test_launch_census(capacity, per_layer):
    """One fused step: the embedding, per layer four products and the attention (split + merge, or the
    split alone with a single-chunk cache), the head and the position update."""
    torch.manual_seed(0)
    model = gpt_tiny(max_len=256).cuda().to(BF)
    depth = len(model.blocks)
    tokens = torch.randint(0, 256, (2, 12), device=DEV)
    counts = {}
    for fused in (False, True):
        kw = {"fused": True} if fused else {}
        cache = KVCache(model, 2, capacity=capacity)
        model.prefill(tokens[:, :8], cache=cache)
        model.decode_step(tokens[:, 8], cache, **kw)  # warm-up
        torch.cuda.synchronize()
        names = _kernels(lambda: model.decode_step(tokens[:, 9], cache, **kw))
        counts[fused] = len(names)
        if fused:
            assert sum("rows_linear_k" in n for n in names) == 4 * depth + 1, names
            assert sum("attn_decode_append_split_k" in n for n in names) == depth, names
            assert sum("attn_decode_merge_k" in n for n in names) == (depth if per_layer == 6 else 0), names
            assert not any("attn_kv_append_k" in n for n in names), names
    print(f"decode_step launches, gpt_tiny depth {depth}, capacity {capacity}: fused {counts[True]} "
          f"unfused {counts[False]}")
    assert counts[True] <= per_layer * depth + 3, (counts, names)
    assert counts[True] < counts[False], counts
