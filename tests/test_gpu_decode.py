"""KV-cache decoding on the native kernels (csrc/attention_decode.hip): ``attn_kv_append``, the
split-KV ``attn_decode`` and its merge, and ``TransformerLM.prefill`` / ``decode_step`` / ``generate``.

The kernel bar is the forward bar of test_gpu_attention.py: relative Frobenius error < 1e-2 against
fp32 math on the bf16 inputs (inputs scaled as there, randn * 1.5).  Every kernel check runs with 64
keys per workgroup and with the default.  Shapes: a single key in a cache of one row; lengths on both
sides of a 64-key chunk edge (63, 64, 65) and inside the last partial chunk (129 of 200, 70 of 70);
lengths that leave most chunks empty (7, 8, 9 of 200); nine chunks (520).
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops import attention as A  # noqa: E402
from torchbooster_amd.ops.attention import (_AttnFn, attention, attention_decode, attention_decode_packed,  # noqa: E402
                                            attention_ref, kv_cache_append)

DEV = "cuda"
SCALE = 1.0 / math.sqrt(64)


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


def _lengths(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _oracle(q, kc, vc, lengths, scale=SCALE):
    """fp32 softmax over the visible keys only, one batch at a time (lengths: host ints, clamped)."""
    q, kc, vc = q.float(), kc.float(), vc.float()
    out = torch.zeros_like(q)
    for b, n in enumerate(lengths):
        n = min(max(n, 1), kc.shape[2])
        s = torch.einsum("hd,hjd->hj", q[b], kc[b, :, :n]) * scale
        out[b] = torch.einsum("hj,hjd->hd", torch.softmax(s, -1), vc[b, :, :n])
    return out


@functools.lru_cache(maxsize=None)
def _case(B, H, cap, lengths, D=64, dtype=torch.bfloat16):
    """q (a strided view into a packed [B, 1, 3*H*D] projection), the caches and the fp32 reference of
    one case: computed once, shared by the chunk settings, never modified."""
    g = torch.Generator(device=DEV).manual_seed(1000 * cap + 10 * B + H)
    packed = torch.randn(B, 1, 3 * H * D, device=DEV, generator=g).mul(1.5).to(dtype)
    kc, vc = (torch.randn(B, H, cap, D, device=DEV, generator=g).mul(1.5).to(dtype) for _ in range(2))
    q = packed.view(B, 3, H, D)[:, 0]
    return q, kc, vc, _oracle(q, kc, vc, lengths, 1.0 / math.sqrt(D))


CASES = [(1, 1, 1, (1,)), (2, 2, 70, (1, 70)), (4, 2, 200, (7, 8, 9, 200)), (4, 3, 200, (63, 64, 65, 129)),
         (2, 2, 520, (128, 520))]


@pytest.mark.parametrize("B,H,cap,lengths", CASES)
def test_decode_matches_fp32(chunk, B, H, cap, lengths):
    q, kc, vc, want = _case(B, H, cap, lengths)
    assert not q.is_contiguous() or B * H == 1
    got = attention_decode(q, kc, vc, _lengths(lengths))
    assert got.shape == (B, H, 64) and got.dtype == torch.bfloat16
    e = _err(got, want)
    print(f"B,H,cap={B},{H},{cap} lengths={lengths} chunk={chunk}: o {e:.2e}")
    assert torch.isfinite(got).all()
    assert e < 1e-2, e


@pytest.mark.parametrize("fill", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_junk_past_the_length_never_enters(chunk, fill):
    B, H, cap, lengths = 4, 3, 200, (63, 64, 65, 1)
    q, kc, vc, _ = _case(B, H, cap, (63, 64, 65, 129))
    hidden = torch.arange(cap, device=DEV)[None, None, :, None] >= _lengths(lengths)[:, None, None, None]

    def run(value):
        k2 = torch.where(hidden, torch.full_like(kc, value), kc)
        v2 = torch.where(hidden, torch.full_like(vc, value), vc)
        return attention_decode(q, k2, v2, _lengths(lengths))

    got = run(fill)
    assert torch.isfinite(got).all()
    assert torch.equal(got, run(0.0))
    assert torch.equal(got[3], vc[3, :, 0])  # one visible key: exactly its value row


def test_lengths_clamped_on_device(chunk):
    B, H, cap = 2, 2, 70
    q, kc, vc, _ = _case(B, H, cap, (1, 70))
    a = attention_decode(q, kc, vc, _lengths((0, cap + 3)))
    b = attention_decode(q, kc, vc, _lengths((1, cap)))
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert torch.equal(a[0], vc[0, :, 0])


def test_deterministic_and_workspace_fully_written(chunk):
    B, H, cap, lengths = 4, 2, 200, (7, 8, 9, 200)
    q, kc, vc, _ = _case(B, H, cap, lengths)
    nat = _ext.native()
    kl = _lengths(lengths)
    a = attention_decode(q, kc, vc, kl)
    assert torch.equal(a, attention_decode(q, kc, vc, kl))
    ws = torch.full((nat.attn_decode_workspace(B, H, cap),), float("nan"), device=DEV)
    o = nat.attn_decode(q, H, kc, vc, kl, 0, SCALE, ws).view(B, H, 64)
    assert torch.isfinite(o).all() and torch.equal(o, a)
    # `add` is applied before the clamp: lengths - 1 with add = 1 is the same call
    assert torch.equal(nat.attn_decode(q, H, kc, vc, kl - 1, 1, SCALE).view(B, H, 64), a)


SENTINEL = -7.25


@pytest.mark.parametrize("T,positions", [(1, (0, 3)), (5, (0, 3)), (5, (-2, 6)), (5, (9, 0))])
def test_append_native(monkeypatch, T, positions):
    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    monkeypatch.setattr(A, "_append_ref", boom)
    B, H, cap, D = 2, 2, 9, 64
    g = torch.Generator(device=DEV).manual_seed(T)
    qkv = torch.randn(B, T, 3 * H * D, device=DEV, generator=g).to(torch.bfloat16)
    kc = torch.full((B, H, cap, D), SENTINEL, device=DEV, dtype=torch.bfloat16)
    vc = torch.full_like(kc, SENTINEL)
    kv_cache_append(kc, vc, qkv, H, _lengths(positions))
    src = qkv.view(B, T, 3, H, D)
    for cache, i in ((kc, 1), (vc, 2)):
        want = torch.full_like(cache, SENTINEL)
        for b in range(B):
            for t in range(T):
                if 0 <= positions[b] + t < cap:
                    want[b, :, positions[b] + t] = src[b, t, i]
        assert torch.equal(cache, want)


def test_decode_agrees_with_causal_kernel(chunk):
    """Prefill rows [0, 65) with one append, decode rows 65 .. 129 one at a time: every decoded row is
    the causal attention's row, and the cache ends up holding exactly k and v."""
    B, H, N = 2, 2, 130
    g = torch.Generator(device=DEV).manual_seed(130)
    qkv = torch.randn(B, N, 3 * H * 64, device=DEV, generator=g).mul(1.5).to(torch.bfloat16)
    q, k, v = (qkv.view(B, N, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    want = attention_ref(q.float(), k.float(), v.float(), SCALE, causal=True)  # [B, H, N, 64]
    kc = torch.empty(B, H, N, 64, device=DEV, dtype=torch.bfloat16)
    vc = torch.empty_like(kc)
    pos = torch.zeros(B, dtype=torch.int32, device=DEV)
    kv_cache_append(kc, vc, qkv[:, :65], H, pos)
    pos.fill_(65)
    rows = []
    for i in range(65, N):
        rows.append(attention_decode_packed(qkv[:, i:i + 1], H, kc, vc, pos))
        pos.add_(1)
    got = torch.cat(rows, dim=1).view(B, N - 65, H, 64).transpose(1, 2)  # [B, H, 65, 64]
    errs = (torch.linalg.vector_norm(got.float() - want[:, :, 65:], dim=(0, 1, 3))
            / torch.linalg.vector_norm(want[:, :, 65:], dim=(0, 1, 3)))
    print(f"decode vs causal rows 65..129: worst row {errs.max().item():.2e}")
    assert torch.isfinite(got).all() and errs.max().item() < 1e-2
    assert torch.equal(kc, k) and torch.equal(vc, v)


def test_dispatch(monkeypatch):
    nat = _ext.native()
    B, H, cap, lengths = 2, 2, 70, (1, 70)
    # fp32 on CUDA and head dim 32 take the PyTorch path
    for D, dtype, bar in ((64, torch.float32, 1e-5), (32, torch.bfloat16, 1e-2)):
        q, kc, vc, want = _case(B, H, cap, lengths, D, dtype)
        assert _err(attention_decode(q, kc, vc, _lengths(lengths)), want) < bar

    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    monkeypatch.setattr(A, "_decode_ref", boom)
    monkeypatch.setattr(A, "_append_ref", boom)
    q, kc, vc, want = _case(B, H, cap, lengths)
    assert _err(attention_decode(q, kc, vc, _lengths(lengths)), want) < 1e-2
    packed = torch.randn(B, 1, 3 * H * 64, device=DEV).to(torch.bfloat16)
    attention_decode_packed(packed, H, kc.clone(), vc.clone(), _lengths((3, 69)))
    for bad in (torch.ones(B, dtype=torch.int64, device=DEV), torch.ones(B + 1, dtype=torch.int32, device=DEV),
                torch.ones(B, 1, dtype=torch.int32, device=DEV)):
        with pytest.raises(RuntimeError):
            attention_decode(q, kc, vc, bad)
        with pytest.raises(RuntimeError):
            nat.attn_decode(q, H, kc, vc, bad, 0, SCALE)
        with pytest.raises(RuntimeError):
            nat.attn_kv_append(packed, H, kc.clone(), vc.clone(), bad)
    with pytest.raises(RuntimeError):
        nat.attn_decode_set_chunk(12)
    with pytest.raises(RuntimeError):
        attention_decode(q.clone().requires_grad_(), kc, vc, _lengths(lengths))
    # existing calls are what they were
    g = torch.Generator(device=DEV).manual_seed(5)
    q4, k4, v4 = (torch.randn(2, 2, 197, 64, device=DEV, generator=g).to(torch.bfloat16) for _ in range(3))
    with torch.no_grad():
        assert torch.equal(attention(q4, k4, v4, causal=True),
                           _AttnFn.apply(q4, k4, v4, SCALE, True, None).permute(0, 2, 1, 3))


def test_graph_replay_follows_positions():
    """The positions are read on the device: a captured decode step replays with their current values."""
    B, H, cap = 2, 2, 200
    _, kc0, vc0, _ = _case(4, 2, 200, (7, 8, 9, 200))
    kc0, vc0 = kc0[:B], vc0[:B]
    packed = torch.randn(B, 1, 3 * H * 64, device=DEV).to(torch.bfloat16)
    pos = _lengths((150, 20))
    kc, vc = kc0.clone(), vc0.clone()
    attention_decode_packed(packed, H, kc0.clone(), vc0.clone(), pos)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = attention_decode_packed(packed, H, kc, vc, pos)
    graph.replay()
    first = out.clone()
    pos.copy_(_lengths((7, 199)))
    graph.replay()
    torch.cuda.synchronize()
    ke, ve = kc0.clone(), vc0.clone()
    assert torch.equal(first, attention_decode_packed(packed, H, ke, ve, _lengths((150, 20))))
    assert torch.equal(out, attention_decode_packed(packed, H, ke, ve, _lengths((7, 199))))
    assert not torch.equal(out, first)
    assert torch.equal(kc, ke) and torch.equal(vc, ve)


def test_gpt_tiny_incremental_vs_reference(monkeypatch):
    """Teacher-forced: prefill 33 tokens, feed tokens 33 .. 68 through decode_step.  Against the same
    weights on the stock fp32 path (full forward), the relative L2 error of the incremental native
    logits is at most 1.5x that of the full-forward native logits at the same positions (the factor of
    test_gpt_tiny_native_vs_reference).  Positions at or past the second sequence's length (41) are
    pad positions, whose logits the model does not define: excluded on both sides."""
    import copy

    from torchbooster_amd.models import gpt_tiny

    torch.manual_seed(0)
    B, N, j = 2, 70, 33
    base = gpt_tiny().cuda()
    tokens = torch.randint(0, 256, (B, N), device=DEV)
    lens = (70, 41)
    lengths = _lengths(lens)
    mnat = copy.deepcopy(base).to(torch.bfloat16)
    with torch.no_grad():
        full = mnat(tokens, lengths)[:, j:N - 1].float()
        with monkeypatch.context() as mp:  # the stock run: every op on its PyTorch path
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            ref = copy.deepcopy(base)(tokens, lengths)[:, j:N - 1].float()
    logits, cache = mnat.prefill(tokens[:, :j], lengths.clamp(max=j))
    assert cache.positions.tolist() == [j, j]
    steps = [mnat.decode_step(tokens[:, t], cache) for t in range(j, N - 1)]
    inc = torch.stack(steps, dim=1).float()
    assert cache.positions.tolist() == [N - 1, N - 1]
    keep = torch.arange(j, N - 1, device=DEV)[None, :] < lengths[:, None]
    e_inc, e_full = _err(inc[keep], ref[keep]), _err(full[keep], ref[keep])
    print(f"gpt_tiny teacher-forced logits vs fp32: incremental {e_inc:.5f} full forward {e_full:.5f} "
          f"({e_inc / e_full:.2f}x)")
    assert torch.isfinite(inc).all()
    assert e_inc <= 1.5 * e_full, (e_inc, e_full)


def test_generate_graph_equals_eager():
    from torchbooster_amd.models import gpt_tiny

    torch.manual_seed(0)
    model = gpt_tiny().cuda().to(torch.bfloat16)
    tokens = torch.randint(0, 256, (2, 9), device=DEV)
    plain, plain_len = model.generate(tokens, 24)
    assert plain_len.tolist() == [24, 24]
    eos = int(plain[0, 5])
    for kw in ({}, {"eos": eos}):
        a, a_len = model.generate(tokens, 24, graph=False, **kw)
        b, b_len = model.generate(tokens, 24, graph=True, **kw)
        assert torch.equal(a, b) and torch.equal(a_len, b_len)
        assert a.shape == (2, 24) and int(a.min()) >= 0 and int(a.max()) < 256
        for r in range(2):
            hits = (plain[r] == eos).nonzero() if kw else []
            n = int(hits[0]) + 1 if len(hits) else 24
            assert int(a_len[r]) == n
            assert torch.equal(a[r, :n], plain[r, :n]) and (a[r, n:] == eos).all()
