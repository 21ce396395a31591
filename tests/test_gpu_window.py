"""Sliding-window attention on the native kernels: the windowed instantiation of the three 128-row
training kernels (csrc/attention.hip), the decode kernels (csrc/attention_decode.hip) and the extend
kernel (csrc/attention_extend.hip), each against fp32 math on the bf16 inputs, plus probes that see one
key too many or too few (Frobenius bars cannot, at large windows).

Bars: those of tests/test_gpu_attention_mask.py for training (relative Frobenius error < 1e-2 on o,
< 2e-2 on each gradient), of tests/test_gpu_decode.py / tests/test_gpu_extend.py for the cache paths
(< 1e-2, for extend per row too), of tests/test_gpu_llama_block.py for the model.
"""
import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.models import gpt_tiny  # noqa: E402
from torchbooster_amd.models.gpt import KVCache  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops import attention as A  # noqa: E402
from torchbooster_amd.ops.attention import (attention, attention_decode, attention_decode_packed,  # noqa: E402
                                            attention_extend, attention_extend_packed, attention_packed,
                                            attention_ref)

DEV = "cuda"
BF = torch.bfloat16
SCALE = 1.0 / math.sqrt(64)
ONE_SPLIT = 1 << 20


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------- training kernels
@functools.lru_cache(maxsize=None)
def _inputs(B, H, N):
    g = torch.Generator(device=DEV).manual_seed(1000 * N + 10 * B + H)
    return tuple(torch.randn(B, H, N, 64, device=DEV, generator=g).mul(s).to(BF) for s in (1.5, 1.5, 1.5, 1.0))


@functools.lru_cache(maxsize=None)
def _case(B, H, N, W, lengths):
    """Inputs, output gradient and the fp32 reference (o, dq, dk, dv): computed once, never modified."""
    q, k, v, do = _inputs(B, H, N)
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    o = attention_ref(qr, kr, vr, SCALE, causal=True, key_lengths=_i32(lengths), window=W)
    o.backward(do.float())
    return q, k, v, do, (o.detach(), qr.grad, kr.grad, vr.grad)


def _check(B, H, N, W, lengths):
    q, k, v, do, (o_ref, dq_ref, dk_ref, dv_ref) = _case(B, H, N, W, lengths)
    q, k, v = (t.clone().requires_grad_() for t in (q, k, v))
    o = attention(q, k, v, causal=True, key_lengths=_i32(lengths), window=W)
    assert o.shape == (B, H, N, 64)
    o.backward(do)
    errs = [_err(o, o_ref), _err(q.grad, dq_ref), _err(k.grad, dk_ref), _err(v.grad, dv_ref)]
    if N == 1 or W == 1:
        # One visible key per row (key i for query i): p = 1 and dP = delta, so dq = scale (dP - delta) k
        # and dk = scale (dP - delta) q are EXACTLY zero in the reference.  As in
        # tests/test_gpu_attention_mask.py the error is taken against the two terms that cancel.
        assert lengths is None
        dp = (do.float() * v.detach().float()).sum(-1, keepdim=True).abs() * SCALE
        assert dq_ref.norm() == 0 and dk_ref.norm() == 0
        errs[1] = (q.grad.float().norm() / (dp * k.detach().float()).norm()).item()
        errs[2] = (k.grad.float().norm() / (dp * q.detach().float()).norm()).item()
        assert torch.equal(o, v)  # a row that sees only itself
    print(f"B,H,N={B},{H},{N} W={W} lengths={lengths}: o {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} "
          f"dv {errs[3]:.2e}")
    assert all(torch.isfinite(t).all() for t in (o, q.grad, k.grad, v.grad))
    assert errs[0] < 1e-2, errs
    assert max(errs[1:]) < 2e-2, errs
    if lengths is not None:  # keys at or past the length: exact zeros
        for b, n in enumerate(lengths):
            assert torch.count_nonzero(k.grad[b, :, n:]) == 0 and torch.count_nonzero(v.grad[b, :, n:]) == 0


GRID = [(N, W) for N in (1, 17, 64, 65, 129, 197, 256, 257, 300, 520) for W in (1, 2, 63, 64, 65, 128, 129)
        if W < N]


@pytest.mark.parametrize("N,W", GRID + [(1, 1)])
def test_window_fwd_bwd(N, W):
    _check(2, 2, N, W, None)


@pytest.mark.parametrize("W", [2, 64, 65])
@pytest.mark.parametrize("N", [197, 300])
def test_window_and_key_lengths_fwd_bwd(N, W):
    _check(4, 2, N, W, (1, 64, 65, N))


@pytest.mark.parametrize("hkv", [4, 2])
def test_packed_window(hkv):
    torch.manual_seed(3)
    B, N, H, W = 2, 197, 4, 64
    kl = _i32((65, 197))
    wq = (H + 2 * hkv) * 64
    qkv = torch.randn(B, N, wq, device=DEV).to(BF).requires_grad_()
    o = attention_packed(qkv, H, causal=True, key_lengths=kl, window=W, **({} if hkv == H else {"kv_heads": hkv}))
    g = torch.randn_like(o)
    o.backward(g)
    ref_in = qkv.detach().float().requires_grad_()
    q = ref_in[..., :H * 64].view(B, N, H, 64).transpose(1, 2)
    k, v = (ref_in[..., s * 64:(s + hkv) * 64].view(B, N, hkv, 64).transpose(1, 2).repeat_interleave(H // hkv, 1)
            for s in (H, H + hkv))
    orf = attention_ref(q, k, v, SCALE, causal=True, key_lengths=kl, window=W).transpose(1, 2).reshape(B, N, H * 64)
    orf.backward(g.float())
    assert torch.isfinite(o).all() and torch.isfinite(qkv.grad).all()
    assert _err(o, orf) < 1e-2
    for lo, hi in ((0, H), (H, H + hkv), (H + hkv, H + 2 * hkv)):  # dq, dk, dv inside the packed gradient
        assert _err(qkv.grad[..., lo * 64:hi * 64], ref_in.grad[..., lo * 64:hi * 64]) < 2e-2, (lo, hi)
    assert torch.count_nonzero(qkv.grad[0, 65:, H * 64:]) == 0


def test_window_at_least_N_is_no_window():
    q, k, v, do = _inputs(2, 2, 300)
    kl = _i32((300, 65))
    with torch.no_grad():
        for W in (300, 303):
            assert torch.equal(attention(q, k, v, causal=True, window=W), attention(q, k, v, causal=True))
            assert torch.equal(attention(q, k, v, causal=True, key_lengths=kl, window=W),
                               attention(q, k, v, causal=True, key_lengths=kl))
        assert not torch.equal(attention(q, k, v, causal=True, window=299), attention(q, k, v, causal=True))
        # the whole-head setting does not reach a windowed call
        nat = _ext.native()
        q2, k2, v2, _ = _inputs(2, 2, 197)
        a = attention(q2, k2, v2, causal=True, window=64)
        old = nat.attn_set_head_mask(0)
        try:
            assert torch.equal(attention(q2, k2, v2, causal=True, window=64), a)
        finally:
            nat.attn_set_head_mask(old)


PROBE_N = 300


def _probe_rows(W):
    return sorted({W - 1, W, 63, 64, 127, 128, PROBE_N - 1})


@pytest.mark.parametrize("W", [64, 65])
def test_exact_visibility_forward(W):
    """Other finite values in every k / v row outside row i's window leave o[:, :, i] bit-identical; another
    first key of the window changes it."""
    N = PROBE_N
    q, k, v, _ = _inputs(2, 2, N)
    g = torch.Generator(device=DEV).manual_seed(W)
    junk_k, junk_v = (torch.randn(2, 2, N, 64, device=DEV, generator=g).mul(3).to(BF) for _ in range(2))
    rows = torch.arange(N, device=DEV)[None, None, :, None]
    with torch.no_grad():
        base = attention(q, k, v, causal=True, window=W)
        for i in _probe_rows(W):
            lo = max(0, i + 1 - W)
            outside = (rows < lo) | (rows > i)
            got = attention(q, torch.where(outside, junk_k, k), torch.where(outside, junk_v, v), causal=True, window=W)
            assert torch.equal(got[:, :, i], base[:, :, i]), (W, i)
            first = rows == lo
            got = attention(q, torch.where(first, junk_k, k), torch.where(first, junk_v, v), causal=True, window=W)
            assert not torch.equal(got[:, :, i], base[:, :, i]), (W, i)


@pytest.mark.parametrize("W", [64, 65])
def test_exact_visibility_backward(W):
    """Other dO rows outside [j, j + W) leave dk[:, :, j] and dv[:, :, j] bit-identical; another dO row
    j + W - 1 (the last query that sees key j) changes them."""
    N = PROBE_N
    nat = _ext.native()
    q, k, v, do = _inputs(2, 2, N)
    other = torch.randn(2, 2, N, 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(W)).to(BF)
    rows = torch.arange(N, device=DEV)[None, None, :, None]
    o, lse = nat.attn_forward(q, k, v, SCALE, True, None, W)
    ov = o.permute(0, 2, 1, 3)

    def grads(d):
        dq, dk, dv = (torch.full_like(q, float("nan")) for _ in range(3))
        nat.attn_backward(q, k, v, ov, d, lse, SCALE, dq, dk, dv, True, None, W)
        assert not any(torch.isnan(t).any() for t in (dq, dk, dv))
        return dk, dv

    dk0, dv0 = grads(do)
    for j in _probe_rows(W):
        outside = (rows < j) | (rows >= j + W)
        dk1, dv1 = grads(torch.where(outside, other, do))
        assert torch.equal(dk1[:, :, j], dk0[:, :, j]) and torch.equal(dv1[:, :, j], dv0[:, :, j]), (W, j)
        last = min(j + W, N) - 1
        dk2, dv2 = grads(torch.where(rows == last, other, do))
        assert not torch.equal(dv2[:, :, j], dv0[:, :, j]), (W, j)


@pytest.mark.parametrize("N,lengths", [(300, (1, 65, 300)), (197, (1, 65, 197))])
@pytest.mark.parametrize("W", [2, 64, 129])
def test_every_gradient_element_written(N, lengths, W):
    nat = _ext.native()
    B, H = len(lengths), 2
    q, k, v, do = _inputs(B, H, N)
    kl = _i32(lengths)
    o, lse = nat.attn_forward(q, k, v, SCALE, True, kl, W)
    assert torch.isfinite(lse).all() and torch.isfinite(o).all()
    dq, dk, dv = (torch.full_like(q, float("nan")) for _ in range(3))
    nat.attn_backward(q, k, v, o.permute(0, 2, 1, 3), do, lse, SCALE, dq, dk, dv, True, kl, W)
    for t in (dq, dk, dv):
        assert not torch.isnan(t).any()
    for b, n in enumerate(lengths):
        assert torch.count_nonzero(dk[b, :, n:]) == 0 and torch.count_nonzero(dv[b, :, n:]) == 0
        assert torch.count_nonzero(dv[b, :, :n]) > 0


# ---------------------------------------------------------------- decode
def _cache_oracle(q, kc, vc, lim, W):
    """fp32 softmax of q [B, T, H, D] over rows max(0, lim[b, t] - W) <= j < lim[b, t] (lim: a host list)."""
    q, kc, vc = q.float(), kc.float(), vc.float()
    G = q.shape[2] // kc.shape[1]
    kc, vc = kc.repeat_interleave(G, 1), vc.repeat_interleave(G, 1)
    lim = torch.tensor(lim, device=DEV)
    j = torch.arange(kc.shape[2], device=DEV)
    vis = (j < lim[..., None]) & (True if W is None else j >= lim[..., None] - W)  # [B, T, cap]
    s = torch.einsum("bthd,bhjd->bhtj", q, kc) * SCALE
    p = torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1)
    return torch.einsum("bhtj,bhjd->bthd", p, vc)


DECODE_H = 12
DECODE_LENS = {128: (1, 100, 128), 129: (128, 129, 64), 512: (127, 129, 512)}


@functools.lru_cache(maxsize=None)
def _decode_case(cap, hkv):
    g = torch.Generator(device=DEV).manual_seed(cap + hkv)
    B, H = 3, DECODE_H
    qkv = torch.randn(B, 1, (H + 2 * hkv) * 64, device=DEV, generator=g).mul(1.5).to(BF)
    kc, vc = (torch.randn(B, hkv, cap, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    lens = DECODE_LENS[cap]
    # the caches as they are after the step's append at row len - 1
    ka, va = kc.clone(), vc.clone()
    for b, n in enumerate(lens):
        ka[b, :, n - 1] = qkv[b, 0, H * 64:(H + hkv) * 64].view(hkv, 64)
        va[b, :, n - 1] = qkv[b, 0, (H + hkv) * 64:].view(hkv, 64)
    return qkv, kc, vc, ka, va, lens


@pytest.mark.parametrize("fused", [False, True], ids=["default", "fused"])
@pytest.mark.parametrize("hkv", [DECODE_H, 2, 1])
@pytest.mark.parametrize("cap", [128, 129, 512])
def test_decode_matches_fp32(cap, hkv, fused):
    nat = _ext.native()
    H = DECODE_H
    qkv, kc, vc, ka, va, lens = _decode_case(cap, hkv)
    q = qkv[:, :, :H * 64].view(3, 1, H, 64)
    pos = _i32([n - 1 for n in lens])
    kw = {} if hkv == H else {"kv_heads": hkv}
    old = nat.attn_decode_set_head_block(-1)
    try:
        for W in (1, 7, 8, 9, 128, 129, 200):
            want = _cache_oracle(q, ka, va, [[n] for n in lens], W).view(3, 1, H * 64)
            for gb in (0, 1, 2, 3, 4):
                if gb and (H // hkv) % gb:
                    continue
                nat.attn_decode_set_head_block(gb)
                k1, v1 = kc.clone(), vc.clone()
                got = attention_decode_packed(qkv, H, k1, v1, pos, fused=fused, window=W, **kw)
                e = _err(got, want)
                assert torch.isfinite(got).all() and e < 1e-2, (cap, hkv, fused, W, gb, e)
                assert torch.equal(k1, ka) and torch.equal(v1, va)
                if W >= cap:
                    k2, v2 = kc.clone(), vc.clone()
                    assert torch.equal(got, attention_decode_packed(qkv, H, k2, v2, pos, fused=fused, **kw))
                if W == 1:
                    own = va[torch.arange(3), :, pos.long()]  # [B, Hkv, 64]: the step's own value rows
                    assert torch.equal(got.view(3, H, 64), own.repeat_interleave(H // hkv, 1))
    finally:
        nat.attn_decode_set_head_block(old)


@pytest.mark.parametrize("fill", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("hkv", [DECODE_H, 1])
def test_decode_junk_outside_the_window_never_enters(hkv, fill):
    H, cap = DECODE_H, 512
    qkv, _, _, ka, va, lens = _decode_case(cap, hkv)
    q = qkv[:, 0, :H * 64].view(3, H, 64)
    lengths = _i32(lens)
    rows = torch.arange(cap, device=DEV)[None, None, :, None]
    n = lengths.long()[:, None, None, None]
    kw = {} if hkv == H else {"kv_heads": hkv}
    for W in (1, 7, 8, 9, 128, 129, 200):
        hidden = (rows >= n) | (rows < n - W)
        k2 = torch.where(hidden, torch.full_like(ka, fill), ka)
        v2 = torch.where(hidden, torch.full_like(va, fill), va)
        clean = attention_decode(q, ka, va, lengths, window=W, **kw)
        got = attention_decode(q, k2, v2, lengths, window=W, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, clean), W
        assert torch.equal(clean, attention_decode(q, ka, va, lengths, window=W, **kw))  # two runs
        assert _err(clean.view(3, 1, H, 64), _cache_oracle(q[:, None], ka, va, [[x] for x in lens], W)) < 1e-2
    assert torch.equal(attention_decode(q, ka, va, lengths, window=cap, **kw),
                       attention_decode(q, ka, va, lengths, **kw))
    assert not torch.equal(attention_decode(q, ka, va, lengths, window=cap - 1, **kw),
                           attention_decode(q, ka, va, lengths, **kw))


def test_decode_head_block_policy_counts_live_chunks():
    nat = _ext.native()
    # 64 * 12 * 32 chunks = 24576 one-head waves share loads (G = 12); a window of 512 leaves 5 live chunks
    assert nat.attn_decode_head_block(64, 12, 1, 4096) == 4
    assert nat.attn_decode_head_block(64, 12, 1, 4096, 512) == 1
    assert nat.attn_decode_head_block(64, 12, 1, 4096, 4096) == 4  # hides nothing: no window


def test_decode_graph_replay_follows_lengths_across_a_window_edge():
    H, cap, W = DECODE_H, 512, 64
    qkv, _, _, ka, va, _ = _decode_case(cap, 2)
    q = qkv[:, 0, :H * 64].view(3, H, 64)
    lengths = _i32((130, 60, 512))
    attention_decode(q, ka, va, lengths, kv_heads=2, window=W)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = attention_decode(q, ka, va, lengths, kv_heads=2, window=W)
    graph.replay()
    first = out.clone()
    lengths.copy_(_i32((300, 200, 65)))  # the window moves into other chunks
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, attention_decode(q, ka, va, _i32((130, 60, 512)), kv_heads=2, window=W))
    assert torch.equal(out, attention_decode(q, ka, va, _i32((300, 200, 65)), kv_heads=2, window=W))
    assert not torch.equal(out, first)


# ---------------------------------------------------------------- extend
@pytest.fixture(params=[64, ONE_SPLIT, 0], ids=["split64", "one_split", "default"])
def split(request):
    nat = _ext.native()
    old = nat.attn_extend_set_split(-1)
    nat.attn_extend_set_split(request.param)
    try:
        yield request.param
    finally:
        nat.attn_extend_set_split(old)


def _row_err(got, want):
    """worst per-(batch, query) relative error of [B, T, H, D] tensors"""
    d = torch.linalg.vector_norm(got.float() - want.float(), dim=(2, 3))
    return (d / torch.linalg.vector_norm(want.float(), dim=(2, 3)).clamp_min(1e-12)).max().item()


@functools.lru_cache(maxsize=None)
def _extend_case(T, hkv=2):
    """cap 300; positions (100, 3, 230): with W = 15 .. 65 the windows start inside a 64-row tile and inside
    a 64-row split, at row 0, and several splits past the first."""
    B, H, cap = 3, 2, 300
    g = torch.Generator(device=DEV).manual_seed(T + hkv)
    packed = torch.randn(B, T, 3 * H * 64, device=DEV, generator=g).mul(1.5).to(BF)
    kc, vc = (torch.randn(B, hkv, cap, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    pos = (100, 3, 230)
    lim = [[min(max(p + t + 1, 1), cap) for t in range(T)] for p in pos]
    return packed.view(B, T, 3, H, 64)[:, :, 0], kc, vc, pos, lim


@pytest.mark.parametrize("hkv", [2, 1])
@pytest.mark.parametrize("T", [1, 5, 16, 17, 40])
def test_extend_matches_fp32(split, T, hkv):
    q, kc, vc, pos, lim = _extend_case(T, hkv)
    kw = {} if hkv == 2 else {"kv_heads": hkv}
    rows = torch.arange(kc.shape[2], device=DEV)[None, None, :, None]
    first = torch.tensor([l[0] for l in lim], device=DEV)[:, None, None, None]
    for W in (1, 15, 16, 17, 64, 65):
        want = _cache_oracle(q, kc, vc, lim, W)
        got = attention_extend(q, kc, vc, _i32(pos), window=W, **kw)
        e, worst = _err(got, want), _row_err(got, want)
        assert got.shape == want.shape and torch.isfinite(got).all(), (T, W)
        assert e < 1e-2 and worst < 1e-2, (T, W, split, e, worst)
        # NaN below the call's smallest lower limit changes nothing; neither does a second run
        below = rows < first - W
        k2 = torch.where(below, torch.full_like(kc, float("nan")), kc)
        v2 = torch.where(below, torch.full_like(vc, float("nan")), vc)
        assert torch.equal(attention_extend(q, k2, v2, _i32(pos), window=W, **kw), got), (T, W)
        if W == 1:
            own = torch.stack([vc[b, :, [x - 1 for x in lim[b]]] for b in range(3)]).transpose(1, 2)
            assert torch.equal(got, own.repeat_interleave(2 // hkv, 2))
    assert torch.equal(attention_extend(q, kc, vc, _i32(pos), window=300, **kw),
                       attention_extend(q, kc, vc, _i32(pos), **kw))


def test_extend_T1_is_decode_packed(split):
    B, H, W = 3, 2, 17
    _, kc, vc, pos, _ = _extend_case(5)
    packed = torch.randn(B, 1, 3 * H * 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(BF)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    a = attention_extend_packed(packed, H, k1, v1, _i32(pos), window=W)
    b = attention_decode_packed(packed, H, k2, v2, _i32(pos), window=W)
    assert torch.equal(a, b) and torch.equal(k1, k2) and torch.equal(v1, v2)
    assert not torch.equal(a, attention_decode_packed(packed, H, kc.clone(), vc.clone(), _i32(pos)))
    q = packed.view(B, 1, 3, H, 64)[:, :, 0]
    assert _err(attention_extend(q, k1, v1, _i32(pos), window=W).view(B, 1, H * 64), b) < 1e-2


def test_extend_workspace_fully_written_and_deterministic(split):
    nat = _ext.native()
    B, H, T, cap, W = 3, 2, 40, 300, 65
    q, kc, vc, pos, _ = _extend_case(T)
    p = _i32(pos)
    a = attention_extend(q, kc, vc, p, window=W)
    assert torch.equal(a, attention_extend(q, kc, vc, p, window=W))
    need = nat.attn_extend_workspace(B, H, T, cap)
    ws = torch.full((max(need, 4),), float("nan"), device=DEV)
    o = nat.attn_extend(q, kc, vc, p, SCALE, ws, 0, W).view(B, T, H, 64)
    assert torch.isfinite(o).all() and torch.equal(o, a)
    if need:  # every max and sum is written, "empty" leading splits included
        nparts = B * H * ((T + 15) // 16) * nat.attn_extend_splits(B, H, T, cap)
        assert not torch.isnan(ws[nparts * 16 * 64:nparts * 16 * 66]).any()


# ---------------------------------------------------------------- dispatch
def test_dispatch(monkeypatch):
    nat = _ext.native()
    W = 3
    # fp32 on CUDA, head dim 32, CPU tensors and TBAMD_FORCE_REFERENCE=1 take PyTorch -- and the window with them
    for D, dtype, dev, bar in ((64, torch.float32, DEV, 1e-5), (32, BF, DEV, 1e-2), (64, torch.float32, "cpu", 1e-5)):
        g = torch.Generator().manual_seed(D)
        q, k, v = (torch.randn(2, 2, 9, D, generator=g).to(dev, dtype) for _ in range(3))
        want = attention_ref(q.float(), k.float(), v.float(), 1 / math.sqrt(D), causal=True, window=W)
        assert _err(attention(q, k, v, causal=True, window=W), want) < bar
        kc, vc = (torch.randn(2, 2, 12, D, generator=g).to(dev, dtype) for _ in range(2))
        pos = torch.tensor((8, 2), dtype=torch.int32, device=dev)
        lim = [[9], [3]]
        got = attention_decode(q[:, :, 0], kc, vc, pos + 1, window=W)
        ref = torch.stack([torch.einsum("hj,hjd->hd", torch.softmax(
            torch.einsum("hd,hjd->hj", q[b, :, 0].float(), kc[b, :, n[0] - W:n[0]].float()) / math.sqrt(D), -1),
            vc[b, :, n[0] - W:n[0]].float()) for b, n in enumerate(lim)])
        assert _err(got, ref) < bar
    q, k, v, _ = _inputs(2, 2, 197)
    qkv, kc, vc, ka, va, lens = _decode_case(512, 2)
    with monkeypatch.context() as mp:
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        with torch.no_grad():
            ref = attention(q, k, v, causal=True, window=64)
            dref = attention_decode(qkv[:, 0, :DECODE_H * 64].view(3, DECODE_H, 64), ka, va, _i32(lens), kv_heads=2,
                                    window=64)

    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    for name in ("_sdpa", "_decode_ref", "_extend_ref", "_append_ref"):
        monkeypatch.setattr(A, name, boom)
    monkeypatch.setattr(A.F, "scaled_dot_product_attention", boom)
    x = q.clone().requires_grad_()
    o = attention(x, k, v, causal=True, window=64)
    o.sum().backward()
    assert _err(o, ref) < 1e-2
    p = torch.randn(2, 10, 3 * 2 * 64, device=DEV, dtype=BF, requires_grad=True)
    attention_packed(p, 2, causal=True, window=4).sum().backward()
    got = attention_decode(qkv[:, 0, :DECODE_H * 64].view(3, DECODE_H, 64), ka, va, _i32(lens), kv_heads=2, window=64)
    assert _err(got, dref) < 1e-2
    qe, ke, ve, pos, _ = _extend_case(5)
    attention_extend(qe, ke, ve, _i32(pos), window=17)
    packed = torch.randn(3, 5, 3 * 2 * 64, device=DEV).to(BF)
    attention_extend_packed(packed, 2, ke.clone(), ve.clone(), _i32(pos), window=17)
    attention_decode_packed(packed[:, :1], 2, ke.clone(), ve.clone(), _i32(pos), window=17, fused=True)
    # the bindings check what the Python layer checks
    with pytest.raises(RuntimeError):
        nat.attn_forward(q, k, v, SCALE, False, None, 4)  # needs causal
    with pytest.raises(RuntimeError):
        nat.attn_forward(q, k, v, SCALE, True, None, -1)
    with pytest.raises(RuntimeError):
        nat.attn_extend(qe, ke, ve, _i32(pos), SCALE, None, 0, -1)


# ---------------------------------------------------------------- the model
W_MODEL = 16


def _tiny(window=W_MODEL, **kw):
    torch.manual_seed(0)
    return gpt_tiny(window=window, **kw).cuda()


def test_gpt_tiny_training_step_vs_reference():
    """One training step at 2 x 70 tokens with window 16 (and a per-layer (16, None)): every gradient finite,
    the loss within the bf16 bar (1e-2 relative) of the fp32 PyTorch path, block 0's qkv weight gradient
    within 1.5x of the error the model without a window shows (the bars of tests/test_gpu_llama_block.py)."""
    tokens = torch.randint(0, 256, (2, 70), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    lengths = _i32((70, 41))
    errs = {}
    for name, window in (("window", W_MODEL), ("mixed", (W_MODEL, None)), ("default", None)):
        base = _tiny(window)
        mnat = copy.deepcopy(base).to(BF)
        loss = mnat.loss(tokens, lengths)
        loss.backward()
        for pname, p in mnat.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, (name, pname)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            mref = copy.deepcopy(base)
            loss_ref = mref.loss(tokens, lengths)
            loss_ref.backward()
        assert abs(loss.item() - loss_ref.item()) < 1e-2 * abs(loss_ref.item()), (name, loss.item(), loss_ref.item())
        errs[name] = _err(mnat.blocks[0].attn.qkv.weight.grad, mref.blocks[0].attn.qkv.weight.grad)
    print(f"block 0 qkv weight gradient vs fp32: {errs}")
    assert errs["window"] <= 1.5 * errs["default"] and errs["mixed"] <= 1.5 * errs["default"], errs


@pytest.mark.parametrize("window", [W_MODEL, (None, 5)], ids=["w16", "global-w5"])
def test_gpt_tiny_generate(window):
    """Greedy generation past the window: graph replay and the two-turn cache equal the eager run bit for
    bit, the fused path equals itself under a graph, decode_step is extend(one token, last_only), and the
    teacher-forced incremental logits sit within 1.5x of the full forward's error against fp32."""
    base = _tiny(window)
    model = copy.deepcopy(base).to(BF)
    tokens = torch.randint(0, 256, (2, 9), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    n = 30
    a, a_len = model.generate(tokens, n, graph=False)
    b, b_len = model.generate(tokens, n, graph=True)
    assert torch.equal(a, b) and torch.equal(a_len, b_len) and a_len.tolist() == [n, n]
    f, _ = model.generate(tokens, n, fused=True, graph=False)
    g, _ = model.generate(tokens, n, fused=True, graph=True)
    assert torch.equal(f, g) and int(f.min()) >= 0 and int(f.max()) < 256
    # two turns on a caller's cache equal one shot (the second turn's prompt re-enters through extend)
    turn2 = torch.randint(0, 256, (2, 5), device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    turns = []
    for graph in (False, True):
        cache = KVCache(model, 2, capacity=80)
        out1, _ = model.generate(tokens, 12, cache=cache, graph=graph)
        out2, _ = model.generate(torch.cat([out1[:, -1:], turn2], dim=1), 10, cache=cache, graph=graph)
        assert out2.shape == (2, 10) and cache.positions.tolist() == [9 + 11 + 6 + 9] * 2
        turns.append((out1, out2))
    assert all(torch.equal(x, y) for x, y in zip(*turns))
    # a draft with another window: speculative decoding emits the target's greedy tokens wherever its argmax
    # is unambiguous -- the shape and the range are checked, and the first token, which is the prefill's
    draft = copy.deepcopy(_tiny(4)).to(BF)
    s, s_len = model.generate(tokens, 12, draft=draft, draft_tokens=3)
    assert s.shape == (2, 12) and s_len.tolist() == [12, 12] and torch.equal(s[:, 0], a[:, 0])
    # decode_step IS extend(one token, last_only)
    _, c1 = model.prefill(tokens)
    _, c2 = model.prefill(tokens)
    for t in range(20):
        x = model.decode_step(a[:, t], c1)
        y = model.extend(a[:, t:t + 1], c2, last_only=True)
        assert torch.equal(x, y), t
    # teacher-forced logits against the fp32 PyTorch path
    seq = torch.cat([tokens, a], dim=1)
    j, N = 9, seq.shape[1]
    with torch.no_grad():
        full = model(seq)[:, j:].float()
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            ref = copy.deepcopy(base)(seq)[:, j:].float()
    e_full = _err(full, ref)
    for fused in (False, True):
        _, cache = model.prefill(seq[:, :j])
        inc = torch.stack([model.decode_step(seq[:, t], cache, fused=fused) for t in range(j, N)], dim=1).float()
        e_inc = _err(inc, ref)
        print(f"gpt_tiny(window={window}) teacher-forced logits vs fp32, fused={fused}: incremental {e_inc:.5f} "
              f"full forward {e_full:.5f}")
        assert torch.isfinite(inc).all() and e_inc <= 1.5 * e_full, (fused, e_inc, e_full)
    _, cache = model.prefill(seq[:, :j])
    ext = torch.cat([model.extend(seq[:, t:t + 7], cache) for t in range(j, N, 7)], dim=1).float()
    assert _err(ext, ref) <= 1.5 * e_full
