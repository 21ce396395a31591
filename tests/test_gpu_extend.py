"""Multi-token KV-cache extend on the native kernels (csrc/attention_extend.hip): ``attn_extend`` and
its merge, ``attention_extend_packed``, and ``TransformerLM.extend`` / ``generate(cache=)`` /
``generate(draft=)``.

The kernel bar is the forward bar of test_gpu_attention.py / test_gpu_decode.py: relative Frobenius
error < 1e-2 against fp32 math on the bf16 inputs (inputs randn * 1.5).  Every kernel check runs with
64 keys per split, with a single split and with the default policy.
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
from torchbooster_amd.models.gpt import KVCache, TransformerLM  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops import attention as A  # noqa: E402
from torchbooster_amd.ops.attention import (_AttnFn, attention, attention_decode, attention_decode_packed,  # noqa: E402
                                            attention_extend, attention_extend_packed, attention_ref)

DEV = "cuda"
SCALE = 1.0 / math.sqrt(64)
ONE_SPLIT = 1 << 20


@pytest.fixture(params=[64, ONE_SPLIT, 0], ids=["split64", "one_split", "default"])
def split(request):
    nat = _ext.native()
    old = nat.attn_extend_set_split(-1)
    nat.attn_extend_set_split(request.param)
    try:
        yield request.param
    finally:
        nat.attn_extend_set_split(old)


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _row_err(got, want):
    """worst per-(batch, query) relative error of [B, T, H, D] tensors"""
    d = torch.linalg.vector_norm(got.float() - want.float(), dim=(2, 3))
    return (d / torch.linalg.vector_norm(want.float(), dim=(2, 3)).clamp_min(1e-12)).max().item()


def _pos(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _oracle(q, kc, vc, pos, scale):
    """fp32 softmax per query over its visible rows only (pos: host ints)."""
    q, kc, vc = q.float(), kc.float(), vc.float()
    out = torch.zeros_like(q)
    cap = kc.shape[2]
    for b in range(q.shape[0]):
        for t in range(q.shape[1]):
            n = min(max(pos[b] + t + 1, 1), cap)
            s = torch.einsum("hd,hjd->hj", q[b, t], kc[b, :, :n]) * scale
            out[b, t] = torch.einsum("hj,hjd->hd", torch.softmax(s, -1), vc[b, :, :n])
    return out


@functools.lru_cache(maxsize=None)
def _case(B, H, T, cap, pos, D=64, dtype=torch.bfloat16):
    """q (a strided view into a packed [B, T, 3*H*D] projection), fully written caches and the fp32
    reference of one case: computed once, shared by the split settings, never modified."""
    g = torch.Generator(device=DEV).manual_seed(1000 * cap + 10 * T + H)
    packed = torch.randn(B, T, 3 * H * D, device=DEV, generator=g).mul(1.5).to(dtype)
    kc, vc = (torch.randn(B, H, cap, D, device=DEV, generator=g).mul(1.5).to(dtype) for _ in range(2))
    q = packed.view(B, T, 3, H, D)[:, :, 0]
    return q, kc, vc, _oracle(q, kc, vc, pos, 1.0 / math.sqrt(D))


CASES = [
    (1, 1, 1, 1, (0,)),           # minimal shape
    (2, 2, 8, 200, (60, 0)),      # limits 61..68 straddle the 64-key edge
    (2, 2, 15, 200, (3, 100)),    # query-tile edge
    (2, 2, 16, 200, (3, 100)),
    (2, 2, 17, 200, (3, 100)),    # padded second tile
    (2, 3, 33, 200, (0, 167)),    # three tiles, pos + T == cap
    (2, 2, 8, 70, (66, -5)),      # rows dropped, clamp at both ends
    (1, 2, 40, 520, (480,)),      # nine 64-key splits, most empty for the first tile
]


@pytest.mark.parametrize("B,H,T,cap,pos", CASES)
def test_extend_matches_fp32(split, B, H, T, cap, pos):
    q, kc, vc, want = _case(B, H, T, cap, pos)
    assert not q.is_contiguous() or B * T * H == 1
    got = attention_extend(q, kc, vc, _pos(pos))
    assert got.shape == (B, T, H, 64) and got.dtype == torch.bfloat16
    e, worst = _err(got, want), _row_err(got, want)
    print(f"B,H,T,cap={B},{H},{T},{cap} pos={pos} split={split} "
          f"nsplit={_ext.native().attn_extend_splits(B, H, T, cap)}: o {e:.2e} worst row {worst:.2e}")
    assert torch.isfinite(got).all()
    assert e < 1e-2, e
    assert worst < 1e-2, worst


def test_split_policy():
    nat = _ext.native()
    old = nat.attn_extend_set_split(-1)
    try:
        nat.attn_extend_set_split(64)
        assert nat.attn_extend_splits(1, 2, 40, 520) == 9 and nat.attn_extend_workspace(1, 2, 40, 520) == 2 * 3 * 9 * 16 * 66
        nat.attn_extend_set_split(ONE_SPLIT)
        assert nat.attn_extend_splits(1, 2, 40, 520) == 1 and nat.attn_extend_workspace(1, 2, 40, 520) == 0
        nat.attn_extend_set_split(0)
        assert nat.attn_extend_splits(1, 12, 8, 1024) > 1  # 12 tiles cannot occupy the chip
        # 8 * 12 * ceil(512 / 16) tiles can: a long continuation needs no workspace
        assert nat.attn_extend_splits(8, 12, 512, 1024) == 1 and nat.attn_extend_workspace(8, 12, 512, 1024) == 0
        for bad in (12, 4, (1 << 20) + 8):
            with pytest.raises(RuntimeError):
                nat.attn_extend_set_split(bad)
        assert nat.attn_extend_set_split(-1) == 0
    finally:
        nat.attn_extend_set_split(old)


@pytest.mark.parametrize("fill", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_junk_at_or_past_pos_plus_T_never_enters(split, fill):
    B, H, T, cap, pos = 2, 3, 33, 200, (0, 130)
    q, kc, vc, _ = _case(B, H, 33, 200, (0, 167))
    hidden = torch.arange(cap, device=DEV)[None, None, :, None] >= (_pos(pos) + T)[:, None, None, None]

    def run(value):
        k2 = torch.where(hidden, torch.full_like(kc, value), kc)
        v2 = torch.where(hidden, torch.full_like(vc, value), vc)
        return attention_extend(q, k2, v2, _pos(pos))

    got = run(fill)
    assert torch.isfinite(got).all()
    assert torch.equal(got, run(0.0))
    assert torch.equal(got[0, 0], vc[0, :, 0])  # one visible key: exactly its value row


@pytest.mark.parametrize("fill", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_poisoned_new_token_stays_out_of_earlier_query_tiles(split, fill):
    """New token 16's k / v are poison.  Queries 0 .. 15 are the first 16-query tile: its largest limit
    is pos + 16, row pos + 16 is at or past it and is never loaded for them.  (Queries of the SAME tile
    as a poisoned later token multiply its v by an exact-zero probability -- the documented contract --
    so the guarantee is per tile; a finite token gives an exact 0 contribution.)"""
    B, H, T, cap = 2, 2, 20, 200
    g = torch.Generator(device=DEV).manual_seed(16)
    qkv = torch.randn(B, T, 3 * H * 64, device=DEV, generator=g).mul(1.5).to(torch.bfloat16)
    kc0, vc0 = (torch.randn(B, H, cap, 64, device=DEV, generator=g).mul(1.5).to(torch.bfloat16) for _ in range(2))
    pos = _pos((50, 0))
    clean = attention_extend_packed(qkv, H, kc0.clone(), vc0.clone(), pos)
    bad = qkv.clone()
    bad.view(B, T, 3, H, 64)[:, 16, 1:] = fill
    got = attention_extend_packed(bad, H, kc0.clone(), vc0.clone(), pos)
    assert torch.isfinite(got[:, :16]).all()
    assert torch.equal(got[:, :16], clean[:, :16])


def test_positions_clamped_on_device(split):
    B, H, T, cap = 2, 2, 8, 70
    q, kc, vc, _ = _case(B, H, T, cap, (66, -5))
    # every limit clamps: batch 0 to cap (as from cap - 1), batch 1 to 1 (as from -7, the largest
    # position at which all eight do)
    a = attention_extend(q, kc, vc, _pos((cap + 1000, -(2 ** 31))))
    b = attention_extend(q, kc, vc, _pos((cap - 1, -7)))
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert torch.equal(a[1], vc[1, :, 0].expand(T, H, 64))
    c = attention_extend(q, kc, vc, _pos((2 ** 31 - 1, 2 ** 31 - 1)))  # pos + t + 1 needs 64 bits
    assert torch.equal(c[0], a[0]) and torch.isfinite(c).all()


def test_deterministic_and_workspace_fully_written(split):
    B, H, T, cap, pos = 1, 2, 40, 520, (480,)
    q, kc, vc, _ = _case(B, H, T, cap, pos)
    nat = _ext.native()
    p = _pos(pos)
    a = attention_extend(q, kc, vc, p)
    assert torch.equal(a, attention_extend(q, kc, vc, p))
    need = nat.attn_extend_workspace(B, H, T, cap)
    assert (need == 0) == (nat.attn_extend_splits(B, H, T, cap) == 1)
    ws = torch.full((max(need, 4),), float("nan"), device=DEV)
    o = nat.attn_extend(q, kc, vc, p, SCALE, ws).view(B, T, H, 64)
    assert torch.isfinite(o).all() and torch.equal(o, a)
    if need:
        with pytest.raises(RuntimeError):
            nat.attn_extend(q, kc, vc, p, SCALE, ws[:need - 16])


def test_packed_from_empty_cache_agrees_with_causal_kernel(split):
    B, H, N = 2, 2, 130
    g = torch.Generator(device=DEV).manual_seed(130)
    qkv = torch.randn(B, N, 3 * H * 64, device=DEV, generator=g).mul(1.5).to(torch.bfloat16)
    q, k, v = (qkv.view(B, N, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    with torch.no_grad():
        want = attention(q, k, v, causal=True).transpose(1, 2)  # [B, N, H, 64], the native causal kernel
    ref = attention_ref(q.float(), k.float(), v.float(), SCALE, causal=True).transpose(1, 2)
    kc = torch.empty(B, H, N, 64, device=DEV, dtype=torch.bfloat16)
    vc = torch.empty_like(kc)
    got = attention_extend_packed(qkv, H, kc, vc, torch.zeros(B, dtype=torch.int32, device=DEV)).view(B, N, H, 64)
    rows = lambda x, y: (torch.linalg.vector_norm(x.float() - y.float(), dim=(0, 2, 3))  # noqa: E731
                         / torch.linalg.vector_norm(y.float(), dim=(0, 2, 3))).max().item()
    print(f"extend vs causal kernel, worst row {rows(got, want):.2e}; vs fp32 {rows(got, ref):.2e}")
    assert torch.isfinite(got).all() and rows(got, want) < 1e-2 and rows(got, ref) < 1e-2
    assert torch.equal(kc, k) and torch.equal(vc, v)


def test_T1_is_decode_packed(split):
    B, H, cap = 2, 2, 200
    _, kc, vc, _ = _case(2, 2, 8, 200, (60, 0))
    packed = torch.randn(B, 1, 3 * H * 64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(torch.bfloat16)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    a = attention_extend_packed(packed, H, k1, v1, _pos((150, 0)))
    b = attention_decode_packed(packed, H, k2, v2, _pos((150, 0)))
    assert a.shape == (B, 1, H * 64) and torch.equal(a, b)
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    # the extend kernel itself at T = 1 is the decode kernel's result to rounding
    q = packed.view(B, 1, 3, H, 64)[:, :, 0]
    assert _err(attention_extend(q, k1, v1, _pos((150, 0))).view(B, 1, H * 64), b) < 1e-2


def test_dispatch(monkeypatch):
    nat = _ext.native()
    B, H, T, cap, pos = 2, 2, 17, 200, (3, 100)
    # fp32 on CUDA and head dim 32 take the PyTorch path
    for D, dtype, bar in ((64, torch.float32, 1e-5), (32, torch.bfloat16, 1e-2)):
        q, kc, vc, want = _case(B, H, T, cap, pos, D, dtype)
        assert _err(attention_extend(q, kc, vc, _pos(pos)), want) < bar
    q, kc, vc, want = _case(B, H, T, cap, pos)
    decode_before = attention_decode(q[:, 0], kc, vc, _pos((7, 200)))

    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    monkeypatch.setattr(A, "_extend_ref", boom)
    monkeypatch.setattr(A, "_append_ref", boom)
    assert _err(attention_extend(q, kc, vc, _pos(pos)), want) < 1e-2
    packed = torch.randn(B, T, 3 * H * 64, device=DEV).to(torch.bfloat16)
    attention_extend_packed(packed, H, kc.clone(), vc.clone(), _pos(pos))
    for bad in (torch.ones(B, dtype=torch.int64, device=DEV), torch.ones(B + 1, dtype=torch.int32, device=DEV),
                torch.ones(B, 1, dtype=torch.int32, device=DEV)):
        with pytest.raises(RuntimeError):
            attention_extend(q, kc, vc, bad)
        with pytest.raises(RuntimeError):
            attention_extend_packed(packed, H, kc.clone(), vc.clone(), bad)
        with pytest.raises(RuntimeError):
            nat.attn_extend(q, kc, vc, bad, SCALE)
    with pytest.raises(RuntimeError):
        nat.attn_extend(q, kc, vc, _pos(pos).cpu(), SCALE)
    with pytest.raises(RuntimeError):
        nat.attn_extend(q.float(), kc, vc, _pos(pos), SCALE)
    with pytest.raises(RuntimeError):
        nat.attn_extend(q[:, :, :1], kc, vc, _pos(pos), SCALE)  # heads differ
    with pytest.raises(RuntimeError):
        attention_extend(q.clone().requires_grad_(), kc, vc, _pos(pos))
    # existing calls are what they were
    assert torch.equal(attention_decode(q[:, 0], kc, vc, _pos((7, 200))), decode_before)
    g = torch.Generator(device=DEV).manual_seed(5)
    q4, k4, v4 = (torch.randn(2, 2, 197, 64, device=DEV, generator=g).to(torch.bfloat16) for _ in range(3))
    with torch.no_grad():
        assert torch.equal(attention(q4, k4, v4, causal=True),
                           _AttnFn.apply(q4, k4, v4, SCALE, True, None).permute(0, 2, 1, 3))


def test_graph_replay_follows_positions(split):
    """The positions are read on the device: a captured extend replays with their current values."""
    B, H, T, cap = 2, 2, 17, 200
    _, kc0, vc0, _ = _case(B, H, T, cap, (3, 100))
    packed = torch.randn(B, T, 3 * H * 64, device=DEV).to(torch.bfloat16)
    pos = _pos((150, 20))
    kc, vc = kc0.clone(), vc0.clone()
    attention_extend_packed(packed, H, kc0.clone(), vc0.clone(), pos)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = attention_extend_packed(packed, H, kc, vc, pos)
    graph.replay()
    first = out.clone()
    pos.copy_(_pos((7, 183)))
    graph.replay()
    torch.cuda.synchronize()
    ke, ve = kc0.clone(), vc0.clone()
    assert torch.equal(first, attention_extend_packed(packed, H, ke, ve, _pos((150, 20))))
    assert torch.equal(out, attention_extend_packed(packed, H, ke, ve, _pos((7, 183))))
    assert not torch.equal(out, first)
    assert torch.equal(kc, ke) and torch.equal(vc, ve)


# ---------------------------------------------------------------- models/gpt.py, bf16
def test_gpt_tiny_extend_vs_reference(monkeypatch):
    """Teacher-forced: prefill 33 tokens, feed tokens 33 .. 68 through ``extend`` in blocks of 7 (the last
    block holds 1).  Against the same weights on the stock fp32 path (full forward), the relative L2 error
    of the extended native logits is at most 1.5x that of the full-forward native logits at the same
    positions (the factor of test_gpt_tiny_incremental_vs_reference).  Positions at or past the second
    sequence's length (41) are pad positions: excluded on both sides."""
    torch.manual_seed(0)
    B, N, j = 2, 70, 33
    base = gpt_tiny().cuda()
    tokens = torch.randint(0, 256, (B, N), device=DEV)
    lengths = _pos((70, 41))
    mnat = copy.deepcopy(base).to(torch.bfloat16)
    with torch.no_grad():
        full = mnat(tokens, lengths)[:, j:N - 1].float()
        with monkeypatch.context() as mp:  # the stock run: every op on its PyTorch path
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            ref = copy.deepcopy(base)(tokens, lengths)[:, j:N - 1].float()
    monkeypatch.setattr(A, "_extend_ref", lambda *a, **k: pytest.fail("fell back to the PyTorch path"))
    _, cache = mnat.prefill(tokens[:, :j], lengths.clamp(max=j))
    assert cache.positions.tolist() == [j, j]
    blocks = [mnat.extend(tokens[:, t:min(t + 7, N - 1)], cache) for t in range(j, N - 1, 7)]
    inc = torch.cat(blocks, dim=1).float()
    assert inc.shape == full.shape and cache.positions.tolist() == [N - 1, N - 1]
    keep = torch.arange(j, N - 1, device=DEV)[None, :] < lengths[:, None]
    e_inc, e_full = _err(inc[keep], ref[keep]), _err(full[keep], ref[keep])
    print(f"gpt_tiny teacher-forced logits vs fp32: extend {e_inc:.5f} full forward {e_full:.5f} "
          f"({e_inc / e_full:.2f}x)")
    assert torch.isfinite(inc).all()
    assert e_inc <= 1.5 * e_full, (e_inc, e_full)


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    base = gpt_tiny().cuda()
    tokens = torch.randint(0, 256, (2, 9), device=DEV)
    return base, copy.deepcopy(base).to(torch.bfloat16), tokens


def test_generate_with_cache_two_turns_and_graph(tiny):
    _, model, tokens = tiny
    outs = {}
    for graph in (False, True):
        cache = KVCache(model, 2, capacity=80)
        out1, len1 = model.generate(tokens, 12, cache=cache, graph=graph)
        assert out1.shape == (2, 12) and len1.tolist() == [12, 12]
        assert cache.positions.tolist() == [9 + 11] * 2
        turn2 = torch.cat([out1[:, -1:], tokens[:, :4]], dim=1)
        out2, len2 = model.generate(turn2, 10, cache=cache, graph=graph)
        assert out2.shape == (2, 10) and len2.tolist() == [10, 10]
        assert int(out2.min()) >= 0 and int(out2.max()) < 256
        assert cache.positions.tolist() == [9 + 11 + 5 + 9] * 2
        outs[graph] = (out1, out2)
    assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1])
    with pytest.raises(ValueError):
        model.generate(tokens, 12, cache=KVCache(model, 2, capacity=20))


@pytest.mark.parametrize("which", ["self", "one_layer"])
def test_speculative_generate(tiny, monkeypatch, which):
    """Against plain greedy ``generate``: equal up to the first position where they differ, if any.  There,
    with z the stock fp32 logits of the common prefix and d the largest absolute deviation of the native
    full-forward logits from z at that position, the two tokens must satisfy |z[a] - z[b]| <= 3 d: an
    argmax can flip only within twice the deviation, and 1.5 is the project's incremental-over-full
    factor."""
    base, model, tokens = tiny
    if which == "self":
        draft = model
    else:
        torch.manual_seed(1)
        draft = TransformerLM(256, 128, 1, 2, 128).cuda().to(torch.bfloat16)
    n, gamma = 24, 4
    plain, plain_len = model.generate(tokens, n)
    calls = []
    real = TransformerLM.extend

    def counted(self, *a, **k):
        calls.append(a[0].shape[1])
        return real(self, *a, **k)

    monkeypatch.setattr(TransformerLM, "extend", counted)
    out, out_len = model.generate(tokens, n, draft=draft, draft_tokens=gamma)
    rounds = len(calls)
    again, again_len = model.generate(tokens, n, draft=draft, draft_tokens=gamma)
    assert out.shape == (2, n) and out.dtype == torch.int64 and out_len.tolist() == [n, n]
    assert int(out.min()) >= 0 and int(out.max()) < 256
    assert torch.equal(out, again) and torch.equal(out_len, again_len)
    assert all(c == gamma + 1 for c in calls) and -(-(n - 1) // (gamma + 1)) <= rounds <= n - 1
    print(f"draft={which}: {rounds} rounds for {n - 1} tokens, {(n - 1) / rounds:.2f} tokens per round")
    for b in range(2):
        diff = (out[b] != plain[b]).nonzero()
        if not len(diff):
            continue
        i = int(diff[0])
        prefix = torch.cat([tokens[b], plain[b, :i]])[None]
        with torch.no_grad():
            nat_logits = model(prefix)[0, -1].float()
            with monkeypatch.context() as mp:
                mp.setenv("TBAMD_FORCE_REFERENCE", "1")
                z = copy.deepcopy(base)(prefix)[0, -1].float()
        d = (nat_logits - z).abs().max().item()
        gap = abs(z[out[b, i]] - z[plain[b, i]]).item()
        print(f"draft={which} sequence {b}: first difference at {i}, |z[a] - z[b]| = {gap:.3e}, d = {d:.3e}")
        assert gap <= 3 * d, (b, i, gap, d)

    eos = int(plain[0, 5])
    want, want_len = model.generate(tokens, n, eos=eos)
    got, got_len = model.generate(tokens, n, eos=eos, draft=draft, draft_tokens=gamma)
    assert got.shape == (2, n) and int(got_len.min()) >= 1 and int(got_len.max()) <= n
    for b in range(2):
        m = int(got_len[b])
        assert (got[b, m:] == eos).all() and (m == n or int(got[b, m - 1]) == eos)
        assert not (got[b, :m - 1] == eos).any()
    if torch.equal(out, plain):
        assert torch.equal(got, want) and torch.equal(got_len, want_len)
