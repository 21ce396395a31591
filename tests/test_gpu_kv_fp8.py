"""FP8 (e4m3) KV cache on the native kernels: the FP8 instantiations of the append, decode and extend kernels
(csrc/attention_decode.hip, csrc/attention_extend.hip, csrc/attn_fp8.h).

The quantiser is compared byte for byte with ``kv_quantize`` on the CPU over every bf16 pattern.  The attention
kernels are compared with an fp32 oracle on the DEQUANTISED cache -- dequantisation is exact in fp32 up to the one
product with the scale, so quantisation is not part of the comparison and the bar is the ``1e-2`` of
tests/test_gpu_rolling.py (relative Frobenius error, for extend per row too).  A ring is built from a linear
cache of codes slot by slot, as there.
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
from torchbooster_amd.models.gpt import KVCache, kv_scales  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops import attention as A  # noqa: E402
from torchbooster_amd.ops.attention import (attention_decode, attention_decode_packed, attention_extend,  # noqa: E402
                                            attention_extend_packed, kv_cache_append, kv_dequantize, kv_quantize)

DEV = "cuda"
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
U8 = torch.uint8
SCALE = 1.0 / math.sqrt(64)
ONE_SPLIT = 1 << 20
H = 12
SC = (0.5, 3.0)
NAN_CODE = 0x7F
MARK = 0x55  # what a never-written row holds where the cache is compared byte for byte


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _row_err(got, want):
    d = torch.linalg.vector_norm(got.float() - want.float(), dim=(2, 3))
    return (d / torch.linalg.vector_norm(want.float(), dim=(2, 3)).clamp_min(1e-12)).max().item()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _same(a, b):
    return torch.equal(a.view(U8), b.view(U8))


def _codes(shape, scale, g):
    """fp8 codes of N(0, 1.5) values quantised on the CPU with ``scale`` -> on the device"""
    return kv_quantize(torch.randn(shape, generator=g) * 1.5, scale).to(DEV)


def _new_rows(qkv, hkv):
    """the k and v codes of a packed bf16 ``qkv`` [B, T, (H + 2*hkv)*64], quantised on the CPU -> [B, hkv, T, 64]"""
    B, T, _ = qkv.shape
    c = qkv.cpu()
    k = c[..., H * 64:(H + hkv) * 64].reshape(B, T, hkv, 64).transpose(1, 2)
    v = c[..., (H + hkv) * 64:].reshape(B, T, hkv, 64).transpose(1, 2)
    return kv_quantize(k, SC[0]).to(DEV), kv_quantize(v, SC[1]).to(DEV)


def _cache_oracle(q, kc, vc, lim, W):
    """fp32 softmax of q [B, T, H, D] over the LOGICAL rows max(0, lim[b, t] - W) <= j < lim[b, t] of the linear
    fp8 caches, dequantised with SC (lim: a host list; W None: every row below the limit)."""
    q = q.float()
    kc, vc = kv_dequantize(kc, SC[0], torch.float32), kv_dequantize(vc, SC[1], torch.float32)
    G = q.shape[2] // kc.shape[1]
    kc, vc = kc.repeat_interleave(G, 1), vc.repeat_interleave(G, 1)
    lim = torch.tensor(lim, device=DEV)
    j = torch.arange(kc.shape[2], device=DEV)
    vis = j < lim[..., None]
    if W is not None:
        vis = vis & (j >= lim[..., None] - W)
    s = torch.einsum("bthd,bhjd->bhtj", q, kc) * SCALE
    p = torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1)
    return torch.einsum("bhtj,bhjd->bthd", p, vc)


def _rows_of(n, R):
    n = torch.tensor(n, device=DEV)[:, None]
    return n - 1 - torch.remainder(n - 1 - torch.arange(R, device=DEV)[None, :], R)


def _ring(lin, n, R):
    """The ring of the linear code cache ``lin`` [B, Hkv, N, 64] for the limits ``n``: slot p holds logical row
    j(p), or MARK where none was ever written."""
    j = _rows_of(n, R)
    idx = j.clamp_min(0)[:, None, :, None].expand(lin.shape[0], lin.shape[1], R, 64)
    mark = torch.full((), MARK, dtype=U8, device=DEV)
    return torch.where((j >= 0)[:, None, :, None], lin.view(U8).gather(2, idx), mark).view(FP8)


def _poison(cache, hidden):
    """``cache`` with the NaN code in every hidden row (``hidden``: bool [B, rows])"""
    nan = torch.full((), NAN_CODE, dtype=U8, device=DEV)
    return torch.where(hidden[:, None, :, None], nan, cache.view(U8)).view(FP8)


def _hidden(rows, n, lo, ring):
    """bool [B, rows]: the rows (slots of a ring, by their logical row) at or past ``n[b]`` or below ``lo[b]``"""
    j = _rows_of(n, rows) if ring else torch.arange(rows, device=DEV)[None, :].expand(len(n), rows)
    return (j < 0) | (j >= torch.tensor(n, device=DEV)[:, None]) | (j < torch.tensor(lo, device=DEV)[:, None])


@pytest.fixture
def knobs():
    """Restore the decode chunk and head block and the extend split whatever a test sets."""
    nat = _ext.native()
    old = nat.attn_decode_set_chunk(-1), nat.attn_decode_set_head_block(-1), nat.attn_extend_set_split(-1)
    try:
        yield nat
    finally:
        nat.attn_decode_set_chunk(old[0])
        nat.attn_decode_set_head_block(old[1])
        nat.attn_extend_set_split(old[2])


# ---------------------------------------------------------------- the quantiser
def _all_bf16():
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)


@pytest.mark.parametrize("scales", [(1.0, 1.0), (0.37, 8.0), (8.0, 0.37)], ids=["1-1", "0.37-8", "8-0.37"])
def test_append_quantises_every_bf16_pattern_like_the_cpu(scales):
    x = _all_bf16()
    perm = torch.randperm(65536, generator=torch.Generator().manual_seed(1))
    k, v = x.view(1024, 64), x[perm].view(1024, 64)
    qkv = torch.cat([torch.zeros(1024, 64, dtype=BF), k, v], dim=1)[None].to(DEV)  # B = 1, T = 1024, H = Hkv = 1
    kc, vc = (torch.full((1, 1, 1024, 64), MARK, dtype=U8, device=DEV).view(FP8) for _ in range(2))
    kv_cache_append(kc, vc, qkv, 1, _i32([0]), kv_scales=scales)
    for got, src, s in ((kc, k, scales[0]), (vc, v, scales[1])):
        got, want = got.view(U8).cpu().view(1024, 64), kv_quantize(src, s).view(U8)
        nan = torch.isnan(src)
        assert torch.equal(got[~nan], want[~nan])  # every finite and infinite input: the CPU's bytes
        assert bool(((got[nan] & 0x7F) == NAN_CODE).all()) and int(nan.sum()) == 254  # NaN stays a NaN code
        assert not bool(((got[~nan] & 0x7F) == NAN_CODE).any())
    # the fused decode step quantises its row with the same code: one step per pattern row, B = 1024, cap = 1
    step = qkv.view(1024, 1, 192)
    for fused in (False, True):
        k1, v1 = (torch.full((1024, 1, 1, 64), MARK, dtype=U8, device=DEV).view(FP8) for _ in range(2))
        attention_decode_packed(step, 1, k1, v1, _i32([0] * 1024), fused=fused, kv_scales=scales)
        assert _same(k1.view(1, 1, 1024, 64), kc) and _same(v1.view(1, 1, 1024, 64), vc), fused


# ---------------------------------------------------------------- decode
# (rows, window, ring, lengths): linear caches of one and of several chunks, a window, and a ring of 40 rows with
# W = 24 up to a context of 1000
DECODE_CASES = ((40, None, False, (1, 17, 40)), (40, 24, False, (1, 17, 40)),
                (300, None, False, (1, 130, 300)), (300, 24, False, (1, 130, 300)),
                (40, 24, True, (5, 40, 1000)))


@functools.lru_cache(maxsize=None)
def _decode_case(rows, ring, lens, hkv):
    """The packed step; the linear code caches after the step's append at logical row len - 1; the cache under
    test before the step and after it."""
    g = torch.Generator().manual_seed(rows + hkv + len(lens))
    B, N = len(lens), max(lens)
    qkv = (torch.randn(B, 1, (H + 2 * hkv) * 64, generator=g) * 1.5).to(BF).to(DEV)
    ka, va = _codes((B, hkv, N, 64), SC[0], g), _codes((B, hkv, N, 64), SC[1], g)
    nk, nv = _new_rows(qkv, hkv)
    for b, n in enumerate(lens):
        ka.view(U8)[b, :, n - 1] = nk.view(U8)[b, :, 0]
        va.view(U8)[b, :, n - 1] = nv.view(U8)[b, :, 0]
    if ring:
        before = tuple(_ring(c, [n - 1 for n in lens], rows) for c in (ka, va))
        after = tuple(_ring(c, list(lens), rows) for c in (ka, va))
    else:
        after = (ka, va)
        before = tuple(c.clone() for c in after)
        for c in before:
            for b, n in enumerate(lens):
                c.view(U8)[b, :, n - 1] = MARK
    return qkv, ka, va, before, after


@pytest.mark.parametrize("fused", [False, True], ids=["default", "fused"])
@pytest.mark.parametrize("hkv", [12, 4, 1])
def test_decode_matches_the_oracle_on_the_dequantised_cache(knobs, hkv, fused):
    nat = knobs
    kw0 = {} if hkv == H else {"kv_heads": hkv}
    for rows, W, ring, lens in DECODE_CASES:
        qkv, ka, va, before, after = _decode_case(rows, ring, lens, hkv)
        B = len(lens)
        kw = dict(kw0, kv_scales=SC, **({} if W is None else {"window": W}), **({"rolling": True} if ring else {}))
        q = qkv[:, :, :H * 64].view(B, 1, H, 64)
        pos = _i32([n - 1 for n in lens])
        want = _cache_oracle(q, ka, va, [[n] for n in lens], W).view(B, 1, H * 64)
        hid = _hidden(rows, list(lens), [0 if W is None else n - W for n in lens], ring)
        assert bool(hid.any())
        for chunk in (128, 8):
            nat.attn_decode_set_chunk(chunk)
            first = None
            for gb in (1, 2, 4, 0):
                if gb and (H // hkv) % gb:
                    continue
                nat.attn_decode_set_head_block(gb)
                k1, v1 = before[0].clone(), before[1].clone()
                got = attention_decode_packed(qkv, H, k1, v1, pos, fused=fused, **kw)
                e = _err(got, want)
                assert got.dtype == BF and torch.isfinite(got).all() and e < 1e-2, (rows, W, ring, hkv, chunk, gb, e)
                assert _same(k1, after[0]) and _same(v1, after[1]), (rows, W, ring, chunk, gb)
                # the bits of the unfused call, of a second run and of head block 1
                k2, v2 = before[0].clone(), before[1].clone()
                again = attention_decode_packed(qkv, H, k2, v2, pos, **kw)
                assert torch.equal(got, again) and _same(k2, k1) and _same(v2, v1), (rows, W, ring, chunk, gb)
                k3, v3 = before[0].clone(), before[1].clone()
                assert torch.equal(got, attention_decode_packed(qkv, H, k3, v3, pos, fused=fused, **kw))
                first = got if first is None else first
                assert torch.equal(got, first), (rows, W, ring, chunk, gb)
                # the NaN code in every hidden row changes no bit
                dec = attention_decode(q[:, 0], *after, _i32(lens), **kw)
                assert torch.equal(dec.view(B, 1, H * 64), got)
                bad = attention_decode(q[:, 0], _poison(after[0], hid), _poison(after[1], hid), _i32(lens), **kw)
                assert torch.equal(bad, dec), (rows, W, ring, chunk, gb)


def test_scales_enter_as_the_rule_says(knobs):
    """The same codes under other scales: the output is the oracle's for those scales (k_scale moves the softmax,
    v_scale the magnitude), and unit scales are the default."""
    qkv, ka, va, _, after = _decode_case(300, False, (1, 130, 300), 4)
    q = qkv[:, 0, :H * 64].view(3, H, 64)
    lens = _i32((1, 130, 300))
    base = attention_decode(q, *after, lens, kv_heads=4)
    assert torch.equal(base, attention_decode(q, *after, lens, kv_heads=4, kv_scales=(1.0, 1.0)))
    twice = attention_decode(q, *after, lens, kv_heads=4, kv_scales=(1.0, 2.0))
    assert torch.equal(twice.float(), base.float() * 2)  # a power of two commutes with every rounding
    for pair in ((0.25, 1.0), (0.37, 2.9)):
        got = attention_decode(q, *after, lens, kv_heads=4, kv_scales=pair)
        k32 = kv_dequantize(ka, pair[0], torch.float32).repeat_interleave(3, 1)
        v32 = kv_dequantize(va, pair[1], torch.float32).repeat_interleave(3, 1)
        s = torch.einsum("bhd,bhjd->bhj", q.float(), k32) * SCALE
        vis = torch.arange(300, device=DEV)[None, :] < lens[:, None]
        want = torch.einsum("bhj,bhjd->bhd", torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1), v32)
        assert _err(got, want) < 1e-2, pair


# ---------------------------------------------------------------- extend
@pytest.fixture(params=[64, ONE_SPLIT], ids=["split64", "one_split"])
def split(request, knobs):
    knobs.attn_extend_set_split(request.param)
    return request.param


EXTEND_CASES = ((300, None, False), (300, 24, False), (40, 24, True))  # R - W + 1 = 17 = the largest T


def _positions(rows, T, ring):
    return (3 * rows - 3, 0, 1000 - T) if ring else (0, 130, rows - T)


@functools.lru_cache(maxsize=None)
def _extend_case(rows, ring, T, hkv):
    """The packed call, the linear code caches with its rows at pos[b] + t, and the cache under test before it."""
    g = torch.Generator().manual_seed(rows + 10 * T + hkv)
    pos = _positions(rows, T, ring)
    B, N = len(pos), max(pos) + T
    packed = (torch.randn(B, T, (H + 2 * hkv) * 64, generator=g) * 1.5).to(BF).to(DEV)
    kl, vl = _codes((B, hkv, N, 64), SC[0], g), _codes((B, hkv, N, 64), SC[1], g)
    nk, nv = _new_rows(packed, hkv)
    for b, p in enumerate(pos):
        kl.view(U8)[b, :, p:p + T] = nk.view(U8)[b]
        vl.view(U8)[b, :, p:p + T] = nv.view(U8)[b]
    if ring:
        before = tuple(_ring(c, [max(p, 1) for p in pos], rows) for c in (kl, vl))
        for c in before:
            c.view(U8)[pos.index(0)] = MARK  # an empty ring
        after = tuple(_ring(c, [p + T for p in pos], rows) for c in (kl, vl))
    else:
        after = (kl, vl)
        before = tuple(c.clone() for c in after)
        for c in before:
            for b, p in enumerate(pos):
                c.view(U8)[b, :, p:p + T] = MARK
    lim = [[p + t + 1 for t in range(T)] for p in pos]
    return packed, kl, vl, before, after, pos, lim


@pytest.mark.parametrize("hkv", [12, 4])
@pytest.mark.parametrize("T", [1, 5, 16, 17])
def test_extend_matches_the_oracle_on_the_dequantised_cache(split, T, hkv):
    kw0 = {} if hkv == H else {"kv_heads": hkv}
    for rows, W, ring in EXTEND_CASES:
        packed, kl, vl, before, after, pos, lim = _extend_case(rows, ring, T, hkv)
        B = len(pos)
        kw = dict(kw0, kv_scales=SC, **({} if W is None else {"window": W}), **({"rolling": True} if ring else {}))
        q = packed[..., :H * 64].view(B, T, H, 64)
        want = _cache_oracle(q, kl, vl, lim, W)
        k1, v1 = before[0].clone(), before[1].clone()
        got = attention_extend_packed(packed, H, k1, v1, _i32(pos), **kw).view(B, T, H, 64)
        e, worst = _err(got, want), _row_err(got, want)
        assert got.dtype == BF and torch.isfinite(got).all() and e < 1e-2 and worst < 1e-2, (rows, W, ring, T, e, worst)
        assert _same(k1, after[0]) and _same(v1, after[1]), (rows, W, ring, T)
        ext = attention_extend(q, *after, _i32(pos), **kw)
        e, worst = _err(ext, want), _row_err(ext, want)
        assert e < 1e-2 and worst < 1e-2, (rows, W, ring, T, e, worst)
        assert torch.equal(ext, attention_extend(q, *after, _i32(pos), **kw))  # deterministic
        if T == 1:  # the packed call IS the decode step; the extend kernel agrees with it
            assert _err(ext, got) < 1e-2
            k2, v2 = before[0].clone(), before[1].clone()
            assert torch.equal(got.view(B, 1, H * 64), attention_decode_packed(packed, H, k2, v2, _i32(pos), **kw))
        else:
            assert torch.equal(ext, got)
        # the NaN code in every hidden row: at or past pos + T, below the first query's lower limit
        hid = _hidden(rows, [p + T for p in pos], [0 if W is None else p + 1 - W for p in pos], ring)
        assert bool(hid.any())
        bad = attention_extend(q, _poison(after[0], hid), _poison(after[1], hid), _i32(pos), **kw)
        assert torch.equal(bad, ext), (rows, W, ring, T)


def test_extend_workspace_fully_written(split):
    nat = _ext.native()
    for rows, W, ring in EXTEND_CASES:
        T, hkv = 17, 4
        packed, _, _, _, after, pos, _ = _extend_case(rows, ring, T, hkv)
        B = len(pos)
        q = packed[..., :H * 64].view(B, T, H, 64)
        kw = dict(kv_heads=hkv, kv_scales=SC, **({} if W is None else {"window": W}), **({"rolling": True} if ring else {}))
        a = attention_extend(q, *after, _i32(pos), **kw)
        need = nat.attn_extend_workspace(B, H, T, rows)
        ws = torch.full((max(need, 4),), float("nan"), device=DEV)
        o = nat.attn_extend(q, *after, _i32(pos), SCALE, ws, hkv, W or 0, ring, k_scale=SC[0], v_scale=SC[1])
        assert torch.isfinite(o).all() and torch.equal(o.view(B, T, H, 64), a)
        if need:  # every max and sum is written, those of empty splits included
            nparts = B * H * ((T + 15) // 16) * nat.attn_extend_splits(B, H, T, rows)
            assert not torch.isnan(ws[nparts * 16 * 64:nparts * 16 * 66]).any()


# ---------------------------------------------------------------- graph replay
def test_graph_replay_follows_positions():
    """decode: a ring of 136 rows (two chunks), sequences that wrap and one that crosses the chunk edge; extend:
    T = 3 per replay on a ring of 40 rows that wraps, and on a linear cache across a split edge."""
    hkv, B, steps = 2, 3, 8
    g = torch.Generator().manual_seed(3)
    for rows, W, ring, start, T in ((136, 120, True, (133, 267, 125), 1), (40, 24, True, (35, 70, 3), 3),
                                    (300, None, False, (125, 0, 60), 3)):
        wide = (H + 2 * hkv) * 64
        new = (torch.randn(steps + 1, B, T, wide, generator=g) * 1.5).to(BF).to(DEV)
        kc, vc = _codes((B, hkv, rows, 64), SC[0], g), _codes((B, hkv, rows, 64), SC[1], g)
        kw = dict(kv_heads=hkv, kv_scales=SC, **({} if W is None else {"window": W}), **({"rolling": True} if ring else {}))
        call = (lambda x, k, v, p: attention_decode_packed(x, H, k, v, p, fused=True, **kw)) if T == 1 else \
            (lambda x, k, v, p: attention_extend_packed(x, H, k, v, p, **kw))
        qkv, pos = new[0].clone(), _i32(start)
        k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        call(qkv, k1, v1, pos)  # warm-up
        call(qkv, k2, v2, pos)
        pos.add_(T)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call(qkv, k1, v1, pos)
        outs = []
        for s in range(1, steps + 1):
            qkv.copy_(new[s])
            graph.replay()
            want = call(new[s], k2, v2, pos.clone())
            assert torch.equal(out, want), (rows, s)
            assert _same(k1, k2) and _same(v1, v2), (rows, s)
            outs.append(out.clone())
            pos.add_(T)
        torch.cuda.synchronize()
        assert pos.tolist() == [x + T * (steps + 1) for x in start]
        assert not torch.equal(outs[0], outs[-1])


# ---------------------------------------------------------------- dispatch
class _Recorder:
    """Stands in for the native module: records the name and keywords of every function that is called."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def wrapped(*a, **kw):
            self.calls.append((name, dict(kw)))
            return fn(*a, **kw)
        return wrapped


def test_dispatch(monkeypatch):
    rec = _Recorder(_ext.native())
    monkeypatch.setattr(A, "native", lambda: rec)
    qkv, _, _, before, after = _decode_case(40, False, (1, 17, 40), 4)
    packed, _, _, eb, _, epos, _ = _extend_case(300, False, 5, 4)
    pos, B = _i32((0, 16, 39)), 3
    q = qkv[:, 0, :H * 64].view(B, H, 64)
    want_kw = {"k_scale": SC[0], "v_scale": SC[1]}
    # an fp8 pair reaches the native functions, with its scales
    attention_decode(q, *after, pos + 1, kv_heads=4, kv_scales=SC)
    attention_decode_packed(qkv, H, before[0].clone(), before[1].clone(), pos, kv_heads=4, kv_scales=SC)
    attention_decode_packed(qkv, H, before[0].clone(), before[1].clone(), pos, kv_heads=4, kv_scales=SC, fused=True)
    attention_extend_packed(packed, H, eb[0].clone(), eb[1].clone(), _i32(epos), kv_heads=4, kv_scales=SC)
    assert [n for n, _ in rec.calls] == ["attn_decode", "attn_kv_append", "attn_decode", "attn_decode_append",
                                         "attn_kv_append", "attn_extend"]
    assert all(kw == want_kw for _, kw in rec.calls), rec.calls
    del rec.calls[:]
    attention_decode(q, *after, pos + 1, kv_heads=4)  # None is (1.0, 1.0)
    assert rec.calls == [("attn_decode", {"k_scale": 1.0, "v_scale": 1.0})]
    # a bf16 pair makes the call it made
    del rec.calls[:]
    kb = kv_dequantize(after[0], SC[0])
    attention_decode(q, kb, kb, pos + 1, kv_heads=4)
    assert rec.calls == [("attn_decode", {})]
    # mixed dtypes, e5m2, head dim 32 and TBAMD_FORCE_REFERENCE=1 do not
    del rec.calls[:]
    e5 = after[0].view(U8).view(torch.float8_e5m2)
    for k, v in ((after[0], kb), (kb, after[1]), (e5, e5)):
        try:
            attention_decode(q, k, v, pos + 1, kv_heads=4)
        except (RuntimeError, NotImplementedError):  # what stock PyTorch makes of such a pair is not at issue
            pass
    q32 = torch.randn(B, H, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)).to(BF)
    k32 = after[0][..., :32].contiguous()
    small = attention_decode(q32, k32, k32, pos + 1, kv_heads=4, kv_scales=SC)
    assert torch.isfinite(small).all()
    with monkeypatch.context() as mp:
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        k1, v1 = before[0].clone(), before[1].clone()
        ref = attention_decode_packed(qkv, H, k1, v1, pos, kv_heads=4, kv_scales=SC)
        assert _same(k1, after[0]) and _same(v1, after[1])  # the PyTorch append on the GPU: the same bytes
    assert rec.calls == []
    k1, v1 = before[0].clone(), before[1].clone()
    assert _err(attention_decode_packed(qkv, H, k1, v1, pos, kv_heads=4, kv_scales=SC), ref) < 1e-2
    # the bindings check what the Python layer checks
    nat = _ext.native()
    with pytest.raises(RuntimeError):
        nat.attn_decode(q, H, after[0], kb, pos + 1, 0, SCALE, None, 4)  # a mixed pair
    with pytest.raises(RuntimeError):
        nat.attn_decode(q, H, kb, kb, pos + 1, 0, SCALE, None, 4, k_scale=2.0)  # scales with bf16 caches
    with pytest.raises(RuntimeError):
        nat.attn_decode(q, H, *after, pos + 1, 0, SCALE, None, 4, k_scale=0.0)
    with pytest.raises(RuntimeError):
        nat.attn_decode(q, H, e5, e5, pos + 1, 0, SCALE, None, 4)


# ---------------------------------------------------------------- the model
LLAMA = dict(pos="rope", norm="rms", mlp="swiglu", bias=False, kv_heads=1, mlp_ratio=2.0)


def _tiny(window):
    torch.manual_seed(0)
    return gpt_tiny(window=window, **LLAMA).cuda()


@pytest.mark.parametrize("window", [(16, None)], ids=["w16-global"])
def test_gpt_tiny_on_an_fp8_cache(window):
    """bf16 Llama-style gpt_tiny, fp8 cache, scales calibrated on the prompt (margin 2: headroom for the tokens
    that follow)."""
    base = _tiny(window)
    model = copy.deepcopy(base).to(BF)
    tokens = torch.randint(0, 256, (2, 9), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    sc = kv_scales(model, tokens, margin=2.0)
    assert len(sc) == 2 and all(0 < s < 1 for p in sc for s in p)
    n = 60
    fp8 = dict(kv_dtype=FP8, kv_scales=sc)
    for extra in ({}, {"rolling": True}, {"fused": True}, {"rolling": True, "fused": True}):
        a, a_len = model.generate(tokens, n, **fp8, **extra)
        b, b_len = model.generate(tokens, n, graph=True, **fp8, **extra)
        assert torch.equal(a, b) and torch.equal(a_len, b_len) and a_len.tolist() == [n, n], extra
        assert int(a.min()) >= 0 and int(a.max()) < 256
    probe = KVCache(model, 2, dtype=FP8, rolling=True, scales=sc)
    assert probe.rolling == [True, False] and probe.layers[0][0].shape == (2, 1, 32, 64)
    assert all(k.dtype == FP8 and v.dtype == FP8 for k, v in probe.layers)
    rows = [k.shape[2] for k, _ in probe.layers]
    assert sum(k.numel() * k.element_size() + v.numel() * v.element_size() for k, v in probe.layers) == \
        sum(2 * 2 * 1 * r * 64 for r in rows)  # one byte per element
    # decode_step is extend(one token, last_only=True)
    seq = torch.cat([tokens, model.generate(tokens, n, **fp8)[0]], dim=1)
    j, N = 9, seq.shape[1]
    c1, c2 = (KVCache(model, 2, dtype=FP8, rolling=True, scales=sc) for _ in range(2))
    for c in (c1, c2):  # the bytes are compared below: no uninitialised rows
        for k, v in c.layers:
            k.view(U8).zero_(), v.view(U8).zero_()
    model.prefill(seq[:, :j], cache=c1)
    model.prefill(seq[:, :j], cache=c2)
    for t in range(j, j + 30):
        x, y = model.decode_step(seq[:, t], c1), model.extend(seq[:, t:t + 1], c2, last_only=True)
        assert torch.equal(x, y), t
    assert all(_same(p[0], r[0]) and _same(p[1], r[1]) for p, r in zip(c1.layers, c2.layers))
    # teacher-forced incremental logits against the fp32 PyTorch path running the same fp8 cache rule
    def incremental(m, fused=False):
        cache = KVCache(m, 2, dtype=FP8, rolling=True, scales=sc)
        m.prefill(seq[:, :j], cache=cache)
        return torch.stack([m.decode_step(seq[:, t], cache, fused=fused) for t in range(j, N)], dim=1).float()

    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        ref = incremental(copy.deepcopy(base))
        e_torch = _err(incremental(model), ref)
    for fused in (False, True):
        inc = incremental(model, fused)
        e_native = _err(inc, ref)
        print(f"gpt_tiny(window={window}) fp8 cache, teacher-forced logits vs fp32 on the same rule, fused={fused}: "
              f"native {e_native:.5f} PyTorch path {e_torch:.5f}")
        assert torch.isfinite(inc).all() and e_native <= 1.5 * e_torch, (fused, e_native, e_torch)
