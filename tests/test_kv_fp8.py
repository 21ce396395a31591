"""FP8 (e4m3) KV cache on the PyTorch paths (CPU; the bars of tests/test_rolling.py).

The rule (ops/attention.py): a row is stored as ``rne_e4m3(clamp(f32(x) * inv, -448, 448))`` with ``inv =
float32(1 / scale)`` and read back as ``f32(code) * f32(scale)``; every query that reads the cache sees those
values, a step's own row included.  Here the format is written out a second time -- the 256 codes decoded with
integer arithmetic, the rounding as a brute-force search for the nearest finite code -- and the cache functions
on an fp8 pair are compared against the same functions on the dequantised pair.
"""
import math

import pytest
import torch

import torchbooster_amd.models.vit as vit
from torchbooster_amd.models.gpt import KVCache, TransformerLM, gpt_tiny, kv_scales
from torchbooster_amd.ops.attention import (attention_decode, attention_decode_packed, attention_extend,
                                            attention_extend_packed, kv_cache_append, kv_dequantize, kv_quantize)

FP8 = torch.float8_e4m3fn
NAN_CODE = 0x7F
SCALES = (1.0, 0.37, 8.0)


def _decode_table():
    """The 256 OCP e4m3 codes as float64: 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent 15 with
    mantissa 7 is NaN, there are no infinities, the largest finite value is 448."""
    out = []
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        out.append(-v if s else v)
    return torch.tensor(out, dtype=torch.float64)


TABLE = _decode_table()


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def _nearest_even(y):
    """float32 ``y`` (no NaN) -> uint8 codes: the nearest of the 127 non-negative finite values to ``|y|`` (already
    within 448), ties to the even code, the sign bit of ``y`` on top.  All arithmetic is exact in float64."""
    mag = TABLE[:127]  # codes 0 .. 126, ascending
    a = y.abs().to(torch.float64)
    best = torch.zeros(a.shape, dtype=torch.int64)
    dist = (a - mag[0]).abs()
    for c in range(1, 127):
        d = (a - mag[c]).abs()
        closer = (d < dist) | ((d == dist) & (c % 2 == 0))
        best = torch.where(closer, torch.full_like(best, c), best)
        dist = torch.where(closer, d, dist)
    return (best + 128 * torch.signbit(y).to(torch.int64)).to(torch.uint8)


def _all_bf16():
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


@pytest.mark.parametrize("scale", SCALES)
def test_quantize_is_nearest_even_over_every_bf16_pattern(scale):
    x = _all_bf16()
    got = kv_quantize(x, scale)
    assert got.dtype == FP8 and got.shape == x.shape
    got = got.view(torch.uint8)
    nan = torch.isnan(x)
    assert int(nan.sum()) == 2 * 127
    assert bool(((got[nan] & 0x7F) == NAN_CODE).all())  # a NaN stays a NaN code, of either sign
    y = (x.float() * _f32(1.0 / scale))[~nan]
    y = torch.where(y > 448, torch.full_like(y, 448.0), torch.where(y < -448, torch.full_like(y, -448.0), y))
    want = _nearest_even(y)
    assert torch.equal(got[~nan], want)
    inf = torch.isinf(x)
    assert sorted(got[inf].tolist()) == [0x7E, 0xFE]  # +-inf saturate to +-448
    assert not bool(((got[~nan] & 0x7F) == NAN_CODE).any())
    # beyond +-448 * scale: saturated, not NaN
    big = torch.tensor([449.0, 1e4, -3e38], dtype=torch.bfloat16) * scale
    assert kv_quantize(big, scale).view(torch.uint8).tolist() == [0x7E, 0x7E, 0xFE]


@pytest.mark.parametrize("scale", SCALES)
def test_dequantize_is_the_table_times_the_scale(scale):
    codes = torch.arange(256, dtype=torch.uint8).view(FP8)
    want = (TABLE.to(torch.float32) * _f32(scale))  # one float32 product
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        got = kv_dequantize(codes, scale, dtype)
        assert got.dtype == dtype
        assert torch.equal(torch.isnan(got), torch.isnan(TABLE))
        ok = ~torch.isnan(TABLE)
        assert torch.equal(got[ok], want.to(dtype)[ok])
    assert kv_dequantize(codes).dtype == torch.bfloat16
    assert torch.equal(kv_dequantize(codes, 1.0, torch.float64)[ok], TABLE[ok])  # f32(code) is exact
    # quantising what was dequantised gives the code back (the caches below rely on it)
    back = kv_quantize(kv_dequantize(codes, scale, torch.float32), scale).view(torch.uint8)
    keep = ok & (torch.arange(256) != 0x80)
    assert torch.equal(back[keep], torch.arange(256, dtype=torch.uint8)[keep])


# ---------------------------------------------------------------- append
D = 8
R = 12


def _rand_cache(B, hkv, rows, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randint(0, 256, (B, hkv, rows, D), dtype=torch.uint8, generator=g).view(FP8) for _ in range(2))


@pytest.mark.parametrize("hkv", [2, 1])
@pytest.mark.parametrize("T,pos,lengths,rolling", [
    (1, (0, 7, 11, 29), None, False),
    (5, (0, 9, 12, 40), None, False),  # the last one is dropped, the one before cut at the capacity
    (5, (0, 9, 12, 40), None, True),
    (30, (0, 0, 0, 0), (30, 13, 1, 0), True),  # a ragged prefill of N > R
    (7, (5, -3, -9, 2), (7, 7, 2, 50), True),
])
def test_append_stores_the_quantised_rows(T, pos, lengths, rolling, hkv):
    torch.manual_seed(T)
    B, H, rows = 4, 2, (R if rolling else 14)
    sc = (0.5, 3.0)
    qkv = torch.randn(B, T, (H + 2 * hkv) * D, dtype=torch.bfloat16) * 40
    qkv[:, :, H * D] = 1000.0  # the first key element of every token saturates at scale 0.5
    p = torch.tensor(pos, dtype=torch.int32)
    kw = {"rolling": True, "lengths": None if lengths is None else torch.tensor(lengths, dtype=torch.int32)} \
        if rolling else {}
    # where the bf16 call writes, and what
    kb, vb = (torch.full((B, hkv, rows, D), 7.0, dtype=torch.bfloat16) for _ in range(2))
    mark_k, mark_v = kb.clone(), vb.clone()
    kv_cache_append(kb, vb, qkv, H, p, kv_heads=hkv, **kw)
    nan_q = qkv.clone().fill_(float("nan"))
    kv_cache_append(mark_k, mark_v, nan_q, H, p, kv_heads=hkv, **kw)
    written = torch.isnan(mark_k)
    assert torch.equal(written, torch.isnan(mark_v)) and bool(written.any()) and not bool(written.all())
    kc, vc = _rand_cache(B, hkv, rows, 3)
    k0, v0 = kc.clone(), vc.clone()
    kv_cache_append(kc, vc, qkv, H, p, kv_heads=hkv, kv_scales=sc, **kw)
    for got, old, ref, s in ((kc, k0, kb, sc[0]), (vc, v0, vb, sc[1])):
        got, old = got.view(torch.uint8), old.view(torch.uint8)
        assert torch.equal(got[written], kv_quantize(ref, s).view(torch.uint8)[written])
        assert torch.equal(got[~written], old[~written])  # untouched rows keep their bytes
    assert bool(((kc.view(torch.uint8) & 0x7F) == 0x7E)[written].any())  # the saturation case: 448, not NaN
    # None on an fp8 cache is (1.0, 1.0)
    a, b = _rand_cache(B, hkv, rows, 3)
    c, d = _rand_cache(B, hkv, rows, 3)
    kv_cache_append(a, b, qkv, H, p, kv_heads=hkv, **kw)
    kv_cache_append(c, d, qkv, H, p, kv_heads=hkv, kv_scales=(1.0, 1.0), **kw)
    assert torch.equal(a.view(torch.uint8), c.view(torch.uint8)) and torch.equal(b.view(torch.uint8), d.view(torch.uint8))


# ---------------------------------------------------------------- decode / extend, fp64
H = 12
SCALE = 1.0 / math.sqrt(D)
SC = (0.5, 3.0)
RING = 32  # W = 24: room for T = 5 <= R - W + 1


def _slot_row(p, n, rows):
    j = p
    while j + rows < n:
        j += rows
    while j >= n:
        j -= rows
    return j


def _hidden(B, rows, limits, lows, rolling):
    """[B, rows] bool: the rows / slots no query of the call may load -- at or past ``limits[b]`` or below
    ``lows[b]``, over logical rows ``j(p)`` in a ring."""
    h = torch.zeros(B, rows, dtype=torch.bool)
    for b in range(B):
        for p in range(rows):
            j = _slot_row(p, limits[b], rows) if rolling else p
            h[b, p] = not (max(lows[b], 0) <= j < limits[b])
    return h


def _poison(cache, hidden):
    c = cache.clone().view(torch.uint8)
    c[hidden[:, None, :, None].expand_as(c)] = NAN_CODE
    return c.view(FP8)


CASES = [(None, False, 40), (24, False, 40), (24, True, RING)]


@pytest.mark.parametrize("window,rolling,rows", CASES, ids=["global", "w24", "w24-ring"])
@pytest.mark.parametrize("hkv", [12, 4])
def test_decode_is_the_call_on_the_dequantised_cache(hkv, window, rolling, rows):
    torch.manual_seed(hkv)
    lens = (5, rows, 100) if rolling else (5, 33, rows)
    B = len(lens)
    q = torch.randn(B, H, D, dtype=torch.float64)
    kc, vc = _rand_cache(B, hkv, rows, 11)
    nonan = lambda c: ((c.view(torch.uint8) & 0x7F) != NAN_CODE)  # noqa: E731
    kc = torch.where(nonan(kc), kc.view(torch.uint8), torch.zeros((), dtype=torch.uint8)).view(FP8)
    vc = torch.where(nonan(vc), vc.view(torch.uint8), torch.zeros((), dtype=torch.uint8)).view(FP8)
    n = torch.tensor(lens, dtype=torch.int32)
    kw = dict(kv_heads=hkv, window=window, **({"rolling": True} if rolling else {}))
    got = attention_decode(q, kc, vc, n, SCALE, kv_scales=SC, **kw)
    want = attention_decode(q, kv_dequantize(kc, SC[0], torch.float64), kv_dequantize(vc, SC[1], torch.float64), n,
                            SCALE, **kw)
    assert got.dtype == torch.float64 and torch.allclose(got, want, atol=1e-12, rtol=0)
    hid = _hidden(B, rows, lens, [x - (window or x) for x in lens], rolling)
    assert bool(hid.any())
    again = attention_decode(q, _poison(kc, hid), _poison(vc, hid), n, SCALE, kv_scales=SC, **kw)
    assert torch.equal(again, got)
    # scales of 1 are the default
    assert torch.equal(attention_decode(q, kc, vc, n, SCALE, **kw),
                       attention_decode(q, kc, vc, n, SCALE, kv_scales=(1.0, 1.0), **kw))


@pytest.mark.parametrize("window,rolling,rows", CASES, ids=["global", "w24", "w24-ring"])
@pytest.mark.parametrize("hkv", [12, 4])
def test_extend_is_the_call_on_the_dequantised_cache(hkv, window, rolling, rows):
    torch.manual_seed(hkv + 1)
    T = 5
    pos = (0, rows - T, 95) if rolling else (0, 20, rows - T)
    B = len(pos)
    q = torch.randn(B, T, H, D, dtype=torch.float64)
    kc, vc = _rand_cache(B, hkv, rows, 12)
    p = torch.tensor(pos, dtype=torch.int32)
    ends = [x + T for x in pos]
    hid = _hidden(B, rows, ends, [x + 1 - (window or x + 1) for x in pos], rolling)
    assert bool(hid.any())
    # the visible rows hold no NaN code; the hidden ones may hold anything
    for c in (kc, vc):
        u = c.view(torch.uint8)
        u[((u & 0x7F) == NAN_CODE) & ~hid[:, None, :, None]] = 0x31
    kw = dict(kv_heads=hkv, window=window, **({"rolling": True} if rolling else {}))
    got = attention_extend(q, kc, vc, p, SCALE, kv_scales=SC, **kw)
    clean = [torch.where(hid[:, None, :, None], torch.zeros((), dtype=torch.float64), kv_dequantize(c, s, torch.float64))
             for c, s in ((kc, SC[0]), (vc, SC[1]))]
    want = attention_extend(q, clean[0], clean[1], p, SCALE, **kw)
    assert torch.allclose(got, want, atol=1e-12, rtol=0)
    assert torch.equal(attention_extend(q, _poison(kc, hid), _poison(vc, hid), p, SCALE, kv_scales=SC, **kw), got)
    one = attention_extend(q[:, :1], kc, vc, p, SCALE, kv_scales=SC, **kw)
    dec = attention_decode(q[:, 0], kc, vc, p + 1, SCALE, kv_scales=SC, **kw)
    assert torch.allclose(one[:, 0], dec, atol=1e-12, rtol=0)


def test_packed_functions_quantise_then_attend():
    torch.manual_seed(6)
    B, hkv = 2, 4
    kc, vc = _rand_cache(B, hkv, 20, 13)
    for c in (kc, vc):
        u = c.view(torch.uint8)
        u[(u & 0x7F) == NAN_CODE] = 0
    p = torch.tensor((3, 9), dtype=torch.int32)
    for T in (1, 4):
        qkv = torch.randn(B, T, (H + 2 * hkv) * D, dtype=torch.float64) * 3
        k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        got = attention_extend_packed(qkv, H, k1, v1, p, SCALE, kv_heads=hkv, kv_scales=SC)
        kv_cache_append(k2, v2, qkv, H, p, kv_heads=hkv, kv_scales=SC)
        assert torch.equal(k1.view(torch.uint8), k2.view(torch.uint8))
        assert torch.equal(v1.view(torch.uint8), v2.view(torch.uint8))
        q = qkv[..., :H * D].reshape(B, T, H, D)
        want = attention_extend(q, k2, v2, p, SCALE, kv_heads=hkv, kv_scales=SC)  # its own row: quantised
        assert torch.equal(got.view(B, T, H, D), want)
        if T == 1:
            k3, v3 = kc.clone(), vc.clone()
            dec = attention_decode_packed(qkv, H, k3, v3, p, SCALE, kv_heads=hkv, kv_scales=SC)
            assert torch.equal(dec, got) and torch.equal(k3.view(torch.uint8), k1.view(torch.uint8))


# ---------------------------------------------------------------- models/gpt.py
LLAMA = dict(norm="rms", mlp="swiglu", bias=False, pos="rope", kv_heads=2)
LAYER_SCALES = [(0.37, 2.9), (0.011, 0.6)]


def _llama(window=(8, None)):
    torch.manual_seed(0)
    return gpt_tiny(max_len=96, window=window, **LLAMA).double()


def _reference_rule(monkeypatch, scales_of):
    """Make the three cache functions models/vit.py calls run the fp8 rule on a FLOAT32 cache pair, spelled with the
    public functions: append the new rows, round them through ``kv_quantize`` -> ``kv_dequantize`` (the whole cache is
    rounded: quantising what was dequantised gives the code back, and hidden rows cannot matter), then attend.
    The rounding sits between the append and the attention because a step's own row is seen quantised.  Other
    caches go to the real functions.  ``scales_of(k_cache)`` -> the pair of that layer."""
    real = {n: getattr(vit, n) for n in ("kv_cache_append", "attention_decode_packed", "attention_extend_packed")}

    def round_trip(k_cache, v_cache):
        for c, s in zip((k_cache, v_cache), scales_of(k_cache)):
            c.copy_(kv_dequantize(kv_quantize(c, s), s, torch.float32))

    def append(k_cache, v_cache, qkv, heads, positions, **kw):
        if k_cache.dtype != torch.float32:
            return real["kv_cache_append"](k_cache, v_cache, qkv, heads, positions, **kw)
        assert "kv_scales" not in kw
        kv_cache_append(k_cache, v_cache, qkv, heads, positions, **kw)
        round_trip(k_cache, v_cache)

    def extend_packed(qkv, heads, k_cache, v_cache, positions, scale=None, **kw):
        if k_cache.dtype != torch.float32:
            name = "attention_decode_packed" if qkv.shape[1] == 1 else "attention_extend_packed"
            return real[name](qkv, heads, k_cache, v_cache, positions, scale, **kw)
        kw.pop("fused", None)
        B, T, _ = qkv.shape
        hkv = kw.get("kv_heads", heads)
        hd = qkv.shape[2] // (heads + 2 * hkv)
        akw = {k: v for k, v in kw.items() if k in ("kv_heads", "rolling")}
        kv_cache_append(k_cache, v_cache, qkv, heads, positions, **akw)
        round_trip(k_cache, v_cache)
        q = qkv[..., :heads * hd].reshape(B, T, heads, hd)
        return attention_extend(q, k_cache, v_cache, positions, scale, **kw).reshape(B, T, heads * hd)

    monkeypatch.setattr(vit, "kv_cache_append", append)
    monkeypatch.setattr(vit, "attention_decode_packed", extend_packed)
    monkeypatch.setattr(vit, "attention_extend_packed", extend_packed)


def test_model_on_an_fp8_cache_follows_the_rule(monkeypatch):
    model = _llama()
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(0, 256, (2, 60), generator=g)
    lengths = torch.tensor((21, 13), dtype=torch.int32)
    fp8 = KVCache(model, 2, dtype=FP8, rolling=True, lookahead=3, scales=LAYER_SCALES)
    ref = KVCache(model, 2, dtype=torch.float32, rolling=True, lookahead=3)
    assert fp8.rolling == ref.rolling == [True, False] and fp8.scales == LAYER_SCALES and ref.scales == [None, None]
    assert fp8.layers[0][0].dtype == FP8 and fp8.layers[0][0].shape == (2, 2, 16, 64)
    for (k, v) in ref.layers:
        k.zero_(), v.zero_()
    by_ptr = {kv[0].data_ptr(): s for kv, s in zip(ref.layers, LAYER_SCALES)}
    _reference_rule(monkeypatch, lambda k: by_ptr[k.data_ptr()])
    a, _ = model.prefill(tokens[:, :21], lengths, fp8)
    b, _ = model.prefill(tokens[:, :21], lengths, ref)
    assert torch.equal(a, b)  # the prefill attends to its own unquantised qkv
    plain, _ = model.prefill(tokens[:, :21], lengths)
    assert torch.equal(a, plain)
    for t in range(21, 40):
        a, b = model.decode_step(tokens[:, t], fp8), model.decode_step(tokens[:, t], ref)
        assert torch.allclose(a, b, atol=1e-9, rtol=0), t
    for t, n, ln in ((40, 3, None), (43, 1, None), (44, 3, (2, 3)), (47, 2, (1, 1))):
        kw = {} if ln is None else {"lengths": torch.tensor(ln, dtype=torch.int32)}
        a, b = model.extend(tokens[:, t:t + n], fp8, **kw), model.extend(tokens[:, t:t + n], ref, **kw)
        assert torch.allclose(a, b, atol=1e-9, rtol=0), t
        assert torch.equal(fp8.positions, ref.positions)
    a, b = model.decode_step(tokens[:, 52], fp8, fused=True), model.decode_step(tokens[:, 52], ref, fused=True)
    assert torch.allclose(a, b, atol=1e-9, rtol=0)
    # the quantisation is really there: an unquantised cache gives other logits
    lin = KVCache(model, 2)
    model.prefill(tokens[:, :21], lengths, lin)
    assert not torch.allclose(model.decode_step(tokens[:, 21], lin), model.decode_step(tokens[:, 21],
                              model.prefill(tokens[:, :21], lengths, KVCache(model, 2, dtype=FP8, scales=LAYER_SCALES))[1]),
                              atol=1e-6, rtol=0)


def test_generate_on_an_fp8_cache(monkeypatch):
    model = _llama()
    tokens = torch.randint(0, 256, (2, 11), generator=torch.Generator().manual_seed(3))
    lengths = torch.tensor((11, 6), dtype=torch.int32)
    pair = (0.02, 0.7)
    got, gl = model.generate(tokens, 30, lengths, rolling=True, kv_dtype=FP8, kv_scales=pair)
    fused, _ = model.generate(tokens, 30, lengths, rolling=True, kv_dtype=FP8, kv_scales=pair, fused=True)
    assert torch.equal(got, fused)
    # a caller's fp8 cache brings its own dtype and scales
    cache = KVCache(model, 2, capacity=41, dtype=FP8, rolling=True, scales=pair)
    assert cache.scales == [pair, pair]
    own, _ = model.generate(tokens[:, :6], 30, cache=cache)
    assert torch.equal(own, model.generate(tokens[:, :6], 30, rolling=True, kv_dtype=FP8, kv_scales=pair)[0])
    with pytest.raises(ValueError):
        model.generate(tokens, 4, cache=cache, kv_dtype=FP8)
    # speculative decoding: the draft's cache gets the dtype and scales of 1
    made = []
    init = KVCache.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(KVCache, "__init__", spy)
    draft = _llama((4, None))
    spec, _ = model.generate(tokens, 12, draft=draft, draft_tokens=3, kv_dtype=FP8, kv_scales=pair)
    assert [c.scales for c in made] == [[pair, pair], [(1.0, 1.0)] * 2]
    assert all(c.layers[0][0].dtype == FP8 for c in made)
    assert spec.shape == (2, 12)
    monkeypatch.setattr(KVCache, "__init__", init)
    # against the rule on a float32 cache
    _reference_rule(monkeypatch, lambda k: pair)
    want, wl = model.generate(tokens, 30, lengths, rolling=True, kv_dtype=torch.float32)
    assert torch.equal(got, want) and torch.equal(gl, wl)


def test_kv_scales_calibrates_on_the_valid_rows():
    model = _llama().float()
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, 256, (3, 20), generator=g)
    lengths = torch.tensor((20, 7, 1), dtype=torch.int32)
    sc = kv_scales(model, tokens, lengths)
    assert len(sc) == 2 and all(len(p) == 2 and all(math.isfinite(s) and s > 0 for s in p) for p in sc)
    _, cache = model.prefill(tokens, lengths, KVCache(model, 3, capacity=20))
    valid = (torch.arange(20)[None, :] < lengths[:, None])[:, None, :, None]
    for (k, v), pair in zip(cache.layers, sc):
        for c, s in zip((k, v), pair):
            amax = float(c.abs().masked_fill(~valid, 0).max())
            assert s == pytest.approx(amax / 448.0, rel=1e-6)
            x = c[valid.expand_as(c)]
            back = kv_dequantize(kv_quantize(x, s), s, torch.float32)
            # no value saturates: each lands within half a code spacing (2^-4 relative; 2^-10 of a unit below the normals)
            assert bool(((back - x).abs() <= x.abs() / 16 + s * 2.0 ** -10).all())
    # pad rows do not move the result
    other = tokens.clone()
    other[1, 7:] = (other[1, 7:] + 17) % 256
    other[2, 1:] = 3
    assert kv_scales(model, other, lengths) == sc
    assert kv_scales(model, tokens) != sc
    twice = kv_scales(model, tokens, lengths, margin=2.0)
    assert all(b == pytest.approx(2 * a, rel=1e-12) for p, q in zip(sc, twice) for a, b in zip(p, q))
    # an all-zero layer gives 1.0
    with torch.no_grad():
        model.blocks[1].attn.qkv.weight.zero_()
    z = kv_scales(model, tokens, lengths)
    assert z[1] == (1.0, 1.0) and z[0] == sc[0]
    with pytest.raises(ValueError):
        kv_scales(model, tokens, margin=0.0)


def test_errors():
    q = torch.randn(1, 2, D)
    kc = torch.zeros(1, 2, R, D, dtype=torch.uint8).view(FP8)
    kb = torch.zeros(1, 2, R, D, dtype=torch.bfloat16)
    pos = torch.zeros(1, dtype=torch.int32)
    one = torch.randn(1, 1, 6 * D)
    for bad in ((0.0, 1.0), (1.0, -2.0), (float("inf"), 1.0), (1.0, float("nan")), (1.0,), 3.0, ("a", 1.0)):
        with pytest.raises(ValueError):
            attention_decode(q, kc, kc, pos, kv_scales=bad)
        with pytest.raises(ValueError):
            kv_cache_append(kc.clone(), kc.clone(), one, 2, pos, kv_scales=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            kv_quantize(q, bad)
        with pytest.raises(ValueError):
            kv_dequantize(kc, bad)
    with pytest.raises(ValueError):
        kv_dequantize(kb)
    # scales with a cache that is not fp8 (a mixed pair is not one either)
    for k, v in ((kb, kb), (kc, kb), (kb, kc)):
        with pytest.raises(ValueError):
            attention_decode(q, k, v, pos, kv_scales=(1.0, 1.0))
        with pytest.raises(ValueError):
            attention_extend(q[:, None], k, v, pos, kv_scales=(1.0, 1.0))
        with pytest.raises(ValueError):
            attention_decode_packed(one, 2, k.clone(), v.clone(), pos, kv_scales=(1.0, 1.0))
        with pytest.raises(ValueError):
            attention_extend_packed(one, 2, k.clone(), v.clone(), pos, kv_scales=(1.0, 1.0))
        with pytest.raises(ValueError):
            kv_cache_append(k.clone(), v.clone(), one, 2, pos, kv_scales=(1.0, 1.0))
    model = TransformerLM(256, 32, 2, 2, 16)
    with pytest.raises(ValueError):
        KVCache(model, 1, scales=(1.0, 1.0))  # the model's dtype
    with pytest.raises(ValueError):
        KVCache(model, 1, dtype=torch.bfloat16, scales=[(1.0, 1.0)] * 2)
    with pytest.raises(ValueError):
        KVCache(model, 1, dtype=FP8, scales=[(1.0, 1.0)] * 3)  # a wrong length
    with pytest.raises(ValueError):
        KVCache(model, 1, dtype=FP8, scales=[(1.0, 1.0), (0.0, 1.0)])
    with pytest.raises(ValueError):
        KVCache(model, 1, dtype=FP8, scales=[(1.0, 1.0), 2.0])
    assert KVCache(model, 1, dtype=FP8).scales == [(1.0, 1.0)] * 2
    assert KVCache(model, 1, dtype=FP8, scales=(0.5, 2)).scales == [(0.5, 2.0)] * 2
    assert KVCache(model, 1, dtype=FP8, scales=[(0.5, 2.0), (3.0, 4.0)]).scales == [(0.5, 2.0), (3.0, 4.0)]
    assert KVCache(model, 1).scales == [None, None]
    c = KVCache(model, 2, dtype=FP8, capacity=8)
    assert sum(k.numel() * k.element_size() + v.numel() * v.element_size() for k, v in c.layers) == 2 * 2 * 2 * 2 * 8 * 16


def test_other_caches_make_the_calls_they_made(monkeypatch):
    calls = []
    for name in ("kv_cache_append", "attention_decode_packed", "attention_extend_packed"):
        fn = getattr(vit, name)

        def wrapped(*a, _fn=fn, _name=name, **kw):
            calls.append((_name, dict(kw)))
            return _fn(*a, **kw)
        monkeypatch.setattr(vit, name, wrapped)
    torch.manual_seed(0)
    model = TransformerLM(256, 32, 2, 2, 96)  # the default model
    tokens = torch.randint(0, 256, (2, 9), generator=torch.Generator().manual_seed(4))
    lengths = torch.tensor((9, 4), dtype=torch.int32)
    _, cache = model.prefill(tokens, lengths)
    model.decode_step(tokens[:, 0], cache)
    model.decode_step(tokens[:, 0], cache, fused=True)
    model.extend(tokens[:, :3], cache)
    model.generate(tokens, 4)
    model.generate(tokens, 4, draft=TransformerLM(256, 32, 2, 2, 96), draft_tokens=2)
    bf = KVCache(model, 2, dtype=torch.bfloat16)
    model.prefill(tokens, lengths, bf)
    model.decode_step(tokens[:, 0], bf)
    model.extend(tokens[:, :3], bf)
    assert len(calls) > 20
    assert all(kw == ({"fused": True} if "fused" in kw else {}) for _, kw in calls), calls
    # an fp8 cache: every call carries its layer's pair and nothing else new
    del calls[:]
    windowed = TransformerLM(256, 32, 2, 2, 96, window=(4, None), kv_heads=1)
    pairs = [(0.5, 2.0), (0.25, 4.0)]
    c8 = KVCache(windowed, 2, dtype=FP8, rolling=True, lookahead=3, scales=pairs)
    windowed.prefill(tokens, lengths, c8)
    windowed.decode_step(tokens[:, 0], c8)
    windowed.extend(tokens[:, :3], c8)
    assert calls == [
        ("kv_cache_append", {"kv_heads": 1, "rolling": True, "lengths": lengths, "kv_scales": pairs[0]}),
        ("kv_cache_append", {"kv_heads": 1, "kv_scales": pairs[1]}),
        ("attention_decode_packed", {"kv_heads": 1, "window": 4, "rolling": True, "kv_scales": pairs[0]}),
        ("attention_decode_packed", {"kv_heads": 1, "kv_scales": pairs[1]}),
        ("attention_extend_packed", {"kv_heads": 1, "window": 4, "rolling": True, "kv_scales": pairs[0]}),
        ("attention_extend_packed", {"kv_heads": 1, "kv_scales": pairs[1]}),
    ]
