"""Attention sinks on the native kernels: the SINK forward and the sink-gradient kernel (csrc/attention.hip,
csrc/attention_sink.hip) against fp64 on the same bf16 inputs, the decode and extend kernels against an fp32 oracle
over the visible rows with NaN in the hidden ones, ``gpt_tiny(sinks=True)`` against its fp32 PyTorch path.  ``H = 3``,
one sink per regime (+6, 0, -4): a swapped head index or a scaled sink shows.  Bars: those of tests/test_gpu_window.py
for the same kernels (relative Frobenius error < 1e-2 on o and the cache paths, < 2e-2 on dq / dk / dv: a sink only
shrinks probabilities); dsinks within 1.5x the error of the PyTorch bf16 path (as tests/test_gpu_moe.py)."""
import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.models import gpt_tiny  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops.attention import (attention, attention_decode, attention_decode_packed,  # noqa: E402
                                            attention_extend, attention_ref, kv_dequantize, kv_quantize)

DEV, BF, H = "cuda", torch.bfloat16, 3
SCALE = 1.0 / math.sqrt(64)
SINKS = (6.0, 0.0, -4.0)
NOOP = (-1e4,) * H  # exp2((-1e4 - m) * log2e) underflows to an exact 0


def _f32(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


def _err(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


# ---------------------------------------------------------------- training kernels
MODES = {"dense": {}, "causal": {"causal": True}, "ragged": {"causal": True, "ragged": True},
         "window": {"causal": True, "window": 5}}
DRAWS = 64  # output gradients dsinks is pooled over (below)


@functools.lru_cache(maxsize=None)
def _case(N, mode):
    """bf16 inputs, DRAWS output gradients and the fp64 reference on them: computed once, never modified."""
    g = torch.Generator(device=DEV).manual_seed(N)
    q, k, v = (torch.randn(2, H, N, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(3))
    do = torch.randn(DRAWS, 2, H, N, 64, device=DEV, generator=g).to(BF)
    kw = dict(MODES[mode])
    if kw.pop("ragged", False):
        kw["key_lengths"] = _i32((N, (N + 1) // 2))
    return (q, k, v, do), kw, _run(N, mode, (q.double(), k.double(), v.double(), do.double(), kw), attention_ref)


def _run(N, mode, case=None, fn=attention):
    """(o, dq, dk, dv) for the first output gradient and dsinks [DRAWS, H], one row per output gradient."""
    q, k, v, do, kw = case or (*_case(N, mode)[0], _case(N, mode)[1])
    ins = [t.clone().requires_grad_() for t in (q, k, v)] + [_f32(SINKS).requires_grad_()]
    o = fn(*ins[:3], SCALE, sinks=ins[3], **kw)
    first = torch.autograd.grad(o, ins, do[0], retain_graph=True)
    rest = [torch.autograd.grad(o, ins[3], d, retain_graph=True)[0] for d in do[1:]]
    return (o.detach(),) + first[:3] + (torch.stack([first[3]] + rest),)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N", [1, 64, 65, 130, 257])
def test_training_kernels_vs_float64(N, mode):
    """dsinks has H = 3 elements, one of which dominates: the error of one backward is a single noise draw (bf16
    rounding of O in delta natively, of s and dP on the PyTorch path) and the ratio of two such draws says nothing.
    It is therefore pooled over DRAWS independent output gradients -- the error of [DRAWS, H] values -- which puts both
    sides within about 10 % of their expectation."""
    ref = _case(N, mode)[2]
    got = _run(N, mode)
    with pytest.MonkeyPatch.context() as mp:  # the PyTorch bf16 path sets the bar of dsinks
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        bar = _err(_run(N, mode)[4], ref[4])
    errs = [_err(a, b) for a, b in zip(got, ref)]
    print(f"N={N} {mode}: o, dq, dk, dv, dsinks vs float64 {errs}; dsinks of the PyTorch bf16 path {bar:.3e}")
    assert all(torch.isfinite(t).all() for t in got) and got[4].dtype == torch.float32
    assert errs[0] < 1e-2 and max(errs[1:4]) < 2e-2 and errs[4] <= 1.5 * bar, (errs, bar)
    assert torch.equal(got[4], _run(N, mode)[4])  # no atomics: the same bits on every run


@pytest.mark.parametrize("mode", ["dense", "ragged", "window"])
@pytest.mark.parametrize("N", [65, 257])
def test_underflowing_sink_is_an_exact_noop_in_training(N, mode):
    nat = _ext.native()
    (q, k, v, _), kw, _ = _case(N, mode)
    args = (q, k, v, SCALE, kw.get("causal", False), kw.get("key_lengths"), kw.get("window", 0))
    old = nat.attn_set_head_mask(0)  # a call with sinks takes the 128-row kernel: compare that kernel with itself
    try:
        o, lse = nat.attn_forward(*args)
    finally:
        nat.attn_set_head_mask(old)
    o2, lse2 = nat.attn_forward(*args, _f32(NOOP))
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    o3, lse3 = nat.attn_forward(*args, _f32(SINKS))
    assert not torch.equal(o, o3) and (lse3 >= lse).all() and not torch.equal(lse3, lse)


# ---------------------------------------------------------------- decode and extend
def _oracle(q, kl, vl, lim, W, sinks):
    """fp32 softmax of q [B, T, H, 64] over the logical rows max(0, lim[b][t] - W) <= j < lim[b][t] of kl / vl
    [B, Hkv, n, 64] plus the sink column, which is dropped after the softmax."""
    q, kl, vl = q.float(), kl.float(), vl.float()
    kl, vl = (c.repeat_interleave(H // c.shape[1], 1) for c in (kl, vl))
    lim = torch.tensor(lim, device=DEV)
    j = torch.arange(kl.shape[2], device=DEV)
    vis = (j < lim[..., None]) & (True if W is None else j >= lim[..., None] - W)  # [B, T, n]
    s = (torch.einsum("bthd,bhjd->bhtj", q, kl) * SCALE).masked_fill(~vis[:, None], float("-inf"))
    col = _f32(sinks)[None, :, None, None].expand(*s.shape[:3], 1)
    p = torch.softmax(torch.cat((s, col), -1), -1)[..., :-1]
    return torch.einsum("bhtj,bhjd->bthd", p, vl)


def _physical(kl, vl, first, n, rows, ring, scales):
    """The cache a call finds: logical rows first[b] <= j < n[b] of kl / vl in row j (slot j mod rows of a ring), NaN
    everywhere else; with scales, e4m3 codes."""
    out = []
    for src, sc in zip((kl, vl), scales or (None, None)):
        c = torch.full((src.shape[0], src.shape[1], rows, 64), float("nan"), device=DEV)
        for b in range(src.shape[0]):
            j = torch.arange(max(first[b], n[b] - rows if ring else 0), n[b], device=DEV)
            c[b, :, j % rows if ring else j] = src[b, :, j].float()
        out.append(c.to(BF) if sc is None else kv_quantize(c, sc))
    return out


CACHES = {"one-chunk": dict(cap=128, lens=(5, 128)), "chunks": dict(cap=384, lens=(5, 300)),
          "window": dict(cap=384, lens=(5, 300), W=70), "ring": dict(cap=128, lens=(5, 300), W=100, ring=True),
          "fp8": dict(cap=384, lens=(5, 300), scales=(0.05, 0.04))}


@pytest.mark.parametrize("hkv", [3, 1])
@pytest.mark.parametrize("case", list(CACHES))
def test_decode_vs_fp32(case, hkv):
    nat = _ext.native()
    c = CACHES[case]
    cap, lens, W, ring, scales = c["cap"], c["lens"], c.get("W"), c.get("ring", False), c.get("scales")
    g = torch.Generator(device=DEV).manual_seed(cap + hkv)
    qkv = torch.randn(2, 1, (H + 2 * hkv) * 64, device=DEV, generator=g).mul(1.5).to(BF)
    kl, vl = (torch.randn(2, hkv, max(lens), 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    for b, n in enumerate(lens):  # the step's own row is logical row n - 1
        kl[b, :, n - 1] = qkv[b, 0, H * 64:(H + hkv) * 64].view(hkv, 64)
        vl[b, :, n - 1] = qkv[b, 0, (H + hkv) * 64:].view(hkv, 64)
    if scales:  # every query sees the dequantised codes, its own row included
        kl, vl = (kv_dequantize(kv_quantize(t, s), s, torch.float32) for t, s in zip((kl, vl), scales))
    first = [0 if W is None else max(0, n - W) for n in lens]
    cache = _physical(kl, vl, first, [n - 1 for n in lens], cap, ring, scales)  # before the append
    kw = {"kv_heads": hkv, **({} if W is None else {"window": W}), **({"rolling": True} if ring else {}),
          **({"kv_scales": scales} if scales else {})}
    pos = _i32([n - 1 for n in lens])
    want = _oracle(qkv[..., :H * 64].view(2, 1, H, 64), kl, vl, [[n] for n in lens], W, SINKS).view(2, 1, H * 64)
    outs = {}
    old = nat.attn_decode_set_head_block(-1)
    try:
        for gb in (0, 1, 3 if hkv == 1 else 1):  # the policy's block, a block of 1, a whole group of 3
            nat.attn_decode_set_head_block(gb)
            for fused in (False, True):
                for name, s in (("sinks", SINKS), ("noop", NOOP), ("none", None)):
                    k1, v1 = (t.clone() for t in cache)
                    outs[gb, fused, name] = attention_decode_packed(qkv, H, k1, v1, pos, fused=fused, **kw,
                                                                    **({} if s is None else {"sinks": _f32(s)}))
    finally:
        nat.attn_decode_set_head_block(old)
    got = outs[0, False, "sinks"]
    e = _err(got, want)
    print(f"decode {case} hkv={hkv}: {e:.3e}")
    assert torch.isfinite(got).all() and e < 1e-2
    for (gb, fused, name), o in outs.items():  # neither the head block nor the fused append changes a bit
        assert torch.equal(o, outs[0, False, name]), (gb, fused, name)
    assert torch.equal(outs[0, False, "noop"], outs[0, False, "none"]) and not torch.equal(got, outs[0, False, "none"])


@pytest.mark.parametrize("split", [1 << 20, 64], ids=["one_split", "split64"])
@pytest.mark.parametrize("T", [1, 5, 17])
def test_extend_vs_fp32(T, split):
    nat = _ext.native()
    hkv, cap, pos = 1, 300, (100, 3)  # the causal limits fall inside a 64-row tile
    g = torch.Generator(device=DEV).manual_seed(T)
    q = torch.randn(2, T, H, 64, device=DEV, generator=g).mul(1.5).to(BF)
    kl, vl = (torch.randn(2, hkv, cap, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    lim = [[p + t + 1 for t in range(T)] for p in pos]
    kc, vc = _physical(kl, vl, [0, 0], [x[-1] for x in lim], cap, False, None)
    want = _oracle(q, kl, vl, lim, None, SINKS)
    old = nat.attn_extend_set_split(-1)
    nat.attn_extend_set_split(split)
    try:
        got, noop, none = (attention_extend(q, kc, vc, _i32(pos), kv_heads=hkv, **({} if s is None else {"sinks": _f32(s)}))
                           for s in (SINKS, NOOP, None))
    finally:
        nat.attn_extend_set_split(old)
    e = _err(got, want)
    print(f"extend T={T} split={split}: {e:.3e}")
    assert torch.isfinite(got).all() and e < 1e-2
    assert torch.equal(noop, none) and not torch.equal(got, none)
    if T == 1:  # one new token IS a decode step
        dec = attention_decode(q[:, 0], kc, vc, _i32([p + 1 for p in pos]), kv_heads=hkv, sinks=_f32(SINKS))
        assert _err(got[:, 0], dec) < 1e-2


def test_decode_graph_replay_follows_sinks():
    g = torch.Generator(device=DEV).manual_seed(0)
    q = torch.randn(2, H, 64, device=DEV, generator=g).to(BF)
    kc, vc = (torch.randn(2, 1, 384, 64, device=DEV, generator=g).to(BF) for _ in range(2))
    lengths, sinks = _i32((300, 5)), _f32(SINKS)
    eager = [attention_decode(q, kc, vc, lengths, kv_heads=1, sinks=_f32(s)) for s in (SINKS, SINKS[::-1])]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = attention_decode(q, kc, vc, lengths, kv_heads=1, sinks=sinks)
    for want in (eager[0], eager[0], eager[1], eager[1]):  # several replays; the sinks change in place between them
        sinks.copy_(_f32(SINKS if want is eager[0] else SINKS[::-1]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    assert not torch.equal(eager[0], eager[1])


# ---------------------------------------------------------------- the model
def _tiny(sinks=True):
    torch.manual_seed(0)
    model = gpt_tiny(sinks=sinks, norm="rms", mlp="swiglu", pos="rope", kv_heads=2, window=[4, None]).cuda()
    for i, blk in enumerate(model.blocks if sinks else ()):
        blk.attn.sinks.data.copy_(_f32((2.0 - i, -1.0)))
    return model


def _step(model, tokens, lengths, reference=False):
    """(loss, block 0's qkv weight gradient, every layer's sinks gradient) of one training step."""
    with pytest.MonkeyPatch.context() as mp:
        if reference:
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        model.zero_grad()
        loss = model.loss(tokens, lengths)
        loss.backward()
    at = [b.attn for b in model.blocks]
    return loss.item(), at[0].qkv.weight.grad.clone(), torch.cat([x.sinks.grad for x in at if x.sinks is not None] or
                                                                  [_f32([])])


def test_gpt_tiny_training_step_vs_reference():
    """One training step against the fp32 PyTorch path: the loss within the bf16 bar (1e-2 relative) and block 0's qkv
    weight gradient within 1.5x of the error of the model without sinks (tests/test_gpu_window.py).  The sinks' own
    gradients get the bar of that weight gradient; they are 2 values a layer and sums of either sign, so one step's
    error is a single draw and they are pooled over 8 token batches.  (The PyTorch bf16 path on the same bf16 model is
    printed next to it: it forms delta as sum_j p_j dP_j in f32, the kernels as rowsum(dO * O) from the bf16 O, which
    at this model's near-uniform attention is the noisier of the two: 1.05e-2 against 6.5e-3.)"""
    g = torch.Generator(device=DEV).manual_seed(5)
    batches = [torch.randint(0, 256, (2, 70), device=DEV, generator=g) for _ in range(8)]
    lengths, errs = _i32((70, 41)), {}
    for sinks in (False, True):
        base = _tiny(sinks)
        mnat, mref = copy.deepcopy(base).to(BF), copy.deepcopy(base)
        nat, bar, ref = ([_step(m, t, lengths, r) for t in batches[:8 if sinks else 1]]
                         for m, r in ((mnat, False), (copy.deepcopy(mnat), True), (mref, True)))
        assert abs(nat[0][0] - ref[0][0]) < 1e-2 * abs(ref[0][0]), (sinks, nat[0][0], ref[0][0])
        errs[sinks] = _err(nat[0][1], ref[0][1])
    ds, ds_bar = (_err(torch.stack([x[2] for x in m]), torch.stack([x[2] for x in ref])) for m in (nat, bar))
    print(f"block 0 qkv weight gradient vs fp32 {errs}; sinks gradients {ds:.3e}, PyTorch bf16 path {ds_bar:.3e}")
    assert all(b.attn.sinks.grad.dtype == torch.float32 and b.attn.sinks.grad.abs().min() > 0 for b in mnat.blocks)
    assert errs[True] <= 1.5 * errs[False] and ds <= 1.5 * errs[False], (errs, ds, ds_bar)


def test_gpt_tiny_generate():
    """Greedy generation: a graph replay equals the eager run bit for bit, fused or not, and the teacher-forced
    incremental logits sit within 1.5x of the full forward's error against fp32 (tests/test_gpu_window.py)."""
    base = _tiny()
    model = copy.deepcopy(base).to(BF)
    tokens = torch.randint(0, 256, (2, 9), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    a, a_len = model.generate(tokens, 30, graph=False)
    assert torch.equal(a, model.generate(tokens, 30, graph=True)[0]) and a_len.tolist() == [30, 30]
    assert torch.equal(model.generate(tokens, 30, fused=True)[0], model.generate(tokens, 30, fused=True, graph=True)[0])
    seq = torch.cat([tokens, a], dim=1)
    with torch.no_grad():
        full = model(seq)[:, 9:].float()
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            ref = base(seq)[:, 9:].float()
            assert not torch.allclose(ref, _tiny(False)(seq)[:, 9:].float(), atol=1e-3)  # the sinks matter
    e_full = _err(full, ref)
    for fused in (False, True):
        _, cache = model.prefill(seq[:, :9])
        inc = torch.stack([model.decode_step(seq[:, t], cache, fused=fused) for t in range(9, 39)], dim=1).float()
        print(f"teacher-forced logits vs fp32, fused={fused}: incremental {_err(inc, ref):.5f} full {e_full:.5f}")
        assert torch.isfinite(inc).all() and _err(inc, ref) <= 1.5 * e_full
    _, cache = model.prefill(seq[:, :9])
    ext = torch.cat([model.extend(seq[:, t:t + 7], cache) for t in range(9, 39, 7)], dim=1).float()
    assert _err(ext, ref) <= 1.5 * e_full
