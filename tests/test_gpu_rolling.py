"""Rolling KV cache on the native kernels: the RING instantiations of the append, decode and extend kernels
(csrc/attention_decode.hip, csrc/attention_extend.hip, csrc/attn_ring.h) against an fp32 LOGICAL oracle.

The oracle keeps a linear cache of every logical row and attends to rows ``max(0, L - W) <= j < L`` of it; the
ring under test is built from that cache slot by slot, ``ring[p] = linear[j(p)]``, ``j(p)`` the largest
``j = p (mod R)`` below the limit.  Bars: the ``1e-2`` of tests/test_gpu_window.py (relative Frobenius error,
for extend per row too) and that file's model comparison.
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
from torchbooster_amd.ops.attention import (attention_decode, attention_decode_packed, attention_extend,  # noqa: E402
                                            attention_extend_packed, kv_cache_append)

DEV = "cuda"
BF = torch.bfloat16
SCALE = 1.0 / math.sqrt(64)
ONE_SPLIT = 1 << 20
H = 12
MARK = 7.0  # what a never-written slot holds where the cache is compared bit for bit


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _row_err(got, want):
    """worst per-(batch, query) relative error of [B, T, H, D] tensors"""
    d = torch.linalg.vector_norm(got.float() - want.float(), dim=(2, 3))
    return (d / torch.linalg.vector_norm(want.float(), dim=(2, 3)).clamp_min(1e-12)).max().item()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _cache_oracle(q, kc, vc, lim, W):
    """fp32 softmax of q [B, T, H, D] over the LOGICAL rows max(0, lim[b, t] - W) <= j < lim[b, t] of the linear
    caches (lim: a host list)."""
    q, kc, vc = q.float(), kc.float(), vc.float()
    G = q.shape[2] // kc.shape[1]
    kc, vc = kc.repeat_interleave(G, 1), vc.repeat_interleave(G, 1)
    lim = torch.tensor(lim, device=DEV)
    j = torch.arange(kc.shape[2], device=DEV)
    vis = (j < lim[..., None]) & (j >= lim[..., None] - W)  # [B, T, N]
    s = torch.einsum("bthd,bhjd->bhtj", q, kc) * SCALE
    p = torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1)
    return torch.einsum("bhtj,bhjd->bthd", p, vc)


def _rows_of(n, R):
    """j(p) for the limits n (a host list) -> int64 [B, R]"""
    n = torch.tensor(n, device=DEV)[:, None]
    return n - 1 - torch.remainder(n - 1 - torch.arange(R, device=DEV)[None, :], R)


def _ring(lin, n, R, fill=MARK):
    """The ring of the linear cache ``lin`` [B, Hkv, N, 64] for the limits ``n``: slot p holds logical row j(p),
    or ``fill`` where none was ever written."""
    j = _rows_of(n, R)
    idx = j.clamp_min(0)[:, None, :, None].expand(lin.shape[0], lin.shape[1], R, 64)
    mark = torch.full((), fill, dtype=lin.dtype, device=DEV)
    return torch.where((j >= 0)[:, None, :, None], lin.gather(2, idx), mark)


def _poison(ring, n, lo, R, fill):
    """``ring`` with ``fill`` in every hidden slot: never written, or logical row below ``lo`` (host lists)."""
    j = _rows_of(n, R)
    hidden = (j < 0) | (j < torch.tensor(lo, device=DEV)[:, None])
    return torch.where(hidden[:, None, :, None], torch.full((), fill, dtype=ring.dtype, device=DEV), ring)


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


# ---------------------------------------------------------------- decode
RINGS = ((24, (1, 8, 9, 24)), (136, (120, 121, 136)))  # 136: two chunks of 128


def _lens(R):
    return (1, R - 1, R, R + 1, 3 * R + 5)


@functools.lru_cache(maxsize=None)
def _decode_case(R, hkv):
    """The packed step, the linear caches after the step's append at logical row len - 1, the ring before the
    step (the step's slot holds what it held: the row R tokens back, or the mark) and the ring after it."""
    g = torch.Generator(device=DEV).manual_seed(R + hkv)
    lens = _lens(R)
    B, N = len(lens), 3 * R + 5
    qkv = torch.randn(B, 1, (H + 2 * hkv) * 64, device=DEV, generator=g).mul(1.5).to(BF)
    ka, va = (torch.randn(B, hkv, N, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    for b, n in enumerate(lens):
        ka[b, :, n - 1] = qkv[b, 0, H * 64:(H + hkv) * 64].view(hkv, 64)
        va[b, :, n - 1] = qkv[b, 0, (H + hkv) * 64:].view(hkv, 64)
    before = tuple(_ring(c, [n - 1 for n in lens], R) for c in (ka, va))
    after = tuple(_ring(c, list(lens), R) for c in (ka, va))
    return qkv, ka, va, before, after, lens


@pytest.mark.parametrize("fused", [False, True], ids=["default", "fused"])
@pytest.mark.parametrize("hkv", [H, 2, 1])
def test_decode_matches_the_logical_oracle(knobs, hkv, fused):
    nat = knobs
    kw = {} if hkv == H else {"kv_heads": hkv}
    for R, windows in RINGS:
        qkv, ka, va, before, after, lens = _decode_case(R, hkv)
        B = len(lens)
        q = qkv[:, :, :H * 64].view(B, 1, H, 64)
        pos = _i32([n - 1 for n in lens])
        for W in windows:
            want = _cache_oracle(q, ka, va, [[n] for n in lens], W).view(B, 1, H * 64)
            for chunk in (128, 8):  # 8: with R - W >= 8 a whole chunk is hidden
                nat.attn_decode_set_chunk(chunk)
                for gb in (0, 1, 2, 3, 4):
                    if gb and (H // hkv) % gb:
                        continue
                    nat.attn_decode_set_head_block(gb)
                    k1, v1 = before[0].clone(), before[1].clone()
                    got = attention_decode_packed(qkv, H, k1, v1, pos, fused=fused, window=W, rolling=True, **kw)
                    e = _err(got, want)
                    assert torch.isfinite(got).all() and e < 1e-2, (R, W, hkv, fused, chunk, gb, e)
                    assert torch.equal(k1, after[0]) and torch.equal(v1, after[1]), (R, W, chunk, gb)
                    # the bits of the unfused call, and of a second run
                    k2, v2 = before[0].clone(), before[1].clone()
                    again = attention_decode_packed(qkv, H, k2, v2, pos, window=W, rolling=True, **kw)
                    assert torch.equal(got, again), (R, W, hkv, fused, chunk, gb)
                    if W == 1:  # the step's own value row exactly
                        own = qkv[:, 0, (H + hkv) * 64:].view(B, hkv, 64).repeat_interleave(H // hkv, 1)
                        assert torch.equal(got.view(B, H, 64), own)


@pytest.mark.parametrize("fill", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("hkv", [H, 1])
def test_decode_hidden_slots_never_enter(knobs, hkv, fill):
    nat = knobs
    kw = {} if hkv == H else {"kv_heads": hkv}
    for R, windows in RINGS:
        qkv, ka, va, _, after, lens = _decode_case(R, hkv)
        B = len(lens)
        q = qkv[:, 0, :H * 64].view(B, H, 64)
        lengths = _i32(lens)
        for W in windows:
            k2, v2 = (_poison(c, list(lens), [n - W for n in lens], R, fill) for c in after)
            assert W == R or not torch.isfinite(k2).all()
            for chunk in (128, 8):
                nat.attn_decode_set_chunk(chunk)
                clean = attention_decode(q, *after, lengths, window=W, rolling=True, **kw)
                got = attention_decode(q, k2, v2, lengths, window=W, rolling=True, **kw)
                assert torch.isfinite(got).all() and torch.equal(got, clean), (R, W, chunk)
                want = _cache_oracle(q[:, None], ka, va, [[n] for n in lens], W)
                assert _err(clean.view(B, 1, H, 64), want) < 1e-2, (R, W, chunk)
    # add: the limit is lengths + add, never clamped to the ring
    R, W = 24, 9
    qkv, ka, va, _, after, lens = _decode_case(R, hkv)
    q = qkv[:, :, :H * 64]
    shifted = nat.attn_decode(q.view(len(lens), H, 64), H, *after, _i32([n - 1 for n in lens]), 1, SCALE, None,
                              hkv, W, True)
    assert torch.equal(shifted.view(len(lens), H, 64),
                       attention_decode(q.view(len(lens), H, 64), *after, _i32(lens), window=W, rolling=True, **kw))


def test_decode_head_block_policy_sees_a_ring_as_live_rows():
    nat = _ext.native()
    # 64 * 12 * 32 chunks = 24576 one-head waves share loads; a linear window of 512 leaves 5 live chunks, a
    # ring of 4096 rows has all 32 live whatever the window
    assert nat.attn_decode_head_block(64, 12, 1, 4096, 512) == 1
    assert nat.attn_decode_head_block(64, 12, 1, 4096, 512, True) == 4
    assert nat.attn_decode_head_block(8, 12, 1, 528, 512, True) == nat.attn_decode_head_block(8, 12, 1, 528)
    with pytest.raises(RuntimeError):
        nat.attn_decode_head_block(8, 12, 1, 528, 0, True)  # a ring needs a window
    with pytest.raises(RuntimeError):
        nat.attn_decode_head_block(8, 12, 1, 528, 529, True)


def test_decode_graph_replay_follows_positions_across_a_wrap():
    R, W, hkv, B, steps = 136, 120, 2, 3, 8  # two chunks: the merge launch is part of the graph
    g = torch.Generator(device=DEV).manual_seed(3)
    rows = torch.randn(steps + 1, B, 1, (H + 2 * hkv) * 64, device=DEV, generator=g).mul(1.5).to(BF)
    kc, vc = (torch.randn(B, hkv, R, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    start = (R - 3, 2 * R - 5, 300)  # the first two wrap within the replays
    qkv, pos = rows[0].clone(), _i32(start)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    attention_decode_packed(qkv, H, k1, v1, pos, fused=True, kv_heads=hkv, window=W, rolling=True)  # warm-up
    attention_decode_packed(qkv, H, k2, v2, pos, fused=True, kv_heads=hkv, window=W, rolling=True)
    pos.add_(1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = attention_decode_packed(qkv, H, k1, v1, pos, fused=True, kv_heads=hkv, window=W, rolling=True)
    outs = []
    for s in range(1, steps + 1):
        qkv.copy_(rows[s])
        graph.replay()
        want = attention_decode_packed(rows[s], H, k2, v2, pos.clone(), fused=True, kv_heads=hkv, window=W,
                                       rolling=True)
        assert torch.equal(out, want), s
        assert torch.equal(k1, k2) and torch.equal(v1, v2), s
        outs.append(out.clone())
        pos.add_(1)
    torch.cuda.synchronize()
    assert pos.tolist() == [x + steps + 1 for x in start]
    assert not torch.equal(outs[0], outs[-1])


# ---------------------------------------------------------------- append
@pytest.mark.parametrize("hkv", [H, 2])
def test_append_keeps_the_last_valid_rows(hkv):
    R, T, B = 24, 61, 4
    g = torch.Generator(device=DEV).manual_seed(hkv)
    qkv = torch.randn(B, T, (H + 2 * hkv) * 64, device=DEV, generator=g).to(BF)
    kc, vc = (torch.full((B, hkv, R, 64), MARK, device=DEV, dtype=BF) for _ in range(2))
    lengths = (61, 30, 5, 0)  # 0 behaves as 1
    kw = {} if hkv == H else {"kv_heads": hkv}
    kv_cache_append(kc, vc, qkv, H, _i32([0] * B), rolling=True, lengths=_i32(lengths), **kw)
    lin_k = qkv[..., H * 64:(H + hkv) * 64].view(B, T, hkv, 64).transpose(1, 2)
    lin_v = qkv[..., (H + hkv) * 64:].view(B, T, hkv, 64).transpose(1, 2)
    n = [min(max(x, 1), T) for x in lengths]
    # pad rows are dropped: the mark stays where nothing was stored
    assert torch.equal(kc, _ring(lin_k, n, R)) and torch.equal(vc, _ring(lin_v, n, R))
    # the PyTorch path writes the same ring; without lengths every row counts; a negative position stores nothing
    k2, v2 = (torch.full((B, hkv, R, 64), MARK, device=DEV) for _ in range(2))
    kv_cache_append(k2, v2, qkv.float(), H, _i32([0] * B), rolling=True, lengths=_i32(lengths), **kw)
    assert torch.equal(k2.to(BF), kc) and torch.equal(v2.to(BF), vc)
    kv_cache_append(kc, vc, qkv, H, _i32([0] * B), rolling=True, **kw)
    assert torch.equal(kc, _ring(lin_k, [T] * B, R))
    k3 = kc.clone()
    kv_cache_append(k3, vc.clone(), qkv[:, :3], H, _i32([-3] * B), rolling=True, **kw)
    assert torch.equal(k3, kc)
    with pytest.raises(RuntimeError):
        _ext.native().attn_kv_append(qkv, H, kc, vc, _i32([0] * B), 0 if hkv == H else hkv, False, _i32(lengths))


# ---------------------------------------------------------------- extend
@pytest.fixture(params=[64, ONE_SPLIT, 0], ids=["split64", "one_split", "default"])
def split(request, knobs):
    knobs.attn_extend_set_split(request.param)
    return request.param


EXT_RINGS = ((40, (1, 8, 24)), (136, (120,)))  # R - W >= 16 everywhere: T = 17 fits; 136: three splits of 64


def _positions(R):
    return (3 * R - 3, 0, 2 * R + 1)  # the call's own append wraps; an empty ring; past two wraps


@functools.lru_cache(maxsize=None)
def _extend_case(R, T, hkv):
    """The packed call, the linear caches with its rows at pos[b] + t, and the ring before the call."""
    g = torch.Generator(device=DEV).manual_seed(R + 10 * T + hkv)
    pos = _positions(R)
    B, N = len(pos), 3 * R + T
    packed = torch.randn(B, T, (H + 2 * hkv) * 64, device=DEV, generator=g).mul(1.5).to(BF)
    kl, vl = (torch.randn(B, hkv, N, 64, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    for b, p in enumerate(pos):
        kl[b, :, p:p + T] = packed[b, :, H * 64:(H + hkv) * 64].view(T, hkv, 64).transpose(0, 1)
        vl[b, :, p:p + T] = packed[b, :, (H + hkv) * 64:].view(T, hkv, 64).transpose(0, 1)
    before = tuple(_ring(c, [max(p, 1) for p in pos], R) for c in (kl, vl))
    if 0 in pos:  # an empty ring holds the mark alone
        for c in before:
            c[pos.index(0)] = MARK
    lim = [[p + t + 1 for t in range(T)] for p in pos]
    return packed, kl, vl, before, pos, lim


@pytest.mark.parametrize("hkv", [H, 2])
@pytest.mark.parametrize("T", [2, 5, 16, 17])
def test_extend_matches_the_logical_oracle(split, T, hkv):
    kw = {} if hkv == H else {"kv_heads": hkv}
    for R, windows in EXT_RINGS:
        packed, kl, vl, before, pos, lim = _extend_case(R, T, hkv)
        B = len(pos)
        q = packed[..., :H * 64].view(B, T, H, 64)
        ends = [p + T for p in pos]
        after = tuple(_ring(c, ends, R) for c in (kl, vl))
        for W in windows:
            want = _cache_oracle(q, kl, vl, lim, W)
            k1, v1 = before[0].clone(), before[1].clone()
            got = attention_extend_packed(packed, H, k1, v1, _i32(pos), window=W, rolling=True, **kw).view(B, T, H, 64)
            e, worst = _err(got, want), _row_err(got, want)
            assert torch.isfinite(got).all() and e < 1e-2 and worst < 1e-2, (R, T, W, hkv, split, e, worst)
            assert torch.equal(k1, after[0]) and torch.equal(v1, after[1]), (R, T, W)
            # NaN / Inf in every hidden slot (never written, or below the first query's lower limit) changes
            # nothing; neither does a second run
            for fill in (float("nan"), float("inf")):
                k2, v2 = (_poison(c, ends, [p + 1 - W for p in pos], R, fill) for c in after)
                again = attention_extend(q, k2, v2, _i32(pos), window=W, rolling=True, **kw)
                assert torch.equal(again, got), (R, T, W, fill)
            if W == 1:
                own = packed[..., (H + hkv) * 64:].view(B, T, hkv, 64).repeat_interleave(H // hkv, 2)
                assert torch.equal(got, own)


def test_extend_T1_is_decode_packed(split):
    R, W, hkv = 40, 24, 2
    packed, _, _, before, pos, _ = _extend_case(R, 2, hkv)
    one = packed[:, :1].contiguous()
    k1, v1, k2, v2 = before[0].clone(), before[1].clone(), before[0].clone(), before[1].clone()
    a = attention_extend_packed(one, H, k1, v1, _i32(pos), window=W, rolling=True, kv_heads=hkv)
    b = attention_decode_packed(one, H, k2, v2, _i32(pos), window=W, rolling=True, kv_heads=hkv)
    assert torch.equal(a, b) and torch.equal(k1, k2) and torch.equal(v1, v2)
    q = one[..., :H * 64].view(3, 1, H, 64)
    e = attention_extend(q, k1, v1, _i32(pos), window=W, rolling=True, kv_heads=hkv)
    assert _err(e.view(3, 1, H * 64), b) < 1e-2


def test_extend_workspace_fully_written(split):
    nat = _ext.native()
    R, T, W, hkv = 136, 17, 120, 2
    packed, kl, vl, _, pos, _ = _extend_case(R, T, hkv)
    B = len(pos)
    q = packed[..., :H * 64].view(B, T, H, 64)
    kc, vc = (_ring(c, [p + T for p in pos], R) for c in (kl, vl))
    a = attention_extend(q, kc, vc, _i32(pos), window=W, rolling=True, kv_heads=hkv)
    need = nat.attn_extend_workspace(B, H, T, R)
    ws = torch.full((max(need, 4),), float("nan"), device=DEV)
    o = nat.attn_extend(q, kc, vc, _i32(pos), SCALE, ws, hkv, W, True).view(B, T, H, 64)
    assert torch.isfinite(o).all() and torch.equal(o, a)
    if need:  # every max and sum is written, those of empty splits included
        nparts = B * H * ((T + 15) // 16) * nat.attn_extend_splits(B, H, T, R)
        assert not torch.isnan(ws[nparts * 16 * 64:nparts * 16 * 66]).any()


# ---------------------------------------------------------------- dispatch
def test_dispatch(monkeypatch):
    nat = _ext.native()
    R, W, T = 12, 4, 3
    lens, pos = (1, 11, 12, 13, 41), (0, 9, 12, 38, 5)
    # head dim 32, fp32 and CPU tensors take the PyTorch ring path -- and agree with the logical oracle
    for D, dtype, dev, bar in ((32, BF, DEV, 1e-2), (64, torch.float32, DEV, 1e-5), (64, torch.float32, "cpu", 1e-5)):
        g = torch.Generator().manual_seed(D)
        B, N = len(lens), 48
        q = torch.randn(B, T, 2, D, generator=g)
        kl, vl = (torch.randn(B, 2, N, D, generator=g) for _ in range(2))
        for n, lim, x in (([*lens], [[n] for n in lens], q[:, :1]),
                          ([p + T for p in pos], [[p + t + 1 for t in range(T)] for p in pos], q)):
            last = torch.tensor(n)[:, None] - 1
            j = last - torch.remainder(last - torch.arange(R)[None, :], R)
            idx = j.clamp_min(0)[:, None, :, None].expand(B, 2, R, D)
            kr, vr = (torch.where((j >= 0)[:, None, :, None], c.gather(2, idx), torch.full((), float("nan")))
                      for c in (kl, vl))
            xs, kr, vr = (t.to(dev, dtype) for t in (x, kr, vr))
            if x.shape[1] == 1:
                got = attention_decode(xs[:, 0], kr, vr, torch.tensor(n, dtype=torch.int32, device=dev), window=W,
                                       rolling=True)[:, None]
            else:
                got = attention_extend(xs, kr, vr, torch.tensor(pos, dtype=torch.int32, device=dev), window=W,
                                       rolling=True)
            # the oracle on what the path read: the rounded inputs, in fp32
            x32, k32, v32 = (t.to(dtype).float() for t in (x, kl, vl))
            jj = torch.arange(N)
            lm = torch.tensor(lim)
            vis = (jj < lm[..., None]) & (jj >= lm[..., None] - W)
            s = torch.einsum("bthd,bhjd->bhtj", x32, k32) / math.sqrt(D)
            want = torch.einsum("bhtj,bhjd->bthd", torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1), v32)
            assert torch.isfinite(got).all() and _err(got.cpu(), want) < bar, (D, dtype, dev)
    # bf16, head dim 64 on the GPU is native: no PyTorch path may run
    qkv, _, _, before, after, ln = _decode_case(24, 2)
    with monkeypatch.context() as mp:
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        k1, v1 = before[0].clone(), before[1].clone()
        ref = attention_decode_packed(qkv, H, k1, v1, _i32([n - 1 for n in ln]), kv_heads=2, window=9, rolling=True)
        assert torch.equal(k1, after[0]) and torch.equal(v1, after[1])

    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    for name in ("_decode_ref", "_extend_ref", "_append_ref", "_append_ring_ref"):
        monkeypatch.setattr(A, name, boom)
    for fused in (False, True):
        k1, v1 = before[0].clone(), before[1].clone()
        got = attention_decode_packed(qkv, H, k1, v1, _i32([n - 1 for n in ln]), kv_heads=2, window=9, rolling=True,
                                      fused=fused)
        assert _err(got, ref) < 1e-2
    packed, _, _, eb, ep, _ = _extend_case(40, 5, 2)
    attention_extend_packed(packed, H, eb[0].clone(), eb[1].clone(), _i32(ep), kv_heads=2, window=8, rolling=True)
    # the bindings check what the Python layer checks
    q5 = packed[..., :H * 64].view(3, 5, H, 64)
    with pytest.raises(RuntimeError):
        nat.attn_extend(q5, *eb, _i32(ep), SCALE, None, 2, 0, True)  # no window
    with pytest.raises(RuntimeError):
        nat.attn_extend(q5, *eb, _i32(ep), SCALE, None, 2, 41, True)  # W > R
    with pytest.raises(RuntimeError):
        nat.attn_extend(q5, *eb, _i32(ep), SCALE, None, 2, 37, True)  # T > R - W + 1
    with pytest.raises(RuntimeError):
        nat.attn_decode_append(qkv, H, *before, _i32([n - 1 for n in ln]), SCALE, 2, 25, True)


# ---------------------------------------------------------------- the model
W_MODEL = 16
LLAMA = dict(pos="rope", norm="rms", mlp="swiglu", bias=False, kv_heads=1, mlp_ratio=2.0)


def _tiny(window=W_MODEL):
    torch.manual_seed(0)
    return gpt_tiny(window=window, **LLAMA).cuda()


@pytest.mark.parametrize("window", [W_MODEL, (None, 5)], ids=["w16", "global-w5"])
def test_gpt_tiny_generate_rolling(window):
    """Greedy generation on rolling caches (R = 32 / 24 rows) to a context of 118 tokens, more than 3 R: the
    graph replay equals the eager run bit for bit, default and fused; the caller's rolling cache over two
    turns equals itself under a graph; and the teacher-forced incremental logits on a rolling cache sit within
    1.5x of the full forward's error against the fp32 PyTorch path, as the linear cache's do in
    tests/test_gpu_window.py."""
    base = _tiny(window)
    model = copy.deepcopy(base).to(BF)
    tokens = torch.randint(0, 256, (2, 9), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    n = 110
    probe = KVCache(model, 2, rolling=True)
    R = min(k.shape[2] for k, _ in probe.layers)
    assert R == (32 if window == W_MODEL else 24) and 9 + n >= 3 * R  # roundup8(W + 15)
    assert probe.rolling == ([True, True] if window == W_MODEL else [False, True])
    a, a_len = model.generate(tokens, n, rolling=True)
    b, b_len = model.generate(tokens, n, rolling=True, graph=True)
    assert torch.equal(a, b) and torch.equal(a_len, b_len) and a_len.tolist() == [n, n]
    f, _ = model.generate(tokens, n, rolling=True, fused=True)
    g, _ = model.generate(tokens, n, rolling=True, fused=True, graph=True)
    assert torch.equal(f, g) and int(f.min()) >= 0 and int(f.max()) < 256
    # two turns on a caller's rolling cache
    turn2 = torch.randint(0, 256, (2, 5), device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    turns = []
    for graph in (False, True):
        cache = KVCache(model, 2, rolling=True)
        out1, _ = model.generate(tokens, 50, cache=cache, graph=graph)
        out2, _ = model.generate(torch.cat([out1[:, -1:], turn2], dim=1), 40, cache=cache, graph=graph)
        assert out2.shape == (2, 40) and cache.positions.tolist() == [9 + 49 + 6 + 39] * 2
        turns.append((out1, out2))
    assert all(torch.equal(x, y) for x, y in zip(*turns))
    # a draft with another window, both caches rolling
    draft = copy.deepcopy(_tiny(4)).to(BF)
    s, s_len = model.generate(tokens, 100, draft=draft, draft_tokens=3, rolling=True)
    assert s.shape == (2, 100) and s_len.tolist() == [100, 100] and torch.equal(s[:, 0], a[:, 0])
    assert int(s.min()) >= 0 and int(s.max()) < 256
    # teacher-forced logits on a rolling cache against the fp32 PyTorch path
    seq = torch.cat([tokens, a], dim=1)
    j, N = 9, seq.shape[1]
    with torch.no_grad():
        full = model(seq)[:, j:].float()
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            ref = copy.deepcopy(base)(seq)[:, j:].float()
    e_full = _err(full, ref)
    for fused in (False, True):
        cache = KVCache(model, 2, rolling=True)
        model.prefill(seq[:, :j], cache=cache)
        inc = torch.stack([model.decode_step(seq[:, t], cache, fused=fused) for t in range(j, N)], dim=1).float()
        e_inc = _err(inc, ref)
        print(f"gpt_tiny(window={window}) rolling, teacher-forced logits vs fp32, fused={fused}: incremental "
              f"{e_inc:.5f} full forward {e_full:.5f}")
        assert torch.isfinite(inc).all() and e_inc <= 1.5 * e_full, (fused, e_inc, e_full)
    cache = KVCache(model, 2, rolling=True)
    model.prefill(seq[:, :j], cache=cache)
    ext = torch.cat([model.extend(seq[:, t:t + 11], cache) for t in range(j, N, 11)], dim=1).float()
    assert _err(ext, ref) <= 1.5 * e_full
    # a prompt longer than the ring: the prefill keeps the last R valid rows and decoding goes on from there
    cache = KVCache(model, 2, rolling=True)
    model.prefill(seq[:, :70], _i32((70, 41)), cache)
    lin = KVCache(model, 2)
    model.prefill(seq[:, :70], _i32((70, 41)), lin)
    x, y = model.decode_step(seq[:, 70], cache).float(), model.decode_step(seq[:, 70], lin).float()
    # the same step on the linear cache: two bf16 paths, each within the 1e-2 bar of fp32, so 2e-2 apart at most
    print(f"gpt_tiny(window={window}) step after a prompt longer than the ring, rolling vs linear: {_err(x, y):.5f}")
    assert torch.isfinite(x).all() and _err(x, y) < 2e-2
    # bytes: sum_i 2 * B * Hkv * rows_i * 64 * 2
    rows = [k.shape[2] for k, _ in cache.layers]
    assert sum(k.numel() * 2 + v.numel() * 2 for k, v in cache.layers) == sum(2 * 2 * 1 * r * 64 * 2 for r in rows)
    assert rows != [k.shape[2] for k, _ in lin.layers]
