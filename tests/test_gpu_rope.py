"""Rotary position embeddings on the native kernel (csrc/rope.hip): ``rope_packed`` in bf16 with head dim
64, ``embed_rows`` without a position table, and ``TransformerLM(pos="rope")`` on every path.

The kernel bar is derived, not measured.  The oracle is fp64 arithmetic on the same bf16 inputs and the
same f32 table; per element ``|got - ref| <= 2^-8 * |ref| + 2^-20 * (|x[i]| + |x[i + 32]|)``: the first
term is the one bf16 rounding of the result (2^-9 relative) with a factor 2, the second covers the f32
products and the sum of operands that may cancel.  For fp32 inputs (PyTorch path) the first term is
``2^-22 * |ref|``.  Lane totals of the cases: 56 (below one workgroup) up to 2176 (8.5 workgroups).

The model bars are those of tests/test_gpu_decode.py: errors relative to the same weights on the fp32
PyTorch path, the incremental paths at most 1.5x the full forward.  The qkv weights are multiplied by 8
so that positions matter to the logits, which the numerics fixture asserts before anything else.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

import torchbooster_amd.models.vit as vit  # noqa: E402
from torchbooster_amd.models import gpt_tiny  # noqa: E402
from torchbooster_amd.ops import attention as A  # noqa: E402
from torchbooster_amd.ops.attention import attention_packed, rope_packed, rope_table  # noqa: E402
from torchbooster_amd.ops.linear import embed_rows  # noqa: E402

DEV = "cuda"
B, H, D, MAXLEN = 2, 4, 64, 64
BF = torch.bfloat16
POSITIONS = [None, (0, 37), (-3, MAXLEN + 5)]


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


def _err(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def table():
    return rope_table(MAXLEN, D, device=DEV)


def _data(hkv, T, dtype=BF, seed=0):
    g = torch.Generator(device=DEV).manual_seed(100 * hkv + T + seed)
    return torch.randn(B, T, (H + 2 * hkv) * D, device=DEV, generator=g).mul(1.5).to(dtype)


def _oracle(x, hkv, table, positions, inverse=False):
    """fp64 on the given inputs and table -> (reference, |x[i]| + |x[i + 32]| per element); positions: host ints"""
    T, hr = x.shape[1], H + hkv
    p = torch.tensor([[min(max((0 if positions is None else positions[b]) + t, 0), table.shape[0] - 1)
                       for t in range(T)] for b in range(B)], device=DEV)
    cs = table.double()[p]  # [B, T, 2, 32]
    c, s = cs[:, :, None, 0], cs[:, :, None, 1]
    if inverse:
        s = -s
    xx = x.double()[..., :hr * D].reshape(B, T, hr, 2, D // 2)
    lo, hi = xx[..., 0, :], xx[..., 1, :]
    ref = x.double().clone()
    ref[..., :hr * D] = torch.stack((lo * c - hi * s, hi * c + lo * s), dim=3).reshape(B, T, hr * D)
    mag = torch.zeros_like(ref)
    mag[..., :hr * D] = torch.stack((lo.abs() + hi.abs(),) * 2, dim=3).reshape(B, T, hr * D)
    return ref, mag


def _within(got, ref, mag, first=2.0 ** -8):
    excess = (got.double() - ref).abs() - (first * ref.abs() + 2.0 ** -20 * mag)
    assert torch.isfinite(got).all() and excess.max() <= 0, excess.max()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("hkv", [4, 2, 1])
@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("positions", POSITIONS, ids=["none", "0-37", "clamped"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
def test_kernel_matches_fp64(monkeypatch, table, hkv, T, positions, inverse):
    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    monkeypatch.setattr(A, "_rope_ref", boom)
    x = _data(hkv, T)
    keep = x.clone()
    pos = _i32(positions)
    got = rope_packed(x, H, table, pos, kv_heads=hkv, inverse=inverse)
    ref, mag = _oracle(x, hkv, table, positions, inverse)
    assert got.shape == x.shape and got.dtype == BF and torch.equal(x, keep)
    _within(got, ref, mag)
    v0 = (H + hkv) * D
    assert torch.equal(_bits(got[..., v0:]), _bits(x[..., v0:]))  # the value part, bit for bit
    assert torch.equal(got[0, 0], x[0, 0])  # position 0 is c = 1, s = 0: the input bits
    if positions is None:
        assert torch.equal(got[1, 0], x[1, 0])
    elif positions[0] < 0:  # -3 .. 0 are clamped to 0
        assert torch.equal(got[0, :4], x[0, :4])
    assert torch.equal(got, rope_packed(x, H, table, pos, kv_heads=hkv, inverse=inverse))  # deterministic
    # in place: the same rotated bits, and the value part's memory is not written at all
    y = x.clone()
    nan = torch.full_like(_bits(y[..., v0:]), 0x7FC5)
    y.view(torch.int16)[..., v0:] = nan
    ret = rope_packed(y, H, table, pos, kv_heads=hkv, inverse=inverse, inplace=True)
    assert ret.data_ptr() == y.data_ptr()
    assert torch.equal(y[..., :v0], got[..., :v0]) and torch.equal(_bits(y[..., v0:]), nan)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("layout", ["rows_ok", "odd_stride", "misaligned"])
def test_strided_views(table, layout, inverse):
    """Rows cut out of a wider buffer: with a row stride in multiples of 8 the kernel reads the view in
    place; a stride or an offset that is not goes through ``.contiguous()``.  The same answer either way."""
    hkv, T, positions = 2, 5, (0, 37)
    E = (H + 2 * hkv) * D
    g = torch.Generator(device=DEV).manual_seed(7)
    pad, off = {"rows_ok": (16, 8), "odd_stride": (12, 8), "misaligned": (16, 4)}[layout]
    wide = torch.randn(B, T, E + pad, device=DEV, generator=g).mul(1.5).to(BF)
    view = wide[..., off:off + E]
    assert A._rows_ok(view) == (layout == "rows_ok")
    keep = wide.clone()
    got = rope_packed(view, H, table, _i32(positions), kv_heads=hkv, inverse=inverse)
    ref, mag = _oracle(view, hkv, table, positions, inverse)
    _within(got, ref, mag)
    assert torch.equal(got, rope_packed(view.contiguous(), H, table, _i32(positions), kv_heads=hkv, inverse=inverse))
    assert torch.equal(wide, keep)
    # in place on the view: the rotated columns change, nothing else in the wide buffer does
    rope_packed(view, H, table, _i32(positions), kv_heads=hkv, inverse=inverse, inplace=True)
    v0 = (H + hkv) * D
    assert torch.equal(view[..., :v0], got[..., :v0])
    keep[..., off:off + v0] = got[..., :v0]
    assert torch.equal(wide, keep)


@pytest.mark.parametrize("how", ["force_reference", "fp32"])
def test_dispatch_to_the_pytorch_path(monkeypatch, table, how):
    calls = []
    real = A._rope_ref
    monkeypatch.setattr(A, "_rope_ref", lambda *a, **k: calls.append(1) or real(*a, **k))
    hkv, T, positions = 2, 5, (0, 37)
    if how == "force_reference":
        monkeypatch.setenv("TBAMD_FORCE_REFERENCE", "1")
        x, first = _data(hkv, T), 2.0 ** -8
    else:
        x, first = _data(hkv, T, torch.float32), 2.0 ** -22
    for inverse in (False, True):
        got = rope_packed(x, H, table, _i32(positions), kv_heads=hkv, inverse=inverse)
        ref, mag = _oracle(x, hkv, table, positions, inverse)
        assert got.dtype == x.dtype
        _within(got, ref, mag, first)
    assert len(calls) == 2
    with pytest.raises(RuntimeError):
        rope_packed(x, H, table.cpu(), kv_heads=hkv)  # the table lives on the device of qkv


def test_native_binding_checks(table):
    nat = A.native()
    x = _data(2, 3)
    with pytest.raises(RuntimeError):
        nat.rope_packed(x, H, table, None, 3)  # kv_heads does not divide heads
    with pytest.raises(RuntimeError):
        nat.rope_packed(x, H, table, None, 4)  # packed width
    with pytest.raises(RuntimeError):
        nat.rope_packed(x, H, table[..., :16].contiguous(), None, 2)  # table width
    with pytest.raises(RuntimeError):
        nat.rope_packed(x, H, table, torch.zeros(B, dtype=torch.int64, device=DEV), 2)
    with pytest.raises(RuntimeError):
        nat.rope_packed(x, H, table, None, 2, False, x.clone())  # out is qkv itself or nothing


def test_gradient_through_attention():
    """d/dqkv of attention_packed(rope_packed(qkv), causal) on the native path against the same composition
    in fp32 on the PyTorch path: at most 1.5x the error attention_packed alone shows on the same inputs."""
    heads, N = 2, 70
    table = rope_table(128, D, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    qkv = torch.randn(B, N, 3 * heads * D, device=DEV, generator=g).to(BF)
    w = torch.randn(B, N, heads * D, device=DEV, generator=g)
    pos = _i32((0, 37))

    def grad(x, rotate):
        x = x.clone().requires_grad_()
        y = rope_packed(x, heads, table, pos) if rotate else x
        out = attention_packed(y, heads, causal=True)
        (out.float() * w).sum().backward()
        return out.detach(), x.grad

    o_nat, g_nat = grad(qkv, True)
    o_ref, g_ref = grad(qkv.float(), True)
    a_nat, ga_nat = grad(qkv, False)
    a_ref, ga_ref = grad(qkv.float(), False)
    e_rope, e_attn = _err(g_nat, g_ref), _err(ga_nat, ga_ref)
    print(f"dqkv vs fp32: rope + attention {e_rope:.5f}, attention alone {e_attn:.5f} ({e_rope / e_attn:.2f}x); "
          f"forward {_err(o_nat, o_ref):.5f} / {_err(a_nat, a_ref):.5f}")
    assert g_nat.dtype == BF and torch.isfinite(g_nat).all()
    assert _err(g_ref, ga_ref) > 0.1  # the rotation changes the gradient: the comparison is not vacuous
    assert e_rope <= 1.5 * e_attn, (e_rope, e_attn)


def test_graph_replay_follows_positions(table):
    """The positions are read on the device: a captured rotation replays with their current values."""
    hkv, T = 2, 5
    x = _data(hkv, T)
    pos = _i32((3, 20))
    rope_packed(x, H, table, pos, kv_heads=hkv)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = rope_packed(x, H, table, pos, kv_heads=hkv)
    graph.replay()
    first = out.clone()
    pos.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, rope_packed(x, H, table, _i32((3, 20)), kv_heads=hkv))
    assert torch.equal(out, rope_packed(x, H, table, _i32((4, 21)), kv_heads=hkv))
    assert not torch.equal(out, first)


# ---------------------------------------------------------------- embed_rows
def test_embed_rows_without_and_with_a_table():
    g = torch.Generator(device=DEV).manual_seed(3)
    tok = torch.randn(50, 128, device=DEV, generator=g).to(BF)
    posw = torch.randn(16, 128, device=DEV, generator=g).to(BF)
    tokens = torch.tensor([[0, 49, 7], [50, -1, 12]], device=DEV)  # two ids out of range
    positions = _i32((2, 15))
    want = tok[tokens.clamp(0, 49)]
    for got in (embed_rows(tokens, tok, None, positions), embed_rows(tokens, tok), embed_rows(tokens[:, :1], tok, None)):
        assert torch.equal(_bits(got), _bits(want[:, :got.shape[1]]))
    # with a table: the contract it always had, f32 sum and one rounding
    at = (positions.to(torch.int64)[:, None] + torch.arange(3, device=DEV)[None, :]).clamp(0, 15)
    with_table = (tok[tokens.clamp(0, 49)].float() + posw[at].float()).to(BF)
    assert torch.equal(embed_rows(tokens, tok, posw, positions), with_table)


# ---------------------------------------------------------------- the model
def _rope_tiny():
    torch.manual_seed(0)
    base = gpt_tiny(pos="rope").cuda()
    with torch.no_grad():
        for blk in base.blocks:
            blk.attn.qkv.weight.mul_(8)
    return base


@pytest.fixture(scope="module")
def numerics():
    """gpt_tiny(pos="rope"), qkv weights x 8: the bf16 model, the tokens, and the teacher-forced logits of
    the fp32 PyTorch path and of the native full forward -- computed once, never modified."""
    base = _rope_tiny()
    N, j = 70, 33
    tokens = torch.randint(0, 256, (2, N), device=DEV)
    lengths = _i32((70, 41))
    mnat = copy.deepcopy(base).to(BF)
    with torch.no_grad():
        full = mnat(tokens, lengths)[:, j:N - 1].float()
        with pytest.MonkeyPatch.context() as mp:  # the stock run: every op on its PyTorch path
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            mref = copy.deepcopy(base)
            ref = mref(tokens, lengths)[:, j:N - 1].float()
            mp.setattr(vit, "rope_packed", lambda qkv, *a, **k: qkv)
            flat = mref(tokens, lengths)[:, j:N - 1].float()
    keep = torch.arange(j, N - 1, device=DEV)[None, :] < lengths[:, None]
    e_full, moved = _err(full[keep], ref[keep]), _err(flat[keep], ref[keep])
    print(f"gpt_tiny(rope) logits vs fp32: full forward {e_full:.5f}; without the rotation {moved:.5f}")
    # the setup is sensitive to positions; if this fails the test is wrong, not the kernel
    assert moved >= 20 * e_full, (moved, e_full)
    return mnat, tokens, lengths, ref, keep, e_full, j, N


@pytest.mark.parametrize("how", ["decode_step", "fused", "extend4"])
def test_gpt_tiny_incremental_vs_reference(numerics, how):
    """Teacher-forced, ragged: prefill 33 tokens, feed tokens 33 .. 68 one at a time (default and fused) or
    through ``extend`` in chunks of 4; the incremental error is at most 1.5x the full forward's."""
    mnat, tokens, lengths, ref, keep, e_full, j, N = numerics
    logits, cache = mnat.prefill(tokens[:, :j], lengths.clamp(max=j))
    assert cache.positions.tolist() == [j, j]
    if how == "extend4":
        inc = torch.cat([mnat.extend(tokens[:, t:t + 4], cache) for t in range(j, N - 1, 4)], dim=1).float()
    else:
        steps = [mnat.decode_step(tokens[:, t], cache, fused=how == "fused") for t in range(j, N - 1)]
        inc = torch.stack(steps, dim=1).float()
    assert cache.positions.tolist() == [N - 1, N - 1]
    e_inc = _err(inc[keep], ref[keep])
    print(f"gpt_tiny(rope) teacher-forced logits vs fp32, {how}: incremental {e_inc:.5f} full forward {e_full:.5f} "
          f"({e_inc / e_full:.2f}x)")
    assert torch.isfinite(inc).all()
    assert e_inc <= 1.5 * e_full, (e_inc, e_full)


def test_generate_graph_equals_eager():
    model = _rope_tiny().to(BF)
    tokens = torch.randint(0, 256, (2, 9), device=DEV)
    plain, plain_len = model.generate(tokens, 24)
    assert plain_len.tolist() == [24, 24]
    eos = int(plain[0, 5])
    for kw in ({}, {"eos": eos}):
        a, a_len = model.generate(tokens, 24, graph=False, **kw)
        b, b_len = model.generate(tokens, 24, graph=True, **kw)
        assert torch.equal(a, b) and torch.equal(a_len, b_len)
        assert a.shape == (2, 24) and int(a.min()) >= 0 and int(a.max()) < 256
    f, f_len = model.generate(tokens, 24, fused=True)
    assert f.shape == (2, 24) and int(f.min()) >= 0 and int(f.max()) < 256 and f_len.tolist() == [24, 24]
    g, g_len = model.generate(tokens, 24, fused=True, graph=True)
    assert torch.equal(f, g) and torch.equal(f_len, g_len)


def test_training_step():
    """One training step at 2 x 32 tokens: every gradient finite and non-zero, and block 0's qkv weight
    gradient against the fp32 PyTorch path within 1.5x of what the learned-position model shows."""
    tokens = torch.randint(0, 256, (2, 32), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    errs = {}
    for pos in ("rope", "learned"):
        torch.manual_seed(0)
        base = gpt_tiny(pos=pos).cuda()
        mnat = copy.deepcopy(base).to(BF)
        mnat.loss(tokens).backward()
        if pos == "rope":
            assert "pos" not in dict(mnat.named_parameters())
            for name, p in mnat.named_parameters():
                assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            mref = copy.deepcopy(base)
            mref.loss(tokens).backward()
        errs[pos] = _err(mnat.blocks[0].attn.qkv.weight.grad, mref.blocks[0].attn.qkv.weight.grad)
    print(f"block 0 qkv weight gradient vs fp32: rope {errs['rope']:.5f} learned {errs['learned']:.5f} "
          f"({errs['rope'] / errs['learned']:.2f}x)")
    assert errs["rope"] <= 1.5 * errs["learned"], errs
