"""RMSNorm, SwiGLU and the few-row kernel's RMS prologue / SwiGLU epilogue on the GPU, and the Llama-style
``gpt_tiny`` built from them.

``rms_norm`` (csrc/layernorm.hip, RMS instantiation) against an fp64 oracle on the same inputs, per element:
2^-8 |ref| for bf16 (the f32 sum of at most 4096 non-negative squares is off by at most 2^-12 relative,
halved by the square root, and nothing in the forward cancels, so what is left is the one bf16 rounding of
the result: half a unit in the last of 8 significand bits, at most 2^-8 / (1 + 2^-8) of the value); f32:
2^-20 |ref|.  The stream output is the exact sum rounded once: 2^-8 |ref| for bf16 (the one bf16 rounding is
at most 2^-8 / (1 + 2^-8), about 2^-8 - 2^-16, which leaves room for the 2^-24 rounding the f32 sum of two
bf16 values has ahead of the store), 2^-24 |ref| for f32.  Gradients against fp32 autograd with the bars of
tests/test_gpu_layernorm.py.  Shapes: that file's list without its 25216-row case -- every compile-time
row-group layout, the runtime-R kernel (C = 2304, 64, 8) and partial last groups.

``swiglu`` (csrc/swiglu.hip) against fp64: forward 2^-8 |ref| + 2^-30, backward 2^-8 |ref| + 2^-20 |dy|
(|up| (1 + |g|) + |g|), the second term for the cancellation in 1 + g (1 - s(g)) near g = -1.28.

``linear_rows(rms=, act="swiglu")``: the inputs and bars of tests/test_gpu_rows.py, re-stated here: relative
Frobenius error against fp32 math on the bf16 inputs below 1e-2 and at most 1.5x that of the unfused
composition ``rms_norm -> linear -> swiglu``; M * F >= 16 wherever the prologue is on, for the reason given
there (an output that cancels to nearly nothing can be off by more than 1 % of itself).

The model: bars of tests/test_gpu_rope.py -- incremental paths at most 1.5x the error of the full forward
against the same weights on the fp32 PyTorch path.
"""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

import torchbooster_amd.models.vit as vit  # noqa: E402
from torchbooster_amd.models.gpt import gpt_tiny  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops.act import swiglu  # noqa: E402
from torchbooster_amd.ops.linear import linear, linear_gelu, linear_rows  # noqa: E402
from torchbooster_amd.ops.norm import rms_norm  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
EPS = 1e-6


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    _ext.native()


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _within(got, ref, bound, tag):
    """|got - ref| <= bound element by element (ref, bound in fp64)."""
    excess = (got.double() - ref).abs() - bound
    assert torch.isfinite(got).all(), tag
    assert excess.max().item() <= 0, (tag, excess.max().item(), (excess > 0).sum().item())


# ---------------------------------------------------------------- rms_norm
RMS_SHAPES = [(1001, 768), (3, 768), (999, 384), (517, 192), (333, 256), (77, 512), (129, 1024), (41, 1280),
              (17, 1536), (9, 2048), (11, 3072), (5, 4096), (23, 2304), (70, 64), (13, 8)]


@pytest.mark.parametrize("M,C", RMS_SHAPES)
@pytest.mark.parametrize("dt", [BF, torch.float32])
@pytest.mark.parametrize("res", [False, True])
def test_rms_norm_fwd_bwd(M, C, dt, res):
    torch.manual_seed(M + C)
    x = (torch.randn(M, C, device=DEV) * 2 + 0.5).to(dt).requires_grad_()
    r = torch.randn(M, C, device=DEV).to(dt).requires_grad_() if res else None
    w = (torch.rand(C, device=DEV) + 0.5).requires_grad_()
    out = rms_norm(x, w, EPS, r)
    y, xs = out if res else (out, None)
    assert y.dtype == dt and y.shape == (M, C)

    # forward: fp64 oracle on the same inputs
    xs64 = x.detach().double() + r.detach().double() if res else x.detach().double()
    y64 = xs64 * torch.rsqrt(xs64.pow(2).mean(dim=-1, keepdim=True) + EPS) * w.detach().double()
    _within(y.detach(), y64, (2.0 ** -8 if dt == BF else 2.0 ** -20) * y64.abs(), "y")
    if res:
        assert xs.dtype == dt
        _within(xs.detach(), xs64, (2.0 ** -8 if dt == BF else 2.0 ** -24) * xs64.abs(), "stream")

    # gradients: fp32 autograd, the stream gradient consumed too
    xf = x.detach().float().requires_grad_()
    rf = r.detach().float().requires_grad_() if res else None
    wf = w.detach().clone().requires_grad_()
    xsf = xf + rf if res else xf
    yf = xsf * torch.rsqrt(xsf.pow(2).mean(dim=-1, keepdim=True) + EPS) * wf
    dy = torch.randn(M, C, device=DEV)
    loss, lossf = (y.float() * dy).sum(), (yf * dy).sum()
    if res:
        ds = torch.randn(M, C, device=DEV)
        loss = loss + (xs.float() * ds).sum()
        lossf = lossf + (xsf * ds).sum()
    loss.backward()
    lossf.backward()
    tol = 2e-2 if dt == BF else 2e-5
    errs = {"dx": _err(x.grad, xf.grad), "dgamma": _err(w.grad, wf.grad)}
    if res:
        errs["dres"] = _err(r.grad, rf.grad)
    print(f"rms_norm M,C={M},{C} {dt} res={res}: {errs}")
    assert x.grad.dtype == dt and w.grad.dtype == torch.float32
    assert all(e < tol for e in errs.values()), errs


def test_rms_norm_backward_is_deterministic():
    M, C = 4099, 768
    x = torch.randn(M, C, device=DEV, dtype=BF)
    w = torch.rand(C, device=DEV)
    dy = torch.randn(M, C, device=DEV, dtype=BF)
    dadd = torch.randn(M, C, device=DEV, dtype=BF)
    nat = _ext.native()
    y, xsum, rstd = nat.rms_forward(x, None, w, EPS)
    assert xsum is None and rstd.shape == (M,) and rstd.dtype == torch.float32
    outs = [nat.rms_backward(dy, x, w, rstd, dadd) for _ in range(3)]
    for o in outs[1:]:
        for a, c in zip(outs[0], o):
            assert torch.equal(a, c)
    assert torch.equal(nat.rms_forward(x, None, w, EPS)[0], y)


def test_rms_norm_dispatch(monkeypatch):
    """Widths the kernel does not take, fp64 and the forced reference: the formula in the input's dtype."""
    w = torch.rand(12, device=DEV) + 0.5
    x = torch.randn(5, 12, device=DEV)
    want = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w
    assert torch.allclose(rms_norm(x, w, EPS), want, atol=1e-6)
    x64 = torch.randn(5, 16, device=DEV, dtype=F64)
    assert rms_norm(x64, torch.ones(16, device=DEV), EPS).dtype == F64
    xb = torch.randn(5, 16, device=DEV).to(BF)
    nat_y = rms_norm(xb, torch.ones(16, device=DEV), EPS)
    monkeypatch.setenv("TBAMD_FORCE_REFERENCE", "1")
    ref_y = rms_norm(xb, torch.ones(16, device=DEV), EPS)
    assert ref_y.dtype == BF and _err(nat_y, ref_y) < 1e-2


# ---------------------------------------------------------------- swiglu
@pytest.fixture(scope="module")
def gate_data():
    """rows x 2F of randn * 3 and a dy, in fp64 on the device, shared and never modified."""
    g = torch.Generator(device=DEV).manual_seed(11)
    return (torch.randn(257, 2 * 2048, device=DEV, generator=g, dtype=F64) * 3,
            torch.randn(257, 2048, device=DEV, generator=g, dtype=F64))


def _gate_case(gate_data, rows, Fh, dt):
    gu64, dy64 = gate_data
    gu = torch.cat([gu64[:rows, :Fh], gu64[:rows, 2048:2048 + Fh]], dim=1).to(dt)
    return gu, dy64[:rows, :Fh].to(dt)


@pytest.mark.parametrize("Fh", [8, 24, 776, 2048])
@pytest.mark.parametrize("rows", [1, 3, 17, 257])
@pytest.mark.parametrize("dt", [BF, torch.float32])
def test_swiglu_matches_fp64(gate_data, rows, Fh, dt):
    gu, dy = _gate_case(gate_data, rows, Fh, dt)
    gu.requires_grad_()
    y = swiglu(gu)
    assert y.dtype == dt and y.shape == (rows, Fh)
    g, u, d = gu.detach().double()[:, :Fh], gu.detach().double()[:, Fh:], dy.double()
    s = torch.sigmoid(g)
    _within(y.detach(), g * s * u, 2.0 ** -8 * (g * s * u).abs() + 2.0 ** -30, "y")
    (dgu,) = torch.autograd.grad(y, gu, dy)
    assert dgu.dtype == dt and dgu.shape == gu.shape
    ref = torch.cat([d * u * s * (1 + g * (1 - s)), d * g * s], dim=1)
    slack = 2.0 ** -20 * d.abs() * (u.abs() * (1 + g.abs()) + g.abs())
    _within(dgu, ref, 2.0 ** -8 * ref.abs() + torch.cat([slack, slack], dim=1), "dgu")


def test_swiglu_views(gate_data):
    """A row-strided window of a wider tensor is read in place; a misaligned one is copied: same bits."""
    gu, dy = _gate_case(gate_data, 17, 24, BF)
    want = swiglu(gu)
    leaf = gu.clone().requires_grad_()
    (dwant,) = torch.autograd.grad(swiglu(leaf), leaf, dy)
    wide = torch.zeros(17, 48 + 16, device=DEV, dtype=BF)
    wide[:, 8:56] = gu
    view = wide[:, 8:56]
    assert not view.is_contiguous() and view.data_ptr() % 16 == 0
    off = torch.zeros(17, 48 + 3, device=DEV, dtype=BF)
    off[:, 3:] = gu
    odd = off[:, 3:]
    assert odd.data_ptr() % 16 != 0
    cube = gu.view(17, 1, 48).expand(17, 2, 48)  # a stride-0 dim: not viewable as rows
    for v in (view, odd):
        v = v.detach().requires_grad_()
        y = swiglu(v)
        assert torch.equal(y, want)
        (dv,) = torch.autograd.grad(y, v, dy)
        assert torch.equal(dv, dwant)
    assert torch.equal(swiglu(cube)[:, 1], want)
    # F no multiple of 8 and other dtypes: F.silu(a) * b
    small = gu[:, :12]
    assert torch.equal(swiglu(small), F.silu(small[:, :6]) * small[:, 6:])
    assert swiglu(gu.double()).dtype == F64


def test_swiglu_graph_replay_follows_gu(gate_data):
    gu1, _ = _gate_case(gate_data, 17, 776, BF)
    gu2 = gu1.flip(0).contiguous()
    want1, want2 = swiglu(gu1), swiglu(gu2)  # also the warm-up
    assert not torch.equal(want1, want2)
    buf = gu1.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = swiglu(buf)
    graph.replay()
    assert torch.equal(out, want1)
    buf.copy_(gu2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2)


# ---------------------------------------------------------------- linear_rows
# (M, K, F); the last three: one F for each further columns-per-wave setting of the SwiGLU launcher (2, 4, 8),
# none a multiple of a workgroup's share (4 waves x that many columns)
GLU_SHAPES = [(3, 8, 7), (16, 128, 1), (1, 776, 256), (16, 776, 7), (3, 3072, 256), (1, 4096, 256), (16, 4096, 7),
              (1, 768, 2048), (3, 8, 2055), (3, 8, 4099), (2, 8, 8201)]
EPILOGUES = [None, "gelu", "residual"]


def _inputs(M, K, Fh, seed=0):
    """The inputs of tests/test_gpu_rows.py with a [2F, K] weight and a [2F] bias; seeded on the CPU."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * K + Fh)
    mk = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF).to(DEV)  # noqa: E731
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(BF).to(DEV)
    w = mk(2 * Fh, K, scale=K ** -0.5)
    b = mk(2 * Fh, scale=0.5)
    res = mk(M, Fh)
    gamma = (1.0 + 0.2 * torch.randn(K, generator=g)).to(DEV)
    return x, w, b, res, gamma


def _rms32(h, gamma):
    return h * torch.rsqrt(h.pow(2).mean(dim=-1, keepdim=True) + EPS) * gamma


def _ref(x, w, b, gamma, epi, res):
    """fp32 math on the bf16 inputs."""
    h = x.float()
    if gamma is not None:
        h = _rms32(h, gamma)
    y = h @ w.float().t()
    if b is not None:
        y = y + b.float()
    if epi == "gelu":
        y = F.gelu(y)
    if epi == "swiglu":
        half = y.shape[-1] // 2
        y = F.silu(y[..., :half]) * y[..., half:]
    if epi == "residual":
        y = y + res.float()
    return y


def _unfused(x, w, b, gamma, epi, res):
    """The composition on the separate kernels: rms_norm, the GEMM engine's linear, the gate."""
    h = rms_norm(x.contiguous(), gamma, EPS) if gamma is not None else x
    if epi == "gelu":
        return linear_gelu(h, w, b)
    y = linear(h, w, b)
    if epi == "swiglu":
        return swiglu(y)
    return y + res if epi == "residual" else y


def _check(x, w, b, res, gamma, with_rms, epi, with_bias, tag):
    bias = b if with_bias else None
    r = res if epi == "residual" else None
    gm = gamma if with_rms else None
    got = linear_rows(x, w, bias, rms=(gamma, EPS) if with_rms else None,
                      act=epi if epi in ("gelu", "swiglu") else None, residual=r)
    want = _ref(x, w, bias, gm, epi, r)
    assert got.shape == want.shape and got.dtype == BF
    e = _err(got, want)
    with torch.no_grad():
        e_unfused = _err(_unfused(x, w, bias, gm, epi, r), want)
    print(f"{tag} rms={with_rms} epi={epi} bias={with_bias}: rows {e:.2e} unfused {e_unfused:.2e}")
    assert torch.isfinite(got).all(), tag
    assert e < 1e-2, (tag, e)
    if with_rms or epi == "swiglu":
        assert e <= 1.5 * e_unfused, (tag, e, e_unfused)
    return got


def test_glu_shapes_cover_every_launcher_setting():
    nat = _ext.native()
    assert sorted({nat.rows_swiglu_cols_per_wave(s[2]) for s in GLU_SHAPES}) == [1, 2, 4, 8]
    for _, _, Fh in GLU_SHAPES[-3:]:
        assert Fh % (4 * nat.rows_swiglu_cols_per_wave(Fh))


@pytest.mark.parametrize("M,K,Fh", GLU_SHAPES)
def test_rms_prologue_and_swiglu_epilogue(M, K, Fh):
    x, w, b, res, gamma = _inputs(M, K, Fh, seed=1)
    tag = f"M,K,F={M},{K},{Fh}"
    for with_bias in (False, True):
        _check(x, w, b, res, gamma, True, "swiglu", with_bias, tag)  # (every shape has M * F >= 16)
        _check(x, w, b, res, None, False, "swiglu", with_bias, tag)  # the gate alone, after a plain product
    # rms alone ahead of every existing epilogue.  Not for the three wide shapes at the end of the list: they
    # are there for the SwiGLU launcher's columns-per-wave settings, which a plain product does not have, and
    # its own settings and the prologue are covered by the shapes before them.
    if Fh <= 2048:
        wq, bq = w[:Fh], b[:Fh].contiguous()
        for epi, with_bias in itertools.product(EPILOGUES, (False, True)):
            _check(x, wq, bq, res, gamma, True, epi, with_bias, tag)


@pytest.mark.parametrize("K,Fh", [(776, 256), (3072, 7), (128, 2055)])
def test_row_invariant_and_deterministic(K, Fh):
    """Row m has the same bits computed alone, among 3 or among 16 rows."""
    x, w, b, res, gamma = _inputs(16, K, Fh, seed=4)
    for with_rms, with_bias in itertools.product((False, True), (False, True)):
        kw = dict(rms=(gamma, EPS) if with_rms else None, act="swiglu")
        bias = b if with_bias else None
        full = linear_rows(x, w, bias, **kw)
        assert torch.equal(full, linear_rows(x, w, bias, **kw))  # a repeated call
        for m in (0, 7, 15):
            assert torch.equal(linear_rows(x[m:m + 1], w, bias, **kw)[0], full[m]), (with_rms, with_bias, m)
        assert torch.equal(linear_rows(x[5:8], w, bias, **kw), full[5:8]), (with_rms, with_bias)
    # the rms prologue under the residual epilogue
    wq, bq = w[:Fh], b[:Fh].contiguous()
    full = linear_rows(x, wq, bq, rms=(gamma, EPS), residual=res)
    for m in (0, 15):
        assert torch.equal(linear_rows(x[m:m + 1], wq, bq, rms=(gamma, EPS), residual=res[m:m + 1])[0], full[m])


@pytest.mark.parametrize("M,K,Fh", [(3, 776, 7), (16, 128, 2055), (1, 8, 1)])
def test_every_output_element_is_written(M, K, Fh):
    x, w, b, res, gamma = _inputs(M, K, Fh, seed=5)
    out = torch.full((M, Fh), float("nan"), device=DEV, dtype=BF)
    y = _ext.native().rows_linear(x, w, b, gamma, None, EPS, 3, None, out, rms=True)
    assert y.data_ptr() == out.data_ptr()
    assert torch.isfinite(out).all()
    assert torch.equal(out, linear_rows(x, w, b, rms=(gamma, EPS), act="swiglu"))


def test_zero_row_under_rms_stays_finite():
    M, K, Fh = 3, 128, 256
    x, w, b, res, gamma = _inputs(M, K, Fh, seed=3)
    x[1] = 0
    got = _check(x, w, b, res, gamma, True, "swiglu", True, "zero row")
    want_row = F.silu(b.float()[:Fh]) * b.float()[Fh:]  # the normalised row is exactly zero
    assert _err(got[1], want_row) < 1e-2


def test_native_binding_checks():
    nat = _ext.native()
    x, w, b, res, gamma = _inputs(3, 128, 8, seed=6)
    with pytest.raises(RuntimeError):
        nat.rows_linear(x, w[:15], None, None, None, EPS, 3)  # an odd number of weight rows
    with pytest.raises(RuntimeError):
        nat.rows_linear(x, w, b, None, None, EPS, 3, res)  # no residual under swiglu
    with pytest.raises(RuntimeError):
        nat.rows_linear(x, w, b[:8].contiguous(), None, None, EPS, 3)  # the bias covers both halves
    with pytest.raises(RuntimeError):
        nat.rows_linear(x, w, b, gamma, gamma, EPS, 0, rms=True)  # rms takes gamma alone
    with pytest.raises(RuntimeError):
        nat.rows_linear(x, w, b, None, None, EPS, 0, rms=True)
    with pytest.raises(RuntimeError):
        nat.swiglu_fwd(torch.zeros(3, 24, device=DEV, dtype=BF))  # F % 8
    with pytest.raises(RuntimeError):
        nat.swiglu_fwd(torch.zeros(3, 32, device=DEV, dtype=torch.float16))


def test_unsupported_shapes_take_the_composition():
    """More than 16 rows and a K the kernel does not take: rms_norm -> F.linear -> swiglu, inside the bar."""
    for M, K in ((17, 776), (3, 12)):
        x, w, b, res, gamma = _inputs(M, K, 256, seed=7)
        got = linear_rows(x, w, b, rms=(gamma, EPS), act="swiglu")
        e = _err(got, _ref(x, w, b, gamma, "swiglu", None))
        assert got.dtype == BF and got.shape == (M, 256) and e < 1e-2, e
    with pytest.raises(ValueError):
        linear_rows(x, w, b, ln=(gamma, gamma, EPS), rms=(gamma, EPS))


def test_rows_graph_replay_follows_x():
    M, K, Fh = 3, 776, 256
    x, w, b, res, gamma = _inputs(M, K, Fh, seed=8)
    x2 = _inputs(M, K, Fh, seed=9)[0]
    kw = dict(rms=(gamma, EPS), act="swiglu")
    want1, want2 = linear_rows(x, w, b, **kw), linear_rows(x2, w, b, **kw)  # also the warm-up
    assert not torch.equal(want1, want2)
    buf = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = linear_rows(buf, w, b, **kw)
    graph.replay()
    assert torch.equal(out, want1)
    buf.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want2)


# ---------------------------------------------------------------- the model
LLAMA = dict(norm="rms", mlp="swiglu", bias=False, pos="rope")


def _llama_tiny():
    torch.manual_seed(0)
    base = gpt_tiny(**LLAMA).cuda()
    with torch.no_grad():
        for blk in base.blocks:
            blk.attn.qkv.weight.mul_(8)
            blk.mlp.fc1.weight.mul_(8)
    return base


@pytest.fixture(scope="module")
def numerics():
    """The Llama-style gpt_tiny (qkv and fc1 weights x 8): the bf16 model, the tokens, and the teacher-forced
    logits of the fp32 PyTorch path and of the native full forward -- computed once, never modified."""
    base = _llama_tiny()
    N, j = 70, 34
    tokens = torch.randint(0, 256, (2, N), device=DEV)
    lengths = _i32((70, 41))
    mnat = copy.deepcopy(base).to(BF)
    assert mnat.norm.weight.dtype == torch.float32
    with torch.no_grad():
        full = mnat(tokens, lengths)[:, j:N - 1].float()
        with pytest.MonkeyPatch.context() as mp:  # the stock run: every op on its PyTorch path
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            mref = copy.deepcopy(base)
            ref = mref(tokens, lengths)[:, j:N - 1].float()
            mp.setattr(vit, "swiglu", lambda gu: gu[..., :gu.shape[-1] // 2] * gu[..., gu.shape[-1] // 2:])
            flat = mref(tokens, lengths)[:, j:N - 1].float()
    keep = torch.arange(j, N - 1, device=DEV)[None, :] < lengths[:, None]
    e_full, moved = _err(full[keep], ref[keep]), _err(flat[keep], ref[keep])
    print(f"llama-style gpt_tiny logits vs fp32: full forward {e_full:.5f}; without the gate's SiLU {moved:.5f}")
    # the setup is sensitive to the gate; if this fails the test is wrong, not the kernel
    assert moved >= 20 * e_full, (moved, e_full)
    return mnat, tokens, lengths, ref, keep, e_full, j, N


@pytest.mark.parametrize("how", ["decode_step", "decode_step_fused", "extend5", "extend5_fused"])
def test_gpt_tiny_incremental_vs_reference(numerics, how):
    """Teacher-forced, ragged: prefill 34 tokens, feed tokens 34 .. 68 one at a time or through ``extend`` in
    chunks of 5, default and fused; the incremental error is at most 1.5x the full forward's."""
    mnat, tokens, lengths, ref, keep, e_full, j, N = numerics
    fused = how.endswith("fused")
    logits, cache = mnat.prefill(tokens[:, :j], lengths.clamp(max=j))
    assert cache.positions.tolist() == [j, j]
    if how.startswith("extend5"):
        inc = torch.cat([mnat.extend(tokens[:, t:t + 5], cache, fused=fused) for t in range(j, N - 1, 5)], dim=1).float()
    else:
        inc = torch.stack([mnat.decode_step(tokens[:, t], cache, fused=fused) for t in range(j, N - 1)], dim=1).float()
    assert cache.positions.tolist() == [N - 1, N - 1]
    e_inc = _err(inc[keep], ref[keep])
    print(f"llama-style gpt_tiny teacher-forced logits vs fp32, {how}: incremental {e_inc:.5f} full forward "
          f"{e_full:.5f} ({e_inc / e_full:.2f}x)")
    assert torch.isfinite(inc).all()
    assert e_inc <= 1.5 * e_full, (e_inc, e_full)


def test_generate_graph_equals_eager():
    model = _llama_tiny().to(BF)
    tokens = torch.randint(0, 256, (2, 9), device=DEV)
    a, a_len = model.generate(tokens, 24, graph=False)
    b, b_len = model.generate(tokens, 24, graph=True)
    assert torch.equal(a, b) and torch.equal(a_len, b_len) and a_len.tolist() == [24, 24]
    f, f_len = model.generate(tokens, 24, fused=True, graph=False)
    assert f.shape == (2, 24) and int(f.min()) >= 0 and int(f.max()) < 256 and f_len.tolist() == [24, 24]
    g, g_len = model.generate(tokens, 24, fused=True, graph=True)
    assert torch.equal(f, g) and torch.equal(f_len, g_len)


def test_training_step():
    """One training step at 2 x 32 tokens: every gradient finite and non-zero, the loss within the bf16 bar
    (1e-2 relative) of the fp32 PyTorch path, and block 0's qkv weight gradient within 1.5x of what the
    default blocks show (the bar of tests/test_gpu_rope.py; fc1's is printed: the two MLPs differ)."""
    tokens = torch.randint(0, 256, (2, 32), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    errs = {}
    for name, kw in (("llama", LLAMA), ("default", {"pos": "rope"})):
        torch.manual_seed(0)
        base = gpt_tiny(**kw).cuda()
        mnat = copy.deepcopy(base).to(BF)
        loss = mnat.loss(tokens)
        loss.backward()
        for pname, p in mnat.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, (name, pname)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("TBAMD_FORCE_REFERENCE", "1")
            mref = copy.deepcopy(base)
            loss_ref = mref.loss(tokens)
            loss_ref.backward()
        assert abs(loss.item() - loss_ref.item()) < 1e-2 * abs(loss_ref.item()), (name, loss.item(), loss_ref.item())
        errs[name] = (_err(mnat.blocks[0].attn.qkv.weight.grad, mref.blocks[0].attn.qkv.weight.grad),
                      _err(mnat.blocks[0].mlp.fc1.weight.grad, mref.blocks[0].mlp.fc1.weight.grad))
        if name == "llama":
            assert not any(n.endswith("bias") for n, _ in mnat.named_parameters())
            assert mnat.blocks[0].ln1.weight.grad.dtype == torch.float32
    print(f"block 0 (qkv, fc1) weight gradients vs fp32: {errs}")
    assert errs["llama"][0] <= 1.5 * errs["default"][0], errs
