"""QK-norm on the native kernels (csrc/qk_norm_rope.hip): ``qk_norm_rope_packed`` in bf16 with head dim 64, its
backward, and ``TransformerLM(qk_norm=True)`` on every path.  The oracle is fp64 PyTorch on the same bf16
inputs, f32 weights and f32 table; the bars are derived, not measured (``n`` the fp64 normalised vector):

* forward ``|got - ref| <= 2^-8 |ref| + 2^-18 (|n[i]| + |n[i + 32]|)``: the one bf16 rounding with a factor 2,
  plus the f32 sum of 64 squares, the rsqrt and the rotation's products (4x tests/test_gpu_rope.py's 2^-20);
* ``dqkv``: ``2^-8 |ref| + 2^-18 rstd (|gw| + |x^| mean|gw x^|)``, the size of what the last subtraction may cancel;
* the weight gradients, per column: ``(n + 8) 2^-24 sum|u x^|`` over the ``n`` (row, head) terms, f32 accumulation.

The model bars are those of tests/test_gpu_rope.py and tests/test_gpu_llama_block.py: errors relative to the same
weights on the fp32 PyTorch path, incremental paths at most 1.5x the full forward, the loss within 1e-2, and the
norm weights' gradients at most 1.5x the error of block 0's qkv weight gradient, which the same bf16 dqkv feeds."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.models import gpt_tiny  # noqa: E402
from torchbooster_amd.ops import attention as A  # noqa: E402
from torchbooster_amd.ops.attention import qk_norm_rope_packed, rope_table  # noqa: E402

DEV, BF, EPS = "cuda", torch.bfloat16, 1e-6
B, H, D, MAXLEN = 2, 4, 64, 64


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


def _err(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def table():
    return rope_table(MAXLEN, D, device=DEV)


def _no_fallback(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch path")

    monkeypatch.setattr(A, "_qk_norm_rope_ref", boom)


def _data(hkv, T):
    g = torch.Generator(device=DEV).manual_seed(100 * hkv + T)
    x, dy = (torch.randn(B, T, (H + 2 * hkv) * D, device=DEV, generator=g).mul(1.5).to(BF) for _ in range(2))
    qw, kw = (1 + 0.5 * torch.randn(D, device=DEV, generator=g) for _ in range(2))
    return x, dy, qw, kw


def _cs(T, table, positions):
    """cosines and sines [B, T, 1, 32] in fp64 at the clamped positions (host ints); 1 and 0 without a table"""
    if table is None:
        return torch.ones(B, T, 1, 32, device=DEV, dtype=torch.float64), torch.zeros(B, T, 1, 32, device=DEV).double()
    p = torch.tensor([[min(max((0 if positions is None else positions[b]) + t, 0), MAXLEN - 1) for t in range(T)]
                      for b in range(B)], device=DEV)
    cs = table.double()[p]
    return cs[:, :, None, 0], cs[:, :, None, 1]


def _oracle(x, hkv, qw, kw, c, s):
    """fp64 -> (y [B, T, hr, 64], n, rstd, x^, w [hr, 64]) of the normalised heads"""
    hr = H + hkv
    xx = x.double()[..., :hr * D].reshape(B, -1, hr, D)
    w = torch.cat((qw.double().expand(H, D), kw.double().expand(hkv, D)))
    rstd = (xx.square().mean(-1, keepdim=True) + EPS).rsqrt()
    n = xx * rstd * w
    lo, hi = n[..., :32], n[..., 32:]
    return torch.cat((lo * c - hi * s, hi * c + lo * s), dim=-1), n, rstd, xx * rstd, w


def _within(got, ref, slack):
    excess = (got.double() - ref).abs() - (2.0 ** -8 * ref.abs() + 2.0 ** -18 * slack)
    assert torch.isfinite(got).all() and excess.max() <= 0, excess.max()


@pytest.mark.parametrize("hkv", [4, 2, 1])
@pytest.mark.parametrize("T", [1, 5, 17])
@pytest.mark.parametrize("positions", [None, (0, 37), (-3, MAXLEN + 5)], ids=["none", "0-37", "clamped"])
@pytest.mark.parametrize("rotate", [True, False], ids=["table", "notable"])
def test_forward_matches_fp64(monkeypatch, table, hkv, T, positions, rotate):
    _no_fallback(monkeypatch)
    x, _, qw, kw = _data(hkv, T)
    tab, pos, v0 = table if rotate else None, _i32(positions), (H + hkv) * D
    keep = x.clone()
    got = qk_norm_rope_packed(x, H, qw, kw, EPS, tab, pos, kv_heads=hkv)
    ref, n, *_ = _oracle(x, hkv, qw, kw, *_cs(T, tab, positions))
    assert got.shape == x.shape and got.dtype == BF and torch.equal(x, keep)
    _within(got[..., :v0], ref.reshape(B, T, v0), (n[..., :32].abs() + n[..., 32:].abs()).repeat(1, 1, 1, 2).reshape(B, T, v0))
    assert torch.equal(got[..., v0:].view(torch.int16), x[..., v0:].view(torch.int16))  # the value part, bit for bit
    y = x.clone()
    y.view(torch.int16)[..., v0:] = 0x7FC5  # in place: the same bits, the value part's memory not written
    assert qk_norm_rope_packed(y, H, qw, kw, EPS, tab, pos, kv_heads=hkv, inplace=True).data_ptr() == y.data_ptr()
    assert torch.equal(y[..., :v0], got[..., :v0]) and bool((y.view(torch.int16)[..., v0:] == 0x7FC5).all())


@pytest.mark.parametrize("hkv,T,rotate", [(hkv, T, True) for hkv in (4, 2, 1) for T in (1, 5, 17)] + [(2, 5, False)])
def test_backward_matches_fp64_autograd(monkeypatch, table, hkv, T, rotate):
    _no_fallback(monkeypatch)
    x, dy, qw, kw = _data(hkv, T)
    tab, positions, v0 = (table, (0, 37), (H + hkv) * D) if rotate else (None, None, (H + hkv) * D)
    c, s = _cs(T, tab, positions)

    def grads():
        leaves = [t.clone().requires_grad_() for t in (x, qw, kw)]
        return torch.autograd.grad(qk_norm_rope_packed(*leaves[:1], H, *leaves[1:], EPS, tab, _i32(positions), kv_heads=hkv),
                                   leaves, dy)

    got = grads()
    assert all(torch.equal(a, b) for a, b in zip(got, grads()))  # bit-deterministic
    leaves = [t.double().requires_grad_() for t in (x, qw, kw)]
    y, _, rstd, xh, w = _oracle(*leaves[:1], hkv, *leaves[1:], c, s)
    g = dy.double()[..., :v0].reshape(B, T, H + hkv, D)
    ref = torch.autograd.grad(y, leaves, g)
    u = torch.cat((g[..., :32] * c + g[..., 32:] * s, g[..., 32:] * c - g[..., :32] * s), dim=-1)  # the inverse rotation
    rstd, xh, w, gw = rstd.detach(), xh.detach(), w.detach(), u * w.detach()
    slack = rstd * (gw.abs() + xh.abs() * (gw * xh).abs().mean(-1, keepdim=True))
    assert got[0].dtype == BF and got[1].dtype == got[2].dtype == torch.float32
    _within(got[0][..., :v0], ref[0][..., :v0], slack.reshape(B, T, v0))
    assert torch.equal(got[0][..., v0:].view(torch.int16), dy[..., v0:].view(torch.int16))
    for dw, rw, heads in ((got[1], ref[1], slice(0, H)), (got[2], ref[2], slice(H, H + hkv))):
        terms = (u * xh)[:, :, heads].abs()
        bound = (terms[..., 0].numel() + 8) * 2.0 ** -24 * terms.sum(dim=(0, 1, 2))
        assert ((dw.double() - rw).abs() <= bound).all(), ((dw.double() - rw).abs() / bound).max()


def _tiny(pos):
    torch.manual_seed(0)
    base = gpt_tiny(pos=pos, norm="rms", mlp="swiglu", bias=False, kv_heads=1, qk_norm=True).cuda()
    with torch.no_grad():
        for blk in base.blocks:
            blk.attn.qkv.weight.mul_(8)  # positions matter to the logits (tests/test_gpu_rope.py)
            blk.attn.q_norm.weight.copy_(1 + 0.5 * torch.randn(64, device=DEV))
            blk.attn.k_norm.weight.copy_(1 + 0.5 * torch.randn(64, device=DEV))
    return base


@functools.lru_cache(maxsize=None)
def _numerics(pos):
    """The bf16 model, the fp32 model after one backward on the PyTorch path, the tokens, the fp32 teacher-forced
    logits and the native full forward's error against them -- computed once per ``pos``."""
    base, N, j = _tiny(pos), 70, 33
    tokens = torch.randint(0, 256, (2, N), device=DEV)
    mnat = copy.deepcopy(base).to(BF)
    with pytest.MonkeyPatch.context() as mp:  # every op on its PyTorch path
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        mref = copy.deepcopy(base)
        mref.loss(tokens).backward()
        with torch.no_grad():
            ref = mref(tokens)[:, j:N - 1].float()
    with torch.no_grad():
        e_full = _err(mnat(tokens)[:, j:N - 1], ref)
    return mnat, mref, tokens, ref, e_full, j, N


def test_training_step():
    mnat, mref, tokens, *_ = _numerics("rope")
    mnat = copy.deepcopy(mnat)
    loss = mnat.loss(tokens)
    loss.backward()
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        loss_ref = mref.loss(tokens).item()
    a, r = mnat.blocks[0].attn, mref.blocks[0].attn
    errs = [_err(getattr(a, n).weight.grad, getattr(r, n).weight.grad) for n in ("qkv", "q_norm", "k_norm")]
    print(f"loss {loss.item():.5f} vs {loss_ref:.5f}; block 0 (qkv, q_norm, k_norm) weight gradients vs fp32: {errs}")
    assert abs(loss.item() - loss_ref) < 1e-2 * abs(loss_ref)
    assert a.q_norm.weight.grad.dtype == torch.float32 and max(errs[1:]) <= 1.5 * errs[0], errs


@pytest.mark.parametrize("pos,how", [("rope", "decode_step"), ("rope", "fused"), ("rope", "extend4"),
                                     ("learned", "decode_step")])
def test_incremental_vs_full_forward(pos, how):
    """Prefill 33 tokens, then feed 33 .. 68 one at a time (default and ``fused=True``) or through ``extend`` in
    chunks of 4: at most 1.5x the full forward's error against the fp32 logits.  The fused layer step has the
    bits of the unfused one (the other kernels of a fused model step differ, so its logits are held to the bar)."""
    mnat, _, tokens, ref, e_full, j, N = _numerics(pos)
    with torch.no_grad():
        _, cache = mnat.prefill(tokens[:, :j])
        if how == "extend4":
            inc = torch.cat([mnat.extend(tokens[:, t:t + 4], cache) for t in range(j, N - 1, 4)], dim=1)
        else:
            inc = torch.stack([mnat.decode_step(tokens[:, t], cache, fused=how == "fused") for t in range(j, N - 1)], 1)
        if how == "fused":
            attn, (k, v) = mnat.blocks[0].attn, cache.layers[0]
            qkv = torch.randn(2, 1, 4 * 64, device=DEV).to(BF)
            k2, v2, at = k.clone(), v.clone(), cache.positions - 1
            assert torch.equal(attn.cached(qkv.clone(), (k, v), at, fused=True), attn.cached(qkv.clone(), (k2, v2), at))
            assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in ((k, k2), (v, v2)))
    e_inc = _err(inc, ref)
    print(f"qk_norm, pos={pos}: logits vs fp32, {how}: incremental {e_inc:.5f} full forward {e_full:.5f}")
    assert torch.isfinite(inc).all() and e_inc <= 1.5 * e_full, (e_inc, e_full)


def test_generate_graph_equals_eager():
    model = _numerics("rope")[0]
    tokens = torch.randint(0, 256, (2, 9), device=DEV)
    a, a_len = model.generate(tokens, 24, graph=False)
    b, b_len = model.generate(tokens, 24, graph=True)
    assert torch.equal(a, b) and torch.equal(a_len, b_len) and a.shape == (2, 24)
