"""Masked instantiations of the attention kernels (csrc/attention.hip: causal, key_lengths, both)
against the fp32 reference ``attention_ref``, under both whole-head settings.

Bars are those of test_gpu_attention.py: relative Frobenius error < 1e-2 on o, < 2e-2 on each of
dq, dk, dv.  Shapes: a single key; a partial last wave (17, 197); exact tile / block boundaries
(64, 256) and one past them (65, 129, 257); the whole-head limit on both sides (256, 257); the
128-row kernels with several diagonals and five blocks (520); lengths that make whole tiles and
whole key blocks fall away.
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
from torchbooster_amd.ops.attention import _AttnFn, attention, attention_packed, attention_ref  # noqa: E402

DEV = "cuda"
SCALE = 1.0 / math.sqrt(64)


@pytest.fixture(params=[0, 5], ids=["rows128", "wholehead"])
def head_mask(request):
    nat = _ext.native()
    old = nat.attn_set_head_mask(request.param)
    try:
        yield request.param
    finally:
        nat.attn_set_head_mask(old)


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _lengths(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(B, H, N, causal, lengths):
    """Inputs, output gradient and the fp32 reference (o, dq, dk, dv) of one case: computed once,
    shared by the two whole-head settings, never modified."""
    g = torch.Generator(device=DEV).manual_seed(1000 * N + 10 * B + H)
    q, k, v, do = (torch.randn(B, H, N, 64, device=DEV, generator=g).mul(s).to(torch.bfloat16)
                   for s in (1.5, 1.5, 1.5, 1.0))
    qr, kr, vr = (t.float().requires_grad_() for t in (q, k, v))
    o = attention_ref(qr, kr, vr, SCALE, causal=causal, key_lengths=_lengths(lengths))
    o.backward(do.float())
    return q, k, v, do, (o.detach(), qr.grad, kr.grad, vr.grad)


def _check(B, H, N, causal, lengths):
    q, k, v, do, (o_ref, dq_ref, dk_ref, dv_ref) = _case(B, H, N, causal, lengths)
    q, k, v = (t.clone().requires_grad_() for t in (q, k, v))
    o = attention(q, k, v, causal=causal, key_lengths=_lengths(lengths))
    assert o.shape == (B, H, N, 64)
    o.backward(do)
    errs = [_err(o, o_ref), _err(q.grad, dq_ref), _err(k.grad, dk_ref), _err(v.grad, dv_ref)]
    if N == 1:
        # One key: p = 1 and dP = delta, so dq = scale (dP - delta) k and dk = scale (dP - delta) q are
        # EXACTLY zero in the reference and a relative error is undefined.  The error is taken against
        # the size of the two terms that cancel, scale |dP| |k| (resp. |q|), under the same bar.
        dp = (do.float() * v.detach().float()).sum(-1, keepdim=True).abs() * SCALE
        assert dq_ref.norm() == 0 and dk_ref.norm() == 0
        errs[1] = (q.grad.float().norm() / (dp * k.detach().float()).norm()).item()
        errs[2] = (k.grad.float().norm() / (dp * q.detach().float()).norm()).item()
    print(f"B,H,N={B},{H},{N} causal={causal} lengths={lengths}: o {errs[0]:.2e} dq {errs[1]:.2e} "
          f"dk {errs[2]:.2e} dv {errs[3]:.2e}")
    assert all(torch.isfinite(t).all() for t in (o, q.grad, k.grad, v.grad))
    assert errs[0] < 1e-2, errs
    assert max(errs[1:]) < 2e-2, errs
    if lengths is not None:  # keys at or past the length: exact zeros
        for b, n in enumerate(lengths):
            assert torch.count_nonzero(k.grad[b, :, n:]) == 0 and torch.count_nonzero(v.grad[b, :, n:]) == 0


@pytest.mark.parametrize("B,H,N", [(1, 1, 1), (1, 2, 17), (2, 2, 64), (1, 2, 65), (2, 3, 129), (2, 2, 197),
                                   (1, 2, 256), (1, 2, 257), (2, 2, 300), (1, 1, 520)])
def test_causal_fwd_bwd(head_mask, B, H, N):
    _check(B, H, N, True, None)


@pytest.mark.parametrize("N,lengths", [(130, (1, 64, 65, 130)), (256, (1, 64, 65, 256)), (300, (1, 64, 65, 300)),
                                       (520, (520, 1, 128, 129))])
def test_key_lengths_fwd_bwd(head_mask, N, lengths):
    _check(4, 2, N, False, lengths)


@pytest.mark.parametrize("N", [197, 300])
def test_causal_and_key_lengths_fwd_bwd(head_mask, N):
    _check(4, 2, N, True, (1, 64, 65, N))


def test_packed_both_masks(head_mask):
    torch.manual_seed(3)
    B, N, H = 2, 197, 4
    kl = _lengths((65, 197))
    qkv = torch.randn(B, N, 3 * H * 64, device=DEV).to(torch.bfloat16).requires_grad_()
    o = attention_packed(qkv, H, causal=True, key_lengths=kl)
    g = torch.randn_like(o)
    o.backward(g)
    ref_in = qkv.detach().float().requires_grad_()
    t = ref_in.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    orf = attention_ref(t[0], t[1], t[2], SCALE, causal=True, key_lengths=kl).transpose(1, 2).reshape(B, N, H * 64)
    orf.backward(g.float())
    assert _err(o, orf) < 1e-2
    assert _err(qkv.grad, ref_in.grad) < 2e-2
    for i, ref_i in enumerate(ref_in.grad.view(B, N, 3, H, 64).unbind(2)):  # dq, dk, dv inside the packed dqkv
        assert _err(qkv.grad.view(B, N, 3, H, 64)[:, :, i], ref_i) < 2e-2, i
    assert torch.count_nonzero(qkv.grad.view(B, N, 3, H, 64)[0, 65:, 1:]) == 0


@pytest.mark.parametrize("N,lengths", [(300, (1, 65, 300)), (197, (1, 65, 197))])
@pytest.mark.parametrize("causal", [False, True])
def test_every_gradient_element_written(head_mask, N, lengths, causal):
    """dq / dk / dv are torch.empty buffers in the autograd path: pre-filled with NaN here, nothing
    may be left of it, and the rows of dk / dv at or past the length are exactly 0."""
    nat = _ext.native()
    B, H = len(lengths), 2
    q, k, v, do, _ = _case(B, H, N, causal, lengths)
    kl = _lengths(lengths)
    o, lse = nat.attn_forward(q, k, v, SCALE, causal, kl)
    assert torch.isfinite(lse).all()
    dq, dk, dv = (torch.full_like(q, float("nan")) for _ in range(3))
    nat.attn_backward(q, k, v, o.permute(0, 2, 1, 3), do, lse, SCALE, dq, dk, dv, causal, kl)
    for t in (dq, dk, dv):
        assert not torch.isnan(t).any()
    for b, n in enumerate(lengths):
        assert torch.count_nonzero(dk[b, :, n:]) == 0 and torch.count_nonzero(dv[b, :, n:]) == 0
        assert torch.count_nonzero(dv[b, :, :n]) > 0
        if n > 1:  # (one visible key: p = 1 and dP = delta, so dS = 0)
            assert torch.count_nonzero(dk[b, :, :n]) > 0 and torch.count_nonzero(dq[b]) > 0


def test_masked_keys_do_not_reach_the_result(head_mask):
    """Finite junk in masked K / V rows leaves the outputs bit-identical (finite, not NaN: 0 * NaN in
    a diagonal tile's PV product is NaN by IEEE, and robustness to that is not claimed)."""
    N, cut = 300, 150
    q, k, v, _, _ = _case(2, 2, N, True, None)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, cut:] = torch.randn_like(k2[:, :, cut:]) * 3
    v2[:, :, cut:] = torch.randn_like(v2[:, :, cut:]) * 3
    with torch.no_grad():
        a = attention(q, k, v, causal=True)
        b = attention(q, k2, v2, causal=True)
        assert torch.equal(a[:, :, :cut], b[:, :, :cut])
        assert not torch.equal(a[:, :, cut:], b[:, :, cut:])
        kl = _lengths((cut, 70))
        k3, v3 = k.clone(), v.clone()
        k3[0, :, cut:], v3[0, :, cut:] = k2[0, :, cut:], v2[0, :, cut:]
        k3[1, :, 70:], v3[1, :, 70:] = 2.0, -2.0
        for causal in (False, True):
            assert torch.equal(attention(q, k, v, causal=causal, key_lengths=kl),
                               attention(q, k3, v3, causal=causal, key_lengths=kl))


def test_key_lengths_clamped_on_device(head_mask):
    """0 and N + 3 behave as 1 and N (the kernels clamp; a bad value never moves an address)."""
    N = 130
    q, k, v, _, _ = _case(2, 2, N, False, None)
    with torch.no_grad():
        for causal in (False, True):
            a = attention(q, k, v, causal=causal, key_lengths=_lengths((0, N + 3)))
            b = attention(q, k, v, causal=causal, key_lengths=_lengths((1, N)))
            assert torch.equal(a, b) and torch.isfinite(a).all()
        # one visible key: the output of every query is V[0]
        assert torch.equal(a[0], v[0, :, :1].expand_as(a[0]))


def test_dispatch(monkeypatch):
    """Masked calls run natively (never the stock SDPA path); unmasked calls are what they were: the
    dense kernels, bit for bit the outputs of the four-argument _AttnFn.apply."""

    def boom(*a, **k):
        raise AssertionError("fell back to the PyTorch reference")

    monkeypatch.setattr(A.F, "scaled_dot_product_attention", boom)
    kl = _lengths((5, 10))
    q = torch.randn(2, 1, 10, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    A.attention(q, q, q, causal=True).sum().backward()
    A.attention(q, q, q, key_lengths=kl).sum().backward()
    qkv = torch.randn(2, 10, 3 * 2 * 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    A.attention_packed(qkv, 2, causal=True, key_lengths=kl).sum().backward()
    for N in (197, 300):
        q, k, v, _, _ = _case(2, 2, N, False, None)
        with torch.no_grad():
            want = _AttnFn.apply(q, k, v, SCALE).permute(0, 2, 1, 3)
            assert torch.equal(attention(q, k, v), want)
            assert torch.equal(attention(q, k, v, causal=False, key_lengths=None), want)
            # a mask that hides nothing runs the masked kernels and computes the same softmax
            full = attention(q, k, v, key_lengths=_lengths((N, N)))
            assert _err(full, want) < 1e-2
    with pytest.raises(RuntimeError):
        _ext.native().attn_forward(q, k, v, SCALE, False, torch.ones(2, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        _ext.native().attn_forward(q, k, v, SCALE, False, torch.ones(3, dtype=torch.int32, device=DEV))


def test_graph_replay_follows_key_lengths():
    """The lengths are read on the device: a captured forward replays with the tensor's current values."""
    N = 300
    q, k, v, _, _ = _case(2, 2, N, True, None)
    kl = _lengths((300, 64))
    with torch.no_grad():
        attention(q, k, v, causal=True, key_lengths=kl)  # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = attention(q, k, v, causal=True, key_lengths=kl)
        graph.replay()
        first = out.clone()
        kl.copy_(_lengths((65, 200)))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(first, attention(q, k, v, causal=True, key_lengths=_lengths((300, 64))))
        assert torch.equal(out, attention(q, k, v, causal=True, key_lengths=_lengths((65, 200))))
        assert not torch.equal(out, first)


def test_gpt_tiny_native_vs_reference(monkeypatch):
    """gpt_tiny in bf16 on the native kernels against the same weights on the stock fp32 path, at the
    bar of the ViT check in test_gpu_trajectory.py: the error against fp32 of the first-step
    gradients (all parameters, one relative L2 error) is at most 1.5x that of stock bf16 autocast;
    the logits' errors are printed.  Causality (atol of the CPU test): changing tokens[:, j:] leaves
    logits[:, :j] unchanged."""
    import copy

    import torch.nn.functional as F

    from torchbooster_amd.models import gpt_tiny

    torch.manual_seed(0)
    B, N, j = 2, 70, 33
    base = gpt_tiny().cuda()
    tokens = torch.randint(0, 256, (B, N), device=DEV)
    target = torch.randint(0, 256, (B, N), device=DEV)
    lengths = _lengths((70, 41))

    def run(model, autocast=False):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            logits = model(tokens, lengths)
        F.cross_entropy(logits.float().flatten(0, 1), target.flatten()).backward()
        return logits.detach().float(), torch.cat([p.grad.float().reshape(-1) for p in model.parameters()])

    mnat = copy.deepcopy(base).to(torch.bfloat16)
    lnat, gnat = run(mnat)
    with monkeypatch.context() as mp:  # the stock runs: every op on its PyTorch path
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        l32, g32 = run(copy.deepcopy(base))
        lamp, gamp = run(copy.deepcopy(base), autocast=True)
    for name, nat, amp, ref in (("logits", lnat, lamp, l32), ("gradients", gnat, gamp, g32)):
        e_nat, e_amp = _err(nat, ref), _err(amp, ref)
        print(f"gpt_tiny {name} error vs fp32: native {e_nat:.5f} autocast {e_amp:.5f} ({e_nat / e_amp:.2f}x)")
        assert torch.isfinite(nat).all()
        if name == "gradients":
            assert e_nat <= 1.5 * e_amp, (name, e_nat, e_amp)
    other = tokens.clone()
    other[:, j:] = (other[:, j:] + 1 + torch.randint(0, 200, (B, N - j), device=DEV)) % 256
    with torch.no_grad():
        a, b = mnat(tokens).float(), mnat(other).float()
    assert torch.allclose(a[:, :j], b[:, :j], atol=1e-6)
    assert not torch.allclose(a[:, j:], b[:, j:], atol=1e-3)
