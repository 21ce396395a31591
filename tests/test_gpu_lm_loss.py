"""Fused LM-head cross entropy (ops.loss.linear_cross_entropy: the kEpiLse / kEpiDlogits epilogues
of csrc/gemm.hip and the merge of csrc/loss.hip) and TransformerLM.loss on the GPU.

The oracle is fp32 math on the bf16 inputs with autograd; the comparator is the unfused native
route ``ops.linear.linear`` -> ``ops.loss.cross_entropy``, which stores bf16 logits."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd import utils  # noqa: E402
from torchbooster_amd.models.gpt import TransformerLM, gpt_tiny  # noqa: E402
from torchbooster_amd.ops.linear import linear  # noqa: E402
from torchbooster_amd.ops.loss import cross_entropy, linear_cross_entropy  # noqa: E402
from torchbooster_amd.ops.optim import FusedAdamW  # noqa: E402

DEV = "cuda"
IGN = -100


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _labels(M, V, g):
    """Random labels with ~10 % ignored rows, one whole 128-row block of ignored rows (M >= 256), and
    0, V - 1 and the columns on both sides of every multiple of 64 (so of 128 and 256) below V."""
    y = torch.randint(0, V, (M,), device=DEV, generator=g)
    ignored = torch.rand(M, device=DEV, generator=g) < 0.1
    if M >= 256:
        ignored[128:256] = True
    if M == 1:
        ignored[:] = False
    special = [0, V - 1] + [c for b in range(64, V, 64) for c in (b - 1, b)]
    rows = (~ignored).nonzero().flatten().tolist()
    for r, c in zip(rows, special):
        y[r] = c
    y[ignored] = IGN
    return y


@functools.lru_cache(maxsize=None)
def _case(M, V, D, std=2.0):
    """bf16 inputs, labels, and the fp32 oracle / unfused-native results: computed once, never modified."""
    g = torch.Generator(device=DEV).manual_seed(1000 * M + V + D)
    x = torch.randn(M, D, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(V, D, device=DEV, generator=g) * (std / D ** 0.5)).to(torch.bfloat16)
    y = _labels(M, V, g)
    xf, wf = x.float().requires_grad_(), w.float().requires_grad_()
    lo = F.cross_entropy(F.linear(xf, wf), y, ignore_index=IGN)
    lo.backward()
    oracle = (lo.detach(), xf.grad, wf.grad)
    xu, wu = x.clone().requires_grad_(), w.clone().requires_grad_()
    lu = cross_entropy(linear(xu, wu), y, ignore_index=IGN)
    lu.backward()
    return x, w, y, oracle, (lu.detach().float(), xu.grad, wu.grad)


def _fused(x, w, y, chunk=None):
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    loss = linear_cross_entropy(xr, wr, y, IGN, chunk=chunk)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    return loss.detach(), xr.grad, wr.grad


def _check(M, V, D, chunk, std=2.0):
    x, w, y, (lo, dxo, dwo), (lu, dxu, dwu) = _case(M, V, D, std)
    lf, dxf, dwf = _fused(x, w, y, chunk)
    assert torch.isfinite(lf) and torch.isfinite(dxf).all() and torch.isfinite(dwf).all()
    e_f, e_u = abs(float(lf) - float(lo)), abs(float(lu) - float(lo))
    print(f"lm_loss M={M} V={V} D={D} chunk={chunk} std={std}: loss {float(lo):.6f} |fused-oracle| {e_f:.3e} "
          f"|unfused-oracle| {e_u:.3e}")
    errs = {}
    for name, f, u, o in (("dX", dxf, dxu, dxo), ("dW", dwf, dwu, dwo)):
        assert f.dtype == torch.bfloat16 and f.shape == o.shape
        errs[name] = (_err(f, o), _err(u, o))
        print(f"  {name}: fused {errs[name][0]:.5f} unfused {errs[name][1]:.5f} "
              f"({errs[name][0] / max(errs[name][1], 1e-12):.2f}x)")
    assert e_f <= max(e_u, 1e-4 * abs(float(lo))), (e_f, e_u)
    for name, (ef, eu) in errs.items():
        assert ef < 2e-2, (name, ef)
        assert ef <= 1.5 * eu, (name, ef, eu)
    assert not dxf[y == IGN].any()  # ignored rows: exactly zero


@pytest.mark.parametrize("M,V,D,chunk", [(1, 5, 64, None), (129, 255, 72, None), (257, 257, 64, None),
                                         (300, 1031, 256, 256), (300, 1031, 256, 512), (300, 1031, 256, None)])
def test_matches_fp32_oracle_no_worse_than_unfused(M, V, D, chunk):
    _check(M, V, D, chunk)


def test_large_logits():
    """Logits of standard deviation ~20: the per-tile maxima differ by far more than 88, so a merge
    without rescaling or an exp without the max overflows."""
    x, w, *_ = _case(300, 1031, 256, 20.0)
    s = F.linear(x.float(), w.float()).std().item()
    print(f"logit std {s:.2f}")
    assert 15.0 < s < 25.0
    _check(300, 1031, 256, 256, std=20.0)


def test_out_of_range_labels_are_ignored():
    x, w, y, *_ = _case(300, 1031, 256)
    rows = (y != IGN).nonzero().flatten()[:3]
    y_bad, y_ign = y.clone(), y.clone()
    y_bad[rows] = torch.tensor([1031, -1, 2 ** 40], device=DEV)
    y_ign[rows] = IGN
    for a, b in zip(_fused(x, w, y_bad, 512), _fused(x, w, y_ign, 512)):
        assert torch.equal(a, b)
    loss, dx, dw = _fused(x, w, torch.full_like(y, IGN), 512)
    assert torch.isnan(loss)
    assert not dx.any() and not dw.any()
    y_bad[:] = 1031
    loss, dx, dw = _fused(x, w, y_bad, 512)
    assert torch.isnan(loss)
    assert not dx.any() and not dw.any()


def test_deterministic():
    x, w, y, *_ = _case(300, 1031, 256)
    for a, b in zip(_fused(x, w, y, 256), _fused(x, w, y, 256)):
        assert torch.equal(a, b)


def test_leading_dims_and_no_input_gradient():
    x, w, y, *_ = _case(300, 1031, 256)
    ref = _fused(x, w, y, 512)
    xr, wr = x.view(3, 100, 256).clone().requires_grad_(), w.clone().requires_grad_()
    linear_cross_entropy(xr, wr, y.view(3, 100), IGN, chunk=512).backward()
    assert xr.grad.shape == xr.shape
    assert torch.equal(xr.grad.view(300, 256), ref[1]) and torch.equal(wr.grad, ref[2])
    wr = w.clone().requires_grad_()
    linear_cross_entropy(x, wr, y, IGN, chunk=512).backward()  # x needs no gradient
    assert torch.equal(wr.grad, ref[2])


def test_weight_gradient_lands_in_the_optimizer_slot():
    """After zero_grad(set_to_none=True) the chunks' weight-gradient GEMMs write the FusedAdamW grad
    store directly: same values as the accumulate path, no per-step copy."""
    x, w0, y, *_ = _case(300, 1031, 256)
    w = torch.nn.Parameter(w0.clone())
    opt = FusedAdamW([w], lr=0.0, weight_decay=0.0)
    linear_cross_entropy(x, w, y, IGN, chunk=256).backward()
    opt.step()  # builds the grad store (slots)
    opt.zero_grad(set_to_none=False)
    linear_cross_entropy(x, w, y, IGN, chunk=256).backward()
    ref = w.grad.clone()
    opt.zero_grad(set_to_none=True)
    linear_cross_entropy(x, w, y, IGN, chunk=256).backward()
    assert w.grad.data_ptr() == w._tb_slot.data_ptr()
    assert torch.equal(w.grad, ref)
    assert torch.equal(w.grad, _fused(x, w0, y, 256)[2])


def test_peak_memory_is_less_than_half_of_unfused():
    M, V, D = 2048, 16389, 128
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(M, D, device=DEV, generator=g).to(torch.bfloat16).requires_grad_()
    w = (torch.randn(V, D, device=DEV, generator=g) * 0.1).to(torch.bfloat16).requires_grad_()
    y = torch.randint(0, V, (M,), device=DEV, generator=g)

    def fused():
        linear_cross_entropy(x, w, y, IGN, chunk=2048).backward()

    def unfused():
        cross_entropy(linear(x, w), y, ignore_index=IGN).backward()

    peaks = {}
    for name, fn in (("fused", fused), ("unfused", unfused)):
        fn()  # warm-up: first-use tuning
        x.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        x.grad = w.grad = None
    print(f"peak above baseline: fused {peaks['fused'] / 2 ** 20:.1f} MiB, unfused {peaks['unfused'] / 2 ** 20:.1f} MiB "
          f"(logits + dlogits = {2 * M * V * 2 / 2 ** 20:.1f} MiB)")
    assert peaks["unfused"] >= 2 * M * V * 2
    assert peaks["fused"] < 0.5 * peaks["unfused"], peaks


def test_graph_capture_and_replay():
    """Forward + backward read no device value on the host: captured once, replayed on new inputs."""
    x0, w0, y0, *_ = _case(300, 1031, 256)
    x, w, y = x0.clone().requires_grad_(), w0.clone().requires_grad_(), y0.clone()

    def run():
        loss = linear_cross_entropy(x, w, y, IGN, chunk=512)
        return (loss,) + torch.autograd.grad(loss, (x, w))

    run()  # eager warm-up pays for first-use tuning
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    with torch.no_grad():
        x.copy_(x.flip(0) * 1.5)
        y.copy_(torch.where(y == IGN, y, (y * 7 + 3) % 1031).flip(0))
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    assert not torch.equal(out[0], _fused(x0, w0, y0, 512)[0])
    for a, b in zip(out, eager):
        assert torch.equal(a, b)


def test_gpt_tiny_loss_native_vs_reference(monkeypatch):
    """gpt_tiny in bf16 through the fused head against the same weights on the stock fp32 path: the
    error of the loss and of all parameter gradients (one relative L2 error) is at most 1.5x that
    of stock bf16 autocast."""
    torch.manual_seed(0)
    B, N = 2, 70
    base = gpt_tiny().cuda()
    tokens = torch.randint(0, 256, (B, N), device=DEV)
    lengths = torch.tensor([70, 41], dtype=torch.int32, device=DEV)

    def run(model, autocast=False):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            loss = model.loss(tokens, lengths)
        loss.backward()
        return loss.detach().float(), torch.cat([p.grad.float().reshape(-1) for p in model.parameters()])

    lnat, gnat = run(copy.deepcopy(base).to(torch.bfloat16))
    with monkeypatch.context() as mp:  # the stock runs: every op on its PyTorch path
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        l32, g32 = run(copy.deepcopy(base))
        lamp, gamp = run(copy.deepcopy(base), autocast=True)
    e_nat, e_amp = _err(gnat, g32), _err(gamp, g32)
    print(f"gpt_tiny loss fp32 {float(l32):.5f} native {float(lnat):.5f} autocast {float(lamp):.5f}; gradient error "
          f"vs fp32: native {e_nat:.5f} autocast {e_amp:.5f} ({e_nat / e_amp:.2f}x)")
    assert torch.isfinite(lnat) and torch.isfinite(gnat).all()
    assert abs(float(lnat) - float(l32)) <= 1.5 * max(abs(float(lamp) - float(l32)), 1e-4 * abs(float(l32)))
    assert e_nat <= 1.5 * e_amp, (e_nat, e_amp)


def test_training_steps_with_the_real_odd_vocabulary():
    """Five optimizer steps of a shallow GPT-2-vocabulary model stay finite, and a step allocates less
    than one padded bf16 weight copy plus one logits tensor would add on their own."""
    torch.manual_seed(0)
    V, D, B, N = 50257, 128, 2, 64
    model = TransformerLM(V, D, 1, 2, N).cuda().to(torch.bfloat16)
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    tokens = torch.randint(0, V, (B, N), device=DEV)
    peak = 0
    for it in range(5):
        if it >= 2:  # the first steps tune the GEMMs and build the optimizer state
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
        loss = model.loss(tokens)
        utils.step(loss, opt, clip=1.0)
        assert torch.isfinite(loss)
        if it >= 2:
            torch.cuda.synchronize()
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
    bound = (V + 7) // 8 * 8 * D * 2 + B * N * V * 2
    print(f"step peak above baseline {peak / 2 ** 20:.1f} MiB, bound {bound / 2 ** 20:.1f} MiB")
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert peak < bound, (peak, bound)
