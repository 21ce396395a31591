"""The grouped GEMM (csrc/gemm_grouped.hip, ``ops.gemm.grouped_linear``) and ``models.vit.MoE`` on the GPU.

Kernels: every element against the per-expert float64 product of the bf16 inputs, within the allowance the dense
sweep uses (tests/_gemm_ref.py; reduction length ``K``, or the expert's row count for the weight gradient), at
``E = 4``, ``K = 72`` (one k-tile plus an 8-wide tail), ``Q = 136`` (a partial column tile), ``R = 304``.

Layer: ``MoE(64, 96, experts=4, top_k=2)`` in bf16 against a float64 composition; the bar is 1.5x the error of
the PyTorch bf16 path (``TBAMD_FORCE_REFERENCE=1``) against the same float64 (measured: profiles/moe/README.md)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import _gemm_ref as G  # noqa: E402
from torchbooster_amd.models.vit import MoE  # noqa: E402
from torchbooster_amd.ops._ext import native  # noqa: E402
from torchbooster_amd.ops.gemm import group_bounds, grouped_linear  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
E, K, Q, R = 4, 72, 136, 304
OFFSETS = {"mixed": [0, 0, 1, 130, 300], "one": [0, 300, 300, 300, 300], "empty": [0, 0, 0, 0, 0]}
BAD = [[0, 200, 100, 400, 250], [0, -5, 310, 120, 1 << 30]]


@functools.lru_cache(None)
def _data():
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(R, K, generator=g), torch.randn(R, Q, generator=g)
    w = torch.randn(E, Q, K, generator=g) / K ** 0.5
    return tuple(t.to(DEV, BF) for t in (x, dy, w))


def _off(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _run(kind, off):
    x, dy, w = _data()
    C = native()
    if kind == "grouped_nt":
        return C.grouped_rows(x, w, off, False)
    if kind == "grouped_nn":
        return C.grouped_rows(dy, w, off, True)
    return C.grouped_tn(dy, x, off)


@pytest.mark.parametrize("case", list(OFFSETS))
@pytest.mark.parametrize("kind", ["grouped_nt", "grouped_nn", "grouped_tn"])
def test_kernels_vs_float64(kind, case):
    x, dy, w = _data()
    b = group_bounds(_off(OFFSETS[case]), R).tolist()
    got = _run(kind, _off(OFFSETS[case]))
    worst = 0.0
    for e in range(E):
        rows = slice(b[e], b[e + 1])
        if kind == "grouped_nt":
            ref, g = G.gemm_ref(x[rows], w[e]), got[rows]
        elif kind == "grouped_nn":
            ref, g = G.gemm_ref(dy[rows], w[e], tw=True), got[rows]
        else:  # the reduction runs over the expert's rows
            ref, g = G.gemm_ref(dy[rows], x[rows], tx=True, tw=True), got[e]
        if g.numel():
            worst = max(worst, G.err_ratio(g, ref.y, G.allowance(ref.y, ref.A, ref.K)).max().item())
        if case == "empty" or (kind == "grouped_tn" and b[e] == b[e + 1]):
            assert not g.any()  # exact zeros
    print(f"{kind} {case}: largest err / allowance {worst:.3f}")
    assert worst <= 1.0
    if kind != "grouped_tn":
        assert got[b[E]:].shape[0] == R - b[E] and not got[b[E]:].any()  # rows of no expert


@pytest.mark.parametrize("bad", BAD)
def test_bad_offsets_are_clamped(bad):
    clamped = group_bounds(_off(bad), R).to(torch.int32)
    for kind in ("grouped_nt", "grouped_nn", "grouped_tn"):
        assert torch.equal(_run(kind, _off(bad)).view(torch.int16), _run(kind, clamped).view(torch.int16)), kind


def _fwd_bwd(w, off):
    x, dy, _ = _data()
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = grouped_linear(xg, wg, off)
    return (y,) + torch.autograd.grad(y, (xg, wg), dy)


def test_determinism():
    w, off = _data()[2], _off(OFFSETS["mixed"])
    first = _fwd_bwd(w, off)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(first, _fwd_bwd(w, off)))
    # the same row ranges owned by other experts: [0, 1) by 0, [1, 130) by 1, [130, 300) by 3
    y = grouped_linear(_data()[0], w[[1, 2, 0, 3]].contiguous(), _off([0, 1, 130, 130, 300]))
    assert torch.equal(y.view(torch.int16), first[0].view(torch.int16))


# ---------------------------------------------------------------- the layer
def _layer_inputs(seed):
    """Tokens whose router logits are a shuffled (2, 1, 0, -1) +- 0.2: the 2nd and 3rd largest are >= 0.6 apart, so
    no rounding flips an expert.  The router reads the first four features (unit rows)."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(48, 64, generator=g)
    levels = torch.tensor([2.0, 1.0, 0.0, -1.0])
    h[:, :4] = torch.stack([levels[torch.randperm(4, generator=g)] for _ in range(48)]) + 0.4 * torch.rand(48, 4, generator=g) - 0.2
    return h.view(2, 24, 64).to(DEV, BF)


def _layer():
    torch.manual_seed(11)
    moe = MoE(64, 96, experts=4, top_k=2)
    with torch.no_grad():
        moe.router.weight.copy_(torch.eye(4, 64))
    return moe.to(DEV, BF)


def _layer_ref(moe, x, dy):
    """float64, written plainly: a loop over the experts with dense masks."""
    h = x.double().view(-1, 64).requires_grad_()
    rw, fc1, fc2 = (p.detach().double().requires_grad_() for p in (moe.router.weight, moe.fc1, moe.fc2))
    logits = h @ rw.t()
    top = logits.sort(-1, descending=True).values
    assert (top[:, 1] - top[:, 2]).min() >= 0.5
    val, idx = logits.topk(2, dim=-1)
    gate = torch.softmax(val, -1)
    y = torch.zeros_like(h)
    for e in range(4):
        gu = h @ fc1[e].t()
        out = (F.silu(gu[:, :96]) * gu[:, 96:]) @ fc2[e].t()
        y = y + (gate * (idx == e)).sum(-1, keepdim=True) * out
    return (y,) + torch.autograd.grad(y, (h, rw, fc1, fc2), dy.double().view(-1, 64))


def _layer_errs(moe, x, dy, ref):
    xg = x.clone().requires_grad_()
    y = moe(xg)
    got = (y,) + torch.autograd.grad(y, (xg, moe.router.weight, moe.fc1, moe.fc2), dy)
    return [((g.double().reshape(r.shape) - r).abs().max() / r.abs().max()).item() for g, r in zip(got, ref)]


def test_layer_vs_float64():
    moe, x = _layer(), _layer_inputs(1)
    dy = torch.randn(2, 24, 64, device=DEV).to(BF)
    ref = _layer_ref(moe, x, dy)
    with pytest.MonkeyPatch.context() as mp:  # the PyTorch bf16 path sets the bar
        mp.setenv("TBAMD_FORCE_REFERENCE", "1")
        bar = _layer_errs(moe, x, dy, ref)
    errs = _layer_errs(moe, x, dy, ref)
    print("(y, dx, d router, d fc1, d fc2) vs float64: native", errs, "PyTorch bf16 path", bar)
    assert all(e <= 1.5 * b for e, b in zip(errs, bar)), (errs, bar)


def test_layer_under_graph_capture():
    moe, x = _layer(), _layer_inputs(1).clone()
    with torch.no_grad():
        moe(x)  # first-use work happens outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = moe(x)
        x.copy_(_layer_inputs(2))  # other tokens, other routes
        for _ in range(2):
            g.replay()
            assert torch.equal(y.view(torch.int16), moe(x).view(torch.int16))
