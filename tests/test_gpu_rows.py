"""The few-row product kernel of csrc/rows_gemm.hip through ops/linear.py ``linear_rows``.

Every case is measured against fp32 math on the bf16 inputs with the project's bar, relative Frobenius
error < 1e-2 (tests/test_gpu_gemm.py).  The LayerNorm-prologue cases have a second bar: at most 1.5x the
error of today's ``layer_norm -> linear`` composition on the same inputs (the factor of
test_gpt_tiny_incremental_vs_reference).

Shapes: M in {1, 3, 16} (one row, rows that fill no accumulator layout, the limit), K in {8, 128, 776 =
8 * 97 (no multiple of 64: the last chunk round of a wave is partly idle), 3072, 4096 (the limit: 128 KiB
of LDS at M = 16)}, Q in {1, 7, 256, 50257}: one, two and four columns per wave walk, column counts that
are no multiple of a wave's or a workgroup's share, and the vocabulary head.  Without the prologue the
inputs are exact and the only rounding is the store, so every shape is inside the bar whatever its size.
With the prologue the normalised row is rounded to bf16 (2^-9 per element) before the product, and an
output that cancels to nearly nothing can be off by more than 1 % of ITSELF while the product is right;
the relative Frobenius error is a property of the whole result, so the prologue shapes keep M * Q >= 16.
The inputs come from a seeded CPU generator: the same numbers on every machine.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops.linear import linear, linear_gelu, linear_rows  # noqa: E402
from torchbooster_amd.ops.norm import layer_norm  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
EPS = 1e-6
COMBOS = list(itertools.product([False, True], [None, "gelu", "residual"], [False, True]))  # ln, epilogue, bias

PLAIN_SHAPES = [(1, 8, 1), (3, 8, 7), (16, 8, 256), (1, 128, 7), (3, 776, 256), (16, 776, 7), (1, 3072, 256),
                (16, 3072, 1), (3, 4096, 7), (16, 4096, 256), (1, 128, 50257), (16, 128, 50257)]
LN_SHAPES = [(3, 8, 7), (16, 128, 1), (1, 776, 256), (16, 776, 7), (3, 3072, 256), (1, 4096, 256), (16, 4096, 7),
             (3, 128, 50257)]


def _err(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _inputs(M, K, Q, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * K + Q)
    mk = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(BF).to(DEV)  # noqa: E731
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(BF).to(DEV)
    w = mk(Q, K, scale=K ** -0.5)
    b = mk(Q, scale=0.5)
    res = mk(M, Q)
    gamma = (1.0 + 0.2 * torch.randn(K, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(K, generator=g)).to(DEV)
    return x, w, b, res, gamma, beta


def _ref(x, w, b, ln, epi, res):
    """fp32 math on the bf16 inputs."""
    h = x.float()
    if ln is not None:
        h = F.layer_norm(h, (h.shape[-1],), ln[0], ln[1], ln[2])
    y = h @ w.float().t()
    if b is not None:
        y = y + b.float()
    if epi == "gelu":
        y = F.gelu(y)
    if epi == "residual":
        y = y + res.float()
    return y


def _today(x, w, b, ln, epi, res):
    """Today's composition: the LayerNorm kernel, the GEMM engine's linear, the residual added in bf16."""
    h = layer_norm(x.contiguous(), ln[0], ln[1], ln[2])
    y = linear_gelu(h, w, b) if epi == "gelu" else linear(h, w, b)
    return y + res if epi == "residual" else y


def _check(x, w, b, res, gamma, beta, with_ln, epi, with_bias, tag):
    ln = (gamma, beta, EPS) if with_ln else None
    bias = b if with_bias else None
    r = res if epi == "residual" else None
    got = linear_rows(x, w, bias, ln=ln, act="gelu" if epi == "gelu" else None, residual=r)
    want = _ref(x, w, bias, ln, epi, r)
    assert got.shape == want.shape and got.dtype == BF
    e = _err(got, want)
    msg = f"{tag} ln={with_ln} epi={epi} bias={with_bias}: rows {e:.2e}"
    if with_ln:
        with torch.no_grad():
            e_today = _err(_today(x, w, bias, ln, epi, r), want)
        msg += f" today {e_today:.2e}"
    print(msg)
    assert torch.isfinite(got).all(), tag
    assert e < 1e-2, (tag, e)
    if with_ln:
        assert e <= 1.5 * e_today, (tag, e, e_today)
    return got


@pytest.mark.parametrize("M,K,Q", PLAIN_SHAPES)
def test_plain_shapes(M, K, Q):
    x, w, b, res, gamma, beta = _inputs(M, K, Q)
    for with_ln, epi, with_bias in COMBOS:
        if not with_ln:
            _check(x, w, b, res, gamma, beta, False, epi, with_bias, f"M,K,Q={M},{K},{Q}")


@pytest.mark.parametrize("M,K,Q", LN_SHAPES)
def test_layernorm_prologue_shapes(M, K, Q):
    x, w, b, res, gamma, beta = _inputs(M, K, Q, seed=1)
    for with_ln, epi, with_bias in COMBOS:
        if with_ln:
            _check(x, w, b, res, gamma, beta, True, epi, with_bias, f"M,K,Q={M},{K},{Q}")


@pytest.mark.parametrize("with_ln", [False, True])
def test_strided_rows(with_ln):
    """Rows of x addressed through a row stride: a column window of a wider tensor and ``h[:, 0]``."""
    M, K, Q = 5, 776, 256
    x, w, b, res, gamma, beta = _inputs(M, K, Q, seed=2)
    wide = torch.randn(M, K + 24, device=DEV).to(BF)
    wide[:, 8:8 + K] = x
    view = wide[:, 8:8 + K]
    assert not view.is_contiguous() and view.stride(0) == K + 24
    ln = (gamma, beta, EPS) if with_ln else None
    want = linear_rows(x, w, b, ln=ln)
    assert torch.equal(linear_rows(view, w, b, ln=ln), want)
    seq = torch.randn(M, 3, K, device=DEV).to(BF)
    seq[:, 0] = x
    assert torch.equal(linear_rows(seq[:, 0], w, b, ln=ln), want)
    assert torch.equal(linear_rows(seq[:, :1], w, b, ln=ln), want[:, None])  # leading dims are kept
    _check(view, w, b, res, gamma, beta, with_ln, "residual", True, "strided")


def test_constant_row_under_layernorm_stays_finite():
    M, K, Q = 3, 128, 256
    x, w, b, res, gamma, beta = _inputs(M, K, Q, seed=3)
    x[1] = 2.5  # zero variance
    got = _check(x, w, b, res, gamma, beta, True, None, True, "constant row")
    want_row = beta @ w.float().t() + b.float()  # the normalised row is exactly beta
    assert _err(got[1], want_row) < 1e-2


@pytest.mark.parametrize("K,Q", [(776, 256), (128, 50257), (3072, 7)])
def test_row_invariant_and_deterministic(K, Q):
    """Row m has the same bits computed alone, among 3 or among 16 rows, for every prologue / epilogue."""
    x, w, b, res, gamma, beta = _inputs(16, K, Q, seed=4)
    for with_ln, epi, with_bias in COMBOS:
        kw = dict(ln=(gamma, beta, EPS) if with_ln else None, act="gelu" if epi == "gelu" else None)
        bias = b if with_bias else None
        r16 = res if epi == "residual" else None
        full = linear_rows(x, w, bias, residual=r16, **kw)
        assert torch.equal(full, linear_rows(x, w, bias, residual=r16, **kw))  # a repeated call
        for m in (0, 7, 15):
            alone = linear_rows(x[m:m + 1], w, bias, residual=None if r16 is None else r16[m:m + 1], **kw)
            assert torch.equal(alone[0], full[m]), (with_ln, epi, with_bias, m)
        three = linear_rows(x[5:8], w, bias, residual=None if r16 is None else r16[5:8], **kw)
        assert torch.equal(three, full[5:8]), (with_ln, epi, with_bias)


@pytest.mark.parametrize("M,K,Q", [(3, 776, 7), (16, 128, 50257), (1, 8, 1)])
def test_every_output_element_is_written(M, K, Q):
    x, w, b, res, gamma, beta = _inputs(M, K, Q, seed=5)
    out = torch.full((M, Q), float("nan"), device=DEV, dtype=BF)
    y = _ext.native().rows_linear(x, w, b, gamma, beta, EPS, 0, None, out)
    assert y.data_ptr() == out.data_ptr()
    assert torch.isfinite(out).all()
    assert torch.equal(out, linear_rows(x, w, b, ln=(gamma, beta, EPS)))


@pytest.mark.parametrize("M,K", [(17, 776), (3, 4104), (3, 12)])
def test_unsupported_shapes_take_the_composition(M, K, monkeypatch):
    """More than 16 rows, K past the limit, K no multiple of 8: the PyTorch composition, inside the bar."""
    Q = 256
    x, w, b, res, gamma, beta = _inputs(M, K, Q, seed=6)
    called = []
    nat = _ext.native()
    monkeypatch.setattr("torchbooster_amd.ops.linear.native",
                        lambda: called.append(1) or nat)
    for with_ln, epi, with_bias in COMBOS:
        ln = (gamma, beta, EPS) if with_ln else None
        r = res if epi == "residual" else None
        got = linear_rows(x, w, b if with_bias else None, ln=ln, act="gelu" if epi == "gelu" else None, residual=r)
        e = _err(got, _ref(x, w, b if with_bias else None, ln, epi, r))
        print(f"fallback M,K={M},{K} ln={with_ln} epi={epi} bias={with_bias}: {e:.2e}")
        assert got.dtype == BF and got.shape == (M, Q) and e < 1e-2, e
    assert not called
    linear_rows(x[:1, :8].contiguous(), w[:, :8].contiguous(), b)
    assert called  # the same call with a shape the kernel takes does reach it


def test_other_dtypes_and_forced_reference(monkeypatch):
    M, K, Q = 3, 128, 7
    x, w, b, res, gamma, beta = _inputs(M, K, Q, seed=7)
    want = _ref(x, w, b, (gamma, beta, EPS), "gelu", None)
    got = linear_rows(x.float(), w.float(), b.float(), ln=(gamma, beta, EPS), act="gelu")
    assert got.dtype == torch.float32 and _err(got, want) < 1e-5
    monkeypatch.setenv("TBAMD_FORCE_REFERENCE", "1")
    got = linear_rows(x, w, b, ln=(gamma, beta, EPS), act="gelu")
    assert got.dtype == BF and _err(got, want) < 1e-2
    with pytest.raises(RuntimeError):
        linear_rows(x, w.clone().requires_grad_(), b)


def test_graph_replay_follows_x():
    M, K, Q = 3, 776, 256
    x, w, b, res, gamma, beta = _inputs(M, K, Q, seed=8)
    x2 = _inputs(M, K, Q, seed=9)[0]
    kw = dict(ln=(gamma, beta, EPS), residual=res)
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
