"""``linear_rows(mx_scales=)`` on the GPU (csrc/rows_gemm_mx.hip) and ``TransformerLM.quantize_rows``.

The reference is fp64 math on the dequantised weight, the prologue rounded to bf16 as the kernel rounds it.
Bars: relative Frobenius error below 1e-2 (the bar of tests/test_gpu_llama_block.py for this kernel family)
and at most 1.5x the error of the bf16 ``linear_rows`` on ``mx_dequantize(..., bf16)``, which is the same
weight exactly, so the two differ in summation order only.  Both bars also hold for the last 8 columns alone
and for each row alone.  The weights are random codes under scales that vary by 2^+-6 from block to block.
"""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from torchbooster_amd.models.gpt import KVCache, gpt_tiny  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops.linear import linear_rows, mx_dequantize, mx_quantize  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
EPS = 1e-6
PROS = [None, "ln", "rms"]
EPIS = [None, "gelu", "residual", "swiglu"]


def _inputs(M, K, Q, pro, epi, bias, seed=0):
    """(x, codes, scales, bias, keywords of linear_rows); seeded on the CPU."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * K + Q)
    rows = 2 * Q if epi == "swiglu" else Q
    codes = torch.randint(0, 256, (rows, K // 2), generator=g, dtype=torch.uint8).to(DEV)
    # a code is about 2.5 in magnitude: weights of about K^-0.5, times 2^-6 .. 2^6 per block
    mid = 127 - 1 - round(0.5 * torch.log2(torch.tensor(float(K))).item())
    scales = (mid + torch.randint(-6, 7, (rows, K // 32), generator=g)).to(torch.uint8).to(DEV)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(BF).to(DEV)
    b = (torch.randn(rows, generator=g) * 0.5).to(BF).to(DEV) if bias else None
    gamma, beta = (1.0 + 0.2 * torch.randn(K, generator=g)).to(DEV), (0.1 * torch.randn(K, generator=g)).to(DEV)
    kw = {"ln": (gamma, beta, EPS)} if pro == "ln" else {"rms": (gamma, EPS)} if pro == "rms" else {}
    if epi in ("gelu", "swiglu"):
        kw["act"] = epi
    if epi == "residual":
        kw["residual"] = torch.randn(M, Q, generator=g).to(BF).to(DEV)
    return x, codes, scales, b, kw


def _ref(x, wd, b, kw):
    h = x.double()
    if "ln" in kw:
        h = F.layer_norm(h, h.shape[-1:], kw["ln"][0].double(), kw["ln"][1].double(), EPS).to(BF).double()
    if "rms" in kw:
        h = (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + EPS) * kw["rms"][0].double()).to(BF).double()
    y = h @ wd.t()
    if b is not None:
        y = y + b.double()
    if kw.get("act") == "gelu":
        y = F.gelu(y)
    if kw.get("act") == "swiglu":
        y = F.silu(y[:, :y.shape[1] // 2]) * y[:, y.shape[1] // 2:]
    if "residual" in kw:
        y = y + kw["residual"].double()
    return y


def _check(M, K, Q, pro, epi, bias):
    x, codes, scales, b, kw = _inputs(M, K, Q, pro, epi, bias)
    got = linear_rows(x, codes, b, mx_scales=scales, **kw)
    base = linear_rows(x, mx_dequantize(codes, scales, BF), b, **kw)
    ref = _ref(x, mx_dequantize(codes, scales, F64), b, kw)
    assert got.shape == (M, Q) and got.dtype == BF and torch.isfinite(got).all()
    views = [("all", lambda t: t.reshape(1, -1)), ("last 8 columns", lambda t: t[:, -8:].reshape(1, -1)),
             ("rows", lambda t: t)]
    for name, v in views:
        den = v(ref).norm(dim=1).clamp_min(1e-300)
        e = (v(got).double() - v(ref)).norm(dim=1) / den
        e0 = (v(base).double() - v(ref)).norm(dim=1) / den
        print(f"M,K,Q={M},{K},{Q} {pro} {epi} bias={bias} {name}: mx {e.max().item():.2e} bf16 {e0.max().item():.2e}")
        assert (e < 1e-2).all(), (name, e.max().item())
        assert (e <= 1.5 * e0).all(), (name, e.tolist(), e0.tolist())


# every (M, K, Q) of the list, the prologues, epilogues and the bias rotating through it
SHAPES = list(itertools.product([1, 3, 16], [32, 96, 768, 2080, 4096], [1, 7, 67, 2049]))
CASES = [(M, K, Q, PROS[i % 3], EPIS[i % 4], bool(i // 12 % 2)) for i, (M, K, Q) in enumerate(SHAPES)]
# the vocabulary head on one block; three shapes whose waves walk their columns 8, 4 and 16 times (a loop count;
# 1 or 2 in the list above)
CASES += [(3, 32, 50257, "ln", None, False), (2, 768, 50257, "rms", None, False), (8, 2080, 4100, None, "swiglu", True),
          (1, 2080, 16400, None, "swiglu", False)]


@pytest.mark.parametrize("M,K,Q,pro,epi,bias", CASES)
def test_native_against_f64(M, K, Q, pro, epi, bias):
    _check(M, K, Q, pro, epi, bias)


# every lanes-per-column setting (1 .. 64; 2080 and 4096: more than one block per lane) x every row layout
@pytest.mark.parametrize("M", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("K", [32, 64, 128, 256, 512, 1024, 2080, 4096])
def test_every_panel_and_row_layout(M, K):
    _check(M, K, 133, None, None, True)
    _check(M, K, 67, "rms", "swiglu", True)


def test_cases_reach_every_launcher_setting():
    nat = _ext.native()
    assert sorted({nat.rows_mx_block_lanes(K) for K in [32, 64, 128, 256, 512, 1024, 2080]}) == [1, 2, 4, 8, 16, 32, 64]
    walks = {nat.rows_mx_cols_per_wave(Q, K, epi == "swiglu") * nat.rows_mx_block_lanes(K)
             // (64 if epi == "swiglu" else 128) for _, K, Q, _, epi, _ in CASES}
    assert walks == {1, 2, 4, 8, 16}


def test_decode_is_exact():
    """A one-hot row reads column k of the dequantised weight, bit for bit: every code in both nibbles, the
    scale bytes 1, 127 and 254 (under 254 the magnitudes that stay finite, up to 1.5)."""
    Q, K = 16, 96
    codes = (torch.arange(Q * K // 2) % 256).to(torch.uint8).reshape(Q, K // 2)
    codes[0, 32:48] &= 0xBB
    scales = (100 + torch.arange(Q * 3) % 50).to(torch.uint8).reshape(Q, 3)
    scales[0] = torch.tensor([1, 127, 254], dtype=torch.uint8)
    assert {c & 15 for c in codes.flatten().tolist()} == {c >> 4 for c in codes.flatten().tolist()} == set(range(16))
    codes, scales = codes.to(DEV), scales.to(DEV)
    want = mx_dequantize(codes, scales, BF)
    assert torch.isfinite(want).all()
    eye = torch.eye(K, device=DEV, dtype=BF)
    for k in range(K):
        assert torch.equal(linear_rows(eye[k:k + 1], codes, mx_scales=scales)[0], want[:, k]), k


def test_scale_bytes_0_and_255():
    """Never produced by the quantiser, and read by one rule everywhere: a zero scale and +inf."""
    codes = torch.full((2, 32), 0x22, dtype=torch.uint8, device=DEV)  # every element 1.0
    scales = torch.tensor([[0, 128], [127, 255]], dtype=torch.uint8, device=DEV)
    x = torch.ones(1, 64, device=DEV, dtype=BF)
    want = x.double() @ mx_dequantize(codes, scales, F64).t()
    assert want.tolist() == [[64.0, float("inf")]]
    assert torch.equal(linear_rows(x, codes, mx_scales=scales).double(), want)


@pytest.mark.parametrize("K,Q,pro,epi", [(768, 67, None, None), (2080, 135, "rms", "swiglu")])
def test_row_invariant_and_deterministic(K, Q, pro, epi):
    x, codes, scales, b, kw = _inputs(16, K, Q, pro, epi, True, seed=4)
    full = linear_rows(x, codes, b, mx_scales=scales, **kw)
    assert torch.equal(full, linear_rows(x, codes, b, mx_scales=scales, **kw))
    for m in (0, 7, 15):
        assert torch.equal(linear_rows(x[m:m + 1], codes, b, mx_scales=scales, **kw)[0], full[m]), m
    assert torch.equal(linear_rows(x[5:8], codes, b, mx_scales=scales, **kw), full[5:8])


def test_graph_capture():
    x, codes, scales, b, kw = _inputs(3, 768, 67, "ln", "gelu", True, seed=5)
    x2 = _inputs(3, 768, 67, "ln", "gelu", True, seed=6)[0]
    want1, want2 = (linear_rows(t, codes, b, mx_scales=scales, **kw) for t in (x, x2))  # also the warm-up
    buf = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = linear_rows(buf, codes, b, mx_scales=scales, **kw)
    graph.replay()
    assert torch.equal(out, want1)
    for _ in range(2):
        buf.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want2)


@pytest.mark.parametrize("kw", [{}, {"pos": "rope", "norm": "rms", "mlp": "swiglu", "bias": False}])
def test_model_decodes_on_mx_weights(kw):
    torch.manual_seed(21)
    m = gpt_tiny(**kw).to(DEV).to(BF).eval()
    m.quantize_rows()
    assert m.mx_rows["head"][0].dtype == torch.uint8 and set(m.blocks[0].mx_rows) == {"qkv", "proj", "fc1", "fc2"}
    ref = copy.deepcopy(m)
    ref.quantize_rows(None)
    for lin in [ref.head] + [l for b in ref.blocks for l in (b.attn.qkv, b.attn.proj, b.mlp.fc1, b.mlp.fc2)]:
        lin.weight.data = mx_dequantize(*mx_quantize(lin.weight), BF)
    tokens = torch.randint(0, 256, (2, 4), device=DEV)

    def run(model):  # from an empty cache: prefill reads the bf16 parameters
        cache = KVCache(model, 2)
        ext = model.extend(tokens, cache, fused=True)
        return ext, model.decode_step(tokens[:, 0], cache, fused=True)

    for got, want in zip(run(m), run(ref)):
        e = ((got.double() - want.double()).norm() / want.double().norm()).item()
        print(f"{kw}: {tuple(got.shape)} mx against dequantised bf16 {e:.2e}")
        assert e < 1e-2, e
    a, la = m.generate(tokens, 6, fused=True, graph=True)
    c, lc = m.generate(tokens, 6, fused=True, graph=False)
    assert torch.equal(a, c) and torch.equal(la, lc)
