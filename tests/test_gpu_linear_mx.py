"""``ops.linear.linear_mx`` on the GPU (csrc/gemm_mx.hip), ``linear_rows(mx_scales=)`` past 16 rows and
``TransformerLM.prefill(mx=True)``.

Inputs, reference and bars are those of tests/test_gpu_rows_mx.py: random codes under scales that vary by 2^+-6 from
block to block, the fp64 product on ``mx_dequantize(..., float64)``, relative Frobenius error below 1e-2 and at most
1.5x the error of the bf16 engine (``ops.linear.linear``) on ``mx_dequantize(..., bf16)`` -- the same operands and
accumulator type, so the margin covers summation order only -- over all of the result, its last 8 columns and each row.
"""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from tests.test_gpu_rows_mx import _inputs, _ref  # noqa: E402
from torchbooster_amd.models.gpt import gpt_tiny  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops.linear import linear, linear_mx, linear_rows, mx_dequantize, mx_quantize  # noqa: E402

DEV, BF, F64 = "cuda", torch.bfloat16, torch.float64
EPIS = [None, "gelu", "residual"]


def _bar(got, base, ref, what):
    assert got.shape == ref.shape and got.dtype == BF and torch.isfinite(got).all()
    for name, v in [("all", lambda t: t.reshape(1, -1)), ("last 8 columns", lambda t: t[:, -8:].reshape(1, -1)),
                    ("rows", lambda t: t)]:
        den = v(ref).norm(dim=1).clamp_min(1e-300)
        e = (v(got).double() - v(ref)).norm(dim=1) / den
        e0 = (v(base).double() - v(ref)).norm(dim=1) / den
        print(f"{what} {name}: mx {e.max().item():.2e} bf16 {e0.max().item():.2e}")
        assert (e < 1e-2).all(), (name, e.max().item())
        assert (e <= 1.5 * e0).all(), (name, e.tolist(), e0.tolist())


def _check(P, K, Q, epi, bias, strided=False):
    x, codes, scales, b, kw = _inputs(P, K, Q, None, epi, bias)
    if strided:  # every second row of a wider buffer
        x = torch.cat([x, x], 1).repeat_interleave(2, 0)[::2, :K]
        assert not x.is_contiguous()
    got = linear_mx(x, codes, scales, b, **kw)
    base = linear(x, mx_dequantize(codes, scales, BF), b)
    base = F.gelu(base) if epi == "gelu" else base + kw["residual"] if epi == "residual" else base
    _bar(got, base, _ref(x, mx_dequantize(codes, scales, F64), b, kw), f"P,K,Q={P},{K},{Q} {epi} bias={bias}")


# row tails of both tiles, a k below one k-tile and one that is no multiple of it, a single column, columns that cut an
# MFMA group and a tile; the epilogues and the bias rotate through the list.  GELU rotates over Q >= 67 only: with 1 or
# 7 columns a row of the per-row view can consist of far negative pre-activations alone, where an f32 erf GELU
# (gelu_f, and ATen's in the baseline) has no relative accuracy at all -- both sides then show an error of 1.0.
SHAPES = list(itertools.product([17, 64, 65, 257], [32, 96, 128, 160, 2080], [1, 7, 67, 133, 260]))
CASES = [(P, K, Q, EPIS[(i // 5 + i % 5) % 3] if Q >= 67 else EPIS[i // 5 % 2 * 2], bool(i % 2))
         for i, (P, K, Q) in enumerate(SHAPES)] + [(17, 32, 50257, None, True)]


@pytest.mark.parametrize("P,K,Q,epi,bias", CASES)
def test_native_against_f64(P, K, Q, epi, bias):
    _check(P, K, Q, epi, bias)


def test_strided_rows():
    _check(65, 160, 133, "residual", True, strided=True)


def test_decode_is_exact():
    """One-hot rows read columns of the dequantised weight, bit for bit: every code in both nibbles, the scale bytes
    1, 127 and 254 (under 254 the magnitudes that stay finite, up to 1.5)."""
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
    for k in range(0, K, 32):
        assert torch.equal(linear_mx(eye[k:k + 32], codes, scales), want[:, k:k + 32].t()), k


def test_scale_bytes_0_and_255():
    """Never produced by the quantiser: byte 0 makes its block exact zeros, byte 255 makes its own output column
    non-finite and leaves every other column the bits it has without that block."""
    x, codes, scales, _, _ = _inputs(32, 160, 67, None, None, False, seed=2)
    zeroed = codes.clone()
    zeroed[5, 16:32] = 0
    scales[5, 1] = 0
    assert torch.equal(linear_mx(x, codes, scales), linear_mx(x, zeroed, scales))
    scales[5, 1] = 127
    clean = linear_mx(x, zeroed, scales)
    scales[9, 4] = 255
    got = linear_mx(x, zeroed, scales)
    keep = torch.arange(67, device=DEV) != 9
    assert not torch.isfinite(got[:, 9]).any() and torch.equal(got[:, keep], clean[:, keep])


def test_deterministic_row_invariant_and_blind_to_rows_past_p():
    """64 and 65 rows both run the 64-row tile (one and two row tiles): row p has the same bits in both.  Rows past P
    of a larger, NaN-filled buffer reach no output."""
    nat = _ext.native()
    assert nat.gemm_mx_tile_rows(64) == nat.gemm_mx_tile_rows(65) == 64 and nat.gemm_mx_tile_rows(257) == 128
    x, codes, scales, b, _ = _inputs(65, 2080, 133, None, None, True, seed=4)
    full = linear_mx(x, codes, scales, b, act="gelu")
    assert torch.equal(full, linear_mx(x, codes, scales, b, act="gelu"))
    assert torch.equal(full[:64], linear_mx(x[:64], codes, scales, b, act="gelu"))
    for P in (65, 257):
        big = torch.full((P + 200, 2080), float("nan"), device=DEV, dtype=BF)
        big[:P] = x[torch.arange(P, device=DEV) % 65]
        got = linear_mx(big[:P], codes, scales, b, act="gelu")
        assert torch.isfinite(got).all() and torch.equal(got, linear_mx(big[:P].clone(), codes, scales, b, act="gelu"))


def test_graph_capture():
    x, codes, scales, b, kw = _inputs(40, 160, 67, None, "residual", True, seed=5)
    x2 = _inputs(40, 160, 67, None, "residual", True, seed=6)[0]
    want1, want2 = (linear_mx(t, codes, scales, b, **kw) for t in (x, x2))  # also the warm-up
    buf = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = linear_mx(buf, codes, scales, b, **kw)
    graph.replay()
    assert torch.equal(out, want1)
    for _ in range(2):
        buf.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want2)


@pytest.mark.parametrize("M", [17, 40])
@pytest.mark.parametrize("pro,epi", [("rms", "swiglu"), ("ln", "residual")])
def test_linear_rows_past_16_rows(M, pro, epi):
    x, codes, scales, b, kw = _inputs(M, 160, 67, pro, epi, True, seed=7)
    got = linear_rows(x, codes, b, mx_scales=scales, **kw)
    base = linear_rows(x, mx_dequantize(codes, scales, BF), b, **kw)
    _bar(got, base, _ref(x, mx_dequantize(codes, scales, F64), b, kw), f"linear_rows M={M} {pro} {epi}")
    g, be, eps = kw.get("ln", (kw.get("rms", [None])[0], None, 1e-6))
    direct = _ext.native().rows_linear_mx(x[:16].contiguous(), codes, scales, b, g, be, eps, 3 if epi == "swiglu" else 2,
                                          kw["residual"][:16] if epi == "residual" else None, rms=pro == "rms")
    kw16 = {k: v[:16] if k == "residual" else v for k, v in kw.items()}
    assert torch.equal(linear_rows(x[:16], codes, b, mx_scales=scales, **kw16), direct)


def _models(kw, seed):
    """(the quantised bf16 model, a bf16 copy and an f64 copy whose linears hold the dequantised weights); the f64
    copy lives on the CPU, where every layer has an f64 path"""
    torch.manual_seed(seed)
    m = gpt_tiny(**kw).to(DEV).to(BF).eval()
    m.quantize_rows()
    copies = []
    for dtype in (BF, F64):
        c = copy.deepcopy(m)
        c.quantize_rows(None)
        for lin in [c.head] + [l for b in c.blocks for l in (b.attn.qkv, b.attn.proj, b.mlp.fc1, b.mlp.fc2)]:
            lin.weight.data = mx_dequantize(*mx_quantize(lin.weight), BF)
        copies.append(c.to(dtype) if dtype == BF else c.to(dtype).cpu())
    return m, copies[0], copies[1]


@pytest.mark.parametrize("kw", [{}, {"pos": "rope", "norm": "rms", "mlp": "swiglu", "bias": False}])
def test_prefill_mx_against_f64(kw):
    """Logits and cache rows of ``prefill(mx=True)`` stay within 1.5x of the error the bf16 prefill of the dequantised
    weights has against the f64 one.  (The head is bf16 in both: ``prefill`` never reads its snapshot.)"""
    m, bf, ref = _models(kw, 21)
    m.head.weight.data = bf.head.weight.data
    tokens = torch.randint(0, 256, (4, 40), device=DEV)  # 160 rows: the 128-row tile
    runs = [m.prefill(tokens, mx=True), bf.prefill(tokens), ref.prefill(tokens.cpu())]
    outs = [[lg.to(DEV)] + [t[:, :, :40].to(DEV) for kv in c.layers for t in kv] for lg, c in runs]
    for i, (got, base, want) in enumerate(zip(*outs)):
        e, e0 = ((t.double() - want).norm().item() / want.norm().item() for t in (got, base))
        print(f"{kw} tensor {i}: mx {e:.2e} bf16 {e0:.2e}")
        assert e <= 1.5 * e0, (i, e, e0)


def test_generate_mx_prefill_emits_the_bf16_tokens():
    """B = 20: every fused step has more than 16 rows (``linear_rows`` -> ``linear_mx``).  A token counts where the f64
    model's top-two logit gap exceeds twice the largest logit error of the bf16 copy on the same sequence (either of
    the two logits may move by that much) and every earlier token of its sequence agreed; at most one token in ten
    of the reference falls under the gap."""
    m, bf, ref = _models({}, 28)  # of the seeds 20 .. 39 the one whose reference decides the most tokens (0.925)
    m.head.weight.data = bf.head.weight.data  # the prefill's last-row head reads the bf16 parameter, the steps its snapshot
    tokens = torch.randint(0, 256, (20, 6), device=DEV)
    got, _ = m.generate(tokens, 10, fused=True, mx_prefill=True)
    want, _ = bf.generate(tokens, 10)
    seq = torch.cat([tokens, want[:, :-1]], 1)
    with torch.no_grad():
        l64, lbf = ref(seq.cpu())[:, 5:].to(DEV), bf(seq)[:, 5:].double()
    top = l64.topk(2, dim=-1).values
    decided = (top[..., 0] - top[..., 1]) > 2 * (lbf - l64).abs().max()
    print(f"decided {decided.float().mean().item():.3f}, tokens equal {(got == want).float().mean().item():.3f}")
    assert decided.float().mean() >= 0.9
    agreed = torch.cat([torch.ones_like(got[:, :1]), (got == want).cumprod(1)[:, :-1]], 1).bool()
    assert torch.equal(got[decided & agreed], want[decided & agreed])
