"""No vendor convolution by default: a nativize()d model with 5x5/2, non-stem
7x7/2, 3x3/3 and 3x3/4 convolutions trains 3 steps with every conv direction on the native
kernels -- the kernel census of those steps holds no MIOpen kernel (only this package's tbamd::
kernels, ATen elementwise / reduction kernels, and library GEMMs) -- and its first-step gradients
follow the fp32 PyTorch reference.  Reference: every Conv2d of the examples goes through cuDNN
with cudnn.benchmark (/root/reference/torchbooster/utils.py:42); here the native routes replace it."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)


def _model():
    return nn.Sequential(
        nn.Conv2d(64, 128, 5, 2, 2, bias=False), nn.BatchNorm2d(128), nn.ReLU(),
        nn.Conv2d(128, 128, 7, 2, 3, bias=False), nn.BatchNorm2d(128), nn.ReLU(),
        nn.Conv2d(128, 64, 3, 3, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU(),
        nn.Conv2d(64, 64, 3, 4, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU(),
        nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(64, 10))


def _vendor_conv_kernels(names):
    bad = [n for n in names if "miopen" in n.lower() or "igemm" in n.lower() or "naive_conv" in n.lower()
           or "gridwise" in n.lower() or "conv_fwd_gtc" in n.lower() or "grouped_conv" in n.lower()]
    return sorted(set(bad))


@pytest.mark.parametrize("C,K,R,st,pad,H", [(64, 128, 5, 2, 2, 64), (128, 128, 7, 2, 3, 32), (128, 64, 3, 3, 1, 16),
                                             (64, 64, 3, 4, 1, 6)])
def test_strided_conv_directions_match_fp32(C, K, R, st, pad, H):
    """Forward, input gradient and weight gradient of each strided conv of the model against fp32
    PyTorch (bf16 output rounding is ~2e-3)."""
    from torchbooster_amd.ops import conv as CV

    torch.manual_seed(C + K + R + st)
    x = torch.randn(8, C, H, H, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(K, C, R, R, device="cuda") * (C * R * R) ** -0.5).to(torch.bfloat16)
    w = w.contiguous(memory_format=torch.channels_last)
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = CV.conv2d(xa, wa, None, st, pad)
    dy = torch.randn_like(y)
    y.backward(dy)
    xr, wr = x.float().requires_grad_(), w.float().requires_grad_()
    yr = F.conv2d(xr, wr, None, st, pad)
    yr.backward(dy.float())
    for got, ref in ((y, yr), (xa.grad, xr.grad), (wa.grad, wr.grad)):
        assert ((got.float() - ref).norm() / ref.norm()).item() < 5e-3


def test_strided_convs_train_without_miopen():
    from torchbooster_amd.nativize import nativize
    from torchbooster_amd.ops import conv_route
    from torchbooster_amd.ops.optim import FusedAdamW

    assert conv_route._NO_MIOPEN  # the default
    torch.manual_seed(0)
    ref = _model().cuda().to(memory_format=torch.channels_last)
    stock16 = copy.deepcopy(ref).to(torch.bfloat16)
    m = nativize(copy.deepcopy(ref).to(torch.bfloat16))
    x = torch.randn(8, 64, 64, 64, device="cuda").contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 10, (8,), device="cuda")

    # first-step gradients against fp32 PyTorch, measured against the stock bf16 model's own
    # deviation (BN over a 2x2 map at batch 8 makes this net's bf16 gradients ~15 % off fp32 on
    # ANY bf16 path; the per-op errors are ~2e-3, test above)
    F.cross_entropy(ref(x), t).backward()
    F.cross_entropy(stock16(x.to(torch.bfloat16)).float(), t).backward()
    F.cross_entropy(m(x.to(torch.bfloat16)).float(), t).backward()
    for (name, p), pr, ps in zip(m.named_parameters(), ref.parameters(), stock16.parameters()):
        err = ((p.grad.float() - pr.grad).norm() / pr.grad.norm().clamp_min(1e-12)).item()
        bar = ((ps.grad.float() - pr.grad).norm() / pr.grad.norm().clamp_min(1e-12)).item()
        assert err <= 1.25 * bar + 1e-2, (name, err, bar)

    opt = FusedAdamW(m.parameters(), lr=1e-3)
    names = []
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            loss = F.cross_entropy(m(x.to(torch.bfloat16)).float(), t)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert torch.isfinite(loss)
    assert any("conv" in n for n in names), names[:20]
    bad = _vendor_conv_kernels(names)
    assert not bad, bad
    conv_kernels = sorted({n for n in names if "conv" in n.lower()})
    print("conv kernels:", conv_kernels)
    assert all("tbamd::" in n for n in conv_kernels), conv_kernels
