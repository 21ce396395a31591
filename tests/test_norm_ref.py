"""The f64 normalisation references (tests/_norm_ref.py) against the stock functions, on the CPU.

This is the only place ``F.batch_norm`` / ``F.group_norm`` / ``F.instance_norm`` validate the
references the GPU sweep (tests/test_gpu_norm_f64.py) measures the HIP kernels with: forward, every
input gradient, the running statistics, every activation and both residual settings, to 1e-12."""
import pytest
import torch
import torch.nn.functional as F

from tests import _norm_ref as R
from torchbooster_amd.ops.norm import act_ref

ACTS = ["none", "relu", "leaky_relu", "gelu", "silu"]
TOL = 1e-12
F64 = torch.float64


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _leaf(*shape, scale=1.0, shift=0.0, pos=False):
    t = torch.rand(*shape, dtype=F64) + 0.5 if pos else torch.randn(*shape, dtype=F64) * scale + shift
    return t.requires_grad_()


def _grads(y, dy, leaves):
    return torch.autograd.grad(y, [t for t in leaves if t is not None], dy)


@pytest.mark.parametrize("shape", [(3, 5, 4, 7), (6, 11), (4, 6, 9)])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_bn_ref_matches_stock(shape, act, res, training):
    torch.manual_seed(len(shape) * 100 + ACTS.index(act) * 4 + res * 2 + training)
    C = shape[1]
    x, w, b = _leaf(*shape, scale=2.0, shift=0.5), _leaf(C, pos=True), _leaf(C)
    r = _leaf(*shape) if res else None
    rm, rv = torch.randn(C, dtype=F64), torch.rand(C, dtype=F64) + 0.5
    dy = torch.randn(*shape, dtype=F64)
    for momentum in (0.1, 1.0):
        out = R.bn_ref(x, w, b, r, act, 0.2, 1e-5, training, rm, rv, momentum)
        rm2, rv2 = rm.clone(), rv.clone()
        z = F.batch_norm(x, rm2, rv2, w, b, training, momentum, 1e-5)
        if res:
            z = z + r
        ys = act_ref(z, act, 0.2)
        assert _rel(out.y, ys) <= TOL
        assert _rel(out.z, z) <= TOL
        for g, gs in zip(_grads(out.y, dy, (x, w, b, r)), _grads(ys, dy, (x, w, b, r))):
            assert _rel(g, gs) <= TOL
        if training:
            assert _rel(out.running_mean, rm2) <= TOL and _rel(out.running_var, rv2) <= TOL
            dims = [0] + list(range(2, len(shape)))
            assert _rel(out.mean, x.mean(dim=dims)) <= TOL
            assert _rel(out.var, x.var(dim=dims, unbiased=False)) <= TOL
        else:
            assert out.running_mean is None and torch.equal(rm, rm2) and torch.equal(rv, rv2)
            assert torch.equal(out.mean, rm) and torch.equal(out.var, rv)
        # the kernels' affine form reproduces z from the returned coefficients
        xs, sh, rr = R.cond_terms(x, out.scale, out.shift, r)
        assert _rel(xs + sh + (rr if res else 0.0), out.z) <= 1e-11


def test_bn_ref_without_affine():
    torch.manual_seed(7)
    x = _leaf(4, 6, 3, 3, scale=2.0, shift=0.5)
    out = R.bn_ref(x, None, None, None, "gelu", 0.0, 1e-5, True, None, None)
    ys = F.gelu(F.batch_norm(x, None, None, None, None, True, 0.1, 1e-5))
    assert _rel(out.y, ys) <= TOL and out.running_mean is None
    dy = torch.randn_like(x)
    assert _rel(_grads(out.y, dy, (x,))[0], _grads(ys, dy, (x,))[0]) <= TOL


@pytest.mark.parametrize("shape,groups", [((3, 12, 4, 5), 4), ((2, 6, 7), 3), ((2, 8, 1, 1), 2), ((3, 5, 4, 4), 5)])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("res", [False, True])
def test_gn_ref_matches_stock(shape, groups, act, res):
    torch.manual_seed(groups * 10 + ACTS.index(act) * 2 + res)
    C = shape[1]
    x, w, b = _leaf(*shape, scale=2.0, shift=0.5), _leaf(C, pos=True), _leaf(C)
    r = _leaf(*shape) if res else None
    dy = torch.randn(*shape, dtype=F64)
    out = R.gn_ref(x, groups, w, b, r, act, 0.2, 1e-5)
    z = F.group_norm(x, groups, w, b, 1e-5)
    if res:
        z = z + r
    ys = act_ref(z, act, 0.2)
    assert _rel(out.y, ys) <= TOL
    for g, gs in zip(_grads(out.y, dy, (x, w, b, r)), _grads(ys, dy, (x, w, b, r))):
        assert _rel(g, gs) <= TOL
    xs, sh, rr = R.cond_terms(x, out.scale, out.shift, r)
    assert _rel(xs + sh + (rr if res else 0.0), out.z) <= 1e-11
    if groups == C:  # InstanceNorm
        zi = F.instance_norm(x, None, None, w, b, True, 0.1, 1e-5)
        assert _rel(out.z - (r if res else 0.0), zi) <= TOL
    # without affine parameters
    out0 = R.gn_ref(x, groups, None, None, r, act, 0.2, 1e-5)
    z0 = F.group_norm(x, groups, None, None, 1e-5)
    assert _rel(out0.y, act_ref(z0 + r if res else z0, act, 0.2)) <= TOL


def test_block_metric_sees_a_small_channel():
    """One wrong channel of small values: invisible to max-abs over the tensor's largest value,
    plain in the per-channel metric."""
    torch.manual_seed(3)
    ref = torch.randn(4, 6, 5, 5, dtype=F64)
    ref[:, 2] *= 1e-4
    a = ref.clone()
    a[:, 2] *= 1.5
    whole = ((a - ref).abs().max() / ref.abs().max()).item()
    e = R.block_err(a, ref, R.chan_blocks)
    assert whole < 1e-4 and abs(e[2].item() - 0.5) < 1e-12 and e.sum().item() == e[2].item()
    eg = R.block_err(a, ref, lambda t: R.group_blocks(t, 3))  # groups of 2 channels, per sample
    assert eg.shape == (12,) and (eg.view(4, 3)[:, 1] > 1e-5).all() and eg.view(4, 3)[:, 0].sum().item() == 0.0
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[:, 2] = False
    assert R.block_err(a, ref, R.chan_blocks, keep).sum().item() == 0.0
    l2, el = R.vec_err(torch.tensor([1.0, 2.0 + 2e-3], dtype=F64), torch.tensor([1.0, 2.0], dtype=F64))
    assert abs(el - 1e-3) < 1e-9 and abs(l2 - 2e-3 / 5 ** 0.5) < 1e-9


def test_kappa_and_kink():
    torch.manual_seed(4)
    x = torch.randn(8, 3, 4, 4, dtype=F64) * 0.5 + 256.0  # |mean| / std = 512
    w, b = torch.ones(3, dtype=F64), torch.zeros(3, dtype=F64)
    out = R.bn_ref(x, w, b, None, "relu", 0.0, 1e-5, True, None, None)
    k = R.kappa(x, out.scale, out.shift, None, out.z, R.chan_blocks)
    assert ((k > 900) & (k < 1200)).all()  # ~ 2 |mean| / std
    x0 = torch.randn(8, 3, 4, 4, dtype=F64) * 2 + 0.5
    out0 = R.bn_ref(x0, w, b, None, "relu", 0.0, 1e-5, True, None, None)
    k0 = R.kappa(x0, out0.scale, out0.shift, None, out0.z, R.chan_blocks)
    assert (k0 < 4).all() and (k0 >= 1 - 1e-12).all()
    kk = R.kink_mask(x0, out0.scale, out0.shift, None, out0.z)
    assert kk.sum().item() <= 1
    zz = out0.z.clone()
    zz[0, 0, 0, 0] = 1e-9
    assert R.kink_mask(x0, out0.scale, out0.shift, None, zz)[0, 0, 0, 0]
