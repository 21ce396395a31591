"""BatchNorm / GroupNorm / InstanceNorm kernels (csrc/norm_bn.hip) against float64 references.

Every dispatch variant of the file at the smallest shape that reaches it (channel vector width,
channel tiles, samples, the two column-sum finalizers on their single-phase and ticket paths, five
activations with and without a residual, the 1-bit ReLU mask, f32 / bf16 / f16, training and eval).
The inputs are built in the I/O dtype; the reference (tests/_norm_ref.py, validated on the CPU by
tests/test_norm_ref.py) sees those same rounded values as float64.

Error metric: relative L2 per channel (per (sample, group) for GroupNorm), so a wrong channel of
small values cannot hide behind the tensor's largest value.

  y, dx, dres   bf16 / f16:  E <= 2 u  (u = 2^-9 / 2^-12: f32 arithmetic, one rounding)
                f32:         E_c <= 2 kappa_c max(E_stock, 2^-23) for every block c, E_stock the
                             metric (largest block error) of the same formulas in stock f32 torch
                             ops, mean subtracted first, and kappa_c the amplification of the
                             kernels' affine form x * scale + shift, from the reference
  dgamma, dbeta, mean, invstd, running stats:  E <= max(4 E_stock, 2^-20)

ReLU / leaky-ReLU elements within 1e-4 (relative to the addends) of the kink get a zero upstream
gradient in all three evaluations, which removes them from every sum and from dx / dres alike; a
case fails if more than 0.1 % of its elements (2 elements below 2000) are that close.

``TBAMD_NORM_F64_REPORT=<file>`` writes every measured figure as JSON (profiles/norm_f64/README.md).
"""
import json
import os
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import _norm_ref as R  # noqa: E402
from torchbooster_amd.ops import _ext  # noqa: E402
from torchbooster_amd.ops.norm import (BatchNormAct1d, BatchNormAct2d, InstanceNormAct2d,  # noqa: E402
                                       ResidualGradLink, _to_rows, batch_norm_act, group_norm_act, unpack_mask)

DEV = "cuda"
EPS, SLOPE, MOM = 1e-5, 0.2, 0.1
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
UNIT = {BF16: R.U_BF16, F16: R.U_F16}
DTN = {F32: "f32", BF16: "bf16", F16: "f16"}
ACTS = ["none", "relu", "leaky_relu", "gelu", "silu"]
VEC_MARGIN, VEC_FLOOR = 4.0, 2.0 ** -20

# Cases whose ELEMENTWISE relative maximum needs more than the margin 4 (the relative L2 over the
# vector meets 4 everywhere): each is a channel whose sum nearly cancels (|dbeta_c|, |dgamma_c| or
# |mean_c| orders below the sum of its terms' magnitudes), where the kernel and the stock evaluation
# both carry an ABSOLUTE error of a few ulp of that magnitude and the ratio of the two is chance.
# In bf16 / f16 the mean's shifted f32 sums carry ulp(|x - x[0]|), not ulp(|mean|), by design.  Margin = twice the
# measured ratio (profiles/norm_f64/README.md).
EL_MARGIN = {
    (('eval', 'B', 'bf16', 'relu', False), 'dbeta'): 10.8,  # E=1.28e-06 E_stock=0.00e+00
    (('gn', '3d', 'bf16', 'gelu', False), 'dbeta'): 10.6,  # E=9.42e-06 E_stock=1.79e-06
    (('gn', '3d', 'bf16', 'gelu', True), 'dgamma'): 9.4,  # E=8.10e-06 E_stock=1.72e-06
    (('gn', '3d', 'bf16', 'none', True), 'dgamma'): 10.5,  # E=9.77e-06 E_stock=1.87e-06
    (('gn', 'g8', 'bf16', 'gelu', False), 'dbeta'): 28.1,  # E=7.84e-06 E_stock=5.59e-07
    (('gn', 'g8', 'bf16', 'gelu', False), 'dgamma'): 8.6,  # E=8.60e-06 E_stock=2.00e-06
    (('gn', 'g8', 'bf16', 'silu', False), 'dbeta'): 133.5,  # E=6.96e-05 E_stock=1.04e-06
    (('gn', 'g8', 'f16', 'gelu', False), 'dbeta'): 9.7,  # E=1.00e-05 E_stock=2.07e-06
    (('gn', 'hw1', 'bf16', 'gelu', False), 'dbeta'): 8.5,  # E=1.31e-05 E_stock=3.10e-06
    (('gn', 'hw1', 'bf16', 'gelu', False), 'dgamma'): 8.3,  # E=9.20e-06 E_stock=2.23e-06
    (('gn', 'hw1', 'f32', 'silu', True), 'dgamma'): 12.1,  # E=9.07e-05 E_stock=1.50e-05
    (('gn', 'in64', 'bf16', 'silu', False), 'dbeta'): 27.0,  # E=7.79e-05 E_stock=5.78e-06
    (('gn', 'tiny', 'f32', 'gelu', True), 'dgamma'): 16.2,  # E=4.84e-06 E_stock=5.99e-07
    (('gn', 'v1', 'bf16', 'silu', True), 'dbeta'): 15.0,  # E=2.60e-05 E_stock=3.50e-06
    (('gn-samplescale', 'g8', 'f32'), 'dbeta'): 14.0,  # E=5.24e-06 E_stock=7.49e-07
    (('train', 'B', 'bf16', 'leaky_relu', True), 'dbeta'): 24.5,  # E=3.54e-06 E_stock=2.90e-07
    (('train', 'B', 'bf16', 'none', False), 'dgamma'): 8.1,  # E=3.63e-06 E_stock=8.99e-07
    (('train', 'B', 'bf16', 'relu', True), 'dgamma'): 22.0,  # E=7.23e-05 E_stock=6.60e-06
    (('train', 'B', 'bf16', 'silu', True), 'dbeta'): 20.4,  # E=1.64e-05 E_stock=1.61e-06
    (('train', 'B', 'bf16', 'silu', True), 'dgamma'): 24.2,  # E=9.30e-03 E_stock=7.70e-04
    (('train', 'C', 'bf16', 'none', True), 'dgamma'): 21.6,  # E=1.44e-05 E_stock=1.34e-06
    (('train', 'D', 'bf16', 'gelu', True), 'dbeta'): 12.3,  # E=1.37e-04 E_stock=2.24e-05
    (('train', 'D', 'f32', 'leaky_relu', False), 'dgamma'): 8.9,  # E=3.60e-04 E_stock=8.13e-05
    (('train', 'D', 'f32', 'leaky_relu', True), 'dgamma'): 26.6,  # E=1.83e-04 E_stock=1.38e-05
    (('train', 'D', 'f32', 'silu', True), 'running_mean'): 10.8,  # E=1.95e-06 E_stock=3.65e-07
    (('train', 'F', 'bf16', 'gelu', False), 'mean'): 20.0,  # E=2.38e-06 E_stock=4.94e-08
    (('train', 'F', 'bf16', 'relu', True), 'dgamma'): 9.6,  # E=3.66e-03 E_stock=7.67e-04
    (('train', 'F', 'bf16', 'silu', True), 'dgamma'): 10.6,  # E=5.82e-06 E_stock=1.11e-06
    (('train', 'G', 'bf16', 'gelu', False), 'dgamma'): 15.8,  # E=8.19e-06 E_stock=1.04e-06
    (('train', 'G', 'bf16', 'gelu', True), 'dbeta'): 8.4,  # E=5.80e-06 E_stock=1.38e-06
    (('train', 'G', 'f16', 'leaky_relu', True), 'running_mean'): 69.9,  # E=9.40e-06 E_stock=2.69e-07
    (('train', 'J2', 'bf16', 'relu', True), 'dgamma'): 13.6,  # E=2.74e-04 E_stock=4.06e-05
    (('train', 'J2', 'f32', 'relu', True), 'dgamma'): 11.7,  # E=7.14e-05 E_stock=1.23e-05
    (('train', 'J3', 'bf16', 'none', True), 'dgamma'): 10.9,  # E=1.89e-06 E_stock=3.48e-07
}

_RECORDS = []


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    _ext.native()
    yield
    path = os.environ.get("TBAMD_NORM_F64_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_RECORDS, f)


def _seed(*key):
    torch.manual_seed(zlib.crc32(repr(key).encode()))


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def _rec(case, out, dt, **kw):
    _RECORDS.append(dict(case=case, out=out, dtype=DTN[dt], **kw))


_PENDING = []


def _expect(ok, msg):
    """Every figure of a case is measured and recorded before the case fails (_flush)."""
    if not ok:
        _PENDING.append(msg)


@pytest.fixture(autouse=True)
def _fresh_case():
    _PENDING.clear()


def _flush():
    msgs = list(_PENDING)
    _PENDING.clear()
    assert not msgs, "\n".join(msgs)


def _check_blocks(case, out, dt, got, ref, stock, kap, blocks, keep=None):
    """y / dx / dres: per-block relative L2 error against the bound of the I/O dtype."""
    assert got.dtype == dt and got.shape == ref.shape, (case, out, got.dtype, got.shape)
    E = R.block_err(got, ref, blocks, keep)
    if dt == F32:
        Es = R.block_err(stock, ref, blocks, keep)
        bound = 2.0 * kap * max(Es.max().item(), 2.0 ** -23)
    else:
        Es = torch.zeros_like(E)
        bound = torch.full_like(E, 2.0 * UNIT[dt])
    used = E / bound
    i = int(used.argmax())
    # (used_paired: against each block's OWN stock error instead of the tensor's largest -- reported only)
    paired = (E / (2.0 * kap * Es.clamp_min(2.0 ** -23))).max().item() if dt == F32 else None
    _rec(case, out, dt, E=E.max().item(), E_stock=Es.max().item() if dt == F32 else None, used=used[i].item(),
         used_paired=paired, worst=dict(block=i, E=E[i].item(), E_stock=Es[i].item(), kappa=kap[i].item()),
         kappa=kap.max().item())
    _expect(bool((E <= bound).all()),
            f"{case} {out}: block {i} E={E[i].item():.3e} bound={bound[i].item():.3e} "
            f"E_stock={Es.max().item():.3e} kappa={kap[i].item():.2f}")


def _check_vec(case, out, dt, got, ref, stock, margin=VEC_MARGIN):
    """Per-channel vectors: relative L2 over the vector and elementwise relative maximum."""
    assert got.shape == ref.shape, (case, out, got.shape, ref.shape)
    (l2, el), (sl2, sel) = R.vec_err(got, ref), R.vec_err(stock, ref)
    b2, be0 = max(margin * sl2, VEC_FLOOR), max(margin * sel, VEC_FLOOR)
    be = be0 * EL_MARGIN.get((case, out), margin) / margin  # a case's own margin scales margin and floor alike
    _rec(case, out, dt, E=l2, E_stock=sl2, used=l2 / b2, E_el=el, E_el_stock=sel, used_el=el / be0,
         ratio=l2 / sl2 if sl2 > 0 else None, ratio_el=el / sel if sel > 0 else None)
    _expect(l2 <= b2, f"{case} {out}: L2 E={l2:.3e} E_stock={sl2:.3e} bound={b2:.3e}")
    _expect(el <= be, f"{case} {out}: elementwise E={el:.3e} E_stock={sel:.3e} bound={be:.3e} ({el / be0:.2f} of margin 4)")


def _kink(case, dt, act, x, scale, shift, res, z):
    """bool keep-mask (None for smooth activations); fails when too many elements sit on the kink"""
    if act not in ("relu", "leaky_relu"):
        return None
    kink = R.kink_mask(x, scale, shift, res, z)
    n, tot = int(kink.sum()), kink.numel()
    _rec(case, "kink_share", dt, E=n / tot, n=n, numel=tot)
    assert n <= (2 if tot < 2000 else tot // 1000), f"{case}: {n} of {tot} elements on the activation kink"
    return ~kink


def _grads(y, leaves, dy):
    got = iter(torch.autograd.grad(y, [t for t in leaves if t is not None], dy))
    return [None if t is None else next(got) for t in leaves]


# ------------------------------------------------------------------ BatchNorm
# id -> logical shape [N, C, H, W] (channels_last), [M, C] or [N, C, L]
BN_SHAPES = {
    "A": (2, 8, 1, 1),       # one group, 256 rows per pass, M = 2
    "B": (2, 64, 5, 13),     # M = 130: 2 partial blocks, 4-row and 1-row stats tails, odd apply tail
    "C": (2, 64, 46, 46),    # M = 4232: 34 partial rows -> colsum_fin4_k ticket path, one channel block
    "D": (2, 512, 20, 13),   # M = 520: 64 groups, 33 partial rows -> 2 slices over 8 channel blocks
    "E": (1, 520, 7, 11),    # M = 77: 65 groups, second tile of one group, partial ninth fin4 block
    "F": (3, 72, 3, 11),     # M = 99: 9 groups, 28 rows per pass, 4 idle threads
    "G": (2, 68, 9, 9),      # M = 162: VEC = 1, second tile of 4 channels, fin4 with a partial block
    "H": (2, 70, 20, 13),    # M = 520: VEC = 1, two tiles, 33 partial rows: scalar finalizer, tickets
    "I": (2, 6, 52, 52),     # M = 5408: VEC = 1, 6 groups (42 rows per pass), 33 partial rows
    "J2": (64, 1024),        # 2-D rows, two full channel tiles
    "J3": (4, 24, 9),        # 3-D
}


def _bn_M(sid):
    s = BN_SHAPES[sid]
    return (s[0] * s[2] * s[3]) if len(s) == 4 else (s[0] if len(s) == 2 else s[0] * s[2])


def test_partial_block_counts():
    """The shapes above sit where the table says: C, D, H, I on the multi-slice ticket path of the
    column-sum finalize (more than 32 partial rows), B on exactly 2 rows."""
    nb = _ext.native().norm_partial_blocks
    got = {sid: nb(_bn_M(sid), BN_SHAPES[sid][1], 1) for sid in BN_SHAPES}
    for sid in "CDHI":
        assert got[sid] > 32, (sid, got[sid])
    assert got["B"] == 2
    assert got["A"] == 1
    assert nb(23 * 23, 64, 4) > 1  # InstanceNorm 4 x 64 x 23 x 23: several partial blocks per sample
    assert nb(1, 48, 3) == 1       # HW = 1


def _bn_inputs(shape, dt, res, affine, x_fn=None):
    C = shape[1]
    x = torch.randn(*shape, device=DEV) * 2 + 0.5 if x_fn is None else x_fn(shape)
    x = _cl(x.to(dt))
    r = _cl(torch.randn(*shape, device=DEV).to(dt)) if res else None
    w = torch.rand(C, device=DEV) + 0.5 if affine else None
    b = torch.randn(C, device=DEV) if affine else None
    rm = torch.randn(C, device=DEV) * 0.5 + 0.5
    rv = torch.rand(C, device=DEV) * 4 + 2
    return x, r, w, b, rm, rv


def _leaf(t, dtype):
    return None if t is None else t.detach().to(dtype).requires_grad_()


def _bn_eval3(x, r, w, b, rm, rv, act, training, dtype, eps):
    """reference (float64) or stock (float32) evaluation from the rounded inputs"""
    lv = [_leaf(t, dtype) for t in (x, w, b, r)]
    out = R.bn_ref(lv[0], lv[1], lv[2], lv[3], act, SLOPE, eps, training, rm.to(dtype), rv.to(dtype), MOM)
    return lv, out


def _bn_case(case, shape, dt, act, res, training=True, affine=True, x_fn=None, link=False, module=None,
             stats=True, eps=EPS):
    _seed(case)
    x, r, w, b, rm, rv = _bn_inputs(shape, dt, res, affine, x_fn)
    lr, ref = _bn_eval3(x, r, w, b, rm, rv, act, training, torch.float64, eps)
    ls, stk = _bn_eval3(x, r, w, b, rm, rv, act, training, F32, eps)
    keep = _kink(case, dt, act, lr[0], ref.scale, ref.shift, lr[3], ref.z)
    dy = torch.randn(*shape, device=DEV).to(dt)
    if keep is not None:
        dy = dy * keep
    dy = _cl(dy)
    gr = _grads(ref.y, lr, dy.double())
    gs = _grads(stk.y, ls, dy.float())
    kap = R.kappa(lr[0], ref.scale, ref.shift, lr[3], ref.z, R.chan_blocks)

    xa, ra = _leaf(x, dt), _leaf(r, dt)
    nbt = torch.zeros((), dtype=torch.long, device=DEV)
    lk = ResidualGradLink() if link else None
    if module is not None:
        m = module(shape[1], eps, MOM, affine=affine, act=act, slope=SLOPE).to(DEV)
        with torch.no_grad():
            if affine:
                m.weight.copy_(w)
                m.bias.copy_(b)
            m.running_mean.copy_(rm)
            m.running_var.copy_(rv)
        m.train(training)
        y = m(xa, ra)
        wa, ba, rmk, rvk, nbt = m.weight, m.bias, m.running_mean, m.running_var, m.num_batches_tracked
    else:
        wa, ba = _leaf(w, F32), _leaf(b, F32)
        rmk, rvk = rm.clone(), rv.clone()
        y = batch_norm_act(xa, wa, ba, rmk, rvk, training, MOM, eps, ra, act, SLOPE, num_batches_tracked=nbt,
                           link=lk)
    y.backward(dy)
    dres = None
    if res:
        if link:
            # the residual's producer applies the mask itself (ops/conv.py dgrad epilogue)
            assert ra.grad is None
            ldy, mask = lk.take()
            assert mask is not None and mask.dtype == torch.uint8 and mask.numel() == x.numel() // 8
            bits = unpack_mask(mask, y)
            assert torch.equal(bits, y.detach() > 0), f"{case}: mask bits differ from y > 0"
            dres = ldy * bits
        else:
            dres = ra.grad

    _check_blocks(case, "y", dt, y.detach(), ref.y, stk.y, kap, R.chan_blocks)
    _check_blocks(case, "dx", dt, xa.grad, gr[0], gs[0], kap, R.chan_blocks, keep)
    if res:
        _check_blocks(case, "dres", dt, dres, gr[3], gs[3], kap, R.chan_blocks, keep)
    if affine:
        _check_vec(case, "dgamma", dt, wa.grad, gr[1], gs[1])
        _check_vec(case, "dbeta", dt, ba.grad, gr[2], gs[2])
    if training:
        _check_vec(case, "running_mean", dt, rmk, ref.running_mean, stk.running_mean)
        _check_vec(case, "running_var", dt, rvk, ref.running_var, stk.running_var)
        assert int(nbt) == 1
        if stats:
            mean, invstd, scale, shift = _ext.native().bn_stats(_to_rows(x)[0], None, w, b, None, None, True, MOM,
                                                                eps, None)
            _check_vec(case, "mean", dt, mean, ref.mean, stk.mean)
            _check_vec(case, "invstd", dt, invstd, ref.invstd, stk.invstd)
            _check_vec(case, "scale", dt, scale, ref.scale, stk.scale)
    else:
        assert torch.equal(rmk, rm) and torch.equal(rvk, rv) and int(nbt) == 0
    _flush()
    return dict(y=y.detach(), dx=xa.grad, dres=dres, dg=wa.grad if affine else None, db=ba.grad if affine else None,
                kappa=kap, ref=ref, stock=stk)


def _train_cases():
    out = []
    for sid in BN_SHAPES:
        full = sid in "BDFGH"
        for dt in (F32, BF16):
            for act in (ACTS if full else ("none", "relu")):
                for res in (False, True):
                    out.append((sid, dt, act, res))
        if sid in "BDGH":  # f16
            out += [(sid, F16, "relu", True), (sid, F16, "none", False), (sid, F16, "gelu", True),
                    (sid, F16, "silu", False), (sid, F16, "leaky_relu", True)]
    return out


def _ids(cases):
    return ["-".join(DTN.get(v, str(v)) for v in c) for c in cases]


_TRAIN = _train_cases()


@pytest.mark.parametrize("sid,dt,act,res", _TRAIN, ids=_ids(_TRAIN))
def test_bn_train(sid, dt, act, res):
    shape = BN_SHAPES[sid]
    module = BatchNormAct1d if sid in ("J2", "J3") else None
    # A (M = 2): with eps << var the two rows' xhat are +-1 and dx cancels analytically to
    # O(eps / var) * dz, about 1e-6 of its terms -- rounding noise in ANY f32 evaluation, stock
    # included.  eps = 1 (the order of var) keeps dx a number that can be held to the bounds.
    _bn_case(("train", sid, DTN[dt], act, res), shape, dt, act, res, module=module, eps=1.0 if sid == "A" else EPS)


_EVAL = ([(sid, dt, act, res) for sid in "BFG" for dt in (F32, BF16) for act in ("relu", "leaky_relu", "gelu")
          for res in (False, True)]
         + [("B", F16, "relu", True), ("G", F16, "silu", False), ("D", F32, "none", False), ("H", BF16, "silu", True)])


@pytest.mark.parametrize("sid,dt,act,res", _EVAL, ids=_ids(_EVAL))
def test_bn_eval_forward_backward(sid, dt, act, res):
    """Eval mode normalises with the running statistics; its backward (training = 0 in BwdFin) has
    no mean / variance terms: dx = scale * dz."""
    _bn_case(("eval", sid, DTN[dt], act, res), BN_SHAPES[sid], dt, act, res, training=False)


@pytest.mark.parametrize("sid", ["B", "G"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("act,res", [("relu", True), ("gelu", False)])
def test_bn_without_affine(sid, dt, act, res):
    _bn_case(("noaffine", sid, DTN[dt], act, res), BN_SHAPES[sid], dt, act, res, affine=False)


_LINK = [(sid, dt) for sid in "BDE" for dt in (F32, BF16)] + [("B", F16), ("D", F16)]


@pytest.mark.parametrize("sid,dt", _LINK, ids=_ids(_LINK))
def test_bn_relu_residual_mask_link(sid, dt):
    """ReLU after the residual add with a plain ResidualGradLink: the mask-writing apply and the
    MASKIN backward kernels; the residual gradient is dy * mask, applied by the link's consumer."""
    _bn_case(("masklink", sid, DTN[dt]), BN_SHAPES[sid], dt, "relu", True, link=True)


@pytest.mark.parametrize("sid", ["B", "G"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_bn_nchw_input_is_bit_equal(sid, dt):
    """NCHW-contiguous x / residual / dy give the bits of the channels_last call."""
    shape = BN_SHAPES[sid]
    _seed("nchw", sid, DTN[dt])
    x, r, w, b, rm, rv = _bn_inputs(shape, dt, True, True)
    dy = _cl(torch.randn(*shape, device=DEV).to(dt))
    outs = []
    for conv in (_cl, lambda t: t.contiguous()):
        xa, ra, wa, ba = _leaf(conv(x), dt), _leaf(conv(r), dt), _leaf(w, F32), _leaf(b, F32)
        assert xa.is_contiguous() == (conv is not _cl)
        rmk, rvk = rm.clone(), rv.clone()
        y = batch_norm_act(xa, wa, ba, rmk, rvk, True, MOM, EPS, ra, "relu", SLOPE)
        y.backward(conv(dy))
        outs.append((y.detach(), xa.grad, ra.grad, wa.grad, ba.grad, rmk, rvk))
    for a, c in zip(*outs):
        assert a.shape == c.shape and torch.equal(a, c)


@pytest.mark.parametrize("sid", ["C", "H"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_bn_ticket_path_repeats_bit_equal(sid, dt):
    """Two consecutive launches on one stream through the multi-slice finalize: the tickets reset
    themselves and the slice merge order is fixed."""
    shape = BN_SHAPES[sid]
    _seed("repeat", sid, DTN[dt])
    x, r, w, b, rm, rv = _bn_inputs(shape, dt, True, True)
    dy = _cl(torch.randn(*shape, device=DEV).to(dt))
    outs = []
    for _ in range(2):
        xa, ra, wa, ba = _leaf(x, dt), _leaf(r, dt), _leaf(w, F32), _leaf(b, F32)
        rmk, rvk = rm.clone(), rv.clone()
        y = batch_norm_act(xa, wa, ba, rmk, rvk, True, MOM, EPS, ra, "silu", SLOPE)
        y.backward(dy)
        st = _ext.native().bn_stats(_to_rows(x)[0], None, w, b, None, None, True, MOM, EPS, None)
        outs.append((y.detach(), xa.grad, ra.grad, wa.grad, ba.grad, rmk, rvk, *st))
    for a, c in zip(*outs):
        assert torch.equal(a, c)


@pytest.mark.parametrize("sid", ["B", "G"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("momentum", [0.1, 1.0, None])
def test_bn_running_stats_two_steps(sid, dt, momentum):
    """BatchNormAct2d from non-trivial running statistics: momentum 0.1 and 1.0 over two steps,
    the cumulative average (momentum=None) over three; num_batches_tracked after each."""
    shape = BN_SHAPES[sid]
    C = shape[1]
    case = ("running", sid, DTN[dt], momentum)
    _seed(case)
    m = BatchNormAct2d(C, EPS, momentum, act="none").to(DEV).train()
    rm, rv = torch.randn(C, device=DEV) * 0.5 + 0.5, torch.rand(C, device=DEV) * 4 + 2
    with torch.no_grad():
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
    ref_s, stk_s = (rm.double(), rv.double()), (rm.clone(), rv.clone())
    for step in range(1, 4 if momentum is None else 3):
        x = _cl((torch.randn(*shape, device=DEV) * (1 + step) + 0.5 * step).to(dt))
        mom = 1.0 / step if momentum is None else momentum
        m(x)
        ref = R.bn_ref(x.double(), None, None, None, "none", 0.0, EPS, True, ref_s[0], ref_s[1], mom)
        stk = R.bn_ref(x.float(), None, None, None, "none", 0.0, EPS, True, stk_s[0], stk_s[1], mom)
        ref_s, stk_s = (ref.running_mean, ref.running_var), (stk.running_mean, stk.running_var)
        assert int(m.num_batches_tracked) == step
        _check_vec(case + (step,), "running_mean", dt, m.running_mean, ref_s[0], stk_s[0])
        _check_vec(case + (step,), "running_var", dt, m.running_var, ref_s[1], stk_s[1])
    _flush()


# ------------------------------------------------------------------ GroupNorm / InstanceNorm
# id -> (shape, groups)
GN_SHAPES = {
    "g8": ((2, 64, 5, 13), 8),      # VEC = 8, several samples, tail rows
    "hw1": ((3, 48, 1, 1), 6),      # HW = 1: statistics over channels only
    "v1": ((2, 70, 9, 9), 7),       # VEC = 1, two channel tiles, Cg = 10
    "tiny": ((2, 6, 5, 5), 3),      # tiny VEC = 1
    "t65": ((2, 520, 3, 3), 65),    # second tile with one group
    "in64": ((4, 64, 23, 23), 64),  # InstanceNormAct2d, several partial blocks per sample
    "in24": ((2, 24, 7, 7), 24),    # InstanceNormAct2d
    "3d": ((2, 32, 50), 4),         # 3-D input
}
GN_ACTS = ["none", "relu", "gelu", "silu"]


def _gn_case(case, shape, G, dt, act, res, affine=True, inorm=False, x_fn=None):
    _seed(case)
    C = shape[1]
    x, r, w, b, _, _ = _bn_inputs(shape, dt, res, affine, x_fn)
    blocks = lambda t: R.group_blocks(t, G)  # noqa: E731

    def ev(dtype):
        lv = [_leaf(t, dtype) for t in (x, w, b, r)]
        return lv, R.gn_ref(lv[0], G, lv[1], lv[2], lv[3], act, SLOPE, EPS)

    (lr, ref), (ls, stk) = ev(torch.float64), ev(F32)
    keep = _kink(case, dt, act, lr[0], ref.scale, ref.shift, lr[3], ref.z)
    dy = torch.randn(*shape, device=DEV).to(dt)
    if keep is not None:
        dy = dy * keep
    dy = _cl(dy)
    gr, gs = _grads(ref.y, lr, dy.double()), _grads(stk.y, ls, dy.float())
    kap = R.kappa(lr[0], ref.scale, ref.shift, lr[3], ref.z, blocks)

    xa, ra = _leaf(x, dt), _leaf(r, dt)
    if inorm:
        m = InstanceNormAct2d(C, EPS, affine=affine, act=act, slope=SLOPE).to(DEV)
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        wa, ba = m.weight, m.bias
        y = m(xa, ra)
    else:
        wa, ba = _leaf(w, F32), _leaf(b, F32)
        y = group_norm_act(xa, G, wa, ba, EPS, ra, act, SLOPE)
    y.backward(dy)
    _check_blocks(case, "y", dt, y.detach(), ref.y, stk.y, kap, blocks)
    _check_blocks(case, "dx", dt, xa.grad, gr[0], gs[0], kap, blocks, keep)
    if res:
        _check_blocks(case, "dres", dt, ra.grad, gr[3], gs[3], kap, blocks, keep)
    if affine:
        _check_vec(case, "dgamma", dt, wa.grad, gr[1], gs[1])
        _check_vec(case, "dbeta", dt, ba.grad, gr[2], gs[2])
    _flush()
    return ref, stk, x, w, b


def _gn_cases():
    out = [(gid, dt, act, res) for gid in GN_SHAPES for dt in (F32, BF16) for act in GN_ACTS for res in (False, True)]
    for gid in ("g8", "v1"):
        out += [(gid, F16, "relu", True), (gid, F16, "gelu", False), (gid, F16, "silu", True), (gid, F16, "none", False)]
    return out


_GN = _gn_cases()


@pytest.mark.parametrize("gid,dt,act,res", _GN, ids=_ids(_GN))
def test_gn(gid, dt, act, res):
    shape, G = GN_SHAPES[gid]
    _gn_case(("gn", gid, DTN[dt], act, res), shape, G, dt, act, res, inorm=gid.startswith("in"))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("act,res", [("relu", True), ("silu", False)])
def test_gn_without_affine(dt, act, res):
    shape, G = GN_SHAPES["v1"]
    _gn_case(("gn-noaffine", DTN[dt], act, res), shape, G, dt, act, res, affine=False)


@pytest.mark.parametrize("gid", ["g8", "v1"])
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_gn_per_sample_scale(gid, dt):
    """x[n] *= 10**n: a sample that read another sample's statistics would be off by decades."""
    shape, G = GN_SHAPES[gid]

    def x_fn(s):
        x = torch.randn(*s, device=DEV) * 2 + 0.5
        return x * (10.0 ** torch.arange(s[0], device=DEV)).view(-1, 1, 1, 1)

    _gn_case(("gn-samplescale", gid, DTN[dt]), shape, G, dt, "gelu", True, x_fn=x_fn)


# ------------------------------------------------------------------ conditioning (f32)
def _offset(shape):
    return 256.0 + 0.5 * torch.randn(*shape, device=DEV)  # |mean| / std = 512


@pytest.mark.parametrize("sid", ["B", "D"])
@pytest.mark.parametrize("act,res", [("none", False), ("silu", True)])
def test_bn_offset_inputs(sid, act, res):
    """|mean| / std = 512.  The shifted sums keep mean / invstd / running variance at the bound of
    well-centred inputs; y and dx carry the cancellation of the affine form x * scale + shift and
    are held to kappa (about 1000 here) times the stock error.  (Smooth activations: the kink rule
    would exclude every element with |z| < 0.05.)"""
    out = _bn_case(("offset", sid, act, res), BN_SHAPES[sid], F32, act, res, x_fn=_offset)
    assert out["kappa"].min().item() > 100


@pytest.mark.parametrize("act,res", [("none", False), ("silu", True)])
def test_gn_offset_inputs(act, res):
    shape, G = GN_SHAPES["g8"]
    case = ("gn-offset", act, res)
    ref, stk, x, w, b = _gn_case(case, shape, G, F32, act, res, x_fn=_offset)
    N, C = shape[0], shape[1]
    coeff = _ext.native().gn_forward(_to_rows(x)[0], N, G, w, b, EPS, None, 0, 0.0)[1]  # mean, invstd, scale, shift
    per_c = lambda t: t.repeat_interleave(C // G, dim=1)  # noqa: E731
    _check_vec(case, "mean", F32, coeff[0], per_c(ref.mean), per_c(stk.mean))
    _check_vec(case, "invstd", F32, coeff[1], per_c(ref.invstd), per_c(stk.invstd))
    _flush()


def _var_envelope(case, var_k, var_ref, D):
    """|var - var_ref| <= 64 * 2^-24 * (var_ref + D^2): the shifted sums Q = sum (x - x0)^2 carry
    x0's distance D from the mean squared; 64 covers the few rows each lane adds at these shapes."""
    err = (var_k - var_ref).abs().reshape(-1)
    var_ref, D = var_ref.reshape(-1), D.reshape(-1)
    env = 64 * R.U_F32 * (var_ref + D * D)
    used = err / env
    i = int(used.argmax())
    _rec(case, "var_outlier_row0", F32, E=(err / var_ref).max().item(), used=used[i].item(),
         worst=dict(block=i, err=err.reshape(-1)[i].item(), env=env.reshape(-1)[i].item()))
    _expect(bool((err <= env).all()), f"{case}: var error {err[i].item():.3e} > envelope {env[i].item():.3e}")
    _flush()


@pytest.mark.parametrize("sid", ["B", "D"])
def test_bn_outlier_row0(sid):
    """Row 0, the shift of the partial sums, 16 standard deviations out in every channel."""
    shape = BN_SHAPES[sid]
    case = ("outlier", sid)
    _seed(case)
    x = torch.randn(*shape, device=DEV) * 2 + 0.5
    x[0, :, 0, 0] += 16 * 2.0
    x = _cl(x)
    ref = R.bn_ref(x.double(), None, None, None, "none", 0.0, EPS, True, None, None)
    mean, invstd, _, _ = _ext.native().bn_stats(_to_rows(x)[0], None, None, None, None, None, True, MOM, EPS, None)
    var_k = 1.0 / invstd.double() ** 2 - EPS
    D = (x[0, :, 0, 0].double() - ref.mean).abs()
    assert (D > 20).all()  # 16 std, give or take the row's own draw
    _var_envelope(case, var_k, ref.var, D)


def test_gn_outlier_row0():
    shape, G = GN_SHAPES["g8"]
    case = ("gn-outlier",)
    _seed(case)
    N, C = shape[0], shape[1]
    x = torch.randn(*shape, device=DEV) * 2 + 0.5
    x[:, :, 0, 0] += 16 * 2.0
    x = _cl(x)
    ref = R.gn_ref(x.double(), G, None, None, None, "none", 0.0, EPS)
    coeff = _ext.native().gn_forward(_to_rows(x)[0], N, G, None, None, EPS, None, 0, 0.0)[1]
    var_k = (1.0 / coeff[1].double() ** 2 - EPS).view(N, G, C // G)
    assert bool((var_k == var_k[:, :, :1]).all())  # one value per (sample, group)
    # the largest distance of a channel's shift from the group mean
    D = (x[:, :, 0, 0].double().view(N, G, C // G) - ref.mean.unsqueeze(2)).abs().amax(dim=2)
    _var_envelope(case, var_k[:, :, 0], ref.var, D)
