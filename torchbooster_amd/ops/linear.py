"""Linear layers on the native GEMM engine (csrc/gemm.hip, ops/gemm.py).

Reference: ``nn.Linear`` in every example MLP / head
(/root/reference/examples/img_gen/gan/gan.py:35-48, vae.py:37-55,
img_cls/lenet/lenet.py:33-35, resnet.py:112) -> cuBLAS.  Here, per step:

* forward  ``y = x Wᵀ + b`` (bias fused; ``LinearGELU`` also fuses the exact
  GELU and saves the pre-activation for its backward);
* input gradient ``dX = dY W`` (W read transposed from LDS, no Wᵀ copy);
* weight gradient ``dW = dYᵀ X`` (split-K over the batch x tokens rows);
* ``db = Σ dY`` — a native column sum (``LinearGELU``: fused with GELU').

Decoding has 1 - 16 rows per product, nothing for that engine's 128 - 256 row tiles:
``linear_rows`` is the weight-streaming few-row kernel of csrc/rows_gemm.hip with a LayerNorm
prologue and bias / GELU / residual epilogues, ``embed_rows`` the fused token + position embedding
(both forward only).  ``linear_mx`` is the dense product on an MXFP4 weight for any number of rows
(csrc/gemm_mx.hip): what ``linear_rows(mx_scales=)`` runs past 16 rows and a quantised prefill multiplies by.

Weight/bias gradients land straight in the parameter's persistent gradient
slot (ops/_ext.py ``take_slot``) — no accumulate-add or bucket copy per step.
Shapes the engine does not take (a feature count not a multiple of 8, fp32 /
fp16 activations) use ATen.  State-dict compatible with ``nn.Linear``.
"""
from __future__ import annotations

import functools
import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from torchbooster_amd.ops import gemm as G
from torchbooster_amd.ops._ext import native, slot_alias, take_slot, use_native
from torchbooster_amd.ops.act import swiglu
from torchbooster_amd.ops.norm import layer_norm, rms_norm

__all__ = ["Linear", "linear", "LinearGELU", "linear_gelu", "GeluLink", "linear_rows", "embed_rows",
           "mx_quantize", "mx_dequantize", "linear_mx", "linear_rows_experts", "moe_route_rows"]

# The fused epilogue stages the z tile through LDS with coalesced 16-B loads: 0.221 vs 0.273 ms
# unfused, ViT-B/16 5245 / 5241 vs 5134 / 5137 img/s alternated (profiles/r03_gemm_nn/README.md;
# its first form, 8-B z loads in the accumulator layout, lost in the real step on a cold z).
# TBAMD_FUSE_GELU_BWD=0 turns it off.
_FUSE_GELU_BWD = os.environ.get("TBAMD_FUSE_GELU_BWD", "1") == "1"


class GeluLink:
    """``LinearGELU`` (fc1) -> ``Linear`` (fc2) hand-off of the MLP backward.

    fc2's input gradient dH = dY W2 is only ever multiplied by GELU'(z1) (fc1's backward), and
    fc1's bias gradient is the column sum of that product: with a link, fc2's backward computes
    dZ1 = (dY W2) * GELU'(z1) and Σ dZ1 in ONE GEMM epilogue (csrc/gemm8.hip NN mode,
    ``gemm_nn_gelu_bwd``) and hands dZ1 to autograd as "the gradient of H"; fc1's backward
    recognises that very tensor and skips its own GELU / bias pass.  Only valid when fc2 is
    H's sole consumer (the caller wires it that way, e.g. models/vit.py MLP)."""

    __slots__ = ("z", "bias", "dz_ptr", "db")

    def __init__(self) -> None:
        self.z = self.bias = self.dz_ptr = self.db = None

    def take(self, dy: Tensor):
        """(True, bias gradient) when ``dy`` is the fused dZ this link handed out, else (False, None)."""
        ptr, db = self.dz_ptr, self.db
        self.dz_ptr = self.db = None
        if ptr is None:
            return False, None
        if ptr == dy.data_ptr():
            return True, db
        # fc2 already applied GELU' to what it handed out: a different tensor here means a
        # tensor hook or a second consumer rewrote H's gradient, and recomputing GELU' on it
        # would apply it twice -- fail closed instead of returning a wrong gradient
        raise RuntimeError("GeluLink: the hidden activation's gradient was modified between fc2 and fc1 "
                           "(tensor hook or second consumer); build the MLP without gelu_in for this use")


def _wgrad(dy2: Tensor, x2: Tensor, wp: Tensor) -> Tensor:
    """dW = dy2ᵀ x2 into ``wp``'s gradient slot when it has one."""
    s = take_slot(wp)
    if s is not None and not (s.dtype == dy2.dtype and s.is_contiguous()):
        s = None
    if G.supported_tn(dy2, x2):
        dw = G.mm_tn(dy2, x2, out=s)
        return slot_alias(s) if s is not None else dw

    def blas():
        if s is not None:
            torch.mm(dy2.t(), x2, out=s)
            return slot_alias(s)
        return dy2.t() @ x2

    M, K = dy2.shape
    C = x2.shape[1]
    if not (dy2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and K % 64 == 0 and C % 64 == 0
            and M >= 4096 and dy2.is_cuda):
        return blas()

    def nat():
        dy4, x4 = dy2.contiguous().view(M, K, 1, 1), x2.contiguous().view(M, C, 1, 1)
        if s is not None:
            native().conv2d_wgrad(dy4, x4, 1, 1, 1, 0, s.view(K, C, 1, 1))
            return slot_alias(s)
        return native().conv2d_wgrad(dy4, x4, 1, 1, 1, 0).view(K, C)

    from torchbooster_amd.ops.conv_route import _route

    return _route("wgrad", ("linear", M, K, C), [("hipblaslt", blas, 0.0), ("native", nat, 0.0)])


# the fused GELU-backward product on the cached transposed weight (row-read NT kernel) instead of the
# NN kernel's transposing reads (ops/flipcache.py transposed_linear_weight); TBAMD_GELU_BWD_NT=0: NN (A/B)
_GELU_BWD_NT = os.environ.get("TBAMD_GELU_BWD_NT", "1") == "1"


def _gelu_fused_dx(dy2: Tensor, w: Tensor, link: Optional[GeluLink], x_shape,
                   owner: Optional[Tensor] = None) -> Optional[Tensor]:
    """fc2's input gradient fused with fc1's GELU backward + bias gradient (GeluLink)."""
    if link is None or link.z is None or not _FUSE_GELU_BWD:
        return None
    z2 = link.z.reshape(-1, link.z.shape[-1])
    K, Q = w.shape
    if not (dy2.dtype == w.dtype == z2.dtype == torch.bfloat16 and dy2.is_cuda and K % 64 == 0 and Q % 8 == 0
            and tuple(z2.shape) == (dy2.shape[0], Q) and dy2.stride(-1) == 1 and dy2.stride(0) % 8 == 0):
        return None
    bp = link.bias
    sb = take_slot(bp) if bp is not None else None
    if sb is not None and not (sb.dtype == torch.bfloat16 and sb.is_contiguous()):
        sb = None
    wt = None
    if _GELU_BWD_NT and owner is not None:
        from torchbooster_amd.ops.flipcache import transposed_linear_weight

        wt = transposed_linear_weight(w, owner)
    dz, db = native().gemm_nn_gelu_bwd(dy2, w, z2, sb, wt)
    link.dz_ptr = dz.data_ptr()
    link.db = slot_alias(sb) if sb is not None else db.to(bp.dtype) if bp is not None else None
    return dz.view(*x_shape[:-1], Q)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, gelu_in=None):
        ctx.save_for_backward(x, w)
        ctx.params = (w, b)
        ctx.has_bias = b is not None
        ctx.gelu_in = gelu_in
        return _fwd(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        wp, bp = ctx.params
        dx = dw = db = None
        dy2 = dy.reshape(-1, dy.shape[-1])
        # under create_graph (double backward, e.g. a GAN gradient penalty) the
        # ops below are recorded: no out= writes into gradient slots then
        slots_ok = not torch.is_grad_enabled()
        if ctx.needs_input_grad[0]:
            dx = _gelu_fused_dx(dy2, w, ctx.gelu_in, x.shape, wp) if slots_ok else None
            if dx is None:
                dx = G.mm_nn(dy, w, owner=wp) if (slots_ok and G.supported_nn(dy, w)) else dy @ w
        if ctx.needs_input_grad[1]:
            x2 = x.reshape(-1, x.shape[-1])
            dw = _wgrad(dy2, x2, wp) if slots_ok else dy2.t() @ x2
        if ctx.has_bias and ctx.needs_input_grad[2]:
            s = take_slot(bp) if slots_ok else None
            if s is not None and not (s.dtype == dy.dtype and s.is_contiguous()):
                s = None
            if slots_ok and dy2.shape[-1] % 8 == 0:
                db = native().colsum(dy2, s)  # native column sum (into the slot when there is one)
                if s is not None:
                    db = slot_alias(s)
            elif s is not None:
                torch.sum(dy2, 0, out=s)
                db = slot_alias(s)
            else:
                db = dy2.sum(0)
        return dx, dw, db, None


def _fwd(x: Tensor, w: Tensor, b: Optional[Tensor]) -> Tensor:
    if G.supported_nt(x, w) and (b is None or b.dtype == torch.bfloat16):
        return G.mm_nt(x, w, b)
    return F.linear(x, w, b)


def linear(x: Tensor, w: Tensor, b: Optional[Tensor] = None, gelu_in: Optional[GeluLink] = None) -> Tensor:
    """``gelu_in``: ``x`` is the output of the ``LinearGELU`` holding this link (its sole consumer)."""
    if use_native(x) and not torch.is_autocast_enabled("cuda"):
        if torch.is_grad_enabled() and (w.requires_grad or (b is not None and b.requires_grad)
                                        or x.requires_grad):
            return _LinearFn.apply(x, w, b, gelu_in)
        return _fwd(x, w, b)
    return F.linear(x, w, b)


class Linear(nn.Linear):
    """``nn.Linear`` with slot-aware backward (see module docstring)."""

    def forward(self, x: Tensor, act: Optional[str] = None, gelu_in: Optional[GeluLink] = None) -> Tensor:
        """``act="gelu"``: exact GELU fused into this call (nativize's Linear -> GELU fusion);
        ``gelu_in``: see :class:`GeluLink`."""
        if act == "gelu":
            return linear_gelu(x, self.weight, self.bias)
        if act not in (None, "none", "identity"):
            raise ValueError(f"Linear: unsupported fused activation {act!r}")
        return linear(x, self.weight, self.bias, gelu_in)


class _LinearGELUFn(torch.autograd.Function):
    """y = GELU(x Wᵀ + b).  Forward: one native GEMM whose epilogue adds the
    bias, applies the exact GELU and also stores z (saved for backward).
    Backward: ONE native pass computes dZ = dY·GELU'(z) and the bias gradient
    Σ dZ together (csrc/colsum.hip), then the two native GEMMs."""

    @staticmethod
    def forward(ctx, x, w, b, link=None):
        if G.supported_nt(x, w) and b is not None and b.dtype == torch.bfloat16:
            y, z = G.mm_nt(x, w, b, gelu=True)  # bias + GELU in the GEMM epilogue, z saved
        else:
            z = F.linear(x, w, b)
            y = F.gelu(z)
        ctx.save_for_backward(x, w, z)
        ctx.params = (w, b)
        ctx.link = link
        if link is not None:
            link.z, link.bias, link.dz_ptr, link.db = z, b, None, None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, z = ctx.saved_tensors
        wp, bp = ctx.params
        if torch.is_grad_enabled():  # create_graph (double backward): differentiable math on the saved inputs
            zz = F.linear(x, w, bp)
            gp = 0.5 * (1.0 + torch.erf(zz * 0.7071067811865476)) + zz * torch.exp(-0.5 * zz * zz) * 0.3989422804014327
            dz = dy * gp
            dz2 = dz.reshape(-1, dz.shape[-1])
            dx = dz @ w
            dw = dz2.t() @ x.reshape(-1, x.shape[-1])
            db = dz2.sum(0) if bp is not None else None
            return dx, dw, db, None
        C = dy.shape[-1]
        fused, link_db = ctx.link.take(dy) if ctx.link is not None else (False, None)
        if ctx.link is not None:
            ctx.link.z = None
        if fused:
            # fc2's backward already applied GELU' and summed the bias gradient (GeluLink)
            dz, db = dy.reshape(-1, C), link_db
        else:
            dy2, z2 = dy.reshape(-1, C), z.reshape(-1, C)
            sb = take_slot(bp) if bp is not None else None
            if sb is not None and not (sb.dtype == z.dtype and sb.is_contiguous()):
                sb = None
            dz, db = native().gelu_bwd_colsum(dy2, z2, sb)
            if sb is not None:
                db = slot_alias(sb)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = (G.mm_nn(dz, w, owner=wp) if G.supported_nn(dz, w) else dz @ w).view(*x.shape[:-1], w.shape[1])
        if ctx.needs_input_grad[1]:
            dw = _wgrad(dz, x.reshape(-1, x.shape[-1]), wp)
        return dx, dw, (db if bp is not None and ctx.needs_input_grad[2] else None), None


def linear_gelu(x: Tensor, w: Tensor, b: Optional[Tensor] = None, link: Optional[GeluLink] = None) -> Tensor:
    """GELU(linear(x)) with the fused native backward on GPU (``link``: see :class:`GeluLink`)."""
    if use_native(x) and not torch.is_autocast_enabled("cuda") and w.shape[0] % 8 == 0:
        if torch.is_grad_enabled() and (w.requires_grad or (b is not None and b.requires_grad) or x.requires_grad):
            return _LinearGELUFn.apply(x, w, b, link)
        if G.supported_nt(x, w) and b is not None and b.dtype == torch.bfloat16:
            return G.mm_nt(x, w, b, gelu=True)[0]
    return F.gelu(F.linear(x, w, b))


class LinearGELU(nn.Linear):
    """``nn.Linear`` followed by exact GELU (state-dict compatible with ``nn.Linear``)."""

    def forward(self, x: Tensor, link: Optional[GeluLink] = None) -> Tensor:
        return linear_gelu(x, self.weight, self.bias, link)


# ---------------------------------------------------------------- few-row products (forward only)
ROWS_MAX = 16  # rows the few-row kernel takes
ROWS_MAX_K = 4096  # its reduction limit, the limit of ops.norm.layer_norm


def _rows_forward_only(*tensors: Optional[Tensor]) -> None:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError("linear_rows / embed_rows are forward-only: call them under torch.no_grad() or detach "
                           "the inputs")


MX_BLOCK = 32  # elements per MXFP4 block (one e8m0 scale byte each)
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mx_quantize(weight: Tensor) -> Tuple[Tensor, Tensor]:
    """``weight`` ``[Q, K]`` (``K % 32 == 0``) -> ``(codes, scales)`` in the OCP microscaling format MXFP4.

    ``codes`` uint8 ``[Q, K / 2]``: two e2m1 codes per byte, element ``2i`` in the low nibble of byte ``i``
    (the ``torch.float4_e2m1fn_x2`` order); a code ``c`` has sign ``c >> 3`` and magnitude
    ``(0, 0.5, 1, 1.5, 2, 3, 4, 6)[c & 7]``.  ``scales`` uint8 ``[Q, K / 32]``: one e8m0 byte ``s`` per block of
    32 consecutive elements, and an element is ``e2m1(c) * 2^(s - 127)``.

    Per block ``s = clamp(floor(log2(max|w|)) - 2 + 127, 1, 254)`` (127 for an all-zero block; the exponent
    comes from ``frexp``) and each element is ``w / 2^(s - 127)`` clamped to ``[-6, 6]`` and rounded to the
    nearest code, ties to the code with the even low bit.  Computed in f32 (f64 for f64 input).  An offline
    call: it reads one value on the host, and a non-finite ``weight`` raises ``ValueError``."""
    if weight.dim() != 2 or weight.shape[1] % MX_BLOCK or weight.shape[1] == 0:
        raise ValueError(f"mx_quantize: weight must be [Q, K] with K a multiple of {MX_BLOCK}, not "
                         f"{tuple(weight.shape)}")
    with torch.no_grad():
        Q, K = weight.shape
        w = weight.detach().to(torch.float64 if weight.dtype == torch.float64 else torch.float32)
        if not bool(torch.isfinite(w).all()):
            raise ValueError("mx_quantize: weight has a non-finite value")
        w = w.reshape(Q, K // MX_BLOCK, MX_BLOCK)
        amax = w.abs().amax(dim=-1)
        _, e = torch.frexp(amax)  # amax = m * 2^e with m in [0.5, 1): floor(log2(amax)) = e - 1
        s = (e.to(torch.int32) - 3 + 127).clamp(1, 254)
        s = torch.where(amax == 0, torch.full_like(s, 127), s)
        a = (w / torch.ldexp(torch.ones_like(amax), s - 127)[..., None]).clamp(-6.0, 6.0).abs()
        # the midpoints between neighbouring magnitudes; a tie goes to the even code
        c = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5)
             + (a > 5.0)).to(torch.uint8)
        c = (c | (torch.signbit(w).to(torch.uint8) << 3)).reshape(Q, K)
        return (c[:, 0::2] | (c[:, 1::2] << 4)).contiguous(), s.to(torch.uint8).contiguous()


def _mx_check(codes: Tensor, scales: Tensor, who: str) -> None:
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError(f"{who}: MXFP4 codes and scales are uint8, not {codes.dtype} and {scales.dtype}")
    if (codes.dim() != 2 or scales.dim() != 2 or scales.shape[0] != codes.shape[0]
            or scales.shape[1] * (MX_BLOCK // 2) != codes.shape[1]):
        raise ValueError(f"{who}: codes [Q, K / 2] and scales [Q, K / 32] do not fit: {tuple(codes.shape)} and "
                         f"{tuple(scales.shape)}")


@functools.lru_cache(maxsize=None)
def _e2m1_table(device) -> Tensor:
    """The 16 e2m1 values by code, f32 on ``device``: made once, so that a later call copies nothing from the host
    (a captured step may take a few-row fallback)."""
    return torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32, device=device)


def mx_dequantize(codes: Tensor, scales: Tensor, dtype=torch.bfloat16) -> Tensor:
    """The ``[Q, K]`` tensor an MXFP4 pair of :func:`mx_quantize` stands for, in ``dtype``: element by element
    ``e2m1(code) * f32_from_bits(scale << 23)``, which is ``2^(scale - 127)`` for a scale byte in
    ``[1, 254]`` and exact in bf16 and f32.  A scale byte 0 reads as a zero scale and 255 as ``+inf``;
    :func:`mx_quantize` emits neither."""
    _mx_check(codes, scales, "mx_dequantize")
    Q = codes.shape[0]
    table = _e2m1_table(codes.device)
    nib = torch.stack((codes & 0xF, codes >> 4), dim=-1).reshape(Q, -1, MX_BLOCK)
    scale = (scales.to(torch.int32) << 23).view(torch.float32)
    return (table[nib.long()] * scale[..., None]).reshape(Q, -1).to(dtype)


def linear_mx(x: Tensor, codes: Tensor, mx_scales: Tensor, bias: Optional[Tensor] = None, *,
              act: Optional[str] = None, residual: Optional[Tensor] = None) -> Tensor:
    """``epilogue(linear(x, dq(codes, mx_scales), bias))`` on an MXFP4 weight (:func:`mx_quantize`), for any number
    of rows: ``x`` ``[..., K]``, ``codes`` uint8 ``[Q, K / 2]``, ``mx_scales`` uint8 ``[Q, K / 32]``, ``bias`` ``[Q]`` ->
    ``[..., Q]``.  ``act="gelu"``: exact GELU; ``residual`` ``[..., Q]``: added.  Both work on the f32 accumulator,
    which is rounded once at the store; they exclude each other.  Shapes or dtypes that do not fit raise
    ``ValueError``.  Forward only.

    The native kernel (csrc/gemm_mx.hip) takes CUDA bf16 ``x`` / ``bias`` / ``residual`` with ``K % 32 == 0``, any
    number of rows and any ``Q``: the codes are decoded to bf16 in registers (``v_cvt_scalef32_pk_bf16_fp4``,
    exact) on their way into LDS and multiplied on the bf16 MFMA with f32 accumulation; the bf16 weight is never
    written to memory.  Up to 128 rows run a 64-row tile, more a 128-row tile, and a row has the same bits for
    every row count served by the same tile.  Everything else (CPU tensors, other dtypes, autocast,
    ``TBAMD_FORCE_REFERENCE=1``) is ``F.linear`` on ``mx_dequantize(codes, mx_scales, x.dtype)``, then ``F.gelu`` or
    ``+ residual``."""
    _rows_forward_only(x, bias, residual)
    if act not in (None, "gelu"):
        raise ValueError(f"linear_mx: unsupported activation {act!r}")
    if act is not None and residual is not None:
        raise ValueError("linear_mx: one epilogue, act or residual")
    _mx_check(codes, mx_scales, "linear_mx")
    K, Q = x.shape[-1], codes.shape[0]
    if codes.shape[1] * 2 != K:
        raise ValueError(f"linear_mx: MXFP4 codes {tuple(codes.shape)} do not fit x [..., {K}]")
    if bias is not None and tuple(bias.shape) != (Q,):
        raise ValueError(f"linear_mx: bias must be [{Q}], not {tuple(bias.shape)}")
    lead = x.shape[:-1]
    if residual is not None and tuple(residual.shape) != (*lead, Q):
        raise ValueError(f"linear_mx: residual must be {(*lead, Q)}, not {tuple(residual.shape)}")
    with torch.no_grad():
        bf = torch.bfloat16
        if (use_native(x) and x.dtype == bf and codes.is_cuda and mx_scales.is_cuda and K >= MX_BLOCK and Q >= 1
                and x.numel() > 0 and not torch.is_autocast_enabled("cuda")
                and (bias is None or (bias.dtype == bf and bias.is_cuda))
                and (residual is None or (residual.dtype == bf and residual.is_cuda))):
            rows = x.reshape(-1, K)
            if rows.stride(1) != 1 or rows.stride(0) % 8 or rows.stride(0) < K or rows.data_ptr() % 16:
                rows = rows.contiguous()
            res = None
            if residual is not None:
                res = residual.reshape(-1, Q)
                if res.stride(1) != 1 or res.stride(0) < Q:
                    res = res.contiguous()
            y = native().gemm_mx(rows, codes.contiguous(), mx_scales.contiguous(),
                                 None if bias is None else bias.contiguous(),
                                 1 if act == "gelu" else 2 if res is not None else 0, res)
            return y.view(*lead, Q)
        y = F.linear(x, mx_dequantize(codes, mx_scales, x.dtype), None if bias is None else bias.to(x.dtype))
        if act == "gelu":
            y = F.gelu(y)
        if residual is not None:
            y = y + residual.to(y.dtype)
        return y


def linear_rows(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, *, ln=None, act: Optional[str] = None,
                residual: Optional[Tensor] = None, rms=None, mx_scales: Optional[Tensor] = None) -> Tensor:
    """``epilogue(linear(prologue(x), weight, bias))`` for the few rows of a decode step, in ONE kernel.

    ``x`` ``[..., K]``, ``weight`` ``[Q, K]`` (the ``nn.Linear`` layout, read once), ``bias`` ``[Q]`` ->
    ``[..., Q]``.  ``ln = (gamma, beta, eps)``: LayerNorm over ``K`` first (f32 statistics; no normalised
    tensor is written).  ``act="gelu"``: exact GELU; ``residual`` ``[..., Q]``: added.  Both epilogues work
    on the f32 accumulator, which is rounded once at the store; they exclude each other.

    ``rms = (gamma, eps)``: RMSNorm over ``K`` first instead (``ops.norm.rms_norm``; exclusive with ``ln``,
    and not the same thing as ``ln=(gamma, None, eps)``, which stays LayerNorm without a bias).
    ``act="swiglu"``: ``weight`` is ``[2F, K]`` and ``bias`` ``[2F]``, the packed ``gate | up`` projection of
    ``ops.act.swiglu``, and the result is ``silu(gate) * up`` ``[..., F]`` -- both halves are accumulated in
    the same pass and paired in registers; no residual.

    The native kernel (csrc/rows_gemm.hip) takes CUDA bf16 operands with at most 16 rows, ``K % 8 == 0``
    and ``K <= 4096``; row ``m`` of its result has the same bits whether it is computed alone or among 16
    rows.  Everything else (CPU tensors, other dtypes, more rows, another ``K``,
    ``TBAMD_FORCE_REFERENCE=1``) is the PyTorch composition ``F.layer_norm`` / ``rms_norm -> F.linear ->
    F.gelu`` / ``swiglu`` / ``+ residual``, every tensor in the dtype of ``x`` (the two norms take their statistics in
    f32 for 16-bit inputs and round once).  Forward only.

    ``mx_scales``: the weight is MXFP4 (:func:`mx_quantize`): ``weight`` holds the uint8 codes ``[Q, K / 2]``
    (``[2F, K / 2]`` under ``act="swiglu"``) and ``mx_scales`` the uint8 scales ``[Q, K / 32]``; shapes or dtypes
    that do not fit raise ``ValueError``.  The native kernel (csrc/rows_gemm_mx.hip) takes the same operands
    with ``K % 32 == 0``, ``32 <= K <= 4096``, and streams 4.25 bits per weight.  More than 16 rows of CUDA bf16
    operands never dequantise the weight either: they run the norm (``ops.norm.layer_norm`` / ``rms_norm``), then
    :func:`linear_mx` (csrc/gemm_mx.hip, any ``K % 32 == 0``) with the bias / GELU / residual epilogue, then
    ``ops.act.swiglu`` under ``act="swiglu"``.  Everything else is the composition above on
    ``mx_dequantize(weight, mx_scales, x.dtype)``."""
    _rows_forward_only(x, weight, bias, residual, *((ln[0], ln[1]) if ln is not None else ()),
                       *((rms[0],) if rms is not None else ()))
    if act not in (None, "gelu", "swiglu"):
        raise ValueError(f"linear_rows: unsupported activation {act!r}")
    if act is not None and residual is not None:
        raise ValueError("linear_rows: one epilogue, act or residual")
    if ln is not None and rms is not None:
        raise ValueError("linear_rows: one prologue, ln or rms")
    glu = act == "swiglu"
    if glu and weight.shape[0] % 2:
        raise ValueError(f"linear_rows: act='swiglu' needs weight [2F, K], not {weight.shape[0]} rows")
    K, Q = x.shape[-1], weight.shape[0] // 2 if glu else weight.shape[0]
    lead = x.shape[:-1]
    if mx_scales is not None:
        _mx_check(weight, mx_scales, "linear_rows")
        if weight.shape[1] * 2 != K:
            raise ValueError(f"linear_rows: MXFP4 codes {tuple(weight.shape)} do not fit x [..., {K}]")
        _rows_forward_only(mx_scales)
    with torch.no_grad():
        rows = x.reshape(-1, K)
        M = rows.shape[0]
        bf = torch.bfloat16
        mx = mx_scales is not None
        step = MX_BLOCK if mx else 8  # the reduction comes in MX blocks or in 16-B chunks of bf16
        if (use_native(x) and x.dtype == bf and (mx or weight.dtype == bf) and weight.is_cuda
                and (not mx or mx_scales.is_cuda) and 1 <= M <= ROWS_MAX
                and K % step == 0 and step <= K <= ROWS_MAX_K and not torch.is_autocast_enabled("cuda")
                and (bias is None or bias.dtype == bf) and (residual is None or residual.dtype == bf)
                and (ln is None or (ln[0] is not None and ln[1] is not None and ln[0].dtype == torch.float32
                                    and ln[1].dtype == torch.float32))
                and (rms is None or (rms[0] is not None and rms[0].dtype == torch.float32))):
            if rows.stride(1) != 1 or (M > 1 and rows.stride(0) % 8) or rows.data_ptr() % 16:
                rows = rows.contiguous()
            res = None
            if residual is not None:
                res = residual.reshape(-1, Q)
                if res.stride(1) != 1:
                    res = res.contiguous()
            g, b, eps = (ln[0].contiguous(), ln[1].contiguous(), float(ln[2])) if ln is not None else (None, None, 0.0)
            if rms is not None:
                g, eps = rms[0].contiguous(), float(rms[1])
            epi = 3 if glu else 1 if act == "gelu" else 2 if res is not None else 0
            if mx:
                y = native().rows_linear_mx(rows, weight.contiguous(), mx_scales.contiguous(),
                                            None if bias is None else bias.contiguous(), g, b, eps, epi, res,
                                            rms=rms is not None)
            else:
                y = native().rows_linear(rows, weight.contiguous(), None if bias is None else bias.contiguous(), g, b,
                                         eps, epi, res, rms=rms is not None)
            return y.view(*lead, Q)
        if (mx and M > ROWS_MAX and use_native(x) and x.dtype == bf and weight.is_cuda and mx_scales.is_cuda
                and K >= MX_BLOCK and not torch.is_autocast_enabled("cuda") and _norm_native_ok(ln, rms)
                and (bias is None or (bias.dtype == bf and bias.is_cuda))
                and (residual is None or (residual.dtype == bf and residual.is_cuda))):
            # more rows than the few-row kernel takes: the norm, the MFMA product on the codes, the gate
            h = x
            if rms is not None:
                h = rms_norm(h, rms[0], float(rms[1]))
            if ln is not None:
                h = layer_norm(h, ln[0], ln[1], float(ln[2]))
            y = linear_mx(h, weight, mx_scales, bias, act="gelu" if act == "gelu" else None, residual=residual)
            return swiglu(y) if glu else y
        if mx:
            weight = mx_dequantize(weight, mx_scales, x.dtype)
        h = x
        if rms is not None:
            h = rms_norm(h, rms[0], float(rms[1]))
        if ln is not None:
            g, b, eps = ln
            h = F.layer_norm(h, (K,), None if g is None else g.to(h.dtype), None if b is None else b.to(h.dtype),
                             float(eps))
        y = F.linear(h, weight.to(h.dtype), None if bias is None else bias.to(h.dtype))
        if act == "gelu":
            y = F.gelu(y)
        if glu:
            y = swiglu(y)
        if residual is not None:
            y = y + residual.to(y.dtype)
        return y


def _rows_prologue(x: Tensor, ln, rms) -> Tensor:
    """The norm prologue of the few-row fallbacks, in the dtype of ``x``."""
    if rms is not None:
        x = rms_norm(x, rms[0], float(rms[1]))
    if ln is not None:
        g, b, eps = ln
        x = F.layer_norm(x, x.shape[-1:], None if g is None else g.to(x.dtype), None if b is None else b.to(x.dtype),
                         float(eps))
    return x


def _norm_native_ok(ln, rms) -> bool:
    return ((ln is None or (ln[0] is not None and ln[1] is not None and ln[0].dtype == torch.float32
                            and ln[1].dtype == torch.float32 and ln[0].is_cuda and ln[1].is_cuda))
            and (rms is None or (rms[0] is not None and rms[0].dtype == torch.float32 and rms[0].is_cuda)))


def _norm_native_args(ln, rms):
    if rms is not None:
        return rms[0].contiguous(), None, float(rms[1])
    if ln is not None:
        return ln[0].contiguous(), ln[1].contiguous(), float(ln[2])
    return None, None, 0.0


ROUTE_MAX_EXPERTS = 256  # experts the fused router takes
ROUTE_MAX_TOP_K = 16


def linear_rows_experts(x: Tensor, codes: Tensor, mx_scales: Tensor, ids: Tensor, *, ln=None, rms=None,
                        act: Optional[str] = None, gates: Optional[Tensor] = None,
                        residual: Optional[Tensor] = None) -> Tensor:
    """The few-row product of an MoE decode step: every (token, slot) pair against the MXFP4 weight of the
    expert ``ids`` names for it, in ONE kernel.  ``codes`` uint8 ``[E, Qw, K / 2]`` and ``mx_scales`` uint8
    ``[E, Qw, K / 32]`` are the stacked experts (:func:`mx_quantize` on the ``[E * Qw, K]`` view), ``ids`` int32
    ``[M, top_k]`` a device tensor the kernel reads: nothing syncs and the call is capturable.  An id outside
    ``[0, E)`` is CLAMPED into range on every path (the rule of :func:`embed_rows`).  Experts have no bias.

    Pair mode (``gates=None``): ``x`` ``[M, K]`` -> ``[M, top_k, Q]``, pair ``(m, j)`` being
    ``epilogue(prologue(x[m]) . dq(expert ids[m, j])^T)`` with the ``ln=`` / ``rms=`` prologues of
    :func:`linear_rows`; ``Qw = Q``, or ``Qw = 2F`` (``gate | up``) and ``Q = F`` under ``act="swiglu"``.  The pair
    has the bits of ``linear_rows(x[m:m+1], codes[e], mx_scales=mx_scales[e], ...)``.

    Combine mode (``gates`` f32 ``[M, top_k]``): ``x`` ``[M, top_k, K]`` -> ``[M, Q]`` with ``y[m] = residual[m] +
    sum_j gates[m, j] * (x[m, j] . dq(expert ids[m, j])^T)``: the products stay f32, are multiplied by the gates
    and added in slot order onto the f32 residual (0 without one), and rounded once.  No prologue, no ``act``.

    The native kernel (csrc/rows_experts_mx.hip) takes CUDA bf16 ``x`` / ``residual`` with ``K % 32 == 0``,
    ``32 <= K <= 4096`` and at most 16 pairs ``M * top_k``; it streams each DISTINCT expert's weight once,
    and token ``m`` has the same bits alone or among other tokens.  Everything else (CPU, other dtypes, more
    pairs, ``TBAMD_FORCE_REFERENCE=1``) is the PyTorch composition on :func:`mx_dequantize` of the experts in
    the dtype of ``x`` (each expert on every row, the named one kept: no host read either).  Shapes or dtypes
    that do not fit raise ``ValueError``.  Forward only."""
    _rows_forward_only(x, residual, gates, *((ln[0], ln[1]) if ln is not None else ()),
                       *((rms[0],) if rms is not None else ()))
    who = "linear_rows_experts"
    comb = gates is not None
    if act not in (None, "swiglu"):
        raise ValueError(f"{who}: unsupported activation {act!r}")
    if ln is not None and rms is not None:
        raise ValueError(f"{who}: one prologue, ln or rms")
    if comb and (act is not None or ln is not None or rms is not None):
        raise ValueError(f"{who}: the combine mode (gates=) takes no prologue and no act")
    if residual is not None and not comb:
        raise ValueError(f"{who}: residual belongs to the combine mode (gates=)")
    if codes.dim() != 3 or mx_scales.dim() != 3:
        raise ValueError(f"{who}: codes [E, Qw, K / 2] and scales [E, Qw, K / 32] are stacks, not "
                         f"{tuple(codes.shape)} and {tuple(mx_scales.shape)}")
    E, Qw = codes.shape[:2]
    if mx_scales.shape[0] != E or E < 1:
        raise ValueError(f"{who}: {E} experts of codes, {mx_scales.shape[0]} of scales")
    _mx_check(codes.reshape(E * Qw, codes.shape[2]), mx_scales.reshape(E * mx_scales.shape[1], mx_scales.shape[2]), who)
    K = codes.shape[2] * 2
    glu = act == "swiglu"
    if glu and Qw % 2:
        raise ValueError(f"{who}: act='swiglu' needs codes [E, 2F, K / 2], not {Qw} rows")
    Q = Qw // 2 if glu else Qw
    if ids.dim() != 2 or ids.dtype != torch.int32 or ids.shape[1] < 1:
        raise ValueError(f"{who}: ids must be int32 [M, top_k], not {ids.dtype} {tuple(ids.shape)}")
    M, top_k = ids.shape
    if tuple(x.shape) != ((M, top_k, K) if comb else (M, K)):
        raise ValueError(f"{who}: x {tuple(x.shape)} does not fit ids {tuple(ids.shape)} and K = {K}"
                         + (" (combine mode: [M, top_k, K])" if comb else " (pair mode: [M, K])"))
    if comb and (gates.dtype != torch.float32 or gates.shape != ids.shape):
        raise ValueError(f"{who}: gates must be f32 {tuple(ids.shape)}, not {gates.dtype} {tuple(gates.shape)}")
    if residual is not None and tuple(residual.shape) != (M, Q):
        raise ValueError(f"{who}: residual must be [{M}, {Q}], not {tuple(residual.shape)}")
    with torch.no_grad():
        bf = torch.bfloat16
        if (use_native(x) and x.dtype == bf and codes.is_cuda and mx_scales.is_cuda and ids.is_cuda
                and 1 <= M * top_k <= ROWS_MAX and MX_BLOCK <= K <= ROWS_MAX_K
                and not torch.is_autocast_enabled("cuda") and _norm_native_ok(ln, rms)
                and (not comb or gates.is_cuda) and (residual is None or (residual.dtype == bf and residual.is_cuda))):
            g, b, eps = _norm_native_args(ln, rms)
            res = residual if residual is None or residual.stride(1) == 1 else residual.contiguous()
            return native().rows_experts_mx(x.contiguous(), codes.contiguous(), mx_scales.contiguous(),
                                            ids.contiguous(), None if not comb else gates.contiguous(), g, b, eps,
                                            glu, res, rms=rms is not None)
        idc = ids.to(torch.int64).clamp(0, E - 1)
        h = _rows_prologue(x, ln, rms)
        out = torch.zeros(M, top_k, Q, dtype=x.dtype, device=x.device)
        for e in range(E):  # every expert on every row, the named one kept: shapes alone decide the work
            ye = F.linear(h, mx_dequantize(codes[e], mx_scales[e], x.dtype))
            if glu:
                ye = swiglu(ye)
            out = torch.where((idc == e)[:, :, None], ye if comb else ye[:, None, :], out)
        if not comb:
            return out
        acc = torch.promote_types(x.dtype, torch.float32)
        y = torch.zeros(M, Q, dtype=acc, device=x.device) if residual is None else residual.to(acc)
        for j in range(top_k):
            y = y + gates[:, j, None].to(acc) * out[:, j].to(acc)
        return y.to(x.dtype)


def moe_route_rows(x: Tensor, router_weight: Tensor, top_k: int, *, ln=None, rms=None) -> Tuple[Tensor, Tensor]:
    """The router of an MoE decode step in ONE kernel: ``x`` ``[M, K]``, ``router_weight`` ``[E, K]`` -> ``(ids``
    int32 ``[M, top_k]``, ``gates`` f32 ``[M, top_k])`` by the rule of ``models.vit.MoE.route`` on the normed row:
    ``h = prologue(x)`` in the dtype of ``x`` (``ln=`` / ``rms=`` of :func:`linear_rows`), f32 logits ``h . w^T``, the
    ``top_k`` largest in descending order with ties to the lower index, gates = the f32 softmax over those.
    Ids are always in ``[0, E)``.

    The native kernel (csrc/rows_experts_mx.hip) takes CUDA bf16 operands with ``1 <= M <= 16``, ``K % 8 == 0``,
    ``K <= 4096``, ``E <= 256`` and ``top_k <= 16``; identical router rows give bit-identical logits.  Everything
    else is the PyTorch rule: the norm, ``F.linear`` in f32, a stable descending sort, softmax.  Forward only."""
    _rows_forward_only(x, router_weight, *((ln[0], ln[1]) if ln is not None else ()),
                       *((rms[0],) if rms is not None else ()))
    if ln is not None and rms is not None:
        raise ValueError("moe_route_rows: one prologue, ln or rms")
    if x.dim() != 2 or router_weight.dim() != 2 or router_weight.shape[1] != x.shape[1]:
        raise ValueError(f"moe_route_rows: x [M, K] and router_weight [E, K] do not fit: {tuple(x.shape)} and "
                         f"{tuple(router_weight.shape)}")
    M, K = x.shape
    E = router_weight.shape[0]
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= E:
        raise ValueError(f"moe_route_rows: top_k must be an int in [1, E = {E}], not {top_k!r}")
    with torch.no_grad():
        bf = torch.bfloat16
        if (use_native(x) and x.dtype == bf and router_weight.dtype == bf and router_weight.is_cuda
                and 1 <= M <= ROWS_MAX and K % 8 == 0 and 8 <= K <= ROWS_MAX_K and E <= ROUTE_MAX_EXPERTS
                and top_k <= ROUTE_MAX_TOP_K and not torch.is_autocast_enabled("cuda") and _norm_native_ok(ln, rms)):
            rows = x
            if rows.stride(1) != 1 or (M > 1 and rows.stride(0) % 8) or rows.data_ptr() % 16:
                rows = rows.contiguous()
            g, b, eps = _norm_native_args(ln, rms)
            return native().moe_route(rows, router_weight.contiguous(), top_k, g, b, eps, rms=rms is not None)
        h = _rows_prologue(x, ln, rms)
        logits = F.linear(h.float(), router_weight.float())
        top, idx = torch.sort(logits, dim=-1, descending=True, stable=True)  # stable: ties to the lower index
        return idx[:, :top_k].to(torch.int32), torch.softmax(top[:, :top_k], dim=-1)


def embed_rows(tokens: Tensor, tok_weight: Tensor, pos_weight: Optional[Tensor] = None,
               positions: Optional[Tensor] = None) -> Tensor:
    """Token plus learned position embedding of ``tokens`` ``[B, T]`` in one kernel -> ``[B, T, dim]`` in the
    dtype of ``tok_weight`` ``[vocab, dim]``: ``tok_weight[id] + pos_weight[clamp(positions[b] + t, 0,
    max_len - 1)]`` with ``pos_weight`` ``[max_len, dim]`` and ``positions`` int ``[B]`` (zeros when None),
    summed in f32 and rounded once.  ``pos_weight=None`` (a model without learned positions): the clamped
    token row alone, bit for bit.

    The one difference from ``nn.Embedding``: a token id outside ``[0, vocab)`` is CLAMPED into range, on
    every path, instead of raising (CPU) or tripping a device-side assert (GPU) -- a bad id never becomes
    an address.  Forward only."""
    _rows_forward_only(tok_weight, pos_weight)
    if tokens.dim() != 2:
        raise RuntimeError("tokens must be [B, T]")
    B, T = tokens.shape
    if positions is not None and positions.shape != (B,):
        raise RuntimeError("positions must have shape [B]")
    with torch.no_grad():
        bf = torch.bfloat16
        if (use_native(tok_weight) and tokens.is_cuda and tok_weight.dtype == bf
                and (pos_weight is None or (pos_weight.dtype == bf and pos_weight.is_cuda))
                and tok_weight.shape[1] % 8 == 0 and B * T > 0
                and (positions is None or (positions.is_cuda and positions.dtype == torch.int32))):
            return native().embed_rows(tokens.to(torch.int64), tok_weight.contiguous(),
                                       None if pos_weight is None else pos_weight.contiguous(),
                                       None if positions is None else positions.contiguous())
        ids = tokens.to(torch.int64).clamp(0, tok_weight.shape[0] - 1)
        if pos_weight is None:
            return F.embedding(ids, tok_weight)
        at = torch.arange(T, device=tokens.device)[None, :].expand(B, T)
        if positions is not None:
            at = positions.to(torch.int64)[:, None] + at
        at = at.clamp(0, pos_weight.shape[0] - 1)
        return F.embedding(ids, tok_weight) + pos_weight[at].to(tok_weight.dtype)
