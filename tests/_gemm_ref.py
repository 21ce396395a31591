"""Plain float64 reference of the dense GEMM binding (csrc/bind_gemm.cpp ``gemm`` and
``gemm_nn_gelu_bwd``) and the per-element error allowance the GPU sweep
(tests/test_gpu_gemm_f64.py) judges the HIP kernels with.  Validated on the CPU by
tests/test_gemm_ref.py.

The inputs are the bf16 values the kernel sees, taken as float64, on whatever device they live.

Allowance of one output element:  ``|got - ref| <= rnd(|ref| + tau A) + tau A``

  rnd(v) = half a bf16 ulp of v = 2^(floor(log2 v) - 8): the single bf16 rounding of the result.
           It lies between 2^-9 v and 2^-8 v.  (u |ref| with u = 2^-9 is the AVERAGE of that
           rounding, not its bound: round-to-nearest of 1.0039 = 1 + 2^-8 to 8 significant bits
           is off by 2^-8, so a correct kernel misses u |ref| on about a quarter of its elements;
           tests/test_gemm_ref.py pins both facts.)  Taken of |ref| + tau A, the largest value
           the unrounded sum may have, so a binade boundary between the two cannot matter.
  tau = 2 (K + S) 2^-24      the standard-model bound of an f32 accumulation over K terms and S
                             split-K partials, doubled
  A   = |x| . |w| + |bias| + |residual|   the magnitude sum of the element's terms
"""
from __future__ import annotations

import math
import zlib
from typing import NamedTuple, Optional

import torch
from torch import Tensor

U_BF16 = 2.0 ** -9  # mean relative bf16 rounding; the bound is half_ulp_bf16 below
U_F32 = 2.0 ** -24
EPIS = (0, 1, 2, 3, 4, 6, 7)
BIAS_EPIS = (1, 2, 3, 6)
RES_EPIS = (3, 4)
RELU_EPIS = (6, 7)
GELU_GRAD_MAX = 1.13   # max |GELU'| = 1.1289 (at z = sqrt 2)
GELU_ABS = 2.0 ** -20  # absolute slack of the kernels' erf approximation (|error| <= 1.5e-7)


def gelu(z: Tensor) -> Tensor:
    return 0.5 * z * (1.0 + torch.erf(z * math.sqrt(0.5)))


def gelu_grad(z: Tensor) -> Tensor:
    return 0.5 * (1.0 + torch.erf(z * math.sqrt(0.5))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


class GemmRef(NamedTuple):
    z: Tensor  # pre-activation [P][Q]
    y: Tensor  # output
    A: Tensor  # magnitude sum
    K: int     # reduction length


def gemm_ref(x: Tensor, w: Tensor, tx: bool = False, tw: bool = False, bias: Optional[Tensor] = None,
             residual: Optional[Tensor] = None, epi: int = 0) -> GemmRef:
    """x [P][K] ([K][P] with tx), w [Q][K] ([K][Q] with tw); the epilogue code decides which of
    bias / residual enter (as in the kernels)."""
    assert epi in EPIS, epi
    xm = x.double().t() if tx else x.double()
    wm = w.double() if tw else w.double().t()
    assert xm.shape[1] == wm.shape[0], (xm.shape, wm.shape)
    z = xm @ wm
    A = xm.abs() @ wm.abs()
    if epi in BIAS_EPIS:
        z = z + bias.double()
        A = A + bias.double().abs()
    if epi in RES_EPIS:
        z = z + residual.double()
        A = A + residual.double().abs()
    if epi == 2:
        y = gelu(z)
    elif epi in RELU_EPIS:
        y = z.clamp_min(0.0)
    else:
        y = z
    return GemmRef(z, y, A, int(xm.shape[1]))


def tau(K: int, S: int = 1) -> float:
    return 2.0 * (K + S) * U_F32


def half_ulp_bf16(v: Tensor) -> Tensor:
    """Largest round-to-nearest error of a bf16 (8 significant bits) result of magnitude v >= 0."""
    _, e = torch.frexp(v)  # v = m 2^e, 0.5 <= m < 1
    h = torch.ldexp(torch.ones_like(v), e - 9)
    return torch.where(v > 0, h, torch.zeros_like(v))


def allowance(ref: Tensor, A: Tensor, K: int, S: int = 1, scale: float = 1.0) -> Tensor:
    acc = scale * tau(K, S) * A
    return half_ulp_bf16(ref.abs() + acc) + acc


def err_ratio(got: Tensor, ref: Tensor, allow: Tensor) -> Tensor:
    """|got - ref| / allow per element; inf where got is not finite or misses a zero allowance."""
    err = (got.double() - ref).abs()
    r = err / allow.clamp_min(1e-300)
    r = torch.where((allow == 0) & (err == 0), torch.zeros_like(r), r)
    return torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))


def gelu_of_stored_z_allowance(z_stored: Tensor) -> Tensor:
    """y = bf16(GELU(stored z)): one rounding + the erf approximation."""
    return half_ulp_bf16(gelu(z_stored.double()).abs() + GELU_ABS) + GELU_ABS


def relu_keep(z: Tensor, A: Tensor, K: int, S: int = 1) -> Tensor:
    """Elements far enough from the ReLU kink to be judged."""
    return z.abs() >= allowance(z, A, K, S)


def relu_cap(n: int) -> int:
    return 2 if n < 2000 else n // 1000


class Verdict(NamedTuple):
    y: float       # largest err / allowance of the output (1.0 = at the bound)
    z: float       # the same of the stored pre-activation (0.0 where there is none)
    excluded: int  # ReLU elements too close to the kink to judge
    cap: int       # how many may be


def judge(ref: GemmRef, epi: int, got_y: Tensor, got_z: Optional[Tensor] = None, S: int = 1,
          margin: float = 1.0) -> Verdict:
    """The metric of the sweep for one call; ``margin`` scales the accumulation term only
    (a case listed with a measured margin)."""
    a = allowance(ref.y, ref.A, ref.K, S, margin)
    if epi == 2 and got_z is not None:
        rz = err_ratio(got_z, ref.z, allowance(ref.z, ref.A, ref.K, S, margin)).max().item()
        zs = got_z.double()
        ry = err_ratio(got_y, gelu(zs), gelu_of_stored_z_allowance(zs)).max().item()
        return Verdict(ry, rz, 0, 0)
    if epi == 2:
        # GELU of the kernel's rounded z, which is within the z allowance of ref.z
        az = GELU_GRAD_MAX * allowance(ref.z, ref.A, ref.K, S, margin) + GELU_ABS
        az = az + half_ulp_bf16(ref.y.abs() + az)
        return Verdict(err_ratio(got_y, ref.y, az).max().item(), 0.0, 0, 0)
    r = err_ratio(got_y, ref.y, a)
    if epi in RELU_EPIS:
        keep = relu_keep(ref.z, ref.A, ref.K, S)
        n_ex = int((~keep).sum().item())
        r = torch.where(keep, r, torch.where(torch.isfinite(got_y.double()), torch.zeros_like(r), r))
        return Verdict(r.max().item(), 0.0, n_ex, relu_cap(ref.z.numel()))
    return Verdict(r.max().item(), 0.0, 0, 0)


def verdict_ok(v: Verdict) -> bool:
    return v.y <= 1.0 and v.z <= 1.0 and v.excluded <= v.cap


class GeluBwdRef(NamedTuple):
    dz: Tensor   # (dy w) * GELU'(z)
    db: Tensor   # column sums of dz
    A: Tensor    # |dy| . |w|
    K: int


def gelu_bwd_ref(dy: Tensor, w: Tensor, z: Tensor) -> GeluBwdRef:
    """dy [P][K], w [K][Q], z [P][Q]."""
    g = dy.double() @ w.double()
    A = dy.double().abs() @ w.double().abs()
    dz = g * gelu_grad(z.double())
    return GeluBwdRef(dz, dz.sum(0), A, int(dy.shape[1]))


def gelu_bwd_allowances(r: GeluBwdRef, db_f32: bool = False):
    """(per element of dz, per column of db): the product's allowance times max |GELU'| plus the
    rounding of dz; the column's P element allowances plus the rounding to db's dtype."""
    acc = GELU_GRAD_MAX * tau(r.K) * r.A
    a_dz = half_ulp_bf16(r.dz.abs() + acc) + acc
    s = a_dz.sum(0)
    a_db = s + (U_F32 * (r.db.abs() + s) if db_f32 else half_ulp_bf16(r.db.abs() + s))
    return a_dz, a_db


# ---------------------------------------------------------------- inputs (CPU, deterministic)
def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def make_inputs(key, P: int, Q: int, K: int, tx: bool = False, tw: bool = False):
    """bf16 operands in the layout the binding takes, plus a bias and a residual.  Unit-variance
    products: z ~ N(0, 1) before bias / residual, so a ReLU kink is rarely within the allowance."""
    g = _gen(key, P, Q, K, tx, tw)
    x = torch.randn(P, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(Q, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    b = torch.randn(Q, generator=g).to(torch.bfloat16)
    r = torch.randn(P, Q, generator=g).to(torch.bfloat16)
    return (x.t().contiguous() if tx else x), (w.t().contiguous() if tw else w), b, r


# ---------------------------------------------------------------- f32 / bf16 emulation (CPU)
def _gelu_f32(z: Tensor) -> Tensor:
    return (0.5 * z * (1.0 + torch.erf(z * math.sqrt(0.5)))).float()


def emulate(x: Tensor, w: Tensor, tx: bool = False, tw: bool = False, bias: Optional[Tensor] = None,
            residual: Optional[Tensor] = None, epi: int = 0, splits: int = 1, want_z: bool = True):
    """What a correct kernel returns: f32 products accumulated per split over 64-wide k-tiles,
    partials combined in f32, the epilogue in f32, one bf16 rounding (two for the GELU output,
    which is taken of the stored z).  Returns (y, z or None) in bf16."""
    xm = x.float().t() if tx else x.float()
    wm = w.float() if tw else w.float().t()
    K = xm.shape[1]
    KT = (K + 63) // 64
    kts = (KT + splits - 1) // splits
    acc = torch.zeros(xm.shape[0], wm.shape[1])
    for s in range(splits):
        part = torch.zeros_like(acc)
        for kt in range(s * kts, min(KT, (s + 1) * kts)):
            part = part + xm[:, 64 * kt:64 * kt + 64] @ wm[64 * kt:64 * kt + 64]
        acc = acc + part
    if epi in BIAS_EPIS:
        acc = acc + bias.float()
    if epi in RES_EPIS:
        acc = acc + residual.float()
    if epi == 2:
        z = acc.to(torch.bfloat16)
        return _gelu_f32(z.float()).to(torch.bfloat16), (z if want_z else None)
    if epi in RELU_EPIS:
        acc = acc.clamp_min(0.0)
    return acc.to(torch.bfloat16), None


# ---------------------------------------------------------------- cases shared by the CPU and GPU tests
EPI_SHAPES = [(264, 264, 72), (264, 264, 128)]


def epi_inputs(epi: int, tw: bool, shape):
    """The operands of the sweep's epilogue cases (tests/test_gemm_ref.py checks their ReLU cap)."""
    return make_inputs(("epi", epi), *shape, False, tw)
