"""The float64 GEMM reference and its error allowance (tests/_gemm_ref.py), on the CPU.

The reference is checked against explicit loops and against torch's own GELU; the allowance must
accept what a correct kernel produces (f32 accumulation per k-tile and split, one bf16 rounding)
and must reject each subtle corruption the GPU sweep (tests/test_gpu_gemm_f64.py) exists to catch:
a dropped k element, a bias or residual displaced by one element or one store quad, one wrong
element, one wrong quad at the Q tail."""
import pytest
import torch
import torch.nn.functional as F

from tests import _gemm_ref as R

F64 = torch.float64


def _loops(x, w, tx, tw, bias, res, epi):
    P = x.shape[1] if tx else x.shape[0]
    K = x.shape[0] if tx else x.shape[1]
    Q = w.shape[1] if tw else w.shape[0]
    z, A = torch.zeros(P, Q, dtype=F64), torch.zeros(P, Q, dtype=F64)
    for p in range(P):
        for q in range(Q):
            for k in range(K):
                xv = float(x[k, p] if tx else x[p, k])
                wv = float(w[k, q] if tw else w[q, k])
                z[p, q] += xv * wv
                A[p, q] += abs(xv * wv)
            if epi in (1, 2, 3, 6):
                z[p, q] += float(bias[q])
                A[p, q] += abs(float(bias[q]))
            if epi in (3, 4):
                z[p, q] += float(res[p, q])
                A[p, q] += abs(float(res[p, q]))
    return z, A


@pytest.mark.parametrize("tx", [False, True])
@pytest.mark.parametrize("tw", [False, True])
@pytest.mark.parametrize("epi", R.EPIS)
def test_reference_matches_explicit_loops(tx, tw, epi):
    x, w, b, r = R.make_inputs(("loops", epi), 5, 4, 7, tx, tw)
    assert x.shape == ((7, 5) if tx else (5, 7)) and w.shape == ((7, 4) if tw else (4, 7))
    ref = R.gemm_ref(x, w, tx, tw, b, r, epi)
    z, A = _loops(x, w, tx, tw, b, r, epi)
    assert ref.K == 7
    assert (ref.z - z).abs().max() < 1e-13 and (ref.A - A).abs().max() < 1e-13
    y = F.gelu(z) if epi == 2 else (z.clamp_min(0) if epi in (6, 7) else z)
    assert (ref.y - y).abs().max() < 1e-13


def test_gelu_closed_forms_match_torch():
    z = torch.linspace(-9, 9, 4001, dtype=F64).requires_grad_()
    y = F.gelu(z)
    (g,) = torch.autograd.grad(y.sum(), z)
    assert (R.gelu(z.detach()) - y.detach()).abs().max() < 1e-14
    assert (R.gelu_grad(z.detach()) - g).abs().max() < 1e-14
    assert R.gelu_grad(z.detach()).abs().max() <= R.GELU_GRAD_MAX


def test_gelu_bwd_reference_matches_autograd():
    g = R._gen("gelu_bwd")
    dy = torch.randn(9, 16, generator=g).to(torch.bfloat16)
    w = torch.randn(16, 8, generator=g).to(torch.bfloat16)
    z = torch.randn(9, 8, generator=g).to(torch.bfloat16)
    r = R.gelu_bwd_ref(dy, w, z)
    zl = z.double().requires_grad_()
    (dz,) = torch.autograd.grad(F.gelu(zl), zl, dy.double() @ w.double())
    assert (r.dz - dz).abs().max() < 1e-13 and (r.db - dz.sum(0)).abs().max() < 1e-12
    a_dz, a_db = R.gelu_bwd_allowances(r)
    got = (((dy.float() @ w.float()) * R.gelu_grad(z.float())).to(torch.bfloat16))
    assert R.err_ratio(got, r.dz, a_dz).max() <= 1.0
    assert R.err_ratio(got.float().sum(0).to(torch.bfloat16), r.db, a_db).max() <= 1.0
    bad = got.clone()
    bad[4, 3] = bad[4, 2]
    assert R.err_ratio(bad, r.dz, a_dz).max() > 1.0


CASES = [(264, 264, 72), (97, 72, 320), (8, 8, 8), (1, 8, 64)]


@pytest.mark.parametrize("epi,splits", [(e, 1) for e in R.EPIS] + [(0, 3), (0, 4), (0, 16)])  # (split-K: no epilogue)
@pytest.mark.parametrize("tx,tw", [(False, False), (False, True), (True, True), (True, False)])
def test_allowance_accepts_a_correct_kernel(epi, tx, tw, splits):
    for (P, Q, K) in CASES:
        if tx and P % 8:
            continue
        x, w, b, r = R.make_inputs(("accept", epi), P, Q, K, tx, tw)
        ref = R.gemm_ref(x, w, tx, tw, b, r, epi)
        for want_z in ((True, False) if epi == 2 else (False,)):
            y, z = R.emulate(x, w, tx, tw, b, r, epi, splits, want_z)
            v = R.judge(ref, epi, y, z, splits)
            assert R.verdict_ok(v), (P, Q, K, want_z, v)


def test_allowance_accepts_odd_reduction_lengths():
    for K in (203, 67):
        x, w, b, r = R.make_inputs(("odd",), 264, 136, K, True, True)
        ref = R.gemm_ref(x, w, True, True)
        assert ref.K == K
        assert R.verdict_ok(R.judge(ref, 0, R.emulate(x, w, True, True, splits=3)[0], None, 3))


def _bad_outputs(x, w, tw, b, r, epi):
    """name -> (y, z) of a kernel that is wrong in one of the ways the sweep must catch."""
    P, Q = r.shape
    out = {}
    # the last k element dropped (a K tail read one chunk short would drop 8)
    xs, ws = x.clone(), w
    xs[:, -1] = 0
    out["dropped_k"] = R.emulate(xs, ws, False, tw, b, r, epi)
    if epi in R.BIAS_EPIS:
        out["bias_shifted_1"] = R.emulate(x, w, False, tw, torch.roll(b, 1), r, epi)
        out["bias_shifted_4"] = R.emulate(x, w, False, tw, torch.roll(b, 4), r, epi)
        bq = b.clone()  # one quad of the last column tile takes its neighbour's bias
        bq[Q - 4:] = b[Q - 8:Q - 4]
        out["bias_quad_last_tile"] = R.emulate(x, w, False, tw, bq, r, epi)
    if epi in R.RES_EPIS:
        out["residual_shifted_1"] = R.emulate(x, w, False, tw, b, torch.roll(r, 1, 1), epi)
        rr = r.clone()
        rr[P - 1, Q - 1] = r[P - 1, Q - 2]
        out["residual_one_element"] = R.emulate(x, w, False, tw, b, rr, epi)
    y, z = R.emulate(x, w, False, tw, b, r, epi)
    # one wrong element: every row and column holds a judged one (ReLU zeros and kink elements are not)
    y1, z1 = y.clone(), None if z is None else z.clone()
    p, q = (y.float().abs() > 0.25).nonzero()[-1].tolist()
    y1[p, q] = y[p, q] * 1.02
    if z1 is not None:
        z1[p, q] = z[p, q] * 1.02
    out["one_element"] = (y1, z1)
    # one 4-wide store quad at the Q tail displaced by a row
    y4, z4 = y.clone(), None if z is None else z.clone()
    y4[P - 1, Q - 4:] = y[P - 2, Q - 4:]
    if z4 is not None:
        z4[P - 1, Q - 4:] = z[P - 2, Q - 4:]
    out["quad_at_q_tail"] = (y4, z4)
    return out


@pytest.mark.parametrize("epi", R.EPIS)
@pytest.mark.parametrize("tw", [False, True])
def test_allowance_rejects_each_corruption(epi, tw):
    P, Q, K = 1000, 384, 320  # the shape at which a whole-tensor relative L2 of 1e-2 passes all of these
    x, w, b, r = R.make_inputs(("reject", epi), P, Q, K, False, tw)
    ref = R.gemm_ref(x, w, False, tw, b, r, epi)
    good = R.emulate(x, w, False, tw, b, r, epi)
    assert R.verdict_ok(R.judge(ref, epi, *good))
    for name, (y, z) in _bad_outputs(x, w, tw, b, r, epi).items():
        v = R.judge(ref, epi, y, z)
        assert not R.verdict_ok(v), (name, v)
        if epi == 2:  # without the stored z the output alone must give it away
            v = R.judge(ref, epi, y, None)
            assert not R.verdict_ok(v), (name, "want_z=False", v)


def test_a_dropped_k_element_is_far_outside_the_allowance():
    """~A/K against tau A = 2 (K + 1) 2^-24 A: two orders of magnitude at K = 320."""
    x, w, b, r = R.make_inputs(("scale",), 97, 72, 320)
    ref = R.gemm_ref(x, w)
    xs = x.clone()
    xs[:, -1] = 0
    ratio = R.err_ratio(R.emulate(xs, w)[0], ref.y, R.allowance(ref.y, ref.A, ref.K))
    assert ratio.median() > 1.0 and ratio.max() > 10.0


@pytest.mark.parametrize("epi", R.RELU_EPIS)
@pytest.mark.parametrize("tw", [False, True])
@pytest.mark.parametrize("shape", R.EPI_SHAPES)
def test_relu_cases_of_the_sweep_meet_the_exclusion_cap(epi, tw, shape):
    """The reference alone: at most 0.1 % of a case's elements lie within their allowance of the kink."""
    x, w, b, r = R.epi_inputs(epi, tw, shape)
    ref = R.gemm_ref(x, w, False, tw, b, r, epi)
    n_ex = int((~R.relu_keep(ref.z, ref.A, ref.K)).sum())
    assert n_ex <= R.relu_cap(ref.z.numel()), (n_ex, ref.z.numel())


def test_one_bf16_rounding_is_half_an_ulp_not_two_to_the_minus_nine():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.99, 2.0, 0.75, 3e-5, 0.0], dtype=F64)
    h = R.half_ulp_bf16(v)
    assert h.tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -24, 0.0]
    assert ((h >= R.U_BF16 * v) & (h <= 2 * R.U_BF16 * v)).all()
    # it is attained: 1 + 2^-8 + eps rounds to 1 + 2^-7, u |ref| with u = 2^-9 would refuse a correct rounding
    x = torch.tensor(1.0 + 2.0 ** -8 + 2.0 ** -20, dtype=F64)
    err = (x.to(torch.bfloat16).double() - x).abs()
    assert R.U_BF16 * x < err <= R.half_ulp_bf16(x)
    # and a correct kernel's output misses u |ref| on a good part of its elements
    xx, w, b, r = R.make_inputs(("u",), 97, 72, 320)
    ref = R.gemm_ref(xx, w)
    miss = ((R.emulate(xx, w)[0].double() - ref.y).abs() > R.U_BF16 * ref.y.abs() + R.tau(320) * ref.A).double().mean()
    assert miss > 0.05


def test_relu_cap_and_nonfinite_outputs():
    assert R.relu_cap(1999) == 2 and R.relu_cap(2000) == 2 and R.relu_cap(70000) == 70
    x, w, b, r = R.make_inputs(("nan",), 8, 8, 8)
    ref = R.gemm_ref(x, w)
    y = R.emulate(x, w)[0]
    y[3, 3] = float("nan")
    assert not R.verdict_ok(R.judge(ref, 0, y))
    assert not R.verdict_ok(R.Verdict(0.5, 0.0, 3, 2))  # too many elements at the kink is a failure
