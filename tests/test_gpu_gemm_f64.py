"""The dense GEMM engine (csrc/gemm.hip, csrc/gemm8.hip, ops/gemm.py) against float64, per element.

Every (tile, orientation, epilogue, split) combination the autotuner of ops/gemm.py may time and
keep is run at the smallest shapes that reach its tails, and EVERY output element is judged on
its own against the float64 reference of tests/_gemm_ref.py (validated on the CPU by
tests/test_gemm_ref.py):

    |got - ref| <= rnd(|ref| + tau A) + tau A,   tau = 2 (K + S) 2^-24,   A = |x|.|w| + |b| + |r|

(rnd = half a bf16 ulp, the one rounding of the result; derivation in tests/_gemm_ref.py).  The
GELU output is judged against float64 GELU of the kernel's own stored z; ReLU elements within
their allowance of the kink are excluded, at most 0.1 % of a case.

Guards: every output is a view ``buf[g : g + P, :Q]`` of a sentinel-filled buffer (row stride
Q + 8, 8 guard rows above and below; epilogues with a residual or a saved pre-activation need a
contiguous output and keep the guard rows only); after the call everything outside the view must
still be the sentinel, bit for bit.  ``x`` is a view of a NaN-filled parent, so any chunk read
past K (past P for a transposed x) poisons the result.

``TBAMD_GEMM_F64_REPORT=<file>`` writes every case's largest err / allowance as JSON
(profiles/gemm_f64/README.md).
"""
import json
import os
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU collection
    pytest.skip("needs a GPU", allow_module_level=True)

from tests import _gemm_ref as R  # noqa: E402
from torchbooster_amd.ops import gemm as G  # noqa: E402
from torchbooster_amd.ops._ext import native  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
C = native()
NT = int(C.gemm_num_tiles())
SENT = 0x5A5B  # bit pattern of the guard fill (a finite bf16 no product of the inputs hits)
GUARD = 8

# Cases that need more than the derived accumulation bound because of MFMA-internal rounding:
# (case key) -> margin on tau = twice the ratio stock torch.matmul shows on the same operands,
# with both measured figures in a comment.  None needed so far.
MARGIN = {}

ORIENT = {"nt": (False, False), "nn": (False, True), "tn": (True, True), "tx_nt": (True, False)}

_RECORDS = []
_PENDING = []


@pytest.fixture(autouse=True, scope="module")
def _report():
    yield
    path = os.environ.get("TBAMD_GEMM_F64_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_RECORDS, f)


@pytest.fixture(autouse=True)
def _fresh_case():
    _PENDING.clear()


def _flush():
    """Every figure of a test is measured and recorded before it fails."""
    msgs = list(_PENDING)
    _PENDING.clear()
    assert not msgs, "\n".join(msgs[:40]) + (f"\n... {len(msgs)} failures" if len(msgs) > 40 else "")


def _note(group, case, v=None, **kw):
    rec = dict(group=group, case=repr(case), **kw)
    if v is not None:
        rec.update(y=v.y, z=v.z, excluded=v.excluded)
        if not R.verdict_ok(v):
            _PENDING.append(f"{group} {case}: {v}")
    _RECORDS.append(rec)


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events()
            if e.device_type.name == "CUDA" and any(k in e.name for k in ("gemm_k", "gemm8_k", "splitk_reduce_k"))]


# ------------------------------------------------------------------ operands, guards
def _nan_view(t):
    """``t`` ([R][C], C % 8 == 0) as a view of a NaN parent: 8 NaN columns left, 8 right, 8 NaN rows below."""
    R_, C_ = t.shape
    big = torch.full((R_ + 8, C_ + 16), float("nan"), device=DEV, dtype=BF16)
    v = big[:R_, 8:8 + C_]
    v.copy_(t)
    return v


class Guarded:
    def __init__(self, P, Q, strided=True):
        self.ld = Q + 8 if strided else Q
        self.buf = torch.empty(P + 2 * GUARD, self.ld, device=DEV, dtype=BF16)
        self.buf.view(torch.int16).fill_(SENT)
        self.out = self.buf[GUARD:GUARD + P, :Q]
        self.P, self.Q = P, Q

    def intact(self):
        b = self.buf.view(torch.int16)
        ok = bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.P:] == SENT).all())
        return ok and bool((b[:, self.Q:] == SENT).all())


@lru_cache(maxsize=None)
def _case(key, P, Q, K, tx, tw, epi=0):
    """Device operands (x behind NaNs) and the float64 reference; shared, never modified."""
    x, w, b, r = R.make_inputs(key, P, Q, K, tx, tw)
    xd = _nan_view(x.to(DEV))
    wd, bd, rd = w.to(DEV), b.to(DEV), r.to(DEV)
    ref = R.gemm_ref(xd, wd, tx, tw, bd, rd, epi)
    assert torch.isfinite(ref.y).all()
    return xd, wd, bd, rd, ref


def _run(group, case, xd, wd, bd, rd, ref, tx, tw, epi=0, tile=-1, splits=1, want_z=False, strided=True):
    P, Q = ref.y.shape
    contiguous = (not strided) or epi in R.RES_EPIS or (epi == 2 and want_z)
    g = Guarded(P, Q, not contiguous)
    outs = C.gemm(xd, wd, tw, bias=bd if epi in R.BIAS_EPIS else None, residual=rd if epi in R.RES_EPIS else None,
                  epi=epi, want_z=want_z, tile=tile, out=g.out, tx=tx, splits=splits)
    assert outs[0].data_ptr() == g.out.data_ptr()
    z = outs[1] if len(outs) > 1 else None
    assert (z is not None) == (epi == 2 and want_z)
    S = max(1, splits if splits > 0 else int(C.gemm_pick_splits(P, Q, ref.K, tile)))
    v = R.judge(ref, epi, g.out, z, S, MARGIN.get(case, 1.0))
    _note(group, case, v)
    if not g.intact():
        _PENDING.append(f"{group} {case}: wrote outside its output")
    return g.out


# ------------------------------------------------------------------ tiles x orientations x shapes
SHAPES = [(264, 264, 72), (520, 136, 200), (97, 72, 320), (8, 8, 8), (1, 8, 64), (256, 256, 64), (256, 256, 128)]
TN_ODD = [(264, 264, 203), (520, 136, 67)]  # reduction lengths that are no multiple of 8 (tx and tw only)


def _shapes(orient):
    tx, _ = ORIENT[orient]
    s = [t for t in SHAPES if not tx or t[0] % 8 == 0]
    return s + (TN_ODD if orient == "tn" else [])


def _runs_gemm8(orient, P, Q, K, strided=True):
    """Whether tile 16 takes the 8-phase kernel (csrc/gemm.hip gemm_bf16, csrc/gemm8.hip *_supported)."""
    if K < 64 or K % 64:
        return False
    if orient == "nt":
        return True
    if orient == "nn":
        return Q >= 8
    if orient == "tn":
        return not strided and P >= 8 and Q >= 8 and P % 8 == 0
    return False


@pytest.mark.parametrize("orient", list(ORIENT))
@pytest.mark.parametrize("tile", list(range(NT)))
def test_tiles_orientations(tile, orient):
    tx, tw = ORIENT[orient]
    for (P, Q, K) in _shapes(orient):
        case = ("tiles", orient, tile, P, Q, K)
        _run("tiles", case, *_case("tiles", P, Q, K, tx, tw), tx, tw, tile=tile, strided=True)
        if orient == "tn":  # the 8-phase weight-gradient kernel needs a contiguous output
            _run("tiles", case + ("contig",), *_case("tiles", P, Q, K, tx, tw), tx, tw, tile=tile, strided=False)
    _flush()


@pytest.mark.parametrize("orient", list(ORIENT))
@pytest.mark.parametrize("tile", [16, 17, 18])
def test_tile16_and_its_tail_variants_run_the_kernel_the_dispatch_says(tile, orient):
    """gemm8_k where tile 16 supports the shape, gemm_k (tile 10) where it does not; tiles 17 / 18
    have no whole round to split off at these sizes and run as tile 16 does."""
    tx, tw = ORIENT[orient]
    strided = orient != "tn"
    for want8 in (True, False):
        shapes = [s for s in _shapes(orient) if _runs_gemm8(orient, *s, strided=strided) == want8]
        if not shapes:
            continue
        outs = [Guarded(P, Q, strided) for (P, Q, K) in shapes]

        def go():
            for (P, Q, K), g in zip(shapes, outs):
                xd, wd = _case("tiles", P, Q, K, tx, tw)[:2]
                C.gemm(xd, wd, tw, tile=tile, out=g.out, tx=tx)

        names = _kernels(go)
        _note("route", (orient, tile, want8), kernels=len(names))
        assert len(names) == len(shapes), names
        assert all(("gemm8_k" in n) == want8 and ("gemm_k" in n) != want8 for n in names), (want8, shapes, names)
        for (P, Q, K), g in zip(shapes, outs):  # tile 17 / 18: bit-identical to tile 16
            xd, wd = _case("tiles", P, Q, K, tx, tw)[:2]
            g16 = Guarded(P, Q, strided)
            C.gemm(xd, wd, tw, tile=16, out=g16.out, tx=tx)
            assert torch.equal(g.out.view(torch.int16), g16.out.view(torch.int16)), (P, Q, K)


@pytest.mark.parametrize("orient", ["nt", "nn"])
@pytest.mark.parametrize("tile", [17, 18])
def test_whole_rounds_plus_tail(tile, orient):
    """516 tiles of 256 x 256: the 8-phase kernel over the rows of 512 of them, the 128 x 128 tile
    over the remaining 296 rows, whose last tile is ragged in P and Q."""
    tx, tw = ORIENT[orient]
    P, Q, K = 257 * 256 + 40, 264, 64
    x, w, _, _ = R.make_inputs(("rounds", orient), P, Q, K, tx, tw)
    xd, wd = _nan_view(x.to(DEV)), w.to(DEV)
    g = Guarded(P, Q)
    names = _kernels(lambda: C.gemm(xd, wd, tw, tile=tile, out=g.out))
    assert any("gemm8_k" in n for n in names) and any("gemm_k" in n for n in names), names
    worst = 0.0
    for p0 in range(0, P, 8192):  # the reference in row blocks
        ref = R.gemm_ref(xd[p0:p0 + 8192], wd, tx, tw)
        worst = max(worst, R.judge(ref, 0, g.out[p0:p0 + 8192]).y)
    _note("rounds", (orient, tile), R.Verdict(worst, 0.0, 0, 0))
    assert g.intact()
    _flush()


# ------------------------------------------------------------------ epilogues
@pytest.mark.parametrize("tw", [False, True])
@pytest.mark.parametrize("tile", list(range(NT)))
@pytest.mark.parametrize("epi", [1, 2, 3, 4, 6, 7])
def test_epilogues(epi, tile, tw):
    for shape in R.EPI_SHAPES[:2 if tile == 16 else 1]:
        ops = _epi_case(epi, tw, shape)
        for want_z in ((True, False) if epi == 2 else (False,)):
            _run("epi", ("epi", epi, tile, tw, shape, want_z), *ops, False, tw, epi=epi, tile=tile, want_z=want_z)
    _flush()


@lru_cache(maxsize=None)
def _epi_case(epi, tw, shape):
    x, w, b, r = R.epi_inputs(epi, tw, shape)
    xd, wd, bd, rd = _nan_view(x.to(DEV)), w.to(DEV), b.to(DEV), r.to(DEV)
    return xd, wd, bd, rd, R.gemm_ref(xd, wd, False, tw, bd, rd, epi)


def test_saved_pre_activation_needs_a_contiguous_out():
    """The kernels store z with the output's row stride into a [P][Q] allocation: refused."""
    xd, wd, bd, rd, _ = _epi_case(2, False, R.EPI_SHAPES[0])
    g = Guarded(264, 264, strided=True)
    with pytest.raises(RuntimeError, match="contiguous out"):
        C.gemm(xd, wd, False, bias=bd, epi=2, want_z=True, out=g.out)
    assert g.intact() and bool((g.out.view(torch.int16) == SENT).all())


# ------------------------------------------------------------------ split-K
SPLIT_TILES = [0, 3, 5, 8, 10, 13, 15, 16]
# K = 320 is 5 k-tiles: 3 splits of 2 leave the last one short, 4 of 2 leave split 3 empty, 16 of 1
# leave 11 empty (tile 16 TN keeps 3 of 4 and 5 of 16: gemm8_tn_splits)
SPLITS = [1, 3, 4, 16]


@pytest.mark.parametrize("orient", ["tn", "nt"])
@pytest.mark.parametrize("tile", SPLIT_TILES)
@pytest.mark.parametrize("splits", SPLITS)
def test_split_k(splits, tile, orient):
    tx, tw = ORIENT[orient]
    for (P, Q, K) in [(264, 136, 320)] + ([(264, 136, 203)] if orient == "tn" and splits == 3 else []):
        for strided in (False, True):
            _run("split", ("split", orient, tile, splits, P, Q, K, strided), *_case("split", P, Q, K, tx, tw), tx, tw,
                 tile=tile, splits=splits, strided=strided)
    _flush()


@pytest.mark.parametrize("orient", ["tn", "nt"])
def test_split_k_automatic(orient):
    tx, tw = ORIENT[orient]
    P, Q, K = 264, 136, 2048  # 32 k-tiles: gemm_pick_splits gives 4
    assert C.gemm_pick_splits(P, Q, K, 3) > 1
    for tile in (3, 16):
        _run("split", ("auto", orient, tile), *_case("auto", P, Q, K, tx, tw), tx, tw, tile=tile, splits=0)
    _flush()


def test_tile16_tn_keeps_fewer_splits_than_asked():
    P, Q, K = 264, 136, 320
    xd, wd = _case("split", P, Q, K, True, True)[:2]
    names = _kernels(lambda: C.gemm(xd, wd, True, tx=True, tile=16, splits=4))
    assert any("gemm8_k" in n for n in names) and any("splitk_reduce_k" in n for n in names), names


# ------------------------------------------------------------------ ops/gemm.py with the tuner's decision forced
OPS_SHAPES = [(40, 84, 10), (64, 120, 1), (128, 128, 64)]  # (M, K, Q): two on the pad-to-8 path, one not


def _ops_inputs(M, K, Q):
    x, w, b, _ = R.make_inputs(("ops",), M, Q, K)
    dy = torch.randn(M, Q, generator=R._gen("ops-dy", M, Q)).to(BF16)
    return x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)


def _judge_ops(group, case, got, ref, S=1):
    assert got.shape == ref.y.shape and got.dtype == BF16, (case, got.shape)
    _note(group, case, R.judge(ref, 0, got, None, S))  # (no activation in these references)


@pytest.mark.parametrize("tile", list(range(NT)))
def test_mm_nt_and_mm_nn_with_each_tile_forced(tile, monkeypatch):
    for (M, K, Q) in OPS_SHAPES:
        x, w, b, dy = _ops_inputs(M, K, Q)
        monkeypatch.setitem(G._TILE, ("nt", M, G._r8(Q), G._r8(K)), (tile, 1))
        monkeypatch.setitem(G._TILE, ("nn", M, G._r8(K), G._r8(Q)), (tile, 1))
        _judge_ops("mm_nt", (tile, M, K, Q), G.mm_nt(x, w, b), R.gemm_ref(x, w, bias=b, epi=1))
        _judge_ops("mm_nn", (tile, M, K, Q), G.mm_nn(dy, w), R.gemm_ref(dy, w, tw=True))
    _flush()


@pytest.mark.parametrize("tile", [16, 17, 18])
def test_mm_nn_on_the_cached_transposed_weight(tile, monkeypatch):
    M, K, Q = 128, 128, 64
    x, w, b, dy = _ops_inputs(M, K, Q)
    owner = torch.nn.Parameter(w.clone())
    monkeypatch.setitem(G._TILE, ("nn", M, K, Q), (G.TRANS + tile, 1))
    names = _kernels(lambda: G.mm_nn(dy, owner.data, owner=owner))
    assert any("gemm8_k" in n for n in names), names
    _judge_ops("mm_nn", ("trans", tile), G.mm_nn(dy, owner.data, owner=owner), R.gemm_ref(dy, w, tw=True))
    # the same decision without the cached transpose falls back to the NN tile
    _judge_ops("mm_nn", ("trans-no-owner", tile), G.mm_nn(dy, w), R.gemm_ref(dy, w, tw=True))
    _flush()


@pytest.mark.parametrize("tile", list(range(17)))
def test_mm_tn_with_each_tile_and_split_forced(tile, monkeypatch):
    for (M, K, Q) in OPS_SHAPES:
        x, w, b, dy = _ops_inputs(M, K, Q)
        ref = R.gemm_ref(dy, x, tx=True, tw=True)
        for splits in (1, 2, 16):
            monkeypatch.setitem(G._TILE, ("tn", G._r8(Q), G._r8(K), M), (tile, splits))
            _judge_ops("mm_tn", (tile, splits, M, K, Q), G.mm_tn(dy, x), ref, splits)
    _flush()


def test_forced_table_comes_back_through_load_tiles(tmp_path, monkeypatch):
    """The public route: a decision loaded from a JSON table is the one that runs, nothing is timed."""
    M, K, Q = 128, 128, 64
    x, w, b, dy = _ops_inputs(M, K, Q)
    monkeypatch.setattr(G, "_TILE", {})
    monkeypatch.setattr(G, "_time_ms", lambda *a, **k: pytest.fail("the tuner timed a candidate"))
    path = tmp_path / "tiles.json"
    path.write_text(json.dumps({"device": "gfx950", "tiles": [[["nt", M, Q, K], [16, 1]], [["tn", Q, K, M], [5, 4]]]}))
    assert G.load_tiles(str(path)) == 2
    names = _kernels(lambda: G.mm_nt(x, w, b))
    assert any("gemm8_k" in n for n in names), names
    _judge_ops("mm_nt", ("loaded", 16), G.mm_nt(x, w, b), R.gemm_ref(x, w, bias=b, epi=1))
    _judge_ops("mm_tn", ("loaded", 5, 4), G.mm_tn(dy, x), R.gemm_ref(dy, x, tx=True, tw=True), 4)
    _flush()


# ------------------------------------------------------------------ gemm_nn_gelu_bwd
@pytest.mark.parametrize("form", ["w", "wt"])
@pytest.mark.parametrize("P", [300, 256, 513])
@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("Q", [72, 264])
def test_gemm_nn_gelu_bwd(Q, K, P, form):
    g = R._gen("gelu_bwd", P, K, Q)
    dy = _nan_view(torch.randn(P, K, generator=g).to(BF16).to(DEV))
    w = (torch.randn(K, Q, generator=g) / K ** 0.5).to(BF16).to(DEV)
    z = (torch.randn(P, Q, generator=g) * 1.5).to(BF16).to(DEV)
    ref = R.gelu_bwd_ref(dy, w, z)
    wt = w.t().contiguous() if form == "wt" else None
    f32 = (P, K, Q) == (513, 192, 264)  # once into an f32 bias-gradient slot
    db_out = torch.full((Q,), float("nan"), device=DEV, dtype=torch.float32) if f32 else None
    dz, db = C.gemm_nn_gelu_bwd(dy, w, z, db_out, wt)
    assert dz.shape == (P, Q) and dz.dtype == BF16 and db.shape == (Q,)
    assert db.dtype == (torch.float32 if f32 else BF16) and (not f32 or db.data_ptr() == db_out.data_ptr())
    a_dz, a_db = R.gelu_bwd_allowances(ref, f32)
    r_dz, r_db = R.err_ratio(dz, ref.dz, a_dz).max().item(), R.err_ratio(db, ref.db, a_db).max().item()
    _note("gelu_bwd", (form, P, K, Q), R.Verdict(r_dz, 0.0, 0, 0), db=r_db)
    if r_db > 1.0:
        _PENDING.append(f"gelu_bwd db {(form, P, K, Q)}: {r_db}")
    _flush()
