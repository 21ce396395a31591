"""The route autotuner's decision logic (ops/conv_route.py) on fake candidates whose "time" is the
value they return: no GPU needed."""
import pytest
import torch

from torchbooster_amd.ops import conv_route as RT

KEY = ("test_conv_route", 7, 11, 13)  # no shipped row has it


def _cands(native=2.0, miopen=0.1):
    return [("native", lambda: native, 0.0), ("im2col", lambda: 1.0, 0.5), ("splitk", lambda: 1.2, 0.0),
            ("miopen", lambda: miopen, 0.0)]


@pytest.fixture(autouse=True)
def _fake_timer(monkeypatch):
    monkeypatch.setattr(RT, "_time_ms", lambda fn, reps=3: fn())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(RT, "_AUTOTUNE", True)
    monkeypatch.setattr(RT, "_NO_MIOPEN", True)
    monkeypatch.setattr(RT, "_RETIME", ())
    for d in ("fwd", "dgrad", "wgrad"):
        monkeypatch.setitem(RT._FORCE, d, "")
    yield
    for d in ("fwd", "dgrad", "wgrad"):
        RT._CHOICE.pop((d,) + KEY, None)


def test_default_excludes_miopen_counts_penalty_and_stores():
    assert RT._route_choice("fwd", KEY, _cands()) == "splitk"
    assert RT._CHOICE[("fwd",) + KEY] == "splitk"
    assert RT._route("fwd", KEY, _cands()) == 1.2  # runs the stored choice


def test_failing_candidate_drops_out():
    def boom():
        raise RuntimeError("cannot run this shape")

    assert RT._route_choice("fwd", KEY, [("native", boom, 0.0), ("gemm", lambda: 3.0, 0.0)]) == "gemm"


def test_miopen_is_a_candidate_when_allowed(monkeypatch):
    monkeypatch.setattr(RT, "_NO_MIOPEN", False)
    assert RT._route_choice("fwd", KEY, _cands()) == "miopen"


@pytest.mark.parametrize("mio,want", [(0.96, "native"), (0.9, "miopen")])
def test_miopen_margin(monkeypatch, mio, want):
    """MIOpen must beat the best native time by 5 % + 0.005 ms (the module's defaults)."""
    monkeypatch.setattr(RT, "_NO_MIOPEN", False)
    assert (RT._MIOPEN_MARGIN, RT._MIOPEN_MARGIN_MS) == (0.05, 0.005)
    assert RT._route_choice("fwd", KEY, _cands(native=1.0, miopen=mio)) == want


def test_deterministic_mode_excludes_miopen(monkeypatch):
    monkeypatch.setattr(RT, "_NO_MIOPEN", False)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        assert RT._route_choice("fwd", KEY, _cands()) == "splitk"
    finally:
        torch.use_deterministic_algorithms(was)


def test_stored_route_absent_from_candidates_is_retuned():
    RT._CHOICE[("fwd",) + KEY] = "tinyc"
    assert RT._route_choice("fwd", KEY, _cands()) == "splitk"
    assert RT._CHOICE[("fwd",) + KEY] == "splitk"


def test_forced_direction_stores_nothing(monkeypatch):
    monkeypatch.setitem(RT._FORCE, "fwd", "native")
    assert RT._route_choice("fwd", KEY, _cands()) == "native"
    assert ("fwd",) + KEY not in RT._CHOICE


def test_autotune_off_takes_the_first_candidate(monkeypatch):
    monkeypatch.setattr(RT, "_AUTOTUNE", False)
    assert RT._route_choice("fwd", KEY, _cands()) == "native"
    assert ("fwd",) + KEY not in RT._CHOICE
