"""Per-shape route autotuner of the conv (and Linear weight-gradient) dispatchers.

``_route(direction, key, cands)`` runs one of ``cands`` [(name, fn, penalty_ms)].  The choice is made
per (direction, key) the first time a shape is seen (like ``cudnn.benchmark``: the candidates are
timed with HIP events, the fastest is kept -- see :func:`autotune_table`) or comes from the shipped
table ``conv_routes_gfx950.json`` (:func:`load_routes`).  ``TBAMD_CONV_AUTOTUNE=0`` always takes the
first candidate; ``TBAMD_CONV_{FWD,DGRAD,WGRAD}=name`` pins one direction; ``TBAMD_NATIVE_CONV=0``
disables the native conv paths entirely (ops/conv.py reads it from here).

The flags below are this module's globals, read at call time: tests and tools that change one
(``_DISABLE``, ``_AUTOTUNE``, ``_NO_MIOPEN``) set it HERE, and no other module keeps a copy.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Tuple

import torch

from torchbooster_amd.ops import _agree

_DISABLE = os.environ.get("TBAMD_NATIVE_CONV", "1") == "0"
_AUTOTUNE = os.environ.get("TBAMD_CONV_AUTOTUNE", "1") != "0"
# one stderr line per autotune decision (long first steps then show progress)
_TUNE_LOG = os.environ.get("TBAMD_TUNE_LOG", "0") == "1"
_FORCE = {d: os.environ.get(f"TBAMD_CONV_{d.upper()}", "") for d in ("fwd", "dgrad", "wgrad")}
# TBAMD_CONV_NO_MIOPEN (default 1): never route a conv direction to MIOpen -- every shape has a
# native candidate (implicit GEMM, the phase-class strided input gradient, the generic / narrow /
# tiny-channel families, im2col + GEMM), and no first-use MIOpen find is paid.  0: MIOpen is a
# timed candidate again (taken only where it is clearly faster, _MIOPEN_MARGIN).
_NO_MIOPEN = os.environ.get("TBAMD_CONV_NO_MIOPEN", "1") == "1"
_MIOPEN_MARGIN = float(os.environ.get("TBAMD_CONV_MIOPEN_MARGIN", "0.05"))
_MIOPEN_MARGIN_MS = float(os.environ.get("TBAMD_CONV_MIOPEN_MARGIN_MS", "0.005"))
# tuning aid: TBAMD_CONV_RETIME=name,name,... re-times every decided route that has one of these
# candidates against them (kept only where one is faster by 3 %); with TBAMD_CONV_SAVE it writes the
# table to merge (scripts/merge_routes.py)
_RETIME = tuple(n for n in os.environ.get("TBAMD_CONV_RETIME", "").split(",") if n)
_RETIMED: set = set()

_CHOICE: Dict[tuple, str] = {}

# every route a table row may name (_route_choice candidates)
_ROUTE_NAMES = ("native", "miopen", "gemm", "native64", "narrow", "tinyc", "im2col", "split32", "narrow32", "tiny32",
                "tinyhalo", "splitk", "tinyin", "big256x256", "big256x128", "big128x256", "big128x128",
                "big256x256m32", "big256x128m32", "big128x256m32", "big128x128m32")

Cands = List[Tuple[str, Callable[[], object], float]]


def _tuplify(v):
    return tuple(_tuplify(x) for x in v) if isinstance(v, list) else v


def _listify(v):
    return [_listify(x) for x in v] if isinstance(v, tuple) else v


def load_routes(path: Optional[str] = None) -> int:
    """Seed the autotune table from a routes file (like a cuDNN/MIOpen find-db:
    decisions measured once on this GPU model, so a fresh process does not pay
    ~3 minutes of first-step timing — mostly MIOpen find of the losing
    candidates).  ``TBAMD_CONV_ROUTES`` overrides the shipped gfx950 file;
    ``TBAMD_CONV_ROUTES=none`` disables it.  Returns the number of routes."""
    import json

    path = path or os.environ.get("TBAMD_CONV_ROUTES") or os.path.join(os.path.dirname(__file__),
                                                                        "conv_routes_gfx950.json")
    if path == "none" or not os.path.exists(path):
        return 0
    with open(path) as f:
        data = json.load(f)
    n = 0
    for key, name in data.get("routes", []):
        if name in _ROUTE_NAMES:
            _CHOICE.setdefault(_tuplify(key), name)
            n += 1
    return n


def save_routes(path: str) -> None:
    """Write the current autotune table in :func:`load_routes` format."""
    import json

    rows = [json.dumps([list(_listify(k)), v]) for k, v in sorted(_CHOICE.items(), key=str)]
    with open(path, "w") as f:
        f.write('{\n"device": "gfx950",\n"routes": [\n' + ",\n".join(rows) + "\n]}\n")


def autotune_table() -> Dict[tuple, str]:
    """(direction, shapes...) -> route name decided so far."""
    return dict(_CHOICE)


if _AUTOTUNE and not _DISABLE:
    load_routes()

if os.environ.get("TBAMD_CONV_SAVE"):
    # collect this process's decisions for the shipped table (scripts/merge_routes.py)
    import atexit

    atexit.register(lambda: _CHOICE and save_routes(os.environ["TBAMD_CONV_SAVE"]))


def _time_ms(fn: Callable[[], object], reps: int = 3) -> float:
    fn()  # warm (MIOpen runs its own find on first use)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def _route(direction: str, key: tuple, cands: Cands):
    """Run the chosen candidate of ``cands`` [(name, fn, penalty_ms)]; the first
    candidate is the default when autotuning is off or impossible."""
    name = _route_choice(direction, key, cands)
    for n, fn, _ in cands:
        if n == name:
            return fn()
    raise RuntimeError(f"conv route {name} vanished")  # pragma: no cover


def _eligible(cands: Cands) -> Cands:
    """``cands`` without MIOpen where it is excluded (never the last candidate standing).
    Deterministic mode (utils.seed / torch.use_deterministic_algorithms): MIOpen's split-K
    solvers accumulate with float atomics (bitwise run-to-run differences on the few-pixel
    shapes they win), every native route is fixed-order -- so native only."""
    if (_NO_MIOPEN or torch.are_deterministic_algorithms_enabled()) and any(c[0] != "miopen" for c in cands):
        return [c for c in cands if c[0] != "miopen"]
    return cands


def _timed(cands: Cands, runs: int = 1) -> list:
    """[(name, best of ``runs`` timings + penalty in ms, or the RuntimeError of a candidate that
    cannot run this shape, e.g. an ATen 32-bit-index limit)]."""
    out = []
    for n, fn, pen in cands:
        try:
            out.append((n, min(_time_ms(fn) for _ in range(runs)) + pen))
        except RuntimeError as e:
            out.append((n, e))
    return out


def _log(tag: str, k: tuple, name: str, timed: list, note: str = "") -> None:
    if _TUNE_LOG:
        import sys

        times = [f"{n}=failed({str(t)[:60]})" if isinstance(t, RuntimeError) else f"{n}={t:.3f}ms" for n, t in timed]
        print(f"[{tag}] {k} -> {name} ({', '.join(times + [note] * bool(note))})", file=sys.stderr, flush=True)


def _retime(k: tuple, name: str, cands: Cands) -> str:
    """Tuning aid (_RETIME): the decided route ``name`` against the named candidates only; one of
    them replaces it where it is faster by 3 %."""
    _RETIMED.add(k)
    timed = [(n, t) for n, t in _timed([c for c in cands if c[0] == name or c[0] in _RETIME], runs=2)
             if not isinstance(t, RuntimeError)]
    cur = dict(timed).get(name)
    best_n, best_t = min([p for p in timed if p[0] != name], key=lambda p: p[1], default=(None, float("inf")))
    if cur is not None and best_n is not None and best_t < cur * 0.97:
        name = _CHOICE[k] = best_n
    _log("conv-retime", k, name, timed)
    return name


def _tune(k: tuple, cands: Cands) -> str:
    """First use of ``k``: rank 0's decision (multi-rank jobs) or the fastest candidate, stored."""
    names = [c[0] for c in cands]
    name = _agree.shared("conv", k)
    if name in names:
        timed, note = [], "rank 0's decision"
    else:
        timed, note = _timed(cands), ""
        best, name, mio = float("inf"), names[0], float("inf")
        for n, t in timed:
            if isinstance(t, RuntimeError):  # drops out
                continue
            if n == "miopen":
                mio = t
            elif t < best:
                best, name = t, n
        # native first: MIOpen only where it is clearly faster (relative + absolute margin)
        if mio < best * (1.0 - _MIOPEN_MARGIN) - _MIOPEN_MARGIN_MS:
            name = "miopen"
        _agree.publish("conv", k, name)
    _CHOICE[k] = name
    _log("conv-tune", k, name, timed, note)
    return name


def _route_choice(direction: str, key: tuple, cands: Cands) -> str:
    """The name of the candidate :func:`_route` runs (timing the candidates on first use)."""
    cands = _eligible(cands)
    names = [c[0] for c in cands]
    forced = _FORCE[direction]
    if forced in names:
        return forced
    if len(cands) == 1:
        return names[0]
    k = (direction,) + key
    name = _CHOICE.get(k)
    if name is not None and name not in names:  # a shipped / loaded route this process excludes
        name = None
    if (name is not None and _RETIME and k not in _RETIMED and not torch.cuda.is_current_stream_capturing()
            and any(n in _RETIME for n in names)):
        name = _retime(k, name, cands)
    if name is None:
        if not _AUTOTUNE or torch.cuda.is_current_stream_capturing():
            return names[0]
        name = _tune(k, cands)
    return name
