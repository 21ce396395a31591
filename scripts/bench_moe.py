"""Time the grouped GEMM (ops.gemm.grouped_linear, csrc/gemm_grouped.hip) and an MoE training step.

One run, interleaved rounds, medians (device events around each call; every variant is warmed up first):

* ``grouped_linear`` forward and forward + backward at ``R = 8192 * 2`` rows, ``E = 8``, with balanced and skewed
  offsets, against the dense ``mm_nt`` / ``mm_nn`` / ``mm_tn`` on the same total rows (one weight: the work of the
  grouped call without groups) and against the loop of one dense call per expert (row counts known on the host,
  which a model would have to read from the device);
* ``gpt2_small(mlp="moe", experts=8, top_k=2, mlp_ratio=8/3, norm="rms", pos="rope")`` against the dense SwiGLU
  model, forward + backward of ``loss`` at 8 x 1024 tokens.

Writes one JSON line per measurement to ``--out`` (default: stdout only).  Needs a GPU."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import torch  # noqa: E402

from torchbooster_amd.models.gpt import gpt2_small  # noqa: E402
from torchbooster_amd.ops import gemm as G  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
INNER = 25  # calls per timed window of the GEMM variants (a single 0.1 ms call measures the clock)


def interleaved(variants: dict, rounds: int, warmup: int = 3, inner: int = 1) -> dict:
    """name -> median ms per call over ``rounds`` rounds, each round timing ``inner`` back-to-back calls of every
    variant in turn."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(inner):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) / inner)
    return {k: statistics.median(v) for k, v in times.items()}


def offsets_of(kind: str, R: int, E: int):
    if kind == "balanced":
        counts = [R // E] * E
    else:  # skewed: half the rows in one expert, a quarter in the next, ..., odd boundaries
        counts, left = [], R
        for e in range(E - 1):
            counts.append(left // 2 + (3 if left > 16 else 0))
            left -= counts[-1]
        counts.append(left)
    assert sum(counts) == R and min(counts) >= 0
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return off


def bench_gemm(R: int, K: int, Q: int, E: int, kind: str, rounds: int):
    off_host = offsets_of(kind, R, E)
    off = torch.tensor(off_host, dtype=torch.int32, device=DEV)
    x = torch.randn(R, K, device=DEV).to(BF).requires_grad_()
    dy = torch.randn(R, Q, device=DEV).to(BF)
    w = (torch.randn(E, Q, K, device=DEV) / K ** 0.5).to(BF).requires_grad_()
    xd, wd = x.detach(), w.detach()

    def grouped_fb():
        y = G.grouped_linear(x, w, off)
        torch.autograd.grad(y, (x, w), dy)

    def dense_fb():
        G.mm_nt(xd, wd[0])
        G.mm_nn(dy, wd[0])
        G.mm_tn(dy, xd)

    def loop_f():
        for e in range(E):
            if off_host[e + 1] > off_host[e]:
                G.mm_nt(xd[off_host[e]:off_host[e + 1]], wd[e])

    def loop_fb():
        loop_f()
        for e in range(E):
            if off_host[e + 1] > off_host[e]:
                G.mm_nn(dy[off_host[e]:off_host[e + 1]], wd[e])
                G.mm_tn(dy[off_host[e]:off_host[e + 1]], xd[off_host[e]:off_host[e + 1]])

    with torch.no_grad():
        ms = interleaved({"grouped_fwd": lambda: G.grouped_linear(xd, wd, off), "dense_fwd": lambda: G.mm_nt(xd, wd[0]),
                          "loop_fwd": loop_f}, rounds, inner=INNER)
    ms.update(interleaved({"grouped_fwd_bwd": grouped_fb, "dense_fwd_bwd": dense_fb, "loop_fwd_bwd": loop_fb}, rounds,
                          inner=INNER))
    flop = 2.0 * R * K * Q
    return {"what": "grouped_linear", "R": R, "K": K, "Q": Q, "E": E, "offsets": kind, "rounds": rounds,
            "calls_per_round": INNER, "ms": {k: round(v, 4) for k, v in ms.items()},
            "tflops": {k: round(flop * (3 if k.endswith("bwd") else 1) / v / 1e9, 1) for k, v in ms.items()}}


def bench_model(rounds: int):
    tokens = torch.randint(0, 50257, (8, 1024), device=DEV)
    ms, aux = {}, {}
    for name, kw in (("moe", {"mlp": "moe", "experts": 8, "top_k": 2}), ("swiglu", {"mlp": "swiglu"})):
        torch.manual_seed(0)
        model = gpt2_small(mlp_ratio=8 / 3, norm="rms", pos="rope", bias=False, **kw).to(DEV, BF)

        def step(model=model):
            model.loss(tokens).backward()
            model.zero_grad(set_to_none=True)

        ms[name] = interleaved({name: step}, rounds, warmup=2)[name]  # (one model in memory at a time)
        aux[name] = sum(p.numel() for p in model.parameters())
        del model, step
        torch.cuda.empty_cache()
    return {"what": "gpt2_small loss forward + backward, 8 x 1024 tokens", "rounds": rounds,
            "ms": {k: round(v, 3) for k, v in ms.items()}, "parameters": aux}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--model-rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe: needs a GPU")
    rows = []
    for K, Q in ((768, 2 * 2048), (768, 768), (2048, 768)):
        for kind in ("balanced", "skewed"):
            rows.append(bench_gemm(8192 * 2, K, Q, 8, kind, a.rounds))
            print(json.dumps(rows[-1]), flush=True)
    if a.model_rounds > 0:
        rows.append(bench_model(a.model_rounds))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
