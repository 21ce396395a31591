#!/usr/bin/env python
"""Llama-style blocks: RMSNorm against LayerNorm, the SwiGLU gate against ``F.silu(a) * b``, the few-row kernel's
RMS prologue + SwiGLU epilogue against its LayerNorm + GELU call, and a ``gpt2_small``-shaped training step
and decode step, ``norm="rms", mlp="swiglu", mlp_ratio=8/3, bias=False`` against the default model.

norm part.  ``rms_norm`` and ``layer_norm`` at ``--rows`` x ``--dim`` (8192 x 768) in bf16: the forward alone and
the forward followed by its backward (``torch.autograd.grad`` with a ready gradient), each captured into a
graph that makes one call per copy of the input, ``--ws-mb`` of copies in all, so that the case streams from
memory and not from the last-level cache; replays are timed between two device events, the variants
interleaved round by round.  Forward and backward are captured TOGETHER, as ``utils.GraphedStep`` captures a
step: autograd runs a backward node on the stream of its forward, so a backward whose forward ran outside
the capture would launch outside it.  The backward's time is the difference of the two medians.  ``bytes``:
forward x in and y out; backward x and dy in and dx out (statistics and the [C] vectors are not counted).

gate part.  ``swiglu`` and ``F.silu(a) * b`` on the two halves of a packed ``--rows`` x ``2 * --hidden`` bf16 tensor
(8192 x 2 * 2048), forward and forward + backward, the same method.  ``bytes``: forward 2F in and F out per row, backward
2F and F in and 2F out.

rows part.  ``linear_rows(rms=, act="swiglu")`` with a ``[2F, K]`` weight against ``linear_rows(ln=, act="gelu")``
with a ``[Q, K]`` one, K = ``--dim``, F = ``--hidden`` (2048), Q = ``--gelu-hidden`` (3072): the two MLP input
products of equal parameter count.  ``--rows-copies`` weights per graph (they do not stay in the last-level
cache), M in ``--batch``.  ``bytes``: the weight.

train / step parts.  As scripts/bench_rope.py: ``utils.step(model.loss(tokens), FusedAdamW, clip=1.0)`` at
``--tokens``, and a graph-replayed ``decode_step(fused=True)`` with every cache at ``--at`` tokens, B in
``--batch``; the two models alternated round by round.

One JSON line per measurement.  Usage: ``python scripts/bench_llama_block.py [--part norm gate rows train step]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = ["norm", "gate", "rows", "train", "step"]
LLAMA = dict(norm="rms", mlp="swiglu", mlp_ratio=8 / 3, bias=False)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=PARTS, choices=PARTS)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--hidden", type=int, default=2048, help="F of the SwiGLU MLP")
    ap.add_argument("--gelu-hidden", type=int, default=3072, help="Q of the GELU MLP it is compared with")
    ap.add_argument("--tokens", type=int, nargs=2, default=[8, 1024], help="B N of the training shape")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of input copies a kernel graph rotates over")
    ap.add_argument("--max-copies", type=int, default=64)
    ap.add_argument("--rows-copies", type=int, default=48, help="weight copies a few-row graph rotates over")
    ap.add_argument("--kernel-iters", type=int, default=5, help="replays of a kernel graph per timed round")
    ap.add_argument("--iters", type=int, default=20, help="graph replays of a decode step per timed round")
    ap.add_argument("--train-iters", type=int, default=5, help="training steps per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--at", type=int, default=512, help="tokens every cache holds in the step part")
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)

    import torch
    import torch.nn.functional as F

    if not torch.cuda.is_available():
        raise SystemExit("bench_llama_block.py measures on the GPU; none found")
    from torchbooster_amd.ops.act import swiglu
    from torchbooster_amd.ops.linear import linear_rows
    from torchbooster_amd.ops.norm import layer_norm, rms_norm

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def stats(v, nd=2):
        return {"median": round(sorted(v)[len(v) // 2], nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    def time_calls(calls, per_call, iters):
        """Interleaved rounds of ``iters`` calls between device events -> us per unit of work, per variant."""
        times = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / (iters * per_call))
        return times

    def capture(fn, copies_of):
        """one graph that calls ``fn`` once per entry of ``copies_of`` (two untimed calls first)"""
        fn(copies_of[0])
        fn(copies_of[0])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = [fn(c) for c in copies_of]
        g.replay()
        return g, outs

    def fwd_bwd_graphs(variants, make_input, in_bytes, dy_shape):
        """For each named ``y = f(x)``: a graph of the forward alone and a graph of the forward with its
        backward (both inside the capture, the gradient a ready tensor), one call per copy of the input."""
        copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // in_bytes)))
        leaves = [make_input(i).requires_grad_() for i in range(copies)]
        dys = [torch.randn(*dy_shape, device=dev).to(bf) for _ in range(copies)]
        graphs, keep = {}, []
        for name, f in variants.items():
            def fwd(i, f=f):
                with torch.no_grad():
                    return f(leaves[i])

            def both(i, f=f):
                return torch.autograd.grad(f(leaves[i]), leaves[i], dys[i])[0]

            for way, fn in (("forward", fwd), ("forward + backward", both)):
                g, outs = capture(fn, list(range(copies)))
                graphs[(name, way)] = g.replay
                keep.append((g, outs))
        torch.cuda.synchronize()
        return graphs, keep, copies

    def emit_fwd_bwd(bench, shape, times, copies, nbytes):
        """one line per (op, pass); the backward is the difference of the medians of the two graphs"""
        med = {k: stats(v) for k, v in times.items()}
        for (name, way), s in med.items():
            rec = {"bench": bench, "tag": a.tag, "op": name, "pass": way, **shape, "us_median": s["median"],
                   "us_min": s["min"], "us_max": s["max"], "copies": copies, "iters": a.kernel_iters, "rounds": a.rounds}
            if way == "forward":
                rec.update(MB=round(nbytes["forward"] / 1e6, 3), TBps=round(nbytes["forward"] / s["median"] * 1e-6, 2))
            emit(rec)
            if way != "forward":
                us = round(s["median"] - med[(name, "forward")]["median"], 2)
                emit({"bench": bench, "tag": a.tag, "op": name, "pass": "backward (difference)", **shape, "us_median": us,
                      "MB": round(nbytes["backward"] / 1e6, 3), "TBps": round(nbytes["backward"] / us * 1e-6, 2)})

    if "norm" in a.part:
        M, C = a.rows, a.dim
        w = (torch.rand(C, device=dev) + 0.5).requires_grad_()
        b = torch.randn(C, device=dev).requires_grad_()
        variants = {"rms_norm": lambda x: rms_norm(x, w, 1e-6), "layer_norm": lambda x: layer_norm(x, w, b, 1e-6)}
        graphs, keep, copies = fwd_bwd_graphs(variants, lambda i: torch.randn(M, C, device=dev).to(bf), M * C * 2,
                                              (M, C))
        emit_fwd_bwd("llama_norm", {"M": M, "C": C}, time_calls(graphs, copies, a.kernel_iters), copies,
                     {"forward": 2 * M * C * 2, "backward": 3 * M * C * 2})
        del graphs, keep

    if "gate" in a.part:
        M, Fh = a.rows, a.hidden
        variants = {"swiglu": swiglu, "F.silu(a) * b": lambda gu: F.silu(gu[..., :Fh]) * gu[..., Fh:]}
        graphs, keep, copies = fwd_bwd_graphs(variants, lambda i: (torch.randn(M, 2 * Fh, device=dev) * 3).to(bf),
                                              M * 2 * Fh * 2, (M, Fh))
        emit_fwd_bwd("llama_gate", {"M": M, "F": Fh}, time_calls(graphs, copies, a.kernel_iters), copies,
                     {"forward": 3 * M * Fh * 2, "backward": 5 * M * Fh * 2})
        del graphs, keep

    if "rows" in a.part:
        K, Fh, Q = a.dim, a.hidden, a.gelu_hidden
        gamma = torch.rand(K, device=dev) + 0.5
        beta = torch.randn(K, device=dev)
        n = a.rows_copies
        wg = [(torch.randn(2 * Fh, K, device=dev) * K ** -0.5).to(bf) for _ in range(n)]
        wq = [(torch.randn(Q, K, device=dev) * K ** -0.5).to(bf) for _ in range(n)]
        bq = torch.randn(Q, device=dev).to(bf)
        with torch.no_grad():
            for M in a.batch:
                x = (torch.randn(M, K, device=dev) * 1.5).to(bf)
                graphs, keep = {}, []
                for name, ws, f in (
                        ("rms + swiglu", wg, lambda w: linear_rows(x, w, None, rms=(gamma, 1e-6), act="swiglu")),
                        ("ln + gelu", wq, lambda w: linear_rows(x, w, bq, ln=(gamma, beta, 1e-6), act="gelu"))):
                    g, outs = capture(f, ws)
                    graphs[name] = g.replay
                    keep.append((g, outs))
                torch.cuda.synchronize()
                nbytes = {"rms + swiglu": 2 * Fh * K * 2, "ln + gelu": Q * K * 2}
                for name, v in time_calls(graphs, n, a.iters).items():
                    s = stats(v)
                    emit({"bench": "llama_rows", "tag": a.tag, "call": name, "M": M, "K": K,
                          "out": Fh if name == "rms + swiglu" else Q, "us_median": s["median"], "us_min": s["min"],
                          "us_max": s["max"], "weight_MB": round(nbytes[name] / 1e6, 3),
                          "TBps": round(nbytes[name] / s["median"] * 1e-6, 2), "copies": n, "iters": a.iters,
                          "rounds": a.rounds})
                del graphs, keep

    kinds = {"default": {}, "llama": LLAMA}

    if "train" in a.part:
        from torchbooster_amd import utils
        from torchbooster_amd.models.gpt import gpt2_small
        from torchbooster_amd.ops.optim import FusedAdamW

        B, N = a.tokens
        tokens = torch.randint(0, 50257, (B, N), device=dev)
        steps, params = {}, {}
        for kind, kw in kinds.items():
            torch.manual_seed(0)
            model = gpt2_small(**kw).to(dev).to(bf)
            params[kind] = sum(p.numel() for p in model.parameters())
            opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01)

            def step(model=model, opt=opt):
                utils.step(model.loss(tokens), opt, clip=1.0)

            for _ in range(3):
                step()
            steps[kind] = step
        torch.cuda.synchronize()
        t = time_calls(steps, 1, a.train_iters)
        ref = sorted(t["default"])[len(t["default"]) // 2]
        for name, v in t.items():
            s = stats([x / 1e3 for x in v], 3)
            emit({"bench": "llama_train_step", "tag": a.tag, "model": name, "params": params[name], "B": B, "N": N,
                  "ms_median": s["median"], "ms_min": s["min"], "ms_max": s["max"],
                  "vs_default": round(s["median"] / (ref / 1e3), 4), "iters": a.train_iters, "rounds": a.rounds})
        del steps

    if "step" in a.part:
        from torchbooster_amd.models.gpt import KVCache, gpt2_small

        with torch.no_grad():
            for B in a.batch:
                graphs, keep = {}, []
                tokens = torch.randint(0, 50257, (B, a.at), device=dev)
                new = torch.randint(0, 50257, (B,), device=dev)
                for kind, kw in kinds.items():
                    torch.manual_seed(0)
                    model = gpt2_small(**kw).to(dev).to(bf).eval()
                    _, cache = model.prefill(tokens, cache=KVCache(model, B))

                    def run(_=None, model=model, cache=cache):
                        cache.positions.fill_(a.at)
                        return model.decode_step(new, cache, fused=True)

                    g, outs = capture(run, [None])
                    graphs[kind] = g.replay
                    keep.append((g, outs, model, cache))
                torch.cuda.synchronize()
                t = time_calls(graphs, 1, a.iters)
                ref = sorted(t["default"])[len(t["default"]) // 2]
                for kind, v in t.items():
                    s = stats(v, 1)
                    emit({"bench": "llama_decode_step", "tag": a.tag, "model": kind, "B": B, "fused": True, "at": a.at,
                          "graph_us_median": s["median"], "graph_us_min": s["min"], "graph_us_max": s["max"],
                          "vs_default": round(s["median"] / ref, 4), "iters": a.iters, "rounds": a.rounds})
                del graphs, keep
    return 0


if __name__ == "__main__":
    sys.exit(main())
