#!/usr/bin/env python
"""Fused few-row decoding: the ``rows_linear`` kernel alone, one ``gpt2_small`` step fused against
unfused, and ``generate`` with ``fused`` x ``graph``.

Kernel part.  ``linear_rows`` against ``ops.linear.linear`` (the GEMM engine's ``mm_nt`` where it takes
the shape, else ``F.linear``) on the same operands, M in {1, 8, 16}, for the ``gpt2_small`` products
768 -> 2304, 768 -> 768, 768 -> 3072, 3072 -> 768 and 768 -> 50257, bias included (none for the head).
A weight of 1 - 77 MB would sit in the last-level cache between calls, which it does not in a step that
streams 250 MB: every call of a captured graph reads ANOTHER copy of the weight, ``--ws-mb`` of copies
in all (at most ``--max-copies``).  A graph holds one call per copy; its replays are timed between two
device events.  Variants are interleaved round by round; the median round and the min-max spread are
reported, with the weight bytes per second the median amounts to.

Step part.  ``gpt2_small`` in bf16, every sequence's cache at ``--at`` tokens: ``decode_step`` at B in
``--batch`` and ``extend`` of T in ``--stepT`` tokens at B = 1, ``fused=True`` against the default, each
captured into a graph together with the reset of the positions (so every replay runs at the same
length) and timed between device events, interleaved as above.  ``eager`` repeats it without a graph,
a host clock around ``--iters`` steps that end in a device synchronise.  ``--root DIR`` measures the
default ``decode_step`` of another checkout of the package, e.g. the parent commit's, with the same
code in its own process (nothing fused is asked of it).

Gen part.  ``generate`` with prompt ``--prompt`` and ``--new`` new tokens, greedy, ``fused`` x ``graph``:
seconds (a host clock around a run that ends in a device synchronise; one untimed run first) and
tokens per second.

One JSON line per measurement.  Usage: ``python scripts/bench_decode_fused.py [--part kernel step gen]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCTS = [(768, 2304), (768, 768), (768, 3072), (3072, 768), (768, 50257)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "step", "gen"], choices=["kernel", "step", "gen"])
    ap.add_argument("--M", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of weight copies a kernel graph rotates over")
    ap.add_argument("--max-copies", type=int, default=192)
    ap.add_argument("--iters", type=int, default=20, help="graph replays (or eager steps) per timed round")
    ap.add_argument("--kernel-iters", type=int, default=3, help="replays of a kernel graph per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--stepT", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--at", type=int, default=512, help="tokens every cache holds in the step part")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    other = os.path.abspath(a.root) != ROOT
    sys.path.insert(0, os.path.abspath(a.root))

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_fused.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def stats(v, nd=2):
        return {"median": round(sorted(v)[len(v) // 2], nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    def time_graphs(graphs, per_replay, iters):
        """Interleaved rounds of ``iters`` replays between device events -> us per call, per variant."""
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    g.replay()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / (iters * per_replay))
        return times

    if "kernel" in a.part and not other:
        from torchbooster_amd.ops import gemm as G
        from torchbooster_amd.ops.linear import linear, linear_rows

        with torch.no_grad():
            for K, Q in PRODUCTS:
                wbytes = K * Q * 2
                copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // wbytes)))
                torch.manual_seed(K + Q)
                ws = [(torch.randn(Q, K, device=dev) * K ** -0.5).to(bf) for _ in range(copies)]
                bias = None if Q == 50257 else torch.randn(Q, device=dev).to(bf)
                for M in a.M:
                    x = torch.randn(M, K, device=dev).to(bf)
                    base = "mm_nt" if G.supported_nt(x, ws[0]) else "F.linear"
                    fns = {"rows_linear": lambda w: linear_rows(x, w, bias), base: lambda w: linear(x, w, bias)}
                    graphs, keep = {}, []
                    for k, fn in fns.items():
                        fn(ws[0])  # untimed: first-use work (the GEMM tile tuner included)
                        fn(ws[0])
                        torch.cuda.synchronize()
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            keep.append([fn(w) for w in ws])
                        g.replay()
                        graphs[k] = g
                    torch.cuda.synchronize()
                    t = time_graphs(graphs, copies, a.kernel_iters)
                    ref = sorted(t[base])[len(t[base]) // 2]
                    for k, v in t.items():
                        s = stats(v)
                        emit({"bench": "rows_linear", "tag": a.tag, "variant": k, "M": M, "K": K, "Q": Q,
                              "us_median": s["median"], "us_min": s["min"], "us_max": s["max"],
                              "weight_GBps": round(wbytes / s["median"] * 1e-3, 1),
                              "vs_engine": round(s["median"] / ref, 3), "weight_copies": copies,
                              "iters": a.kernel_iters, "rounds": a.rounds})
                    del graphs, keep
                del ws

    if "step" in a.part or "gen" in a.part:
        from torchbooster_amd.models import gpt2_small
        from torchbooster_amd.models.gpt import KVCache

        torch.manual_seed(0)
        model = gpt2_small().to(dev).to(bf).eval()

    if "step" in a.part:
        for B in a.batch:
            tokens = torch.randint(0, 50257, (B, a.at), device=dev)
            _, cache = model.prefill(tokens, cache=KVCache(model, B))
            new = torch.randint(0, 50257, (B, max(a.stepT + [1])), device=dev)

            def make(T, fused):
                kw = {"fused": True} if fused else {}

                def run():
                    cache.positions.fill_(a.at)
                    return model.decode_step(new[:, 0], cache, **kw) if T == 0 else model.extend(new[:, :T], cache, **kw)
                return run

            runs = {"decode_step": make(0, False)}
            if not other:
                runs["decode_step_fused"] = make(0, True)
                if B == 1:
                    for T in a.stepT:
                        runs[f"extend_T{T}"] = make(T, False)
                        runs[f"extend_T{T}_fused"] = make(T, True)
            graphs, keep = {}, []
            for k, fn in runs.items():
                fn()  # untimed: first-use work of every shape (the GEMM tile tuner included)
                fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    keep.append(fn())
                g.replay()
                graphs[k] = g
            torch.cuda.synchronize()
            tg = time_graphs(graphs, 1, a.iters)
            te = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        fn()
                    torch.cuda.synchronize()
                    te[k].append((time.perf_counter() - t0) * 1e6 / a.iters)
            for k in runs:
                sg, se = stats(tg[k], 1), stats(te[k], 1)
                unfused = k.replace("_fused", "")
                emit({"bench": "gpt2_small_fused_step", "tag": a.tag, "variant": k, "B": B,
                      "T": 1 if unfused == "decode_step" else int(unfused.split("T")[1]), "at": a.at,
                      "graph_us_median": sg["median"], "graph_us_min": sg["min"], "graph_us_max": sg["max"],
                      "eager_us_median": se["median"], "eager_us_min": se["min"], "eager_us_max": se["max"],
                      "graph_vs_unfused": round(sg["median"] / sorted(tg[unfused])[len(tg[unfused]) // 2], 3),
                      "eager_vs_unfused": round(se["median"] / sorted(te[unfused])[len(te[unfused]) // 2], 3),
                      "iters": a.iters, "rounds": a.rounds})
            del graphs, keep, cache

    if "gen" in a.part and not other:
        for B in a.batch:
            tokens = torch.randint(0, 50257, (B, a.prompt), device=dev)
            runs = {f"fused={int(f)} graph={int(g)}": (lambda f=f, g=g: model.generate(tokens, a.new, fused=f, graph=g)[0])
                    for f in (False, True) for g in (False, True)}
            outs = {k: fn() for k, fn in runs.items()}  # untimed: first-use work of every shape
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
            for k, v in times.items():
                s = stats(v, 4)
                same = int((outs[k] == outs["fused=0 graph=0"]).to(torch.int64).cumprod(1).sum(1).min())
                emit({"bench": "gpt2_small_generate", "tag": a.tag, "variant": k, "B": B, "prompt": a.prompt,
                      "new": a.new, "s_median": s["median"], "s_min": s["min"], "s_max": s["max"],
                      "tokens_per_s": round(B * a.new / s["median"], 1),
                      "leading_tokens_equal_unfused_eager": same, "rounds": a.rounds})
    return 0


if __name__ == "__main__":
    sys.exit(main())
