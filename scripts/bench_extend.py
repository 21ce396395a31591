#!/usr/bin/env python
"""Multi-token KV-cache extend: the ``attn_extend`` kernels alone, one ``gpt2_small`` extend step
against one decode step, and ``generate(draft=...)``.

Kernel part.  ``attention_extend`` at T in {2, 4, 8, 16, 64}, B*H in {12, 96} and len in {512, 1024}
with cap = len and positions = len - T (the T queries see len - T + 1 .. len rows), for several split
sizes (``attn_extend_set_split``; 0 is the default policy, 1048576 a single split), against T
back-to-back ``attention_decode`` calls on the same cache at length len -- what one had to run for
the same T tokens before.  To keep the host out of the number, ``--inner`` calls are captured into
one graph and the graph's replays are timed between two device events; the calls of a graph rotate
over ``--copies`` cache copies.  Variants are interleaved round by round; the median round and the
min-max spread are reported.

Step part.  ``gpt2_small`` in bf16, every sequence's cache at ``--at`` tokens: ONE ``extend`` of T in
{1, 2, 4, 8, 16} tokens against ONE ``decode_step``, each captured into a graph together with the
reset of the positions (so every replay runs at the same length) and timed between device events,
interleaved as above.  ``eager`` repeats it without a graph, a host clock around ``--iters`` steps
that end in a device synchronise.  ``--root DIR --stepT`` (no sizes) measures the ``decode_step`` of
another checkout of the package, e.g. the parent commit's, with the same code.

Spec part.  ``gpt2_small`` bf16, prompt ``--prompt``, ``--new`` new tokens, greedy: ``generate``,
``generate(graph=True)`` and ``generate(draft=d, draft_tokens=--gamma)`` with d the target itself and
a randomly initialised 2-layer model.  Seconds (a host clock around a run that ends in a device
synchronise; one untimed run first) and the mean tokens emitted per round.  No trained draft exists
here: with random weights this shows the mechanism's overhead, not a speed-up.

One JSON line per measurement.  Usage: ``python scripts/bench_extend.py [--part kernel step spec]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_SPLIT = 1 << 20


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "step", "spec"], choices=["kernel", "step", "spec"])
    ap.add_argument("--bh", type=int, nargs="+", default=[12, 96])
    ap.add_argument("--len", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--T", type=int, nargs="+", default=[2, 4, 8, 16, 64])
    ap.add_argument("--splits", type=int, nargs="+", default=[64, 128, 256, 512, ONE_SPLIT, 0])
    ap.add_argument("--inner", type=int, default=16, help="calls per captured graph")
    ap.add_argument("--copies", type=int, default=8, help="cache copies a graph rotates over")
    ap.add_argument("--iters", type=int, default=20, help="graph replays (or eager steps) per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--at", type=int, default=512, help="tokens every cache holds in the step part")
    ap.add_argument("--stepT", type=int, nargs="*", default=[1, 2, 4, 8, 16],
                    help="extend sizes of the step part; none: decode_step alone (works on a checkout without extend)")
    ap.add_argument("--root", default=ROOT, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--gamma", type=int, default=4)
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.root))

    import torch

    from torchbooster_amd.ops import _ext

    if not torch.cuda.is_available():
        raise SystemExit("bench_extend.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def stats(v, nd=2):
        return {"median": round(sorted(v)[len(v) // 2], nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    def time_graphs(graphs, per_replay):
        """Interleaved rounds of ``--iters`` replays between device events -> us per call, per variant."""
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    g.replay()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / (a.iters * per_replay))
        return times

    if "kernel" in a.part:
        from torchbooster_amd.ops.attention import attention_decode, attention_extend

        nat = _ext.native()
        old = nat.attn_extend_set_split(-1)
        H = 12
        for BH in a.bh:
            B = max(BH // H, 1)
            for n in a.len:
                caches = [(torch.randn(B, H, n, 64, device=dev).to(torch.bfloat16),
                           torch.randn(B, H, n, 64, device=dev).to(torch.bfloat16)) for _ in range(a.copies)]
                kl = torch.full((B,), n, dtype=torch.int32, device=dev)
                for T in a.T:
                    torch.manual_seed(n + T)
                    q = torch.randn(B, T, 3 * H * 64, device=dev).to(torch.bfloat16).view(B, T, 3, H, 64)[:, :, 0]
                    pos = torch.full((B,), n - T, dtype=torch.int32, device=dev)
                    graphs, keep, nsplit = {}, [], {}
                    try:
                        for sp in a.splits:
                            nat.attn_extend_set_split(sp)
                            nsplit[sp] = nat.attn_extend_splits(B, H, T, n)
                            attention_extend(q, *caches[0], pos)  # warm-up outside the capture
                            torch.cuda.synchronize()
                            g = torch.cuda.CUDAGraph()
                            with torch.cuda.graph(g):
                                keep.append([attention_extend(q, *caches[i % a.copies], pos) for i in range(a.inner)])
                            g.replay()
                            graphs[sp] = g
                    finally:
                        nat.attn_extend_set_split(old)
                    attention_decode(q[:, 0], *caches[0], kl)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        keep.append([attention_decode(q[:, t], *caches[i % a.copies], kl)
                                     for i in range(a.inner) for t in range(T)])
                    g.replay()
                    graphs["decode_xT"] = g
                    torch.cuda.synchronize()
                    for k, v in time_graphs(graphs, a.inner).items():
                        s = stats(v)
                        emit({"bench": "attn_extend", "tag": a.tag, "B": B, "H": H, "T": T, "len": n, "variant": k,
                              "nsplit": nsplit.get(k), "us_median": s["median"], "us_min": s["min"], "us_max": s["max"],
                              "cache_copies": a.copies, "inner": a.inner, "iters": a.iters, "rounds": a.rounds})
                    del graphs, keep
                del caches

    if "step" in a.part or "spec" in a.part:
        from torchbooster_amd.models import gpt2_small
        from torchbooster_amd.models.gpt import KVCache, TransformerLM

        torch.manual_seed(0)
        model = gpt2_small().to(dev).to(torch.bfloat16).eval()

    if "step" in a.part:
        for B in a.batch:
            tokens = torch.randint(0, 50257, (B, a.at), device=dev)
            _, cache = model.prefill(tokens, cache=KVCache(model, B))
            new = torch.randint(0, 50257, (B, max(a.stepT + [1])), device=dev)

            def make(T):
                def run():
                    cache.positions.fill_(a.at)
                    return model.decode_step(new[:, 0], cache) if T == 0 else model.extend(new[:, :T], cache)
                return run

            runs = {"decode_step": make(0), **{f"extend_T{T}": make(T) for T in a.stepT}}
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
            tg = time_graphs(graphs, 1)
            te = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        fn()
                    torch.cuda.synchronize()
                    te[k].append((time.perf_counter() - t0) * 1e6 / a.iters)
            base = sorted(tg["decode_step"])[len(tg["decode_step"]) // 2]
            for k in runs:
                sg, se = stats(tg[k], 1), stats(te[k], 1)
                T = 1 if k == "decode_step" else int(k.split("T")[1])
                emit({"bench": "gpt2_small_extend_step", "tag": a.tag, "variant": k, "B": B, "T": T, "at": a.at,
                      "graph_us_median": sg["median"], "graph_us_min": sg["min"], "graph_us_max": sg["max"],
                      "eager_us_median": se["median"], "eager_us_min": se["min"], "eager_us_max": se["max"],
                      "graph_vs_decode_step": round(sg["median"] / base, 3),
                      "graph_us_per_token": round(sg["median"] / T, 1), "iters": a.iters, "rounds": a.rounds})
            del graphs, keep, cache

    if "spec" in a.part:
        torch.manual_seed(1)
        two = TransformerLM(50257, 768, 2, 12, 1024).to(dev).to(torch.bfloat16).eval()
        rounds_seen = []
        real = TransformerLM.extend

        def counted(self, *args, **kw):
            rounds_seen.append(args[0].shape[1])
            return real(self, *args, **kw)

        TransformerLM.extend = counted
        try:
            for B in a.batch:
                tokens = torch.randint(0, 50257, (B, a.prompt), device=dev)
                runs = {
                    "generate": lambda: model.generate(tokens, a.new)[0],
                    "generate_graph": lambda: model.generate(tokens, a.new, graph=True)[0],
                    "draft_self": lambda: model.generate(tokens, a.new, draft=model, draft_tokens=a.gamma)[0],
                    "draft_2layer": lambda: model.generate(tokens, a.new, draft=two, draft_tokens=a.gamma)[0],
                }
                outs, nrounds = {}, {}
                for k, fn in runs.items():  # untimed: first-use work of every shape
                    del rounds_seen[:]
                    outs[k] = fn()
                    nrounds[k] = len(rounds_seen)
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
                    same = int((outs[k] == outs["generate"]).to(torch.int64).cumprod(1).sum(1).min())
                    emit({"bench": "gpt2_small_speculative", "tag": a.tag, "variant": k, "B": B, "prompt": a.prompt,
                          "new": a.new, "gamma": a.gamma if k.startswith("draft") else None, "s_median": s["median"],
                          "s_min": s["min"], "s_max": s["max"], "tokens_per_s": round(B * a.new / s["median"], 1),
                          "rounds_of_draft_and_verify": nrounds[k] or None,
                          "tokens_per_round": round((a.new - 1) / nrounds[k], 2) if nrounds[k] else None,
                          "leading_tokens_equal_generate": same, "rounds": a.rounds})
        finally:
            TransformerLM.extend = real
    return 0


if __name__ == "__main__":
    sys.exit(main())
