#!/usr/bin/env python
"""The few-row MoE kernels (csrc/rows_experts_mx.hip) against what a decode step does without them.

Kernel part.  For (K, F) in ``WIDTHS``, (E, top_k) in ``EXPERTS`` and M in ``--M`` rows: ``moe_route_rows`` (``route``),
``linear_rows_experts`` in pair mode with the RMSNorm prologue and SwiGLU (``fc1``) and in combine mode with the
residual (``fc2``), each alone and the three in a row (``fused``); against (a) ``unfused``: ``x + MoE.forward(norm(x))``,
the dispatch a decode step runs without ``fused=True``, on bf16 experts, and (b) ``per_pair``: one
``linear_rows(mx_scales=)`` call per (token, slot) pair and product with the expert indices known on the host (the
one-weight kernel; gates and sum not included).  The experts are random MXFP4 codes; the ids are what a random
router picks.  As in scripts/bench_rows_mx.py every call of a captured graph reads ANOTHER copy of the weights
(``--ws-mb`` of MXFP4 expert stacks, at most ``--max-copies``; a call touches its distinct experts only), a
graph's replays are timed between two device events, the variants interleaved round by round, and the median of
``--rounds`` rounds is reported with its min-max spread.

Step part.  An MoE ``gpt2_small`` (8 experts, top 2, ``norm="rms"``, ``pos="rope"``) in bf16, every cache at ``--at``
tokens, ``decode_step`` at B in ``--batch`` captured in a graph with the reset of the positions: ``fused=True`` after
``quantize_rows()`` against the default path (``fused=False``) on the same model.

One JSON line per measurement, a markdown table at the end.  Usage: ``python scripts/bench_moe_rows.py
[--part kernel step] [--out profiles/moe_rows/bench.jsonl]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [(768, 2048), (2880, 2880)]
EXPERTS = [(8, 2), (32, 4)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "step"], choices=["kernel", "step"])
    ap.add_argument("--M", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of MXFP4 expert copies a kernel graph rotates over")
    ap.add_argument("--max-copies", type=int, default=24)
    ap.add_argument("--iters", type=int, default=20, help="replays of a step graph per timed round")
    ap.add_argument("--kernel-iters", type=int, default=5, help="replays of a kernel graph per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--at", type=int, default=512, help="tokens every cache holds in the step part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_rows.py measures on the GPU; none found")
    from torchbooster_amd.models import gpt2_small
    from torchbooster_amd.models.gpt import KVCache
    from torchbooster_amd.models.vit import MoE
    from torchbooster_amd.ops.linear import linear_rows, linear_rows_experts, moe_route_rows
    from torchbooster_amd.ops.norm import RMSNorm

    dev, bf = torch.device("cuda", 0), torch.bfloat16
    table = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def med(v):
        return sorted(v)[len(v) // 2]

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

    def capture(fn):
        fn()  # untimed: first-use work
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = fn()
        g.replay()
        return g, keep

    def stack(E, rows, K):
        codes = torch.randint(0, 256, (E, rows, K // 2), device=dev, dtype=torch.uint8)
        mid = 127 - 1 - round(0.5 * torch.log2(torch.tensor(float(K))).item())
        return codes, (mid + torch.randint(-2, 3, (E, rows, K // 32), device=dev)).to(torch.uint8)

    if "kernel" in a.part:
        with torch.no_grad():
            for (K, Fh), (E, top) in ((w, e) for w in WIDTHS for e in EXPERTS):
                torch.manual_seed(K + E)
                copies = max(2, min(a.max_copies, a.ws_mb * (1 << 20) // (E * 3 * Fh * K * 17 // 32)))
                fc1 = [stack(E, 2 * Fh, K) for _ in range(copies)]
                fc2 = [stack(E, K, Fh) for _ in range(copies)]
                with torch.device(dev):
                    moes = [MoE(K, Fh, E, top).to(bf) for _ in range(copies)]
                    norm = RMSNorm(K, eps=1e-6)
                rms = {"rms": (norm.weight, norm.eps)}
                routers = [m.router.weight for m in moes]
                for M in a.M:
                    x = torch.randn(M, K, device=dev).to(bf)
                    ids, gates = moe_route_rows(x, routers[0], top, **rms)
                    h = linear_rows_experts(x, *fc1[0], ids, act="swiglu", **rms)
                    host = ids.tolist()  # (b): the expert of every pair, known on the host
                    distinct = len({e for row in host for e in row})

                    def per_pair(c):
                        a1 = [linear_rows(x[m:m + 1], fc1[c][0][e], mx_scales=fc1[c][1][e], act="swiglu", **rms)
                              for m in range(M) for e in host[m]]
                        return a1, [linear_rows(h[m, j:j + 1], fc2[c][0][e], mx_scales=fc2[c][1][e])
                                    for m in range(M) for j, e in enumerate(host[m])]

                    def fused(c):
                        i, g = moe_route_rows(x, routers[c], top, **rms)
                        return linear_rows_experts(linear_rows_experts(x, *fc1[c], i, act="swiglu", **rms), *fc2[c], i,
                                                   gates=g, residual=x)

                    fns = {
                        "route": lambda c: moe_route_rows(x, routers[c], top, **rms),
                        "fc1": lambda c: linear_rows_experts(x, *fc1[c], ids, act="swiglu", **rms),
                        "fc2": lambda c: linear_rows_experts(h, *fc2[c], ids, gates=gates, residual=x),
                        "fused": fused,
                        "unfused": lambda c: x + moes[c](norm(x)),
                        "per_pair": per_pair,
                    }
                    graphs, keep = {}, []
                    for k, fn in fns.items():
                        graphs[k], out = capture(lambda fn=fn: [fn(c) for c in range(copies)])
                        keep.append(out)
                    torch.cuda.synchronize()
                    t = time_graphs(graphs, copies, a.kernel_iters)
                    for k, v in t.items():
                        emit({"bench": "moe_rows", "variant": k, "M": M, "K": K, "F": Fh, "E": E, "top_k": top,
                              "distinct_experts": distinct, "us_median": round(med(v), 2), "us_min": round(min(v), 2),
                              "us_max": round(max(v), 2), "vs_unfused": round(med(v) / med(t["unfused"]), 3),
                              "vs_per_pair": round(med(v) / med(t["per_pair"]), 3), "weight_copies": copies,
                              "iters": a.kernel_iters, "rounds": a.rounds})
                    cell = " | ".join(f"{med(t[k]):.1f} ({min(t[k]):.1f}-{max(t[k]):.1f})" for k in fns)
                    table.append(f"| {K} / {Fh} | {E} top {top} | {M} ({distinct}) | {cell} | "
                                 f"{med(t['fused']) / med(t['unfused']):.2f} | {med(t['fused']) / med(t['per_pair']):.2f} |")
                    del graphs, keep
                del fc1, fc2, moes

    if "step" in a.part:
        torch.manual_seed(0)
        with torch.device(dev):
            model = gpt2_small(mlp="moe", experts=8, top_k=2, norm="rms", pos="rope").to(bf).eval()
        model.quantize_rows()
        for B in a.batch:
            tokens = torch.randint(0, 50257, (B, a.at), device=dev)
            new = torch.randint(0, 50257, (B,), device=dev)
            graphs, keep = {}, []
            for k, fused in (("default", False), ("fused", True)):
                _, cache = model.prefill(tokens, cache=KVCache(model, B))

                def run(cache=cache, fused=fused):
                    cache.positions.fill_(a.at)
                    return model.decode_step(new, cache, fused=fused)

                graphs[k], out = capture(run)
                keep.append((cache, out))
            torch.cuda.synchronize()
            t = time_graphs(graphs, 1, a.iters)
            for k, v in t.items():
                emit({"bench": "gpt2_small_moe_step", "variant": k, "B": B, "at": a.at,
                      "graph_us_median": round(med(v), 1), "graph_us_min": round(min(v), 1),
                      "graph_us_max": round(max(v), 1), "vs_default": round(med(v) / med(t["default"]), 3),
                      "iters": a.iters, "rounds": a.rounds})
            f_, d_ = t["fused"], t["default"]
            table.append(f"| step B = {B} | {med(d_):.1f} ({min(d_):.1f}-{max(d_):.1f}) | "
                         f"{med(f_):.1f} ({min(f_):.1f}-{max(f_):.1f}) | {med(f_) / med(d_):.2f} |")
    print("\n".join(table))
    return 0


if __name__ == "__main__":
    sys.exit(main())
