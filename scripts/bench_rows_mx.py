#!/usr/bin/env python
"""MXFP4 weight-only decoding against bf16: the few-row kernel alone and one ``gpt2_small`` step.

Kernel part.  ``linear_rows(x, codes, mx_scales=scales)`` against ``linear_rows(x, weight)`` on the bf16
weight the codes stand for, M in {1, 4, 8, 16}, for (K, Q) in ``PRODUCTS``.  As in
scripts/bench_decode_fused.py every call of a captured graph reads ANOTHER copy of the weight (``--ws-mb`` of
bf16 copies, the same number of MX copies), so no weight sits in the last-level cache between calls; a
graph's replays are timed between two device events, the variants interleaved round by round, and the
median of ``--rounds`` rounds is reported with its min-max spread and the weight bytes per second it amounts
to (MX: codes + scales, 17 bytes per 32 weights).  ``fma_per_ns``: the M * K * Q multiply-adds per nanosecond,
the unpack + fma side of the kernel.

Step part.  ``gpt2_small`` in bf16, every cache at ``--at`` tokens, ``decode_step(fused=True)`` at B in
``--batch`` captured in a graph with the reset of the positions, after ``quantize_rows()`` against before,
interleaved as above; and the relative Frobenius distance of the two logits (a statement about the format
on a randomly initialised model).

One JSON line per measurement, a markdown table at the end.  Usage: ``python scripts/bench_rows_mx.py
[--part kernel step] [--out profiles/rows_mx/bench.jsonl]``.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCTS = [(768, 2304), (768, 3072), (3072, 768), (768, 50257), (4096, 4096), (4096, 14336)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "step"], choices=["kernel", "step"])
    ap.add_argument("--M", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of bf16 weight copies a kernel graph rotates over")
    ap.add_argument("--max-copies", type=int, default=192)
    ap.add_argument("--iters", type=int, default=20, help="replays of a step graph per timed round")
    ap.add_argument("--kernel-iters", type=int, default=3, help="replays of a kernel graph per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--at", type=int, default=512, help="tokens every cache holds in the step part")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_rows_mx.py measures on the GPU; none found")
    from torchbooster_amd.models import gpt2_small
    from torchbooster_amd.models.gpt import KVCache
    from torchbooster_amd.ops.linear import linear_rows, mx_dequantize, mx_quantize

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

    if "kernel" in a.part:
        with torch.no_grad():
            for K, Q in PRODUCTS:
                nbytes = {"bf16": K * Q * 2, "mx": K * Q // 2 + K * Q // 32}
                copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // nbytes["bf16"])))
                torch.manual_seed(K + Q)
                mx = [mx_quantize(torch.randn(Q, K, device=dev) * K ** -0.5) for _ in range(copies)]
                ws = [mx_dequantize(c, s, bf) for c, s in mx]
                bias = None if Q == 50257 else torch.randn(Q, device=dev).to(bf)
                for M in a.M:
                    x = torch.randn(M, K, device=dev).to(bf)
                    graphs, keep = {}, []
                    for k, fn in {"bf16": lambda: [linear_rows(x, w, bias) for w in ws],
                                  "mx": lambda: [linear_rows(x, c, bias, mx_scales=s) for c, s in mx]}.items():
                        graphs[k], out = capture(fn)
                        keep.append(out)
                    torch.cuda.synchronize()
                    t = time_graphs(graphs, copies, a.kernel_iters)
                    for k, v in t.items():
                        emit({"bench": "rows_linear_mx", "variant": k, "M": M, "K": K, "Q": Q,
                              "us_median": round(med(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                              "weight_GBps": round(nbytes[k] / med(v) * 1e-3, 1),
                              "fma_per_ns": round(M * K * Q / med(v) * 1e-3, 1),
                              "mx_vs_bf16": round(med(v) / med(t["bf16"]), 3), "weight_copies": copies,
                              "iters": a.kernel_iters, "rounds": a.rounds})
                    m_, b_ = t["mx"], t["bf16"]
                    table.append(f"| {K} -> {Q} | {M} | {med(b_):.2f} ({min(b_):.2f}-{max(b_):.2f}) | "
                                 f"{nbytes['bf16'] / med(b_) * 1e-3:.0f} | {med(m_):.2f} ({min(m_):.2f}-{max(m_):.2f}) | "
                                 f"{nbytes['mx'] / med(m_) * 1e-3:.0f} | {M * K * Q / med(m_) * 1e-3:.0f} | "
                                 f"{med(m_) / med(b_):.2f} |")
                    del graphs, keep
                del ws, mx

    if "step" in a.part:
        torch.manual_seed(0)
        model = gpt2_small().to(dev).to(bf).eval()
        qmodel = copy.deepcopy(model)
        qmodel.quantize_rows()
        for B in a.batch:
            tokens = torch.randint(0, 50257, (B, a.at), device=dev)
            new = torch.randint(0, 50257, (B,), device=dev)
            graphs, outs, keep = {}, {}, []
            for k, mdl in (("bf16", model), ("mx", qmodel)):
                _, cache = mdl.prefill(tokens, cache=KVCache(mdl, B))

                def run(mdl=mdl, cache=cache):
                    cache.positions.fill_(a.at)
                    return mdl.decode_step(new, cache, fused=True)

                graphs[k], outs[k] = capture(run)
                keep.append(cache)
            torch.cuda.synchronize()
            t = time_graphs(graphs, 1, a.iters)
            dist = ((outs["mx"].double() - outs["bf16"].double()).norm() / outs["bf16"].double().norm()).item()
            for k, v in t.items():
                emit({"bench": "gpt2_small_mx_step", "variant": k, "B": B, "at": a.at,
                      "graph_us_median": round(med(v), 1), "graph_us_min": round(min(v), 1),
                      "graph_us_max": round(max(v), 1), "mx_vs_bf16": round(med(v) / med(t["bf16"]), 3),
                      "logits_rel_distance": round(dist, 4), "iters": a.iters, "rounds": a.rounds})
            m_, b_ = t["mx"], t["bf16"]
            table.append(f"| step B = {B} | {med(b_):.1f} ({min(b_):.1f}-{max(b_):.1f}) | "
                         f"{med(m_):.1f} ({min(m_):.1f}-{max(m_):.1f}) | {med(m_) / med(b_):.2f} | {dist:.3f} |")
    print("\n".join(table))
    return 0


if __name__ == "__main__":
    sys.exit(main())
