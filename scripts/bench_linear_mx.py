#!/usr/bin/env python
"""The MXFP4 GEMM (csrc/gemm_mx.hip) against the bf16 engine, and what it changes in ``linear_rows`` and the model.

``kernel``   ``linear_mx(x, codes, scales, bias)`` against ``ops.linear.linear(x, w, bias)`` on ``w = mx_dequantize(codes,
             scales, bf16)``, P in ``--P`` for (K, Q) in ``PRODUCTS``, and the vocabulary head 768 -> 50257 at P = 32.
``rows``     ``linear_rows(x, codes, bias, mx_scales=scales)`` at 32 and 64 rows for the ``gpt2_small`` products.
``prefill``  ``gpt2_small`` after ``quantize_rows()``: ``prefill`` of 8 x 1024 tokens, ``mx=True`` against ``mx=False``.
``step``     the same model's ``decode_step(fused=True)`` at B = 32, captured in a graph.

As in scripts/bench_rows_mx.py every call of a captured kernel graph reads ANOTHER copy of the weight (``--ws-mb`` of
bf16 copies, as many MX copies), the variants are interleaved round by round between device events, and the median of
``--rounds`` rounds is reported with its min-max spread.  ``rows`` and ``step`` have one variant: run them from a
checkout of the parent commit as well (``--root`` names the tree whose package is imported, ``--label`` tags the
lines) and compare the two files.  One JSON line per measurement, a markdown table at the end.

Usage: ``python scripts/bench_linear_mx.py [--part kernel rows prefill step] [--out profiles/linear_mx/bench.jsonl]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCTS = [(768, 2304), (768, 768), (768, 3072), (3072, 768), (4096, 4096), (4096, 14336)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "rows", "prefill", "step"],
                    choices=["kernel", "rows", "prefill", "step"])
    ap.add_argument("--P", type=int, nargs="+", default=[32, 64, 128, 1024, 8192])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of bf16 weight copies a kernel graph rotates over")
    ap.add_argument("--max-copies", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10, help="replays (calls) of a model graph per timed round")
    ap.add_argument("--kernel-iters", type=int, default=3, help="replays of a kernel graph per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--root", default=ROOT, help="the tree whose torchbooster_amd is measured")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, a.root)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_mx.py measures on the GPU; none found")
    from torchbooster_amd.models import gpt2_small
    from torchbooster_amd.models.gpt import KVCache
    from torchbooster_amd.ops import linear as L

    dev, bf = torch.device("cuda", 0), torch.bfloat16
    table = []

    def emit(rec):
        rec["label"] = a.label
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def med(v):
        return sorted(v)[len(v) // 2]

    def stat(v):
        return {"us_median": round(med(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}

    def cell(v):
        return f"{med(v):.1f} ({min(v):.1f}-{max(v):.1f})"

    def time_rounds(fns, per_call, iters):
        """Interleaved rounds of ``iters`` calls between device events -> us per product, per variant."""
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / (iters * per_call))
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

    def weights(K, Q, P):
        # copies so that neither the weights nor the P x Q results of one replay exceed the budget
        copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // (K * Q * 2 + P * Q * 2))))
        torch.manual_seed(K + Q)
        mx = [L.mx_quantize(torch.randn(Q, K, device=dev) * K ** -0.5) for _ in range(copies)]
        return mx, torch.randn(Q, device=dev).to(bf)

    with torch.no_grad():
        if "kernel" in a.part:
            for K, Q, Ps in [(K, Q, a.P) for K, Q in PRODUCTS] + [(768, 50257, [32])]:
                for P in Ps:
                    mx, bias = weights(K, Q, P)
                    ws = [L.mx_dequantize(c, s, bf) for c, s in mx]
                    x = torch.randn(P, K, device=dev).to(bf)
                    graphs, keep = {}, []
                    for k, fn in {"bf16": lambda: [L.linear(x, w, bias) for w in ws],
                                  "mx": lambda: [L.linear_mx(x, c, s, bias) for c, s in mx]}.items():
                        graphs[k], out = capture(fn)
                        keep.append(out)
                    t = time_rounds({k: g.replay for k, g in graphs.items()}, len(mx), a.kernel_iters)
                    for k, v in t.items():
                        emit({"bench": "linear_mx", "variant": k, "P": P, "K": K, "Q": Q, **stat(v),
                              "tflops": round(2e-6 * P * K * Q / med(v), 1), "mx_vs_bf16": round(med(v) / med(t["bf16"]), 3),
                              "weight_copies": len(mx), "iters": a.kernel_iters, "rounds": a.rounds})
                    r = med(t["mx"]) / med(t["bf16"])
                    table.append(f"| {K} -> {Q} | {P} | {cell(t['bf16'])} | {cell(t['mx'])} | "
                                 + (f"**{r:.2f}**" if r > 1 else f"{r:.2f}") + " |")
                    del graphs, keep, ws, mx

        if "rows" in a.part:
            for K, Q in PRODUCTS[:4]:
                for M in (32, 64):
                    mx, bias = weights(K, Q, M)
                    x = torch.randn(M, K, device=dev).to(bf)
                    g, keep = capture(lambda: [L.linear_rows(x, c, bias, mx_scales=s) for c, s in mx])
                    v = time_rounds({"mx": g.replay}, len(mx), a.kernel_iters)["mx"]
                    emit({"bench": "linear_rows_mx", "M": M, "K": K, "Q": Q, **stat(v), "weight_copies": len(mx),
                          "iters": a.kernel_iters, "rounds": a.rounds})
                    table.append(f"| linear_rows {K} -> {Q} | {M} | {cell(v)} |")
                    del g, keep, mx

        if "prefill" in a.part or "step" in a.part:
            torch.manual_seed(0)
            model = gpt2_small().to(dev).to(bf).eval()
            model.quantize_rows()
        if "prefill" in a.part:
            tokens = torch.randint(0, 50257, (8, 1024), device=dev)
            cache = KVCache(model, 8)
            fns = {k: (lambda kw=kw: model.prefill(tokens, cache=cache, **kw)) for k, kw in
                   (("bf16", {}), ("mx", {"mx": True}))}
            for fn in fns.values():
                fn()
            t = time_rounds(fns, 1, a.iters)
            for k, v in t.items():
                emit({"bench": "gpt2_small_prefill_8x1024", "variant": k, **stat(v),
                      "mx_vs_bf16": round(med(v) / med(t["bf16"]), 3), "iters": a.iters, "rounds": a.rounds})
            table.append(f"| prefill 8 x 1024 | {cell(t['bf16'])} | {cell(t['mx'])} | "
                         f"{med(t['mx']) / med(t['bf16']):.2f} |")
        if "step" in a.part:
            B, at = 32, 512
            _, cache = model.prefill(torch.randint(0, 50257, (B, at), device=dev), cache=KVCache(model, B))
            new = torch.randint(0, 50257, (B,), device=dev)

            def run():
                cache.positions.fill_(at)
                return model.decode_step(new, cache, fused=True)

            g, keep = capture(run)
            v = time_rounds({"mx": g.replay}, 1, a.iters)["mx"]
            emit({"bench": "gpt2_small_mx_step", "B": B, "at": at, **stat(v), "iters": a.iters, "rounds": a.rounds})
            table.append(f"| fused step B = {B} | {cell(v)} |")
    print("\n".join(table))
    return 0


if __name__ == "__main__":
    sys.exit(main())
