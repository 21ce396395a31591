#!/usr/bin/env python
"""Forward + backward time of ``attention_packed``: dense, causal and half-length key masks.

The masked kernels skip the key tiles no query of a workgroup sees (csrc/attention.hip), so a
causal call should approach the tile ratio below and a half-length call one half of dense.  Stock
``F.scaled_dot_product_attention`` (causal, and dense) runs beside them for the record.

Method: every variant of a shape is warmed up, then timed in ``--rounds`` interleaved rounds (variant
A, B, C, ... A, B, C, ...) of ``--iters`` forward + backward calls between two device events; the
median round and the min-max spread are reported.  One JSON line per (shape, variant) and a table.

``--tree PATH`` imports ``torchbooster_amd`` from another checkout (its own build), and
``--variants dense`` restricts the run to what an older checkout knows: two processes alternated on
one box give a before / after of the dense kernels.

Usage: ``python scripts/bench_attention.py [--n 197 1024 2048] [--batch 8] [--heads 12]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def causal_tile_ratio(n: int, blk: int = 128, tile: int = 64) -> float:
    """Key tiles the causal forward / dQ kernels visit over those of the dense ones."""
    nt = -(-n // tile)
    visited = sum(-(-min(n, x * blk + blk) // tile) for x in range(-(-n // blk)))
    return visited / (nt * -(-n // blk))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[197, 1024, 2048])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--variants", nargs="+", default=["dense", "causal", "half", "stock_causal", "stock_dense"])
    ap.add_argument("--tree", default=ROOT, help="checkout to import torchbooster_amd from")
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.tree))

    import torch
    import torch.nn.functional as F

    from torchbooster_amd.ops.attention import attention_packed

    if not torch.cuda.is_available():
        raise SystemExit("bench_attention.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    B, H, D = a.batch, a.heads, 64
    lines = []
    for N in a.n:
        torch.manual_seed(N)
        qkv = torch.randn(B, N, 3 * H * D, device=dev).to(torch.bfloat16).requires_grad_()
        g = torch.randn(B, N, H * D, device=dev).to(torch.bfloat16)
        half = torch.full((B,), max(N // 2, 1), dtype=torch.int32, device=dev)

        def stock(causal):
            t = qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
            return F.scaled_dot_product_attention(t[0], t[1], t[2], is_causal=causal).transpose(1, 2).reshape(B, N, H * D)

        calls = {
            "dense": lambda: attention_packed(qkv, H),
            "causal": lambda: attention_packed(qkv, H, causal=True),
            "half": lambda: attention_packed(qkv, H, key_lengths=half),
            "stock_causal": lambda: stock(True),
            "stock_dense": lambda: stock(False),
        }
        calls = {k: calls[k] for k in a.variants}

        def step(fn):
            qkv.grad = None
            fn().backward(g)

        for fn in calls.values():  # warm-up: code objects, allocator, library heuristics
            for _ in range(5):
                step(fn)
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(a.rounds):
            for name, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    step(fn)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.iters)  # us per forward + backward
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for name, v in times.items():
            rec = {"bench": "attention_packed_fwd_bwd", "tag": a.tag, "B": B, "H": H, "N": N, "variant": name,
                   "us_median": round(med[name], 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                   "iters": a.iters, "rounds": a.rounds}
            if "dense" in med and name != "dense":
                rec["vs_dense"] = round(med[name] / med["dense"], 3)
            if name == "causal":
                rec["causal_tile_ratio"] = round(causal_tile_ratio(N), 3)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
