#!/usr/bin/env python
"""KV-cache decoding: the split-KV ``attn_decode`` kernels alone, and ``gpt2_small`` tokens/s.

Kernel part.  ``attention_decode`` at B*H in {12, 96, 384} and len in {128, 512, 1024, 4096} with
cap = len, for several chunk sizes (``attn_decode_set_chunk``).  A decode step must read
``2 * len * 128`` bytes per (batch, head) -- the visible k and v rows -- and the achieved GB/s is those
bytes over the time of one call (both launches: split and merge).  To keep the host out of the number,
``--inner`` calls are captured into one graph and the graph's replays are timed between two device
events; the calls of a graph rotate over enough cache copies that no call finds its rows in the 256 MB
last-level cache left there by the previous one (at most ``--copies``; the small shapes stay cached
whatever one does, and the JSON line says how many copies a shape used).  Chunk sizes are interleaved
round by round; the median round and the min-max spread are reported.

Model part.  ``gpt2_small`` in bf16, prompt ``--prompt`` tokens, ``--new`` new tokens, greedy, batch in
``--batch``: (a) the recompute loop -- the full ``forward`` on the growing sequence for every token, what
one had to write before ``generate`` existed; (b) ``generate(graph=False)``; (c) ``generate(graph=True)``.
Each variant runs once untimed (code objects, allocator, the GEMM tile tuner's first-use timing of every
shape it meets), then the three are timed in ``--rounds`` interleaved rounds, a host clock around a run
that ends in a device synchronise.  tokens/s = batch * new tokens / time, prefill included in all three.

One JSON line per measurement.  Usage: ``python scripts/bench_decode.py [--part kernel model]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "model"], choices=["kernel", "model"])
    ap.add_argument("--bh", type=int, nargs="+", default=[12, 96, 384])
    ap.add_argument("--len", type=int, nargs="+", default=[128, 512, 1024, 4096])
    ap.add_argument("--chunks", type=int, nargs="+", default=[32, 64, 128, 256])
    ap.add_argument("--inner", type=int, default=32, help="calls per captured graph")
    ap.add_argument("--copies", type=int, default=16, help="most cache copies a graph rotates over")
    ap.add_argument("--iters", type=int, default=20, help="graph replays per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--variants", nargs="+", default=["recompute", "generate", "generate_graph"])
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)

    import torch

    from torchbooster_amd.ops import _ext
    from torchbooster_amd.ops.attention import attention_decode

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    if "kernel" in a.part:
        nat = _ext.native()
        default_chunk = nat.attn_decode_set_chunk(-1)
        H = 12
        for BH in a.bh:
            B = max(BH // H, 1)
            for n in a.len:
                torch.manual_seed(n)
                need = 2 * n * 128 * B * H  # bytes one call must read
                copies = int(min(a.copies, max(1, -(-(512 << 20) // need))))
                q = torch.randn(B, H, 64, device=dev).to(torch.bfloat16)
                caches = [(torch.randn(B, H, n, 64, device=dev).to(torch.bfloat16),
                           torch.randn(B, H, n, 64, device=dev).to(torch.bfloat16)) for _ in range(copies)]
                kl = torch.full((B,), n, dtype=torch.int32, device=dev)
                graphs = {}
                try:
                    for ck in a.chunks:
                        nat.attn_decode_set_chunk(ck)
                        attention_decode(q, *caches[0], kl)  # warm-up outside the capture
                        torch.cuda.synchronize()
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            outs = [attention_decode(q, *caches[i % copies], kl) for i in range(a.inner)]
                        g.replay()
                        graphs[ck] = (g, outs)
                finally:
                    nat.attn_decode_set_chunk(default_chunk)
                torch.cuda.synchronize()
                times = {ck: [] for ck in graphs}
                for _ in range(a.rounds):
                    for ck, (g, _) in graphs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.iters):
                            g.replay()
                        e1.record()
                        e1.synchronize()
                        times[ck].append(e0.elapsed_time(e1) * 1e3 / (a.iters * a.inner))  # us per call
                for ck, v in times.items():
                    med = sorted(v)[len(v) // 2]
                    emit({"bench": "attn_decode", "tag": a.tag, "B": B, "H": H, "len": n, "chunk": ck,
                          "default_chunk": ck == default_chunk, "us_median": round(med, 2), "us_min": round(min(v), 2),
                          "us_max": round(max(v), 2), "bytes": need, "GBps_median": round(need / med * 1e-3, 1),
                          "cache_copies": copies, "inner": a.inner, "iters": a.iters, "rounds": a.rounds})
                del graphs, caches

    if "model" in a.part:
        from torchbooster_amd.models import gpt2_small

        torch.manual_seed(0)
        model = gpt2_small().to(dev).to(torch.bfloat16).eval()
        for B in a.batch:
            tokens = torch.randint(0, 50257, (B, a.prompt), device=dev)

            def recompute():
                cur = tokens
                with torch.no_grad():
                    for _ in range(a.new):
                        cur = torch.cat([cur, model(cur)[:, -1].argmax(-1, keepdim=True)], dim=1)
                return cur[:, a.prompt:]

            runs = {
                "recompute": recompute,
                "generate": lambda: model.generate(tokens, a.new)[0],
                "generate_graph": lambda: model.generate(tokens, a.new, graph=True)[0],
            }
            runs = {k: runs[k] for k in a.variants}
            outs = {}
            for name, fn in runs.items():  # untimed: first-use work of every shape
                outs[name] = fn()
            torch.cuda.synchronize()
            same = {k: bool(torch.equal(v, outs["generate"])) for k, v in outs.items()} if "generate" in outs else {}
            times = {k: [] for k in runs}
            for _ in range(a.rounds):
                for name, fn in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[name].append(time.perf_counter() - t0)
            for name, v in times.items():
                med = sorted(v)[len(v) // 2]
                emit({"bench": "gpt2_small_generate", "tag": a.tag, "variant": name, "B": B, "prompt": a.prompt,
                      "new": a.new, "s_median": round(med, 4), "s_min": round(min(v), 4), "s_max": round(max(v), 4),
                      "tokens_per_s": round(B * a.new / med, 1), "rounds": a.rounds,
                      "tokens_equal_generate": same.get(name)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
