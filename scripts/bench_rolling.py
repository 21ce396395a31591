#!/usr/bin/env python
"""Rolling KV cache: what a ring of about ``W`` rows saves a windowed decode step, a model step and the memory.

Decode part.  ``attention_decode`` with ``H = 12`` query heads (``Hkv`` in ``--kv``), ``B`` in ``--batch``, ``W =
--window``, every sequence at ``len`` in ``--len`` tokens of context.  Three calls, captured into one graph each
and interleaved round by round: ``rolling`` (a ring of ``R = roundup8(W + 15)`` rows, ``lengths = len``,
``rolling=True``), ``linear`` (the windowed call on a cache of ``cap = len`` rows: the code path of the commit
before the rolling cache) and ``short`` (``window=None`` on a cache of ``cap = len = R`` rows: what streaming
``R`` rows costs without any per-slot test).  As in ``bench_window.py`` every call of a graph reads another
copy of the caches; ``rolling`` and ``short`` rotate over the same number of copies of the same size.

Step part.  ``gpt2_small(window=--window)`` (``max_len`` raised to fit ``--at``): ``decode_step`` (default and
``fused=True``) at ``--at`` cached tokens on a ``KVCache`` of full capacity, ``rolling=True`` against the linear
cache, captured into a graph together with the reset of the positions.

Memory part.  ``torch.cuda.memory_allocated`` around the construction of the two caches against the formula
``sum_i 2 * B * Hkv * rows_i * 64 * 2`` bytes.

Replays are timed between two device events; the median round and the min-max spread are reported.  One JSON
line per measurement.  Usage: ``python scripts/bench_rolling.py [--part decode step memory]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 12


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["decode", "step", "memory"], choices=["decode", "step", "memory"])
    ap.add_argument("--kv", type=int, nargs="+", default=[12, 1])
    ap.add_argument("--len", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--batch", type=int, nargs="+", default=[8])
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--at", type=int, nargs="+", default=[512, 4096], help="cached tokens of the decode steps")
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of cache copies a kernel graph rotates over")
    ap.add_argument("--max-copies", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20, help="graph replays of a model step per timed round")
    ap.add_argument("--kernel-iters", type=int, default=3, help="replays of a kernel graph per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_rolling.py measures on the GPU; none found")
    from torchbooster_amd.ops.attention import attention_decode

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    W = a.window
    R = (W + 15 + 7) // 8 * 8  # the ring KVCache(rolling=True) gives a layer of window W at the default lookahead

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def stats(v, nd=2):
        return {"us_median": round(sorted(v)[len(v) // 2], nd), "us_min": round(min(v), nd),
                "us_max": round(max(v), nd)}

    def time_rounds(calls, per_call, iters):
        """Interleaved rounds of ``iters`` calls between device events -> us per call, per variant."""
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
        """One graph that calls ``fn`` once per entry of ``copies_of`` (two untimed calls first)."""
        fn(copies_of[0])
        fn(copies_of[0])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = [fn(c) for c in copies_of]
        g.replay()
        return g, outs

    def caches(B, hkv, n, copies, seed):
        torch.manual_seed(seed)
        return [tuple(torch.randn(B, hkv, n, 64, device=dev).to(bf) for _ in range(2)) for _ in range(copies)]

    def n_copies(B, hkv, n):
        return max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // (B * hkv * n * 64 * 2 * 2))))

    if "decode" in a.part:
        with torch.no_grad():
            for B in a.batch:
                for n in a.len:
                    for hkv in a.kv:
                        q = torch.randn(B, H, 64, device=dev).to(bf)
                        kw = {} if hkv == H else {"kv_heads": hkv}
                        long = caches(B, hkv, n, n_copies(B, hkv, n), n + hkv)
                        rings = caches(B, hkv, R, n_copies(B, hkv, R), R + hkv)
                        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                        lens_r = torch.full((B,), R, dtype=torch.int32, device=dev)
                        variants = {
                            "rolling": (lambda kv: attention_decode(q, kv[0], kv[1], lens, window=W, rolling=True,
                                                                    **kw), rings),
                            "linear": (lambda kv: attention_decode(q, kv[0], kv[1], lens, window=W, **kw), long),
                            "short": (lambda kv: attention_decode(q, kv[0], kv[1], lens_r, **kw), rings),
                        }
                        keep, times = [], {}
                        graphs = {}
                        for name, (fn, cs) in variants.items():
                            g, o = capture(fn, cs)
                            graphs[name] = (g.replay, len(cs))
                            keep.append((g, o))
                        torch.cuda.synchronize()
                        # one per_call per variant: the graphs hold different numbers of calls
                        for _ in range(a.rounds):
                            for name, (replay, per_call) in graphs.items():
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                for _ in range(a.kernel_iters):
                                    replay()
                                e1.record()
                                e1.synchronize()
                                us = e0.elapsed_time(e1) * 1e3 / (a.kernel_iters * per_call)
                                times.setdefault(name, []).append(us)
                        for name, v in times.items():
                            rows = n if name == "linear" else R
                            emit({"bench": "rolling_decode", "tag": a.tag, "variant": name, "B": B, "H": H, "Hkv": hkv,
                                  "context": n if name != "short" else R, "cache_rows": rows,
                                  "window": None if name == "short" else W, **stats(v),
                                  "cache_MB": round(B * hkv * rows * 64 * 2 * 2 / 1e6, 2),
                                  "cache_copies": graphs[name][1], "iters": a.kernel_iters, "rounds": a.rounds})
                        del graphs, keep, long, rings

    if "step" in a.part or "memory" in a.part:
        from torchbooster_amd.models import gpt2_small
        from torchbooster_amd.models.gpt import KVCache

        max_len = max([1024] + [at + 1 for at in a.at])  # the step appends row `at`
        torch.manual_seed(0)
        model = gpt2_small(max_len=max_len, window=W).to(dev).to(bf).eval()

    if "memory" in a.part:
        for B in a.batch:
            for rolling in (False, True):
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                cache = KVCache(model, B, rolling=rolling)
                got = torch.cuda.memory_allocated() - before
                rows = [k.shape[2] for k, _ in cache.layers]
                hkv = cache.layers[0][0].shape[1]
                formula = sum(2 * B * hkv * r * 64 * 2 for r in rows)
                emit({"bench": "rolling_memory", "tag": a.tag, "model": "gpt2_small", "window": W, "B": B,
                      "capacity": cache.capacity, "rolling": rolling, "rows_per_layer": rows[0], "layers": len(rows),
                      "formula_bytes": formula, "allocated_bytes": got,  # + the positions, one allocator block
                      "over_formula_bytes": got - formula})
                del cache

    if "step" in a.part:
        with torch.no_grad():
            for B in a.batch:
                for at in a.at:
                    graphs, keep = {}, []
                    new = torch.randint(0, 50257, (B,), device=dev)
                    for rolling in (False, True):
                        cache = KVCache(model, B, rolling=rolling)
                        for kc, vc in cache.layers:
                            kc.normal_(), vc.normal_()
                        for fused in (False, True):
                            def run(_=None, cache=cache, kw={"fused": True} if fused else {}):
                                cache.positions.fill_(at)
                                return model.decode_step(new, cache, **kw)
                            g, o = capture(run, [None])
                            graphs[(rolling, fused)] = g.replay
                            keep.append((g, o, cache))
                    torch.cuda.synchronize()
                    t = time_rounds(graphs, 1, a.iters)
                    for (rolling, fused), v in t.items():
                        s = stats(v, 1)
                        ref = sorted(t[(False, fused)])[len(v) // 2]
                        emit({"bench": "rolling_decode_step", "tag": a.tag, "model": "gpt2_small", "B": B, "at": at,
                              "window": W, "capacity": max_len, "rolling": rolling, "fused": fused, **s,
                              "vs_linear": round(s["us_median"] / ref, 3), "iters": a.iters, "rounds": a.rounds})
                    del graphs, keep
    return 0


if __name__ == "__main__":
    sys.exit(main())
