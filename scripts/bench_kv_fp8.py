#!/usr/bin/env python
"""FP8 (e4m3) KV cache against the bf16 cache: kernels, model steps, memory and accuracy.

Decode part.  ``attention_decode`` with ``H = 12`` query heads (``Hkv`` in ``--kv``), ``B = --batch``: unwindowed at
every ``--len`` (cache of ``cap = len`` rows), and with ``W = --window`` at ``--wlen`` tokens of context on a linear
cache and on a ring of ``R = roundup8(W + 15)`` rows.  Each shape runs twice in the same process, on a bf16 cache
(the comparator: the code of the commit before this one, csrc instantiations unchanged) and on an fp8 cache of the
same values' codes, captured into one graph each and interleaved round by round.  As in ``bench_rolling.py`` every
call of a graph reads another copy of its caches.  ``GB/s`` counts the cache bytes the visible rows hold.

Extend part.  ``attention_extend`` with ``T = 16`` new tokens at the same unwindowed shapes.

Step part.  ``gpt2_small`` (``max_len`` raised to fit ``--at``): a graph-replayed ``decode_step`` (default and
``fused=True``) at ``--at`` cached tokens, ``B`` in ``--step-batch``, bf16 cache against fp8 cache.

Memory part.  ``torch.cuda.memory_allocated`` around the construction of the two caches against the formula
``sum_i 2 * B * Hkv * rows_i * 64 * itemsize``.

Accuracy part.  Randomly initialised ``gpt2_small``: teacher-forced decode logits on an fp8 cache against the same
steps on a bf16 cache (relative Frobenius error), with scales calibrated by ``kv_scales`` on the prompt and with
unit scales.

Replays are timed between two device events; the median round and the min-max spread are reported.  One JSON line
per measurement.  Usage: ``python scripts/bench_kv_fp8.py [--part decode extend step memory accuracy]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 12
PARTS = ["decode", "extend", "step", "memory", "accuracy"]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=PARTS, choices=PARTS)
    ap.add_argument("--kv", type=int, nargs="+", default=[12, 1])
    ap.add_argument("--len", type=int, nargs="+", default=[512, 4096, 16384])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--wlen", type=int, default=4096, help="context of the windowed decode calls")
    ap.add_argument("--extend-len", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--at", type=int, nargs="+", default=[512, 4096], help="cached tokens of the decode steps")
    ap.add_argument("--step-batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of bf16 cache copies a kernel graph rotates over")
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
        raise SystemExit("bench_kv_fp8.py measures on the GPU; none found")
    from torchbooster_amd.ops.attention import attention_decode, attention_extend, kv_quantize

    dev = torch.device("cuda", 0)
    bf, fp8 = torch.bfloat16, torch.float8_e4m3fn
    W = a.window
    R = (W + 15 + 7) // 8 * 8
    B = a.batch

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def stats(v, nd=2):
        return {"us_median": round(sorted(v)[len(v) // 2], nd), "us_min": round(min(v), nd),
                "us_max": round(max(v), nd)}

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

    def time_graphs(graphs, iters):
        """``graphs``: name -> (replay, calls per replay); interleaved rounds -> us per call, per name."""
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, (replay, per_call) in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    replay()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / (iters * per_call))
        return times

    def cache_pairs(hkv, n, seed):
        """The same number of bf16 and fp8 copies of a [B, hkv, n, 64] cache pair (the codes of the bf16 values)."""
        copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // (B * hkv * n * 64 * 2 * 2))))
        torch.manual_seed(seed)
        wide = [tuple(torch.randn(B, hkv, n, 64, device=dev).to(bf) for _ in range(2)) for _ in range(copies)]
        return wide, [tuple(kv_quantize(c) for c in kv) for kv in wide]

    def kernel_table(bench, call, shapes):
        """``shapes``: (label, hkv, cache rows, visible rows, keywords); ``call(q-like, kv, keywords)``."""
        for label, hkv, rows, seen, kw in shapes:
            wide, narrow = cache_pairs(hkv, rows, rows + hkv)
            graphs, keep = {}, []
            for name, cs in (("bf16", wide), ("fp8", narrow)):
                g, o = capture(lambda kv: call(kv, hkv, kw), cs)
                graphs[name] = (g.replay, len(cs))
                keep.append((g, o))
            torch.cuda.synchronize()
            t = time_graphs(graphs, a.kernel_iters)
            ref = sorted(t["bf16"])[len(t["bf16"]) // 2]
            for name, v in t.items():
                s = stats(v)
                nbytes = B * hkv * seen * 64 * 2 * (2 if name == "bf16" else 1)
                emit({"bench": bench, "tag": a.tag, "cache": name, "shape": label, "B": B, "H": H, "Hkv": hkv,
                      "cache_rows": rows, "rows_seen": seen, **s, "GBps": round(nbytes / s["us_median"] / 1e3, 1),
                      "vs_bf16": round(s["us_median"] / ref, 3), "cache_copies": graphs[name][1],
                      "iters": a.kernel_iters, "rounds": a.rounds})
            del graphs, keep, wide, narrow

    if "decode" in a.part:
        with torch.no_grad():
            q = torch.randn(B, H, 64, device=dev).to(bf)

            def dec(kv, hkv, kw):
                return attention_decode(q, kv[0], kv[1], kw["lengths"], **({} if hkv == H else {"kv_heads": hkv}),
                                        **{k: v for k, v in kw.items() if k != "lengths"})

            def lens(n):
                return torch.full((B,), n, dtype=torch.int32, device=dev)

            shapes = []
            for hkv in a.kv:
                shapes += [(f"len {n}", hkv, n, n, {"lengths": lens(n)}) for n in a.len]
                shapes.append((f"W {W} linear, context {a.wlen}", hkv, a.wlen, W, {"lengths": lens(a.wlen), "window": W}))
                shapes.append((f"W {W} ring of {R}, context {a.wlen}", hkv, R, W,
                               {"lengths": lens(a.wlen), "window": W, "rolling": True}))
            kernel_table("kv_fp8_decode", dec, shapes)

    if "extend" in a.part:
        with torch.no_grad():
            T = 16
            qe = torch.randn(B, T, H, 64, device=dev).to(bf)

            def ext(kv, hkv, kw):
                return attention_extend(qe, kv[0], kv[1], kw["positions"], **({} if hkv == H else {"kv_heads": hkv}))

            shapes = [(f"T {T}, len {n}", hkv, n, n,
                       {"positions": torch.full((B,), n - T, dtype=torch.int32, device=dev)})
                      for hkv in a.kv for n in a.extend_len]
            kernel_table("kv_fp8_extend", ext, shapes)

    if set(a.part) & {"step", "memory", "accuracy"}:
        from torchbooster_amd.models import gpt2_small
        from torchbooster_amd.models.gpt import KVCache, kv_scales

        max_len = max([1024] + [at + 1 for at in a.at])  # the step appends row `at`
        torch.manual_seed(0)
        model = gpt2_small(max_len=max_len).to(dev).to(bf).eval()

    if "memory" in a.part:
        for dtype in (bf, fp8):
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            cache = KVCache(model, B, dtype=dtype)
            got = torch.cuda.memory_allocated() - before
            rows = [k.shape[2] for k, _ in cache.layers]
            size = cache.layers[0][0].element_size()
            formula = sum(2 * B * H * r * 64 * size for r in rows)
            emit({"bench": "kv_fp8_memory", "tag": a.tag, "model": "gpt2_small", "B": B, "capacity": cache.capacity,
                  "cache": "fp8" if dtype == fp8 else "bf16", "rows_per_layer": rows[0], "layers": len(rows),
                  "formula_bytes": formula, "allocated_bytes": got, "over_formula_bytes": got - formula})
            del cache

    if "step" in a.part:
        with torch.no_grad():
            for SB in a.step_batch:
                for at in a.at:
                    graphs, keep = {}, []
                    new = torch.randint(0, 50257, (SB,), device=dev)
                    for dtype in (bf, fp8):
                        cache = KVCache(model, SB, dtype=dtype)
                        for kc, vc in cache.layers:
                            if dtype == fp8:
                                kc.copy_(kv_quantize(torch.randn(kc.shape, device=dev)))
                                vc.copy_(kv_quantize(torch.randn(vc.shape, device=dev)))
                            else:
                                kc.normal_(), vc.normal_()
                        for fused in (False, True):
                            def run(_=None, cache=cache, kw={"fused": True} if fused else {}):
                                cache.positions.fill_(at)
                                return model.decode_step(new, cache, **kw)
                            g, o = capture(run, [None])
                            graphs[("fp8" if dtype == fp8 else "bf16", fused)] = (g.replay, 1)
                            keep.append((g, o, cache))
                    torch.cuda.synchronize()
                    t = time_graphs(graphs, a.iters)
                    for (name, fused), v in t.items():
                        s = stats(v, 1)
                        ref = sorted(t[("bf16", fused)])[len(v) // 2]
                        emit({"bench": "kv_fp8_decode_step", "tag": a.tag, "model": "gpt2_small", "B": SB, "at": at,
                              "capacity": max_len, "cache": name, "fused": fused, **s,
                              "vs_bf16": round(s["us_median"] / ref, 3), "iters": a.iters, "rounds": a.rounds})
                    del graphs, keep

    if "accuracy" in a.part:
        with torch.no_grad():
            g = torch.Generator(device=dev).manual_seed(1)
            seq = torch.randint(0, 50257, (2, 288), device=dev, generator=g)
            n0 = 256

            def logits(**ckw):
                cache = KVCache(model, 2, capacity=seq.shape[1], **ckw)
                model.prefill(seq[:, :n0], cache=cache)
                return torch.stack([model.decode_step(seq[:, t], cache) for t in range(n0, seq.shape[1])], 1).float()

            want = logits()
            sc = kv_scales(model, seq[:, :n0], margin=2.0)
            for name, ckw in (("calibrated, margin 2", {"scales": sc}), ("unit", {})):
                got = logits(dtype=fp8, **ckw)
                emit({"bench": "kv_fp8_accuracy", "tag": a.tag, "model": "gpt2_small (random init)", "scales": name,
                      "prompt": n0, "steps": seq.shape[1] - n0,
                      "rel_err_vs_bf16_cache": round(((got - want).norm() / want.norm()).item(), 5),
                      "argmax_agree": round((got.argmax(-1) == want.argmax(-1)).float().mean().item(), 4),
                      "k_scale_range": [round(min(p[0] for p in sc), 6), round(max(p[0] for p in sc), 6)],
                      "v_scale_range": [round(min(p[1] for p in sc), 6), round(max(p[1] for p in sc), 6)]})
    return 0


if __name__ == "__main__":
    sys.exit(main())
