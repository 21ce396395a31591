#!/usr/bin/env python
"""Sliding-window attention: what a window saves a decode step, a training call and a model step.

Decode part.  ``attention_decode`` with ``H = 12`` query heads (``Hkv`` in ``--kv``), ``B`` in ``--batch``,
every sequence at ``len = cap`` in ``--len``, ``W = --window``.  Three calls, captured into one graph
each and interleaved round by round: ``window`` (this length, windowed), ``full`` (this length,
``window=None``) and ``short`` (``window=None`` on a cache of ``cap = len = W``: the rows a windowed call
streams, without the waves that write "empty").  As in ``bench_gqa.py`` every call of a graph reads
another copy of the caches (``--ws-mb`` of copies in all), so the last-level cache does not serve them.
``--no-window`` times ``full`` alone: run from a checkout of another commit it is that commit's kernel.

Train part.  ``attention`` forward + backward, ``B * H = 8 * 12``, ``N`` in ``--train-len``: ``causal`` with
and without the window, interleaved, with the key tiles (64 keys x 128 queries of a workgroup) each
visits in the forward.

Step part.  ``gpt2_small`` (``max_len`` raised to fit ``--at``) with and without ``window=--step-window``: a
training step at 8 x 1024 tokens (loss, backward; no optimizer), and ``decode_step`` (default and
``fused=True``) with every cache at ``--at`` tokens, captured into a graph together with the reset of the
positions.

Replays are timed between two device events; the median round and the min-max spread are reported.
One JSON line per measurement.  Usage: ``python scripts/bench_window.py [--part decode train step]``.
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
    ap.add_argument("--part", nargs="+", default=["decode", "train", "step"], choices=["decode", "train", "step"])
    ap.add_argument("--kv", type=int, nargs="+", default=[12, 1])
    ap.add_argument("--len", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--batch", type=int, nargs="+", default=[8])
    ap.add_argument("--window", type=int, default=512)
    ap.add_argument("--no-window", action="store_true", help="decode part: time the unwindowed call alone")
    ap.add_argument("--train-len", type=int, nargs="+", default=[4096])
    ap.add_argument("--at", type=int, nargs="+", default=[512, 4096], help="cached tokens of the decode steps")
    ap.add_argument("--step-window", type=int, default=256)
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
        raise SystemExit("bench_window.py measures on the GPU; none found")
    from torchbooster_amd.ops.attention import attention, attention_decode

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16

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

    if "decode" in a.part:
        W = a.window
        with torch.no_grad():
            for B in a.batch:
                for n in a.len:
                    for hkv in a.kv:
                        nbytes = B * hkv * n * 64 * 2 * 2
                        copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // nbytes)))
                        q = torch.randn(B, H, 64, device=dev).to(bf)
                        kw = {} if hkv == H else {"kv_heads": hkv}
                        long = caches(B, hkv, n, copies, n + hkv)
                        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                        graphs, keep = {}, []
                        g, o = capture(lambda kv: attention_decode(q, kv[0], kv[1], lens, **kw), long)
                        graphs["full"] = g.replay
                        keep.append((g, o))
                        if not a.no_window:
                            g, o = capture(lambda kv: attention_decode(q, kv[0], kv[1], lens, window=W, **kw), long)
                            graphs["window"] = g.replay
                            keep.append((g, o))
                            short, lens_w = caches(B, hkv, W, copies, W + hkv), torch.full((B,), W, dtype=torch.int32,
                                                                                           device=dev)
                            g, o = capture(lambda kv: attention_decode(q, kv[0], kv[1], lens_w, **kw), short)
                            graphs["short"] = g.replay
                            keep.append((g, o))
                        torch.cuda.synchronize()
                        t = time_rounds(graphs, copies, a.kernel_iters)
                        for name, v in t.items():
                            rows = n if name == "full" else W
                            emit({"bench": "window_decode", "tag": a.tag, "variant": name, "B": B, "H": H, "Hkv": hkv,
                                  "len": n if name != "short" else W, "cap": n if name != "short" else W,
                                  "window": W if name == "window" else None, **stats(v),
                                  "rows_streamed_MB": round(B * hkv * rows * 64 * 2 * 2 / 1e6, 2),
                                  "cache_copies": copies, "iters": a.kernel_iters, "rounds": a.rounds})
                        del graphs, keep, long

    if "train" in a.part:
        W, B = a.window, 8
        for N in a.train_len:
            torch.manual_seed(N)
            q, k, v = (torch.randn(B, H, N, 64, device=dev).to(bf).requires_grad_() for _ in range(3))
            do = torch.randn(B, H, N, 64, device=dev).to(bf)

            def fwd_bwd(window):
                o = attention(q, k, v, causal=True, window=window)
                o.backward(do)
                q.grad = k.grad = v.grad = None

            def fwd(window):
                with torch.no_grad():
                    attention(q, k, v, causal=True, window=window)

            for fn in (fwd_bwd, fwd):
                fn(None), fn(W)
            torch.cuda.synchronize()
            t = time_rounds({("fwd+bwd", None): lambda: fwd_bwd(None), ("fwd+bwd", W): lambda: fwd_bwd(W),
                             ("fwd", None): lambda: fwd(None), ("fwd", W): lambda: fwd(W)}, 1, a.kernel_iters)
            # key tiles a 128-query workgroup stages in the forward: up to its last query, from its first query's window
            tiles = {None: sum(-(-min(N, x + 128) // 64) for x in range(0, N, 128))}
            tiles[W] = sum(-(-min(N, x + 128) // 64) - max(0, x + 1 - W) // 64 for x in range(0, N, 128))
            for (what, w), vv in t.items():
                emit({"bench": "window_train", "tag": a.tag, "what": what, "B": B, "H": H, "N": N, "window": w,
                      **stats(vv, 1), "fwd_key_tiles_per_head": tiles[w],
                      "tile_ratio": round(tiles[w] / tiles[None], 3), "iters": a.kernel_iters, "rounds": a.rounds})

    if "step" in a.part:
        from torchbooster_amd.models import gpt2_small
        from torchbooster_amd.models.gpt import KVCache

        W = a.step_window
        max_len = max([1024] + [at + 1 for at in a.at])  # the step appends row `at`
        models = {}
        for w in (None, W):
            torch.manual_seed(0)
            models[w] = gpt2_small(max_len=max_len, window=w).to(dev).to(bf)
        tokens = torch.randint(0, 50257, (8, 1024), device=dev)

        def train(w):
            m = models[w]
            m.loss(tokens).backward()
            for p in m.parameters():
                p.grad = None

        for w in models:
            train(w), train(w)
        torch.cuda.synchronize()
        t = time_rounds({w: (lambda w=w: train(w)) for w in models}, 1, 2)
        ref = sorted(t[None])[len(t[None]) // 2]
        for w, v in t.items():
            s = stats(v, 0)
            emit({"bench": "window_train_step", "tag": a.tag, "model": "gpt2_small", "tokens": "8x1024", "window": w,
                  **s, "vs_no_window": round(s["us_median"] / ref, 3), "iters": 2, "rounds": a.rounds})
        with torch.no_grad():
            for B in a.batch:
                for at in a.at:
                    graphs, keep = {}, []
                    new = torch.randint(0, 50257, (B,), device=dev)
                    for w, model in models.items():
                        model.eval()
                        cache = KVCache(model, B, capacity=at + 1)
                        for kc, vc in cache.layers:
                            kc.normal_(), vc.normal_()
                        for fused in (False, True):
                            def run(_=None, model=model, cache=cache, kw={"fused": True} if fused else {}):
                                cache.positions.fill_(at)
                                return model.decode_step(new, cache, **kw)
                            g, o = capture(run, [None])
                            graphs[(w, fused)] = g.replay
                            keep.append((g, o, cache))
                    torch.cuda.synchronize()
                    t = time_rounds(graphs, 1, a.iters)
                    for (w, fused), v in t.items():
                        s = stats(v, 1)
                        ref = sorted(t[(None, fused)])[len(v) // 2]
                        emit({"bench": "window_decode_step", "tag": a.tag, "model": "gpt2_small", "B": B, "at": at,
                              "window": w, "fused": fused, **s, "vs_no_window": round(s["us_median"] / ref, 3),
                              "iters": a.iters, "rounds": a.rounds})
                    del graphs, keep
    return 0


if __name__ == "__main__":
    sys.exit(main())
