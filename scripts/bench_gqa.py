#!/usr/bin/env python
"""Grouped-query attention: the shared-load decode kernel against the one-head-per-wave kernel on the
expanded cache, the head-block size, one ``gpt2_small``-shaped decode step per ``kv_heads``, and extend.

Kernel part.  ``attention_decode`` with ``H = 12`` query heads, ``Hkv`` in ``--kv``, every sequence at
``len = cap`` in ``--len``, B in ``--batch``.  Variants, captured into one graph each and interleaved
round by round: ``gqa`` (``kv_heads=Hkv``, the default head block), ``expanded`` (the same queries on the
cache expanded with ``repeat_interleave``, no ``kv_heads``: the kernel and the bytes of plain multi-head
attention) and ``gb1`` .. ``gb4`` (the head block forced where it divides ``G`` and is not what ``gqa``
already runs; ``gb1`` is the head mapping alone, where only the L2 can serve the group's repeats; ``--no-expanded`` times these alone,
for batch sizes at which the expanded copies would not fit).  A cache of 1.5 - 100 MB would sit
in the last-level cache between calls, which it does not in a model step that streams the weights in
between: every call of a graph reads ANOTHER copy of the caches, ``--ws-mb`` of copies in all.  Replays
are timed between two device events; the median round and the min-max spread are reported, with the
bytes of cache per second the median amounts to (the bytes the variant's cache holds: ``G`` times fewer
for ``gqa`` than for ``expanded``).

Step part.  ``TransformerLM(50257, 768, 12, 12, 1024, kv_heads=Hkv)`` in bf16, every cache at ``--at``
tokens: cache bytes, and ``decode_step`` (default and ``fused=True``) captured into a graph together with
the reset of the positions, timed as above.

Extend part.  ``attention_extend`` of ``--T`` tokens, ``H = 12``, ``Hkv = 4``, against the expanded cache;
with the tiles of 16 queries the kernel runs (one query head per tile: ``B * H * ceil(T / 16)``) and the
tiles a kernel that packed the ``(t, g)`` rows of a group into one tile would run
(``B * Hkv * ceil(T * G / 16)``).

One JSON line per measurement.  Usage: ``python scripts/bench_gqa.py [--part kernel step extend]``.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 12


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "step", "extend"], choices=["kernel", "step", "extend"])
    ap.add_argument("--kv", type=int, nargs="+", default=[12, 6, 4, 2, 1])
    ap.add_argument("--len", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of cache copies a kernel graph rotates over")
    ap.add_argument("--max-copies", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20, help="graph replays of a model step per timed round")
    ap.add_argument("--kernel-iters", type=int, default=3, help="replays of a kernel graph per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-expanded", action="store_true",
                    help="kernel part: leave the expanded-cache baseline out (head-block sweeps at large B * len)")
    ap.add_argument("--at", type=int, default=512, help="tokens every cache holds in the step part")
    ap.add_argument("--step-kv", type=int, nargs="+", default=[12, 4, 1])
    ap.add_argument("--blocks", type=int, nargs="+", default=[1, 2, 3, 4], help="forced head blocks of the kernel part")
    ap.add_argument("--T", type=int, nargs="+", default=[5])
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_gqa.py measures on the GPU; none found")
    from torchbooster_amd.ops._ext import native
    from torchbooster_amd.ops.attention import attention_decode, attention_extend

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    nat = native()

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

    def capture(graphs, name, fn, copies_of):
        """graphs[name] = one graph that calls ``fn`` once per entry of ``copies_of`` (two untimed calls
        first); returns the outputs, which the caller keeps alive."""
        fn(copies_of[0])
        fn(copies_of[0])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = [fn(c) for c in copies_of]
        g.replay()
        graphs[name] = g
        return outs

    def caches(B, hkv, n, copies, seed):
        torch.manual_seed(seed)
        return [tuple(torch.randn(B, hkv, n, 64, device=dev).to(bf) for _ in range(2)) for _ in range(copies)]

    @contextlib.contextmanager
    def head_block(gb):
        old = nat.attn_decode_set_head_block(gb)
        try:
            yield
        finally:
            nat.attn_decode_set_head_block(old)

    with torch.no_grad():
        if "kernel" in a.part:
            for B in a.batch:
                for n in a.len:
                    full_bytes = B * H * n * 64 * 2 * 2
                    copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // full_bytes)))
                    lengths = torch.full((B,), n, dtype=torch.int32, device=dev)
                    q = torch.randn(B, H, 64, device=dev).to(bf)
                    for hkv in a.kv:
                        G = H // hkv
                        small = caches(B, hkv, n, copies, n + hkv)

                        def gqa(kv):
                            return attention_decode(q, kv[0], kv[1], lengths, kv_heads=hkv)

                        graphs, keep, big = {}, [], None
                        if not a.no_expanded:
                            big = [tuple(c.repeat_interleave(G, dim=1) for c in kv) for kv in small]
                            keep.append(capture(graphs, "expanded",
                                                lambda kv: attention_decode(q, kv[0], kv[1], lengths), big))
                        keep.append(capture(graphs, "gqa", gqa, small))
                        for gb in a.blocks:
                            if G > 1 and G % gb == 0 and gb != nat.attn_decode_head_block(B, H, hkv, n):
                                with head_block(gb):  # the grid is fixed at capture
                                    keep.append(capture(graphs, f"gb{gb}", gqa, small))
                        torch.cuda.synchronize()
                        assert all(torch.equal(keep[0][0], k[0]) for k in keep), "bits differ between the variants"
                        t = time_graphs(graphs, copies, a.kernel_iters)
                        ref = None if a.no_expanded else sorted(t["expanded"])[len(t["expanded"]) // 2]
                        for name, v in t.items():
                            s = stats(v)
                            nbytes = full_bytes if name == "expanded" else full_bytes // G
                            emit({"bench": "gqa_decode", "tag": a.tag, "variant": name, "B": B, "H": H, "Hkv": hkv,
                                  "len": n, "head_block": 1 if name == "expanded" else
                                  (int(name[2:]) if name.startswith("gb") else nat.attn_decode_head_block(B, H, hkv, n)),
                                  "us_median": s["median"], "us_min": s["min"], "us_max": s["max"],
                                  "cache_MB": round(nbytes / 1e6, 2), "cache_GBps": round(nbytes / s["median"] * 1e-3, 1),
                                  "vs_expanded": None if ref is None else round(s["median"] / ref, 3),
                                  "cache_copies": copies, "iters": a.kernel_iters, "rounds": a.rounds})
                        del graphs, keep, small, big

        if "extend" in a.part:
            hkv, G = 4, 3
            for B in a.batch:
                for n in a.len[:1] + [512]:
                    for T in a.T:
                        full_bytes = B * H * n * 64 * 2 * 2
                        copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // full_bytes)))
                        small = caches(B, hkv, n, copies, n + T)
                        big = [tuple(c.repeat_interleave(G, dim=1) for c in kv) for kv in small]
                        pos = torch.full((B,), n - T, dtype=torch.int32, device=dev)
                        q = torch.randn(B, T, H, 64, device=dev).to(bf)
                        graphs = {}
                        keep = [capture(graphs, "expanded", lambda kv: attention_extend(q, kv[0], kv[1], pos), big),
                                capture(graphs, "gqa",
                                        lambda kv: attention_extend(q, kv[0], kv[1], pos, kv_heads=hkv), small)]
                        torch.cuda.synchronize()
                        assert torch.equal(keep[0][0], keep[1][0]), "bits differ from the expanded cache"
                        t = time_graphs(graphs, copies, a.kernel_iters)
                        ref = sorted(t["expanded"])[len(t["expanded"]) // 2]
                        for name, v in t.items():
                            s = stats(v)
                            emit({"bench": "gqa_extend", "tag": a.tag, "variant": name, "B": B, "H": H, "Hkv": hkv,
                                  "T": T, "len": n, "tiles": B * H * -(-T // 16),
                                  "tiles_if_group_packed": B * hkv * -(-T * G // 16),
                                  "nsplit": nat.attn_extend_splits(B, H, T, n),
                                  "us_median": s["median"], "us_min": s["min"], "us_max": s["max"],
                                  "vs_expanded": round(s["median"] / ref, 3), "cache_copies": copies,
                                  "iters": a.kernel_iters, "rounds": a.rounds})
                        del graphs, keep, small, big

        if "step" in a.part:
            from torchbooster_amd.models.gpt import KVCache, TransformerLM

            for B in a.batch:
                graphs, keep, info = {}, [], {}
                tokens = torch.randint(0, 50257, (B, a.at), device=dev)
                new = torch.randint(0, 50257, (B,), device=dev)
                for hkv in a.step_kv:
                    torch.manual_seed(0)
                    model = TransformerLM(50257, 768, 12, H, 1024, kv_heads=hkv).to(dev).to(bf).eval()
                    _, cache = model.prefill(tokens, cache=KVCache(model, B))
                    info[hkv] = sum(c.numel() * 2 for kv in cache.layers for c in kv), \
                        sum(c[:, :, :a.at].numel() * 2 for kv in cache.layers for c in kv)
                    for fused in (False, True):
                        def run(_=None, model=model, cache=cache, kw={"fused": True} if fused else {}):
                            cache.positions.fill_(a.at)
                            return model.decode_step(new, cache, **kw)
                        keep.append((capture(graphs, (hkv, fused), run, [None]), model, cache))
                torch.cuda.synchronize()
                t = time_graphs(graphs, 1, a.iters)
                for (hkv, fused), v in t.items():
                    s = stats(v, 1)
                    ref = sorted(t[(H, fused)])[len(v) // 2] if (H, fused) in t else None
                    emit({"bench": "gqa_decode_step", "tag": a.tag, "B": B, "H": H, "Hkv": hkv, "fused": fused,
                          "at": a.at, "cache_MB": round(info[hkv][0] / 1e6, 1),
                          "cache_read_per_step_MB": round(info[hkv][1] / 1e6, 1),
                          "graph_us_median": s["median"], "graph_us_min": s["min"], "graph_us_max": s["max"],
                          "vs_kv12": None if ref is None else round(s["median"] / ref, 3),
                          "iters": a.iters, "rounds": a.rounds})
                del graphs, keep
    return 0


if __name__ == "__main__":
    sys.exit(main())
