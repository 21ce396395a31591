#!/usr/bin/env python
"""Rotary position embeddings: the ``rope_packed`` kernel, a ``gpt2_small`` training step and a decode step,
``pos="rope"`` against ``pos="learned"``.

Kernel part.  ``rope_packed`` on a packed bf16 projection with ``H = 12``, ``D = 64``: the training shape
``--tokens`` (8 x 1024) with ``Hkv`` in ``--kv`` and the decode shapes ``B`` in ``--batch``, ``T`` in ``--T``;
forward and inverse, out of place and in place.  A call is captured into a graph that makes one call per
copy of the input, ``--ws-mb`` of copies in all, so that the large case streams from memory instead of
the last-level cache; replays are timed between two device events, the variants of a shape interleaved
round by round.  ``bytes`` is what the call has to move: out of place every element of the row once in
and once out, in place the rotated ``q | k`` part once in and once out, plus one 256-B table row per token.
With ``--copy-baseline`` the same graph shape is timed for ``Tensor.copy_`` of the packed tensor, the
plain bf16 copy of the same bytes as the out-of-place call.

Train part.  ``gpt2_small`` in bf16 at ``--tokens``: ``utils.step(model.loss(tokens), opt, clip=1.0)`` with
FusedAdamW, ``pos="rope"`` and ``pos="learned"`` alternated round by round, ms per step between device events.

Step part.  ``decode_step`` (default and ``fused=True``) of both models captured into a graph together with
the reset of the positions, every cache at ``--at`` tokens, B in ``--batch``; the rope column has one more
launch per layer.

One JSON line per measurement.  Usage: ``python scripts/bench_rope.py [--part kernel train step]``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, D = 12, 64


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["kernel", "train", "step"], choices=["kernel", "train", "step"])
    ap.add_argument("--kv", type=int, nargs="+", default=[12, 4, 1])
    ap.add_argument("--tokens", type=int, nargs=2, default=[8, 1024], help="B N of the training shape")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--T", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of input copies a kernel graph rotates over")
    ap.add_argument("--max-copies", type=int, default=64)
    ap.add_argument("--kernel-iters", type=int, default=5, help="replays of a kernel graph per timed round")
    ap.add_argument("--iters", type=int, default=20, help="graph replays of a decode step per timed round")
    ap.add_argument("--train-iters", type=int, default=5, help="training steps per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--at", type=int, default=512, help="tokens every cache holds in the step part")
    ap.add_argument("--copy-baseline", action="store_true", help="kernel part: time Tensor.copy_ of the same tensors")
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_rope.py measures on the GPU; none found")
    from torchbooster_amd.ops.attention import rope_packed, rope_table

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def stats(v, nd=2):
        return {"median": round(sorted(v)[len(v) // 2], nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    def time_calls(calls, per_call, iters):
        """Interleaved rounds of ``iters`` calls between device events -> us per unit of work, per variant."""
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
        """one graph that calls ``fn`` once per entry of ``copies_of`` (two untimed calls first)"""
        fn(copies_of[0])
        fn(copies_of[0])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = [fn(c) for c in copies_of]
        g.replay()
        return g, outs

    if "kernel" in a.part:
        table = rope_table(1024, D, device=dev)
        shapes = [(a.tokens[0], a.tokens[1], hkv) for hkv in a.kv] + [(B, T, 12) for B in a.batch for T in a.T]
        with torch.no_grad():
            for B, T, hkv in shapes:
                E = (H + 2 * hkv) * D
                full = B * T * E * 2
                copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // (2 * full))))
                torch.manual_seed(B * T + hkv)
                xs = [torch.randn(B, T, E, device=dev).to(bf) for _ in range(copies)]
                pos = torch.zeros(B, dtype=torch.int32, device=dev)
                graphs, keep, nbytes = {}, [], {}
                for inverse in (False, True):
                    for inplace in (False, True):
                        name = ("inverse" if inverse else "forward") + (" in place" if inplace else "")
                        g, outs = capture(lambda x: rope_packed(x, H, table, pos, kv_heads=hkv, inverse=inverse,
                                                                inplace=inplace), xs)
                        graphs[name] = g.replay
                        keep.append((g, outs))
                        nbytes[name] = (2 * B * T * (H + hkv) * D * 2 if inplace else 2 * full) + B * T * 256
                if a.copy_baseline:
                    dst = [torch.empty_like(x) for x in xs]
                    g, outs = capture(lambda p: p[0].copy_(p[1]), list(zip(dst, xs)))
                    graphs["copy_"] = g.replay
                    keep.append((g, outs))
                    nbytes["copy_"] = 2 * full
                torch.cuda.synchronize()
                for name, v in time_calls(graphs, copies, a.kernel_iters).items():
                    s = stats(v)
                    emit({"bench": "rope_kernel", "tag": a.tag, "variant": name, "B": B, "T": T, "H": H, "Hkv": hkv,
                          "us_median": s["median"], "us_min": s["min"], "us_max": s["max"],
                          "MB": round(nbytes[name] / 1e6, 3), "GBps": round(nbytes[name] / s["median"] * 1e-3, 1),
                          "copies": copies, "iters": a.kernel_iters, "rounds": a.rounds})
                del graphs, keep, xs

    if "train" in a.part:
        from torchbooster_amd import utils
        from torchbooster_amd.models.gpt import gpt2_small
        from torchbooster_amd.ops.optim import FusedAdamW

        B, N = a.tokens
        tokens = torch.randint(0, 50257, (B, N), device=dev)
        steps = {}
        for pos_kind in ("learned", "rope"):
            torch.manual_seed(0)
            model = gpt2_small(pos=pos_kind).to(dev).to(bf)
            opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01)

            def step(model=model, opt=opt):
                utils.step(model.loss(tokens), opt, clip=1.0)

            for _ in range(3):
                step()
            steps[pos_kind] = step
        torch.cuda.synchronize()
        t = time_calls(steps, 1, a.train_iters)
        ref = sorted(t["learned"])[len(t["learned"]) // 2]
        for name, v in t.items():
            s = stats([x / 1e3 for x in v], 3)
            emit({"bench": "rope_train_step", "tag": a.tag, "pos": name, "B": B, "N": N, "ms_median": s["median"],
                  "ms_min": s["min"], "ms_max": s["max"], "vs_learned": round(s["median"] / (ref / 1e3), 4),
                  "iters": a.train_iters, "rounds": a.rounds})
        del steps

    if "step" in a.part:
        from torchbooster_amd.models.gpt import KVCache, gpt2_small

        with torch.no_grad():
            for B in a.batch:
                graphs, keep = {}, []
                tokens = torch.randint(0, 50257, (B, a.at), device=dev)
                new = torch.randint(0, 50257, (B,), device=dev)
                for pos_kind in ("learned", "rope"):
                    torch.manual_seed(0)
                    model = gpt2_small(pos=pos_kind).to(dev).to(bf).eval()
                    _, cache = model.prefill(tokens, cache=KVCache(model, B))
                    for fused in (False, True):
                        def run(_=None, model=model, cache=cache, kw={"fused": True} if fused else {}):
                            cache.positions.fill_(a.at)
                            return model.decode_step(new, cache, **kw)
                        g, outs = capture(run, [None])
                        graphs[(pos_kind, fused)] = g.replay
                        keep.append((g, outs, model, cache))
                torch.cuda.synchronize()
                t = time_calls(graphs, 1, a.iters)
                for (pos_kind, fused), v in t.items():
                    s = stats(v, 1)
                    ref = sorted(t[("learned", fused)])[len(v) // 2]
                    emit({"bench": "rope_decode_step", "tag": a.tag, "pos": pos_kind, "B": B, "fused": fused, "at": a.at,
                          "graph_us_median": s["median"], "graph_us_min": s["min"], "graph_us_max": s["max"],
                          "vs_learned": round(s["median"] / ref, 4), "iters": a.iters, "rounds": a.rounds})
                del graphs, keep
    return 0


if __name__ == "__main__":
    sys.exit(main())
