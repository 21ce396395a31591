#!/usr/bin/env python
"""QK-norm: the fused ``qk_norm_rope_packed`` kernels against ``rope_packed`` alone and against the unfused
composition, and ``gpt2_small(pos="rope", norm="rms")`` with and without ``qk_norm``.

Kernel part.  A packed bf16 projection of ``--tokens`` (8 x 1024) with ``H = Hkv = 12``, ``D = 64``.  Variants:
``rope`` (``rope_packed``), ``fused`` (``qk_norm_rope_packed``) and ``unfused`` (``rms_norm`` on the q and the k
view of the projection, a ``cat`` with the value part, ``rope_packed``) -- each forward out of place, forward in
place (unfused: the rotation alone is in place) and forward + backward (gradients of the projection and, where
there are any, of both weights).  A variant is captured into a graph that makes one call per copy of the input,
``--ws-mb`` of copies in all, so that it streams from memory instead of the last-level cache; replays are timed
between two device events, all variants interleaved round by round, medians and spreads over ``--rounds``.

Train part.  ``utils.step(model.loss(tokens), opt, clip=1.0)`` with FusedAdamW in bf16 at ``--tokens``, ``qk_norm``
on and off alternated round by round.  Step part: ``decode_step(fused=True)`` of both models captured into a graph
with the reset of the positions, every cache at ``--at`` tokens, B in ``--batch``.

One JSON line per measurement into ``<out-dir>/bench.jsonl`` and a table of them into ``<out-dir>/README.md``.
Usage: ``python scripts/bench_qk_norm.py [--part kernel train step] [--out-dir profiles/qk_norm]``.
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
    ap.add_argument("--tokens", type=int, nargs=2, default=[8, 1024], help="B N of the training shape")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--ws-mb", type=int, default=512, help="bytes of input copies a kernel graph runs over")
    ap.add_argument("--kernel-iters", type=int, default=5, help="replays of a kernel graph per timed round")
    ap.add_argument("--iters", type=int, default=20, help="graph replays of a decode step per timed round")
    ap.add_argument("--train-iters", type=int, default=5, help="training steps per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--at", type=int, default=512, help="tokens every cache holds in the step part")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "qk_norm"))
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_qk_norm.py measures on the GPU; none found")
    from torchbooster_amd.ops.attention import qk_norm_rope_packed, rope_packed, rope_table
    from torchbooster_amd.ops.norm import rms_norm

    dev, bf = torch.device("cuda", 0), torch.bfloat16
    os.makedirs(a.out_dir, exist_ok=True)
    records = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)

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
        B, T = a.tokens
        E, W = 3 * H * D, H * D
        table = rope_table(max(T, 1024), D, device=dev)
        pos = torch.zeros(B, dtype=torch.int32, device=dev)
        copies = max(2, min(64, -(-a.ws_mb * (1 << 20) // (4 * B * T * E))))
        torch.manual_seed(0)
        xs = [torch.randn(B, T, E, device=dev).to(bf).requires_grad_() for _ in range(copies)]
        gy = torch.randn(B, T, E, device=dev).to(bf)
        qw, kw = ((1 + 0.5 * torch.randn(D, device=dev)).requires_grad_() for _ in range(2))

        def unfused(x, inplace=False):
            q = rms_norm(x[..., :W].reshape(B, T, H, D), qw, 1e-6).reshape(B, T, W)
            k = rms_norm(x[..., W:2 * W].reshape(B, T, H, D), kw, 1e-6).reshape(B, T, W)
            return rope_packed(torch.cat((q, k, x[..., 2 * W:]), dim=-1), H, table, pos, inplace=inplace)

        fwd = {"rope": lambda x, inplace=False: rope_packed(x, H, table, pos, inplace=inplace),
               "fused": lambda x, inplace=False: qk_norm_rope_packed(x, H, qw, kw, 1e-6, table, pos, inplace=inplace),
               "unfused": unfused}
        graphs, keep = {}, []
        for name, f in fwd.items():
            with torch.no_grad():
                for inplace in (False, True):
                    g, outs = capture(lambda x: f(x.detach(), inplace), xs)
                    graphs[name + (" forward in place" if inplace else " forward")] = g.replay
                    keep.append((g, outs))
            leaves = (lambda x: [x]) if name == "rope" else (lambda x: [x, qw, kw])
            g, outs = capture(lambda x: torch.autograd.grad(f(x), leaves(x), gy, allow_unused=True), xs)
            graphs[name + " forward + backward"] = g.replay
            keep.append((g, outs))
        torch.cuda.synchronize()
        for name, v in time_calls(graphs, copies, a.kernel_iters).items():
            s = stats(v)
            emit({"bench": "qk_norm_kernel", "variant": name, "B": B, "T": T, "H": H, "Hkv": H, "us_median": s["median"],
                  "us_min": s["min"], "us_max": s["max"], "copies": copies, "iters": a.kernel_iters, "rounds": a.rounds})
        del graphs, keep, xs

    if "train" in a.part or "step" in a.part:
        from torchbooster_amd import utils
        from torchbooster_amd.models.gpt import KVCache, gpt2_small
        from torchbooster_amd.ops.optim import FusedAdamW

        def model_of(qk):
            torch.manual_seed(0)
            return gpt2_small(pos="rope", norm="rms", qk_norm=qk).to(dev).to(bf)

    if "train" in a.part:
        B, N = a.tokens
        tokens = torch.randint(0, 50257, (B, N), device=dev)
        steps = {}
        for qk in (False, True):
            model = model_of(qk)
            opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01)

            def step(model=model, opt=opt):
                utils.step(model.loss(tokens), opt, clip=1.0)

            for _ in range(3):
                step()
            steps[qk] = step
        torch.cuda.synchronize()
        t = time_calls(steps, 1, a.train_iters)
        ref = sorted(t[False])[len(t[False]) // 2]
        for qk, v in t.items():
            s = stats([x / 1e3 for x in v], 3)
            emit({"bench": "qk_norm_train_step", "qk_norm": qk, "B": B, "N": N, "ms_median": s["median"],
                  "ms_min": s["min"], "ms_max": s["max"], "vs_off": round(s["median"] / (ref / 1e3), 4),
                  "iters": a.train_iters, "rounds": a.rounds})
        del steps

    if "step" in a.part:
        with torch.no_grad():
            for B in a.batch:
                graphs, keep = {}, []
                tokens = torch.randint(0, 50257, (B, a.at), device=dev)
                new = torch.randint(0, 50257, (B,), device=dev)
                for qk in (False, True):
                    model = model_of(qk).eval()
                    _, cache = model.prefill(tokens, cache=KVCache(model, B))

                    def run(_=None, model=model, cache=cache):
                        cache.positions.fill_(a.at)
                        return model.decode_step(new, cache, fused=True)

                    g, outs = capture(run, [None])
                    graphs[qk] = g.replay
                    keep.append((g, outs, model, cache))
                torch.cuda.synchronize()
                t = time_calls(graphs, 1, a.iters)
                ref = sorted(t[False])[len(t[False]) // 2]
                for qk, v in t.items():
                    s = stats(v, 1)
                    emit({"bench": "qk_norm_decode_step", "qk_norm": qk, "B": B, "fused": True, "at": a.at,
                          "graph_us_median": s["median"], "graph_us_min": s["min"], "graph_us_max": s["max"],
                          "vs_off": round(s["median"] / ref, 4), "iters": a.iters, "rounds": a.rounds})
                del graphs, keep

    with open(os.path.join(a.out_dir, "bench.jsonl"), "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in records)
    lines = ["# QK-norm: measurements", "",
             f"`python scripts/bench_qk_norm.py` on one device ({torch.cuda.get_device_name(0)}); every figure is the median of "
             f"{a.rounds} interleaved rounds (min .. max behind it), timed between device events over graph replays "
             "(kernels, decode step) or eager steps (training).  `bench.jsonl` holds the records.", "",
             "| measurement | case | median | min .. max |", "|---|---|---|---|"]
    for r in records:
        if r["bench"] == "qk_norm_kernel":
            lines.append(f"| kernel, {r['B']} x {r['T']} tokens, H = Hkv = {H} | {r['variant']} | {r['us_median']} us | "
                         f"{r['us_min']} .. {r['us_max']} |")
        elif r["bench"] == "qk_norm_train_step":
            lines.append(f"| gpt2_small training step, {r['B']} x {r['N']} | qk_norm={r['qk_norm']} | {r['ms_median']} ms "
                         f"({r['vs_off']}x) | {r['ms_min']} .. {r['ms_max']} |")
        else:
            lines.append(f"| decode_step(fused=True) graph, B = {r['B']}, {r['at']} cached | qk_norm={r['qk_norm']} | "
                         f"{r['graph_us_median']} us ({r['vs_off']}x) | {r['graph_us_min']} .. {r['graph_us_max']} |")
    with open(os.path.join(a.out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
