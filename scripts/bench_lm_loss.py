#!/usr/bin/env python
"""Fused LM-head cross entropy against the unfused route: time and peak memory.

Op part.  Forward + backward (gradients of ``x`` and of the weight) of

* ``unfused``: ``ops.linear.linear`` -> ``ops.loss.cross_entropy`` (bf16 logits stored and saved), and
* ``fused_<B>MiB``: ``ops.loss.linear_cross_entropy`` with the backward's chunk buffer sized for a budget
  of ``B`` MiB (``--budgets``),

at ``--shapes`` (M, V, D; default 8192 x 50257 x 768 and 8192 x 32000 x 768).  Every variant runs twice
untimed (code objects, allocator, the GEMM tuner's first-use timing of each shape), then the variants
are timed in ``--rounds`` interleaved rounds: ``--iters`` calls between two device events.  The median
round and the min-max spread are reported.  Peak memory is ``max_memory_allocated`` over one more call
above the memory allocated before it (inputs and weight excluded, gradients included).  The fused
results are compared with the unfused ones on the same inputs (relative L2 difference).

Model part.  One ``gpt2_small`` training step (bf16, FusedAdamW, clip) at ``--batch`` x ``--seq`` tokens with
``model.loss(tokens)`` against ``cross_entropy(model(tokens).flatten(0, 1), targets)``: a host clock around
``--steps`` steps that end in a device synchronise, the two alternated for ``--rounds`` rounds on the same
model, and the peak memory of a step.

One JSON line per measurement.  Usage: ``python scripts/bench_lm_loss.py [--part op model]``.
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
    ap.add_argument("--part", nargs="+", default=["op", "model"], choices=["op", "model"])
    ap.add_argument("--shapes", type=int, nargs="+", default=[8192, 50257, 768, 8192, 32000, 768],
                    help="M V D triples")
    ap.add_argument("--budgets", type=int, nargs="+", default=[64, 256, 1024], help="chunk buffer budgets, MiB")
    ap.add_argument("--iters", type=int, default=10, help="calls per timed round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5, help="training steps per timed round")
    ap.add_argument("--tag", default="", help="copied into every JSON line")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args(argv)
    if len(a.shapes) % 3:
        ap.error("--shapes takes M V D triples")
    sys.path.insert(0, ROOT)

    import torch

    from torchbooster_amd import utils
    from torchbooster_amd.ops import _ext
    from torchbooster_amd.ops.linear import linear
    from torchbooster_amd.ops.loss import _default_chunk, cross_entropy, linear_cross_entropy
    from torchbooster_amd.ops.optim import FusedAdamW

    if not torch.cuda.is_available():
        raise SystemExit("bench_lm_loss.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    tile_q = int(_ext.native().lm_loss_tile_q())

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    def rel(x, y):
        return float((x.float() - y.float()).norm() / y.float().norm().clamp_min(1e-20))

    if "op" in a.part:
        for M, V, D in zip(a.shapes[0::3], a.shapes[1::3], a.shapes[2::3]):
            g = torch.Generator(device=dev).manual_seed(V)
            x = torch.randn(M, D, device=dev, generator=g).to(torch.bfloat16).requires_grad_()
            w = (torch.randn(V, D, device=dev, generator=g) * (2.0 / D ** 0.5)).to(torch.bfloat16).requires_grad_()
            y = torch.randint(0, V, (M,), device=dev, generator=g)

            def unfused():
                loss = cross_entropy(linear(x, w), y)
                return (loss.detach(),) + torch.autograd.grad(loss, (x, w))

            def fused(chunk):
                def run():
                    loss = linear_cross_entropy(x, w, y, chunk=chunk)
                    return (loss.detach(),) + torch.autograd.grad(loss, (x, w))
                return run

            runs = {"unfused": (unfused, None)}
            for b in a.budgets:
                chunk = min(_default_chunk(M, tile_q, b << 20), -(-V // tile_q) * tile_q)
                runs[f"fused_{b}MiB"] = (fused(chunk), chunk)
            peaks, outs = {}, {}
            for name, (fn, _) in runs.items():
                fn()
                fn()
                peaks[name], outs[name] = peak_of(fn)
            times = {k: [] for k in runs}
            for _ in range(a.rounds):
                for name, (fn, _) in runs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) / a.iters)
            ref = outs["unfused"]
            for name, v in times.items():
                med = sorted(v)[len(v) // 2]
                o = outs[name]
                emit({"bench": "lm_loss_op", "tag": a.tag, "variant": name, "M": M, "V": V, "D": D,
                      "chunk": runs[name][1], "ms_median": round(med, 3), "ms_min": round(min(v), 3),
                      "ms_max": round(max(v), 3), "peak_MiB": round(peaks[name] / 2 ** 20, 1),
                      "loss": float(o[0]), "loss_minus_unfused": float(o[0]) - float(ref[0]),
                      "dx_rel_vs_unfused": rel(o[1], ref[1]), "dw_rel_vs_unfused": rel(o[2], ref[2]),
                      "iters": a.iters, "rounds": a.rounds})
            del x, w, y, outs, ref, runs

    if "model" in a.part:
        from torchbooster_amd.models import gpt2_small

        torch.manual_seed(0)
        model = gpt2_small(max_len=a.seq).to(dev).to(torch.bfloat16)
        opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
        tokens = torch.randint(0, 50257, (a.batch, a.seq), device=dev)
        targets = torch.roll(tokens, -1, dims=1)
        targets[:, -1] = -100

        def step_fused():
            loss = model.loss(tokens)
            utils.step(loss, opt, clip=1.0)
            return loss

        def step_unfused():
            loss = cross_entropy(model(tokens).flatten(0, 1), targets.flatten())
            utils.step(loss, opt, clip=1.0)
            return loss

        runs = {"model.loss": step_fused, "unfused": step_unfused}
        peaks = {}
        for name, fn in runs.items():
            fn()
            fn()
            peaks[name], _ = peak_of(fn)
        times = {k: [] for k in runs}
        for _ in range(a.rounds):
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss = fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
                assert bool(torch.isfinite(loss))
        for name, v in times.items():
            med = sorted(v)[len(v) // 2]
            emit({"bench": "gpt2_small_train_step", "tag": a.tag, "variant": name, "B": a.batch, "N": a.seq,
                  "ms_median": round(med, 2), "ms_min": round(min(v), 2), "ms_max": round(max(v), 2),
                  "tokens_per_s": round(a.batch * a.seq / med * 1e3, 1), "step_peak_MiB": round(peaks[name] / 2 ** 20, 1),
                  "steps": a.steps, "rounds": a.rounds})
    return 0


if __name__ == "__main__":
    sys.exit(main())
