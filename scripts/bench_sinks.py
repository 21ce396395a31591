#!/usr/bin/env python
"""Attention sinks: what the sink fold costs each attention call and a model step.

Kernel part.  ``H = 12`` heads, bf16, head dim 64; every call with ``sinks`` against the same call without, captured
into one graph each and interleaved round by round (the method of ``bench_window.py``):

* ``attention`` forward and forward + backward, causal, ``B = 8``, ``N`` in ``--train-len``.  Without sinks ``N <= 256``
  takes the whole-head forward and with sinks the 128-row one, so that row compares two kernels;
* ``attention_decode``, ``B`` in ``--batch``, every sequence at ``len = cap`` in ``--len`` (``Hkv`` in ``--kv``), and the
  fused single-chunk step ``attention_decode_packed(fused=True)`` at ``cap = 128``;
* ``attention_extend``, ``T = 8`` new tokens at the same lengths (key splits by the default policy).

As in ``bench_gqa.py`` every call of a decode / extend graph reads another copy of the caches (``--ws-mb`` of copies in
all), so the last-level cache does not serve them.

Step part.  ``gpt2_small`` with and without ``sinks=True``: a training step at 8 x 1024 tokens (loss, backward; no
optimizer) and a graph-replayed ``decode_step`` (default and ``fused=True``) with every cache at ``--at`` tokens.

``--no-sinks`` times the sinks-free calls alone and passes no ``sinks`` keyword anywhere: run from a checkout of
another commit it measures that commit's kernels.  Replays are timed between two device events; the median round and
the min-max spread are reported.  One JSON line per measurement.
Usage: ``python scripts/bench_sinks.py [--part kernel step] [--no-sinks]``.
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
    ap.add_argument("--part", nargs="+", default=["kernel", "step"], choices=["kernel", "step"])
    ap.add_argument("--no-sinks", action="store_true", help="time the sinks-free calls alone (any commit)")
    ap.add_argument("--kv", type=int, nargs="+", default=[12, 1])
    ap.add_argument("--len", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--batch", type=int, nargs="+", default=[8])
    ap.add_argument("--train-len", type=int, nargs="+", default=[197, 1024, 4096])
    ap.add_argument("--at", type=int, nargs="+", default=[512], help="cached tokens of the decode steps")
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
        raise SystemExit("bench_sinks.py measures on the GPU; none found")
    from torchbooster_amd.ops.attention import attention, attention_decode, attention_decode_packed, attention_extend

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    variants = [False] if a.no_sinks else [False, True]
    sinks = torch.linspace(-4.0, 6.0, H, device=dev)

    def skw(on):
        return {"sinks": sinks} if on else {}

    def emit(rec):
        rec.update(tag=a.tag, rounds=a.rounds)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(rec) + "\n")

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

    def report(bench, t, nd=2, **rec):
        """One line per variant: median, spread and the median against the sinks-free variant of the same run."""
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        for on, v in t.items():
            emit({"bench": bench, **rec, "sinks": on, "us_median": round(med[on], nd), "us_min": round(min(v), nd),
                  "us_max": round(max(v), nd), "vs_no_sinks": round(med[on] / med[False], 3)})

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

    def measure(bench, make, copies_of, iters, **rec):
        """``make(on)`` -> the call of one cache copy; a graph per variant, interleaved."""
        keep = {on: capture(make(on), copies_of) for on in variants}
        torch.cuda.synchronize()
        report(bench, time_rounds({on: g.replay for on, (g, _) in keep.items()}, len(copies_of), iters), **rec)

    if "kernel" in a.part:
        for N in a.train_len:
            torch.manual_seed(N)
            q, k, v = (torch.randn(8, H, N, 64, device=dev).to(bf).requires_grad_() for _ in range(3))
            do = torch.randn(8, H, N, 64, device=dev).to(bf)
            s = sinks.clone().requires_grad_()

            def fwd_bwd(on):
                o = attention(q, k, v, causal=True, **({"sinks": s} if on else {}))
                o.backward(do)
                q.grad = k.grad = v.grad = s.grad = None

            def fwd(on):
                with torch.no_grad():
                    attention(q, k, v, causal=True, **skw(on))

            for what, fn in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
                for on in variants:
                    fn(on), fn(on)
                torch.cuda.synchronize()
                t = time_rounds({on: (lambda on=on, fn=fn: fn(on)) for on in variants}, 1, a.kernel_iters)
                report("sinks_attention", t, 1, what=what, B=8, H=H, N=N)
        with torch.no_grad():
            for B in a.batch:
                for n in a.len:
                    for hkv in a.kv:
                        nbytes = B * hkv * n * 64 * 2 * 2
                        copies = max(2, min(a.max_copies, -(-a.ws_mb * (1 << 20) // nbytes)))
                        torch.manual_seed(n + hkv)
                        kvs = [tuple(torch.randn(B, hkv, n, 64, device=dev).to(bf) for _ in range(2))
                               for _ in range(copies)]
                        kw = {} if hkv == H else {"kv_heads": hkv}
                        q = torch.randn(B, H, 64, device=dev).to(bf)
                        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
                        measure("sinks_decode", lambda on: lambda kv: attention_decode(q, kv[0], kv[1], lens, **kw,
                                                                                       **skw(on)),
                                kvs, a.kernel_iters, B=B, H=H, Hkv=hkv, len=n, cache_copies=copies)
                        qe = torch.randn(B, 8, H, 64, device=dev).to(bf)
                        pos = torch.full((B,), n - 8, dtype=torch.int32, device=dev)
                        measure("sinks_extend", lambda on: lambda kv: attention_extend(qe, kv[0], kv[1], pos, **kw,
                                                                                       **skw(on)),
                                kvs, a.kernel_iters, B=B, H=H, Hkv=hkv, T=8, len=n, cache_copies=copies)
                        del kvs
                # the fused single-chunk step: the split kernel's own epilogue normalises
                kvs = [tuple(torch.randn(B, H, 128, 64, device=dev).to(bf) for _ in range(2)) for _ in range(64)]
                qkv = torch.randn(B, 1, 3 * H * 64, device=dev).to(bf)
                pos = torch.full((B,), 127, dtype=torch.int32, device=dev)
                measure("sinks_decode_fused", lambda on: lambda kv: attention_decode_packed(qkv, H, kv[0], kv[1], pos,
                                                                                            fused=True, **skw(on)),
                        kvs, a.kernel_iters, B=B, H=H, Hkv=H, len=128, cache_copies=64)
                del kvs

    if "step" in a.part:
        from torchbooster_amd.models import gpt2_small
        from torchbooster_amd.models.gpt import KVCache

        models = {}
        for on in variants:
            torch.manual_seed(0)
            models[on] = gpt2_small(**({"sinks": True} if on else {})).to(dev).to(bf)
        tokens = torch.randint(0, 50257, (8, 1024), device=dev)

        def train(on):
            m = models[on]
            m.loss(tokens).backward()
            for p in m.parameters():
                p.grad = None

        for on in models:
            train(on), train(on)
        torch.cuda.synchronize()
        report("sinks_train_step", time_rounds({on: (lambda on=on: train(on)) for on in models}, 1, 2), 0,
               model="gpt2_small", tokens="8x1024")
        with torch.no_grad():
            for B in a.batch:
                for at in a.at:
                    new = torch.randint(0, 50257, (B,), device=dev)
                    for fused in (False, True):
                        graphs, keep = {}, []
                        for on, model in models.items():
                            model.eval()
                            cache = KVCache(model, B, capacity=at + 1)
                            for kc, vc in cache.layers:
                                kc.normal_(), vc.normal_()

                            def run(_=None, model=model, cache=cache, kw={"fused": True} if fused else {}):
                                cache.positions.fill_(at)
                                return model.decode_step(new, cache, **kw)
                            g, o = capture(run, [None])
                            graphs[on] = g.replay
                            keep.append((g, o, cache))
                        torch.cuda.synchronize()
                        report("sinks_decode_step", time_rounds(graphs, 1, a.iters), 1, model="gpt2_small", B=B, at=at,
                               fused=fused)
    return 0


if __name__ == "__main__":
    sys.exit(main())
