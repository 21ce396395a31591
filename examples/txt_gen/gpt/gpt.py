"""Byte-level GPT language model on a local text file.

Every byte of the file is a token (vocabulary 256), a batch is ``batch_size`` random windows of
``seq_len`` bytes, and the loss is ``TransformerLM.loss``: the next-token cross entropy through the
fused vocabulary projection (ops/loss.py ``linear_cross_entropy``), which never stores the logits.
Fused AdamW + clip, cosine CycleScheduler; at the end a short greedy ``generate`` sample is printed.
Nothing is downloaded: ``text`` defaults to the repository's README.md.  Not in the reference (no
attention models there).
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch  # noqa: E402

import torchbooster_amd.distributed as dist  # noqa: E402
import torchbooster_amd.utils as utils  # noqa: E402
from common import max_iters, prepare_model, report_sync  # noqa: E402
from torchbooster_amd.config import BaseConfig, EnvironementConfig, OptimizerConfig, SchedulerConfig  # noqa: E402
from torchbooster_amd.metrics import RunningAverage  # noqa: E402
from torchbooster_amd.models import gpt  # noqa: E402

REPO = Path(__file__).resolve().parents[3]


@dataclass
class Config(BaseConfig):
    steps: int
    seed: int
    arch: str
    text: str
    seq_len: int
    batch_size: int
    clip: float
    log_every: int
    sample_prompt: str
    sample_tokens: int
    env: EnvironementConfig
    optim: OptimizerConfig
    scheduler: SchedulerConfig
    pos: str = "learned"  # "rope": rotary position embeddings (models/gpt.py)
    norm: str = "layer"  # "rms": RMSNorm
    mlp: str = "gelu"  # "swiglu": the gated SiLU MLP
    window: int = 0  # > 0: sliding-window attention, a token sees itself and the window - 1 tokens before it
    rolling: bool = False  # the sample's KV cache keeps only about `window` rows per layer (needs window > 0)
    kv_dtype: str = ""  # "fp8": the sample's KV cache holds e4m3 codes, scales calibrated on the prompt


def load_bytes(path: str) -> torch.Tensor:
    p = Path(path) if path else REPO / "README.md"
    if not p.is_absolute() and not p.exists():
        p = REPO / p
    data = torch.frombuffer(bytearray(p.read_bytes()), dtype=torch.uint8)
    return data.to(torch.int64)


def main(conf: Config) -> None:
    data = conf.env.make(load_bytes(conf.text))
    if data.numel() <= conf.seq_len:
        raise ValueError(f"{conf.text or 'README.md'}: {data.numel()} bytes, need more than seq_len = {conf.seq_len}")
    net = getattr(gpt, conf.arch)(vocab=256, max_len=conf.seq_len, pos=conf.pos, norm=conf.norm, mlp=conf.mlp,
                                  window=conf.window or None)
    model = prepare_model(net, conf, channels_last=False)
    net = getattr(model, "module", model)
    optim = conf.optim.make(model.parameters())
    sched = conf.scheduler.make(optim)
    g = torch.Generator(device=data.device)
    g.manual_seed(conf.seed + dist.get_rank())
    window = torch.arange(conf.seq_len, device=data.device)
    run = RunningAverage()
    for it in range(max_iters(conf.steps)):
        start = torch.randint(0, data.numel() - conf.seq_len, (conf.batch_size, 1), generator=g, device=data.device)
        tokens = data[start + window]
        loss = net.loss(tokens)
        utils.step(loss, optim, sched, clip=conf.clip)
        run.update(loss.detach())
        if (it + 1) % conf.log_every == 0 or it == 0:
            if dist.is_primary():
                print(f"step {it + 1} loss {run.value:.4f}", flush=True)
            run = RunningAverage()
    if dist.is_primary() and conf.sample_tokens > 0:
        prompt = list(conf.sample_prompt.encode())[:conf.seq_len - conf.sample_tokens] or [10]
        tokens = torch.tensor([prompt], dtype=torch.int64, device=data.device)
        model.eval()
        kw = {"rolling": True} if conf.rolling else {}
        if conf.kv_dtype:
            if conf.kv_dtype != "fp8":
                raise ValueError(f"kv_dtype must be 'fp8' or empty, not {conf.kv_dtype!r}")
            kw.update(kv_dtype=torch.float8_e4m3fn, kv_scales=gpt.kv_scales(net, tokens, margin=2.0))
        out, _ = net.generate(tokens, conf.sample_tokens, **kw)
        text = bytes(prompt + out[0].tolist()).decode("utf-8", errors="replace")
        print(f"sample: {text!r}", flush=True)
    report_sync(model)


if __name__ == "__main__":
    conf = Config.load(Path(os.environ.get("TBAMD_CONFIG", Path(__file__).with_name("gpt.yml"))))
    utils.seed(conf.seed, deterministic=False)
    utils.boost(enable=True)
    dist.launch(main, conf.env.n_gpu, conf.env.n_machine, conf.env.machine_rank, conf.env.dist_url, args=(conf,))
