"""bench.py's ``--dump-outputs`` / ``--full`` options: the arrays of the last timed step are written
as float32 ``.npy`` files, a large parameter vector is cut to a fixed seeded sample, and a run with
the same arguments writes the same arrays again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_parser_has_full_and_dump_outputs():
    a = bench._parser().parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    a = bench._parser().parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float32_and_samples_large_models(tmp_path, monkeypatch):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 10)).to(torch.bfloat16)
    n = sum(p.numel() for p in model.parameters())
    logits, loss = torch.randn(4, 10, dtype=torch.bfloat16), torch.tensor(1.5, dtype=torch.bfloat16)
    bench._dump_outputs(str(tmp_path / "all"), loss, logits, model)
    got = {f: np.load(tmp_path / "all" / f) for f in sorted(os.listdir(tmp_path / "all"))}
    assert sorted(got) == ["logits.npy", "loss.npy", "params.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss.npy"].tolist() == [1.5] and got["logits.npy"].shape == (4, 10)
    flat = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()]).numpy()
    assert np.array_equal(got["params.npy"], flat) and flat.size == n
    # above the cap: the same sorted sample of distinct positions on every call
    monkeypatch.setattr(bench, "_DUMP_PARAM_SAMPLE", 100)
    for d in ("s1", "s2"):
        bench._dump_outputs(str(tmp_path / d), loss, logits, model)
    s1, s2 = np.load(tmp_path / "s1" / "params.npy"), np.load(tmp_path / "s2" / "params.npy")
    assert s1.shape == (100,) and np.array_equal(s1, s2)
    idx = np.sort(np.random.RandomState(0).choice(n, 100, replace=False))
    assert len(set(idx.tolist())) == 100 and np.array_equal(s1, flat[idx])


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_bench_run_dumps_its_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--model", "resnet18", "--batch", "8", "--image", "64", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["unit"] == "images/s" and res["dtype"] == "bf16"
    assert abs(res["value"] - 8 / (res["ms_per_step"] * 1e-3)) <= 1e-3 * res["value"]
    got = {f: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["logits.npy", "loss.npy", "params.npy"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert got["logits.npy"].shape == (8, 1000) and got["loss.npy"].shape == (1,)
    assert got["params.npy"].shape == (1 << 22,)  # ResNet-18 has 11.7 M parameters: the sample
    assert abs(float(got["loss.npy"][0]) - res["final_loss"]) <= 1e-6 * abs(res["final_loss"])
    assert sum(v.nbytes for v in got.values()) <= 64 * 10**6
