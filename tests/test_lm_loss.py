"""Language-model loss on the CPU (reference) path: ``ops.loss.linear_cross_entropy``,
``TransformerLM.features`` / ``loss`` and the byte-level GPT example."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from torchbooster_amd.models.gpt import gpt_tiny
from torchbooster_amd.ops.loss import linear_cross_entropy

EX = Path(__file__).resolve().parent.parent / "examples"


def _pair(M, V, D, seed=0, lead=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*(lead or (M,)), D, generator=g)
    w = torch.randn(V, D, generator=g) * 0.3
    y = torch.randint(0, V, lead or (M,), generator=g)
    return x, w, y


def _grads(fn, x, w):
    x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
    loss = fn(x, w)
    loss.backward()
    return loss.detach(), x.grad, w.grad


def test_matches_linear_then_cross_entropy():
    x, w, y = _pair(37, 11, 16)
    got = _grads(lambda a, b: linear_cross_entropy(a, b, y), x, w)
    ref = _grads(lambda a, b: F.cross_entropy(F.linear(a, b), y), x, w)
    assert got[0].dtype == torch.float32 and got[0].dim() == 0
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)


def test_leading_dims_and_ignore_index():
    x, w, y = _pair(0, 13, 8, seed=1, lead=(3, 5))
    y[0, 1] = y[2, 4] = -100
    got = _grads(lambda a, b: linear_cross_entropy(a, b, y), x, w)
    ref = _grads(lambda a, b: F.cross_entropy(F.linear(a, b).flatten(0, 1), y.flatten(), ignore_index=-100), x, w)
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)
    assert got[1].shape == x.shape
    assert not got[1][0, 1].any() and not got[1][2, 4].any()
    # another ignore_index
    y2 = y.clone()
    y2[y2 == -100] = 7
    a = linear_cross_entropy(x, w, y2, ignore_index=7)
    b = F.cross_entropy(F.linear(x, w).flatten(0, 1), y2.flatten(), ignore_index=7)
    torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("bad", [13, -1, 2 ** 40])
def test_out_of_range_label_is_ignored(bad):
    x, w, y = _pair(9, 13, 8, seed=2)
    y_bad, y_ign = y.clone(), y.clone()
    y_bad[3], y_ign[3] = bad, -100
    got = _grads(lambda a, b: linear_cross_entropy(a, b, y_bad), x, w)
    ref = _grads(lambda a, b: linear_cross_entropy(a, b, y_ign), x, w)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_all_rows_ignored_gives_nan_loss_and_zero_gradients():
    x, w, y = _pair(6, 5, 8, seed=3)
    loss, dx, dw = _grads(lambda a, b: linear_cross_entropy(a, b, torch.full_like(y, -100)), x, w)
    assert torch.isnan(loss)
    assert not dx.any() and not dw.any()


def _model():
    torch.manual_seed(0)
    return gpt_tiny(vocab=61, max_len=24).eval()


def test_forward_is_head_of_features():
    model = _model()
    tokens = torch.randint(0, 61, (2, 17))
    lengths = torch.tensor([17, 9], dtype=torch.int32)
    with torch.no_grad():
        for ln in (None, lengths):
            h = model.features(tokens, ln)
            assert h.shape == (2, 17, 128)
            assert torch.equal(model(tokens, ln), model.head(h))


def test_loss_is_shifted_cross_entropy_of_forward():
    model = _model()
    tokens = torch.randint(0, 61, (3, 20))
    with torch.no_grad():
        logits = model(tokens)
        ref = F.cross_entropy(logits[:, :-1].reshape(-1, 61).float(), tokens[:, 1:].reshape(-1))
        got = model.loss(tokens)
    assert 2.0 < float(ref) < 8.0
    torch.testing.assert_close(got, ref, rtol=0, atol=1e-5)


def test_loss_with_lengths_ignores_tokens_at_and_past_each_length():
    model = _model()
    tokens = torch.randint(0, 61, (3, 20))
    lengths = torch.tensor([20, 7, 1], dtype=torch.int32)
    with torch.no_grad():
        logits = model(tokens, lengths)
        rows = [F.cross_entropy(logits[b, :n - 1].float(), tokens[b, 1:n], reduction="sum")
                for b, n in enumerate(lengths.tolist())]
        ref = sum(rows) / (19 + 6 + 0)
        got = model.loss(tokens, lengths)
        torch.testing.assert_close(got, ref, rtol=0, atol=1e-5)
        other = tokens.clone()
        other[1, 7:] = (other[1, 7:] + 5) % 61
        other[2, 1:] = (other[2, 1:] + 9) % 61
        assert torch.equal(model.loss(other, lengths), got)
        # ... and a token before the length does count
        other = tokens.clone()
        other[1, 6] = (other[1, 6] + 5) % 61
        assert not torch.equal(model.loss(other, lengths), got)


def test_loss_gradients_match_the_unfused_route():
    model = _model()
    tokens = torch.randint(0, 61, (2, 12))
    model.loss(tokens).backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    F.cross_entropy(model(tokens)[:, :-1].reshape(-1, 61), tokens[:, 1:].reshape(-1)).backward()
    for n, p in model.named_parameters():
        torch.testing.assert_close(got[n], p.grad, rtol=1e-4, atol=1e-6, msg=lambda m, n=n: f"{n}: {m}")


def test_explicit_targets_are_honoured():
    model = _model()
    tokens = torch.randint(0, 61, (2, 10))
    targets = torch.randint(0, 61, (2, 10))
    targets[0, 3] = -100
    targets[1, 9] = 5  # the last position counts when the caller says so
    with torch.no_grad():
        ref = F.cross_entropy(model(tokens).reshape(-1, 61).float(), targets.reshape(-1), ignore_index=-100)
        torch.testing.assert_close(model.loss(tokens, targets=targets), ref, rtol=0, atol=1e-5)
        t9 = targets.clone()
        t9[t9 == -100] = -9
        torch.testing.assert_close(model.loss(tokens, targets=t9, ignore_index=-9), ref, rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        model.loss(tokens, targets=targets[:, :5])


def test_single_token_sequences_raise():
    model = _model()
    with pytest.raises(ValueError):
        model.loss(torch.zeros(2, 1, dtype=torch.int64))
    # explicit targets need no next token
    assert torch.isfinite(model.loss(torch.zeros(2, 1, dtype=torch.int64), targets=torch.ones(2, 1, dtype=torch.int64)))


def test_gpt_example_trains_on_cpu(tmp_path):
    base = EX / "txt_gen" / "gpt" / "gpt.yml"
    cfg = tmp_path / "conf.yml"
    cfg.write_text(f"#include {base}\nseq_len: 32\nbatch_size: 8\nlog_every: 10\nsample_tokens: 8\n"
                   "env:\n  n_gpu: 0\noptim:\n  name: adamw\n  lr: 3e-3\n"
                   "scheduler:\n  name: cycle\n  n_iter: 30\n  warmup: 3\n  decay: lin, cos\n")
    env = dict(os.environ, TBAMD_CONFIG=str(cfg), TBAMD_EXAMPLE_MAX_ITERS="30", CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, str(EX / "txt_gen" / "gpt" / "gpt.py")], env=env, capture_output=True,
                       text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = [float(m) for m in re.findall(r"^step \d+ loss ([0-9.]+)$", r.stdout, re.M)]
    assert len(losses) == 4, r.stdout  # steps 1, 10, 20, 30
    assert losses[-1] < losses[0], losses
    assert "sample: " in r.stdout
