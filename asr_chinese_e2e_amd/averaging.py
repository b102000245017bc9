"""Checkpoint averaging: the mean of the last or best N checkpoints of an experiment directory (the form in which WeNet, ESPnet and
fairseq report their results), beside the exponential moving average the training step keeps (config.ema_decay).

    paths = select_checkpoints("ckpt/exp", 10, mode="best", metric="dev/loss")
    model.load_state_dict(average_state_dicts(paths))

Host code on purpose: N files are read from disk once, so a kernel would buy nothing.  The mean is taken in float64 and rounded once to
the tensor's dtype, so it does not depend on how many checkpoints there are beyond that rounding, and identical inputs come back
bit for bit.
"""
import json
import math
import os
import re

import torch

_CKPT = re.compile(r"^e(\d+)_s(\d+)\.model$")
_CKPT_EMA = re.compile(r"^e(\d+)_s(\d+)\.ema\.model$")


def _load(x):
    if isinstance(x, (str, os.PathLike)):
        if not os.path.isfile(x):
            raise FileNotFoundError(f"checkpoint not found: {os.fspath(x)!r}")
        return torch.load(x, map_location="cpu", weights_only=True)
    return x


def average_state_dicts(dicts_or_paths, weights=None):
    """The weighted mean of state dicts (or of the files that hold them).  Per floating-point tensor: float64(w_i) * float64(x_i) is
    accumulated in the order given, divided by sum w in float64 and rounded once to the tensor's dtype.  Non-floating entries, and entries
    that are equal in every input (the positional-encoding buffers), are copied from the first input; non-floating entries that differ
    raise.  Differing key sets, shapes or dtypes, non-finite values, negative or all-zero weights and an empty list are refused by name."""
    items = list(dicts_or_paths)
    if not items:
        raise ValueError("average_state_dicts: the list of checkpoints is empty")
    n = len(items)
    if weights is None:
        w = [1.0] * n
    else:
        w = [float(x) for x in weights]
        if len(w) != n:
            raise ValueError(f"average_state_dicts: {len(w)} weights for {n} checkpoints")
        if any(not math.isfinite(x) or x < 0 for x in w):
            raise ValueError(f"average_state_dicts: weights must be finite and not negative: {w}")
        if sum(w) <= 0:
            raise ValueError("average_state_dicts: the weights are all zero")
    total = math.fsum(w)
    first = _load(items[0])
    keys = list(first.keys())
    acc, same = {}, {}
    for i, item in enumerate(items):
        sd = first if i == 0 else _load(item)
        if set(sd.keys()) != set(keys):
            odd = sorted(set(sd.keys()) ^ set(keys))
            raise KeyError(f"average_state_dicts: checkpoint {i} has other keys than checkpoint 0: {odd[:5]}")
        for k in keys:
            x, x0 = sd[k], first[k]
            if not torch.is_tensor(x) or not torch.is_tensor(x0):
                if torch.is_tensor(x) != torch.is_tensor(x0) or (not torch.is_tensor(x) and x != x0):
                    raise ValueError(f"average_state_dicts: entry {k!r} of checkpoint {i} differs from checkpoint 0 and cannot be averaged")
                continue
            if tuple(x.shape) != tuple(x0.shape):
                raise ValueError(f"average_state_dicts: {k!r} has shape {tuple(x.shape)} in checkpoint {i}, {tuple(x0.shape)} in checkpoint 0")
            if x.dtype != x0.dtype:
                raise ValueError(f"average_state_dicts: {k!r} has dtype {x.dtype} in checkpoint {i}, {x0.dtype} in checkpoint 0")
            if not x.dtype.is_floating_point:
                if not torch.equal(x, x0):
                    raise ValueError(f"average_state_dicts: integer entry {k!r} of checkpoint {i} differs from checkpoint 0 and cannot be averaged")
                continue
            x64 = x.detach().to(device="cpu", dtype=torch.float64)
            if not bool(torch.isfinite(x64).all()):
                raise ValueError(f"average_state_dicts: {k!r} of checkpoint {i} holds non-finite values")
            same[k] = same.get(k, True) and (i == 0 or torch.equal(x.detach().cpu(), x0.detach().cpu()))
            term = x64 * w[i]
            acc[k] = term if i == 0 else acc[k] + term
    out = {}
    for k in keys:
        x0 = first[k]
        if k in acc and not same[k]:
            out[k] = (acc[k] / total).to(x0.dtype)
        else:
            out[k] = x0.detach().cpu().clone() if torch.is_tensor(x0) else x0
    return out


def _read_metric(exp_root, tag):
    """{step: value} of `tag` in exp_root/scalars.jsonl (the last record of a step wins)."""
    path = os.path.join(exp_root, "scalars.jsonl")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"select_checkpoints: {path} not found (mode='best' reads the metric from it)")
    out = {}
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            rec = json.loads(line)
            if rec.get("tag") == tag:
                out[int(rec["step"])] = float(rec["value"])
    return out


def select_checkpoints(exp_root, num, mode="last", metric="dev/loss", which="model", report=None):
    """Paths of `num` checkpoints of an experiment directory, in ascending step order.
    mode "last": the `num` highest steps among e*_s*.model (which="ema": e*_s*.ema.model).
    mode "best": the `num` checkpoints whose step has the lowest value of `metric` in scalars.jsonl; a leading '+' in `metric` means
    highest; ties go to the later step.  A checkpoint with no record at exactly its step is skipped and reported (appended to the list
    `report`, printed when report is None).  Fewer than `num` usable checkpoints raise."""
    if which not in ("model", "ema"):
        raise ValueError(f"select_checkpoints: which={which!r} (model or ema)")
    if mode not in ("last", "best"):
        raise ValueError(f"select_checkpoints: mode={mode!r} (last or best)")
    num = int(num)
    if num < 1:
        raise ValueError(f"select_checkpoints: num={num}")
    pat = _CKPT if which == "model" else _CKPT_EMA
    found = []
    for name in os.listdir(exp_root):
        m = pat.match(name)
        if m:
            found.append((int(m.group(2)), int(m.group(1)), os.path.join(exp_root, name)))
    found.sort()
    if mode == "best":
        higher = metric.startswith("+")
        tag = metric[1:] if metric[:1] in "+-" else metric
        values = _read_metric(exp_root, tag)
        usable = []
        for step, epoch, path in found:
            if step not in values or not math.isfinite(values[step]):
                msg = f"select_checkpoints: {os.path.basename(path)} skipped: no finite {tag!r} record at step {step}"
                if report is None:
                    print(msg)
                else:
                    report.append(msg)
                continue
            usable.append((step, epoch, path))
        # best first; among equal values the later step first
        usable.sort(key=lambda t: ((-values[t[0]] if higher else values[t[0]]), -t[0]))
        found = usable
        chosen = found[:num]
    else:
        chosen = found[-num:]
    if len(chosen) < num:
        raise ValueError(f"select_checkpoints: {len(found)} usable checkpoints under {exp_root}, {num} asked for")
    return [p for _, _, p in sorted(chosen)]
