#!/usr/bin/env python3
"""average.py - the mean of the last or best N checkpoints of an experiment directory, written as one state dict.

    python average.py --exp=ckpt/exp --num=10 --mode=best --metric=dev/loss --out=avg.model
    python transcribe.py --ckpt=avg.model ...          (or evaluate.py, spot.py, the reference)

  --exp      the experiment directory of a Trainer11 / BaseTrainer run: e{epoch}_s{step}.model files and scalars.jsonl
  --num      checkpoints to average (10)
  --mode     last (default): the highest steps; best: the steps with the best value of --metric in scalars.jsonl
  --metric   the tag read for --mode=best (dev/loss: lowest is best; a leading '+', as in +dev/acc, means highest is best); ties go to
             the later step, and a checkpoint with no record at exactly its step is skipped and reported
  --which    model (default) or ema: average the e*_s*.ema.model files a run with --ema_decay writes beside the raw ones
  --out      the file to write (required)
Prints the chosen files, one per line, then the output path.  The mean is taken in float64 and rounded once per tensor
(asr_chinese_e2e_amd/averaging.py); no GPU is needed.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd.averaging import average_state_dicts, select_checkpoints  # noqa: E402

CLI_KEYS = ("exp", "num", "mode", "metric", "which", "out")


def parse(argv):
    out = {}
    for a in argv:
        if not a.startswith("--") or "=" not in a:
            raise SystemExit(f"average.py: unexpected argument {a!r} (flags are --key=value)")
        k, v = a[2:].split("=", 1)
        k = k.replace("-", "_")
        if k not in CLI_KEYS:
            raise SystemExit(f"average.py: unknown flag --{k} (known: {', '.join(CLI_KEYS)})")
        out[k] = v
    return out


def main(argv):
    cli = parse(argv)
    if not cli.get("out"):
        raise SystemExit("average.py: give --out=<file to write>")
    try:
        if not cli.get("exp") or not os.path.isdir(cli["exp"]):
            raise SystemExit(f"average.py: give --exp=<experiment directory> (got {cli.get('exp')!r})")
        paths = select_checkpoints(cli["exp"], int(cli.get("num", 10)), mode=cli.get("mode", "last"), metric=cli.get("metric", "dev/loss"),
                                   which=cli.get("which", "model"))
        for p in paths:
            print(p)
        state = average_state_dicts(paths)
    except (ValueError, KeyError, FileNotFoundError) as e:
        raise SystemExit(f"average.py: {e}") from e
    torch.save(state, cli["out"])
    print(f"average of {len(paths)} checkpoints written to {cli['out']}")
    return paths


if __name__ == "__main__":
    main(sys.argv[1:])
