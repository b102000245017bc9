#!/usr/bin/env python3
"""compute_cmvn.py - global CMVN statistics of a corpus, one pass on the GPU.

    python tools/compute_cmvn.py --collector_path=data/aishell1 --out=exp/cmvn.npz [--part=train] [--n_mels=40] [--batch_size=32]
                                 [--resample=1] [--frontend=kaldi]

Reads the manifest `<collector_path>_<part>.json` train.py reads, decodes the files, and for every batch runs the training front
end's own log-mel kernel and adds the per-bin sums of its valid frames to float64 accumulators on the device (data_handler/cmvn.py);
the audio is never perturbed or augmented.  With --resample=1 files at another rate than 16 kHz are converted on the GPU first (one
launch per batch, data_handler/resample.py) instead of ending the run.  Writes mean, istd, count, n_mels and the front end as .npz: pass it to train.py --cmvn and to
transcribe.py --cmvn.  --frontend=kaldi takes the statistics over Kaldi fbank features; --out=<file>.json writes WeNet's global_cmvn JSON
(the raw sums; read back as statistics of the Kaldi front end).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd.data_handler import AudioParser, CmvnAccumulator, load_wav, save_cmvn, save_wenet_cmvn  # noqa: E402
from asr_chinese_e2e_amd.data_handler.cmvn import finalize_stats  # noqa: E402
from train import parse_flags  # noqa: E402


def manifest_waves(collector_path, part):
    with open(f"{collector_path}_{part}.json", encoding="utf-8") as f:
        return [json.loads(line)["wave"] for line in f if line.strip()]


def compute(files, n_mels=40, batch_size=32, sample_rate=16000, device="cuda", resample=False, frontend="reference", sums=False):
    """-> (mean, istd, count) over the frames of `files`; sums=True: the raw (sum x, sum x^2, count) instead."""
    from asr_chinese_e2e_amd.data_handler import resample as resample_mod
    acc = CmvnAccumulator(AudioParser(sample_rate=sample_rate, n_mels=n_mels, device=device, frontend=frontend))
    order = sorted(range(len(files)), key=lambda i: os.path.getsize(files[i]))      # batches of similar length: little padding
    for i in range(0, len(order), batch_size):
        waves, rates = [], []
        for j in order[i:i + batch_size]:
            pcm, sr = load_wav(files[j])
            if sr != sample_rate:
                if not resample:
                    raise SystemExit(f"compute_cmvn.py: {files[j]}: sample rate {sr}, expected {sample_rate}")
                try:
                    resample_mod.plan(sr)
                except ValueError as e:
                    raise SystemExit(f"compute_cmvn.py: {files[j]}: {e}") from e
            waves.append(pcm)
            rates.append(sr)
        S = max(256, max(len(w) for w in waves))
        wav = np.zeros((len(waves), S), dtype=np.float32)
        for b, w in enumerate(waves):
            wav[b, :len(w)] = w
        dev_wav, dev_len = torch.from_numpy(wav).to(device), torch.tensor([len(w) for w in waves], dtype=torch.int32, device=device)
        if any(r != sample_rate for r in rates):      # one launch for the batch, whatever rates it mixes
            n16 = [resample_mod.plan(r).n_out(len(w)) for w, r in zip(waves, rates)]
            dev_wav, dev_len, _ = resample_mod.resample_batch(dev_wav, [len(w) for w in waves], rates, max(256, max(n16)))
        acc.update(dev_wav, dev_len)
    return acc.sums() if sums else acc.finalize()


def main(argv):
    flags = parse_flags(argv)
    if not flags.get("collector_path") or not flags.get("out"):
        raise SystemExit("compute_cmvn.py: give --collector_path=<manifest prefix> and --out=<file.npz>")
    if not torch.cuda.is_available():
        raise SystemExit("compute_cmvn.py needs an MI355X: the front end has no CPU fallback")
    files = manifest_waves(flags["collector_path"], str(flags.get("part", "train")))
    n_mels = int(flags.get("n_mels", 40))
    frontend, out = str(flags.get("frontend", "reference")), str(flags["out"])
    if out.endswith(".json") and frontend != "kaldi":
        raise SystemExit("compute_cmvn.py: WeNet's JSON describes Kaldi fbank features: give --frontend=kaldi with --out=<file>.json")
    sum_x, sum_xx, n = compute(files, n_mels=n_mels, batch_size=int(flags.get("batch_size", 32)), sample_rate=int(flags.get("sample_rate", 16000)),
                               resample=bool(int(flags.get("resample", 0))), frontend=frontend, sums=True)
    mean, istd, count = finalize_stats(sum_x, sum_xx, n)
    if out.endswith(".json"):
        save_wenet_cmvn(out, sum_x, sum_xx, count)
    else:
        save_cmvn(out, mean, istd, count, frontend=frontend)
    print(json.dumps({"out": str(flags["out"]), "files": len(files), "frames": count, "n_mels": n_mels, "frontend": frontend,
                      "mean_range": [float(mean.min()), float(mean.max())], "std_range": [float(1 / istd.max()), float(1 / istd.min())]}))


if __name__ == "__main__":
    main(sys.argv[1:])
