#!/usr/bin/env python3
"""Filler frames in the long-recording alignment: what asr_ctc_align_long_filler costs beside asr_ctc_align_long.  One JSON object on
stdout, written to --out.

  python tools/align_filler_bench.py [--rounds 3] [--calls 3] [--out profiles/align_filler_bench.json]
  rocprofv3 --kernel-trace --stats -- python tools/align_filler_bench.py --rounds 1      (kernel durations: a run of its own)

The shapes of tools/align_long_bench.py: (T, L) = (20 000, 3 000) and (60 000, 8 192), V = 4232, bf16 rows of random logits, random labels
(both reach the P = 8 instantiation).  star = the frame's best log posterior - 2.  Three contenders per shape, alternated in one process
over --rounds rounds, HIP events around --calls back-to-back calls, medians:
  plain_ms        asr_ctc_align_long
  filler_20_ms    asr_ctc_align_long_filler, the gap in front of every 20th token and the tail wide
  filler_all_ms   asr_ctc_align_long_filler, every gap and the tail wide
and the ratios of the two filler runs to the plain one of the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.align_long_bench import DEV, V, case, rounds_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from asr_chinese_e2e_amd import kernels as K
    out = {"device": torch.cuda.get_device_name(0), "V": V, "dtype": "bf16", "penalty": 2.0, "shapes": {}}
    for T, L in ((20000, 3000), (60000, 8192)):
        rows, lse, lab = case(torch, np, K, T, L, L)
        _, best, _, _, _ = K.ctc_frame_stats(rows.view(1, T, V), None, 0)
        star = (best.view(T) - 2.0).contiguous()
        every, sparse = np.ones(L, np.uint8), np.zeros(L, np.uint8)
        sparse[::20] = 1
        ws = K.Workspace(DEV)
        plain = lambda: K.ctc_align_long(rows, lse, [0, T], lab, [0, L], ws=ws)      # noqa: E731
        fill = lambda gap: K.ctc_align_long_filler(rows, lse, star, [0, T], lab, [0, L], gap, [1], ws=ws)      # noqa: E731
        res, med = rounds_of(torch, {"plain_ms": plain, "filler_20_ms": lambda: fill(sparse), "filler_all_ms": lambda: fill(every)}, a.rounds, a.calls)
        p20, pall = fill(sparse), fill(every)
        out["shapes"][f"T{T}_L{L}"] = {"T": T, "L": L, "rounds": res, "median_ms": med,
                                       "filler_20_over_plain": round(med["filler_20_ms"] / med["plain_ms"], 4),
                                       "filler_all_over_plain": round(med["filler_all_ms"] / med["plain_ms"], 4),
                                       "scores": {"plain": float(plain()[3][0]), "filler_20": float(p20[3][0]), "filler_all": float(pall[3][0])},
                                       "filler_frames": {"filler_20": int((p20[0] == -2).sum()), "filler_all": int((pall[0] == -2).sum())}}
        del rows, lse, star, ws, p20, pall
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
