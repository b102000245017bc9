#!/usr/bin/env python3
"""CTC forced alignment at configs[2] shapes (B = 32, T = 500, V = 4232, bf16 logits in the engine's padded rows, ~22 labels per
utterance): microseconds per K.ctc_align, per K.ctc_fwd_bwd(want_grad=False) on the same inputs, and per alignment written with torch
ops (log_softmax, gather, a loop over frames for the max recursion and another for the backtrace).  Prints one JSON line.

    python tools/ctc_align_bench.py [--iters 50] [--out profiles/ctc_align_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd import kernels as K  # noqa: E402


def time_us(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def torch_align(logits, in_len, labels, lab_len, blank=0):
    """The same Viterbi alignment with torch ops (fp32 log domain): returns (score (B,), states (B, T))."""
    B, T, V = logits.shape
    L = labels.shape[1]
    S = 2 * L + 1
    dev = logits.device
    logp = torch.log_softmax(logits.float(), -1)
    ext = torch.full((B, S), blank, dtype=torch.long, device=dev)
    ext[:, 1::2] = labels.long()
    y = logp.gather(2, ext.unsqueeze(1).expand(B, T, S))                      # (B, T, S)
    s_idx = torch.arange(S, device=dev)
    valid = s_idx.unsqueeze(0) <= 2 * lab_len.long().unsqueeze(1)
    skip = torch.zeros(B, S, dtype=torch.bool, device=dev)
    skip[:, 3::2] = labels[:, 1:].long() != labels[:, :-1].long()
    neg = torch.tensor(float("-inf"), device=dev)
    delta = torch.full((B, S), float("-inf"), device=dev)
    delta[:, 0] = y[:, 0, 0]
    delta[:, 1] = y[:, 0, 1]
    delta = torch.where(valid, delta, neg)
    bps = []
    for t in range(1, T):
        d1 = torch.cat([delta.new_full((B, 1), float("-inf")), delta[:, :-1]], 1)
        d2 = torch.where(skip, torch.cat([delta.new_full((B, 2), float("-inf")), delta[:, :-2]], 1), neg)
        cand = torch.stack([delta, d1, d2], -1)
        best, arg = cand.max(-1)
        new = torch.where(valid, best + y[:, t], neg)
        live = (t < in_len).unsqueeze(1)
        delta = torch.where(live, new, delta)
        bps.append(torch.where(live, arg, torch.zeros_like(arg)))
    Lb = lab_len.long()
    fb = delta.gather(1, (2 * Lb).unsqueeze(1)).squeeze(1)
    fl = delta.gather(1, (2 * Lb - 1).clamp(min=0).unsqueeze(1)).squeeze(1)
    fl = torch.where(Lb > 0, fl, neg)
    s = torch.where(fb >= fl, 2 * Lb, 2 * Lb - 1)
    score = torch.maximum(fb, fl)
    states = torch.empty(B, T, dtype=torch.long, device=dev)
    for t in range(T - 1, -1, -1):
        states[:, t] = s
        if t > 0:
            s = s - bps[t - 1].gather(1, s.unsqueeze(1)).squeeze(1)
    return score, states


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T, V, L = 32, 500, 4232, 22
    ld = (V + 63) // 64 * 64
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    buf = (torch.randn(B * T, ld, generator=g, device=dev) * 3.0).to(torch.bfloat16)
    logits = buf[:, :V].view(B, T, V)
    in_len = torch.randint(T * 3 // 5, T + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    in_len[0] = T
    lab_len = torch.randint(L - 6, L + 7, (B,), generator=g, device=dev, dtype=torch.int32)
    Lmax = int(lab_len.max())
    labels = torch.randint(1, V, (B, Lmax), generator=g, device=dev, dtype=torch.int32)
    ws = K.Workspace(dev)
    ws_fb = K.Workspace(dev)
    align_us = time_us(lambda: K.ctc_align(logits, in_len, labels, lab_len, ws=ws), a.iters)
    fb_us = time_us(lambda: K.ctc_fwd_bwd(logits, in_len, labels, lab_len, ws_fb, want_grad=False), a.iters)
    torch_us = time_us(lambda: torch_align(logits, in_len, labels, lab_len), 2, warmup=1)
    path, spans, tlp, score = K.ctc_align(logits, in_len, labels, lab_len, ws=ws)
    t_score, t_states = torch_align(logits, in_len, labels, lab_len)
    torch.cuda.synchronize()
    rel = float(((score - t_score).abs() / t_score.abs()).max())
    line = dict(tool="ctc_align_bench", B=B, T=T, V=V, ld=ld, dtype="bf16", mean_L=float(lab_len.float().mean()),
                ctc_align_us=round(align_us, 2), ctc_fwd_bwd_nograd_us=round(fb_us, 2), ratio=round(align_us / fb_us, 3),
                torch_ops_us=round(torch_us, 1), speedup_vs_torch=round(torch_us / align_us, 1),
                score_max_rel_diff_vs_torch_fp32=rel, iters=a.iters, device=torch.cuda.get_device_name(0))
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
