#!/usr/bin/env python3
"""What the CR-CTC consistency term costs: the kernel alone, the same value and gradient from torch ops with autograd, and the training
step with and without it.  One JSON object on stdout (and in --out: profiles/cr_ctc_bench.json).

  python tools/cr_ctc_bench.py [--rounds 3] [--out profiles/cr_ctc_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/cr_ctc_bench.py --trace-run      # TRACE_CALLS calls of kernels.cr_ctc alone, to be started under rocprofv3 --kernel-trace

Shape: 32 pairs (64 rows) x 500 frames x V = 4232, bf16, rows of ld = 4288, accumulate=True onto a gradient block laid out like the logits.
  (a) kernel: kernels.cr_ctc(logits, in_len, grad_scale, dlogits=block, accumulate=True).
  (b) torch:  log_softmax / exp / the two KL terms with detached targets on the same buffers, autograd, the gradient added onto the block.
  (c) step:   the plain TransformerCTC step (6 layers, bf16, no dropout) on the 64 rows against the step with cr_ctc_weight = 0.2 on the
      same rows (the second half is the first with a block of frames and mel bins zeroed).
Contenders alternated in one process, --rounds rounds, medians.  call_ms / step_ms: host wall time of CALLS calls (STEPS eager steps)
between two synchronisations, per call.  kernels_us: per-kernel medians from a kernel trace of its own.

Expected, written down before the first run (nobody had measured this kernel):
  * bytes: the kernel reads 274 MB of logits (64 x 500 x 4288 x 2; 271 MB of them inside V) and reads and writes 549 MB of gradient,
    ~0.82 GB: 0.13 ms at the ~6.3 TB/s a copy reaches, 0.22 ms at the 3.66 TB/s the CTC kernels reach.  Two expf per element and ~15 fp64
    instructions per pair of elements ride beside the traffic at 3 waves per SIMD: nearer 0.22 than 0.13 ms; 0.2 - 0.3 ms.
  * torch: two log_softmax, exp, products, sums, a mask and their autograd on float32 copies, more than ten passes over 0.54 GB each: 5 - 10 ms,
    20 - 40 times the kernel.
  * step: the kernel's time plus one more block-sized buffer (the CTC gradient goes out of place) and the hand-over without the armed
    launch: + 0.2 - 0.4 ms on a ~6 ms step of 64 rows.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd import Models  # noqa: E402
from asr_chinese_e2e_amd import kernels as K  # noqa: E402
from asr_chinese_e2e_amd.data_handler import Vocab, synthetic_pack  # noqa: E402
from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt  # noqa: E402

DEV = "cuda"
P, T, V, LD = 32, 500, 4232, 4288
CALLS, TORCH_CALLS, STEPS, WARMUP, TRACE_CALLS, SCALE, WEIGHT = 50, 5, 20, 5, 20, 0.2 / 32, 0.2
TRACED = ("cr_ctc_kernel", "cr_ctc_pair_sum_kernel")
BYTES = {"logits_read": 2 * P * T * V * 2, "gradient_read_and_written": 2 * 2 * P * T * V * 2}
EXPECTED = {"kernel_ms": "0.2 - 0.3 (0.13 at 6.3 TB/s, 0.22 at the 3.66 TB/s of the CTC kernels)", "torch_ms": "5 - 10, 20 - 40 x the kernel",
            "step_ms": "the plain step + 0.2 - 0.4"}


class Buffers:
    def __init__(self):
        g = torch.Generator().manual_seed(7)
        base = torch.randn(P, T, V, generator=g) * 3.0
        two = torch.cat([base, base + 0.5 * torch.randn(P, T, V, generator=g)])      # the second view: the first, moved a little
        self.buf = torch.zeros(2 * P, T, LD, dtype=torch.bfloat16)
        self.buf[:, :, :V] = two.to(torch.bfloat16)
        self.buf = self.buf.to(DEV)
        self.logits = self.buf[:, :, :V]
        lens = torch.randint(T // 2, T + 1, (P,), generator=g).to(torch.int32)
        self.in_len = torch.cat([lens, lens]).to(DEV)
        self.gbuf = torch.zeros_like(self.buf)
        self.grad = self.gbuf[:, :, :V]

    def kernel(self):
        return K.cr_ctc(self.logits, self.in_len, grad_scale=SCALE, dlogits=self.grad, accumulate=True)["cr"]

    def torch_ops(self):
        z = self.logits.float().requires_grad_(True)
        lp = torch.log_softmax(z, -1)
        lpa, lpb = lp[:P], lp[P:]
        ya, yb = lpa.exp(), lpb.exp()
        live = torch.arange(T, device=DEV).view(1, T) < torch.minimum(self.in_len[:P], self.in_len[P:]).view(P, 1)
        frame = 0.5 * ((yb.detach() * (lpb.detach() - lpa)).sum(-1) + (ya.detach() * (lpa.detach() - lpb)).sum(-1)) * live
        cr = frame.sum(1)
        g, = torch.autograd.grad(cr.sum() * SCALE, z)
        self.grad += g.to(torch.bfloat16)
        return cr

    def ms(self, fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n


class Step:
    def __init__(self, **over):
        M = Models.TransformerCTC
        cfg = M.get_default_config()()
        cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, layer_num=6, ctc_weight=1.0, dtype="bf16", warm_up=4000, **over))
        torch.manual_seed(0)
        self.model = M(cfg, Vocab.synthetic(V)).to(DEV)
        self.opt = NoamOpt(cfg.d_model, 1, cfg.warm_up, FusedAdam(self.model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
        one = synthetic_pack(P, T, 80, V, seed=1234, device=DEV, dtype=torch.bfloat16)
        view1 = one.wave.clone()
        view1[:, 100:140, :] = 0
        view1[:, :, 20:30] = 0
        self.pack = type(one)({k: torch.cat([v, v]) for k, v in one.items()})
        self.pack["wave"] = torch.cat([one.wave, view1])

    def run(self, n):
        for _ in range(n):
            self.model.iterate(self.pack, optimizer=self.opt, is_train=True)

    def ms(self, n=STEPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n


def kernel_durations(path):
    """Median duration (us) and calls of the traced kernels, from a --trace-run under rocprofv3 --kernel-trace."""
    out = {}
    for r in csv.DictReader(open(path, newline="")):
        name = r.get("Kernel_Name", "")
        for k in TRACED:
            if k in name:
                out.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "calls": len(v)} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-csv", default="")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    b = Buffers()
    if a.trace_run:
        for _ in range(TRACE_CALLS):
            b.kernel()
        torch.cuda.synchronize()
        return
    # the two give the same value and gradient (bf16 block: one rounding of the added gradient apart)
    b.gbuf.zero_()
    cr_k = b.kernel().clone()
    g_k = b.grad.float().clone()
    b.gbuf.zero_()
    cr_t = b.torch_ops().detach().clone()
    g_t = b.grad.float().clone()
    agree = {"cr_max_rel": float(((cr_k - cr_t).abs() / cr_t.abs().clamp_min(1e-30)).max()), "grad_max_abs": float((g_k - g_t).abs().max()),
             "grad_max": float(g_t.abs().max()), "cr_mean": float(cr_t.mean())}
    del g_k, g_t
    steps = {"plain": Step(), "cr_ctc": Step(cr_ctc_weight=WEIGHT)}
    for s in steps.values():
        s.run(WARMUP)
    b.ms(b.kernel, 5)
    b.ms(b.torch_ops, 2)
    t = {}
    for _ in range(a.rounds):
        t.setdefault("kernel", []).append(b.ms(b.kernel, CALLS))
        t.setdefault("torch", []).append(b.ms(b.torch_ops, TORCH_CALLS))
        for name, s in steps.items():
            t.setdefault("step_" + name, []).append(s.ms())
    med = {k: statistics.median(v) for k, v in t.items()}
    total = sum(BYTES.values())
    res = {"device": torch.cuda.get_device_name(0), "expected_before_measuring": EXPECTED,
           "protocol": f"contenders alternated in one process, {a.rounds} rounds, medians; host wall time of {CALLS} kernel calls / {TORCH_CALLS} torch "
                       f"calls / {STEPS} eager steps between two synchronisations, per call; kernels_us from a kernel trace of its own",
           "workload": f"{P} pairs ({2 * P} rows) x {T} frames x V = {V}, bf16, ld = {LD}, accumulate=True; step: TransformerCTC, 6 layers, bf16, no dropout, {2 * P} rows",
           "bytes": dict(BYTES, total=total),
           "ms": {k: {"median": round(med[k], 4), "rounds": [round(x, 4) for x in v]} for k, v in t.items()},
           "kernel_call_bytes_per_s": round(total / (med["kernel"] * 1e-3), 1), "torch_over_kernel": round(med["torch"] / med["kernel"], 2),
           "step_gain_ms": round(med["step_cr_ctc"] - med["step_plain"], 4), "step_over_plain": round(med["step_cr_ctc"] / med["step_plain"], 4),
           "kernel_and_torch_agree": agree, "cr_of_the_step": float(steps["cr_ctc"].model._engine.last_cr[1].mean())}
    if a.kernels_csv:
        res["kernels_us"] = kernel_durations(a.kernels_csv)
        k_us = res["kernels_us"].get("cr_ctc_kernel", {}).get("median_us")
        if k_us:
            res["kernel_bytes_per_s"] = round(total / (k_us * 1e-6), 1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
