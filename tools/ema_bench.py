#!/usr/bin/env python3
"""What the exponential moving average of the parameters costs per optimizer step: asr_adam_step, asr_adam_ema_step (the average inside
the Adam pass) and asr_adam_step + asr_ema_update (the average as a pass of its own) over flat buffers of the CTC-only and the joint
model's size, and the whole joint training step with ema_decay 0 and 0.999.  One JSON object on stdout (and in --out:
profiles/ema_bench.json).

  python tools/ema_bench.py [--rounds 3] [--out profiles/ema_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/ema_bench.py --trace-run      # the launches alone, in a fixed order, to be started under rocprofv3 --kernel-trace

Contenders alternated in one process, --rounds rounds, medians.  *_us of the contenders: device events around REPS back-to-back calls,
per call.  step_ms: host wall time of STEPS eager steps between two synchronisations, per step (bench.py's joint workload: batch 32, 500
frames, 6 layers, vocabulary 4232, bf16, no dropout).  The kernels' own durations come from a trace run of its own with --kernels-csv.

Expected, written down before the first run (nothing here had been measured):
  * bytes per parameter: the plain Adam pass moves 30 - 34 (p, g, m, v read and p, m, v written in fp32 = 28, the bf16 shadow 2, the
    clipped gradient 4 when something was clipped); the fused average adds 8 (ema read and written), the stand-alone pass adds 12 (it
    reads p again).
  * at the joint model's size (flat.g is ~160 MB, 40 M parameters) that is ~320 MB more per step fused against ~480 MB stand-alone; at
    4 - 5 TB/s, which is what element-wise kernels of this kind reach on an MI355X, 65 - 80 us against 100 - 120 us, on a step of ~5 ms:
    1.3 - 1.6 % against 2 - 2.4 %, below what two runs of the step differ by.
  * the plain pass: 1.36 GB (34 B x 40 M) -> 270 - 340 us; the fused one (42 B) 340 - 420 us, ratio 1.24; plain + stand-alone (46 B
    and one more launch) ratio 1.35 - 1.4.
  * the CTC-only model (~19 M parameters, ~76 MB per buffer): the same ratios at about half the times.
  * asr_adam_step itself: the same code object as before this tool existed (profiles/ema_resource_usage.txt), so its time is the
    parent's.
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
REPS, STEPS, TRACE_CALLS = 20, 20, 5
KERNELS = (("adam_kernel<false>", "adam_kernelILb0"), ("adam_kernel<true>", "adam_kernelILb1"), ("ema_update_kernel",))      # demangled or not
EXPECTED = {"bytes_per_parameter": {"adam_step": "30 - 34", "adam_ema_step": "+ 8", "adam_step + ema_update": "+ 12"},
            "joint": {"adam_step_us": "270 - 340", "adam_ema_step_us": "340 - 420", "ema_update_us": "100 - 120", "fused_over_plain": "1.24",
                      "separate_over_plain": "1.35 - 1.4", "extra_bytes_fused_MB": "~320", "extra_bytes_separate_MB": "~480"},
            "ctc": "the same ratios at about half the times",
            "joint_step": {"step_ms": "~5", "ema_0.999_over_ema_0": "1.013 - 1.016, inside the spread of two runs"}}


def model_of(kind, ema_decay=0.0):
    M = Models.TransformerOffical if kind == "joint" else Models.TransformerCTC
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, layer_num=6, ctc_weight=0.3 if kind == "joint" else 1.0, dtype="bf16", warm_up=4000,
                      ema_decay=ema_decay))
    torch.manual_seed(0)
    return M(cfg, Vocab.synthetic(4232)), cfg


class Flat:
    """Buffers of a model's flat size with a gradient whose norm is above the clipping threshold, as in training."""

    def __init__(self, n):
        g = torch.Generator(device=DEV).manual_seed(n % 9973)
        r = lambda s: torch.randn(n, generator=g, device=DEV) * s      # noqa: E731
        self.n = n
        self.p, self.g, self.m, self.v, self.ema = r(0.05), r(0.01), r(0.001), r(0.001).abs(), r(0.05)
        self.lp = self.p.bfloat16()
        self.hyper = torch.tensor([1e-4, 0.5, 0.5, 100.0], device=DEV)
        self.sumsq = torch.zeros(1, device=DEV)
        K.grad_sumsq(self.g, self.sumsq, K.Workspace(DEV))

    def plain(self):
        K.adam_step(self.p, self.g, self.m, self.v, self.lp, self.hyper, self.sumsq, 5.0, 0.9, 0.98, 1e-9)

    def fused(self):
        K.adam_ema_step(self.p, self.g, self.m, self.v, self.lp, self.hyper, self.sumsq, 5.0, 0.9, 0.98, 1e-9, self.ema, 0.999, True)

    def update(self):
        K.ema_update(self.p, self.ema, 0.999, 100, True)

    def separate(self):
        self.plain()
        self.update()


def device_us(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


class Step:
    def __init__(self, ema_decay):
        self.model, cfg = model_of("joint", ema_decay)
        self.model = self.model.to(DEV)
        self.opt = NoamOpt(cfg.d_model, 1, cfg.warm_up, FusedAdam(self.model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
        self.pack = synthetic_pack(32, 500, 80, 4232, seed=1234, device=DEV, dtype=torch.bfloat16)

    def run(self, n):
        for _ in range(n):
            self.model.iterate(self.pack, optimizer=self.opt, is_train=True)

    def ms(self, n=STEPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n


def kernel_durations(path, sizes):
    """Median duration (us) of each kernel per size, from the trace run's fixed order: per size TRACE_CALLS x (plain, fused, update)."""
    rows = sorted((r for r in csv.DictReader(open(path, newline="")) if any(k in r.get("Kernel_Name", "") for alt in KERNELS for k in alt)),
                  key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[-len(sizes) * TRACE_CALLS * 3:]
    assert len(rows) == len(sizes) * TRACE_CALLS * 3, len(rows)
    out = {}
    for i, name in enumerate(sizes):
        mine = rows[i * TRACE_CALLS * 3:(i + 1) * TRACE_CALLS * 3]
        for j, alt in enumerate(KERNELS):
            sel = mine[j::3]
            assert all(any(k in r["Kernel_Name"] for k in alt) for r in sel), (name, alt, sel[0]["Kernel_Name"])
            out.setdefault(name, {})[alt[0]] = round(statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sel), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-csv", default="")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--no-step", action="store_true", help="skip the whole joint training step")
    a = ap.parse_args()
    sizes = {kind: model_of(kind)[0]._flat.numel for kind in ("ctc", "joint")}
    flats = {kind: Flat(n) for kind, n in sizes.items()}
    for f in flats.values():      # warm-up: code objects loaded, every buffer touched
        f.plain(), f.fused(), f.update()
    torch.cuda.synchronize()
    if a.trace_run:
        for kind in sizes:
            for _ in range(TRACE_CALLS):
                flats[kind].plain(), flats[kind].fused(), flats[kind].update()
        torch.cuda.synchronize()
        return
    med = lambda v: round(statistics.median(v), 3)      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "expected_before_measuring": EXPECTED,
           "protocol": f"contenders alternated in one process, {a.rounds} rounds, medians; *_us: device events around {REPS} back-to-back calls, per call; "
                       f"step_ms: host wall time of {STEPS} eager joint steps between two synchronisations, per step; kernels_us from a kernel trace of its own",
           "parameters": sizes, "buffer_MB": {k: round(4 * n / 1e6, 1) for k, n in sizes.items()}}
    t = {}
    for _ in range(a.rounds):
        for kind, f in flats.items():
            for name in ("plain", "fused", "update", "separate"):
                t.setdefault(f"{kind}_{name}_us", []).append(device_us(getattr(f, name)))
    steps = None
    if not a.no_step:
        for f in flats.values():
            del f.p, f.g, f.m, f.v, f.ema, f.lp
        flats.clear()
        torch.cuda.empty_cache()
        steps = {"ema_0": Step(0.0), "ema_0.999": Step(0.999)}
        for s in steps.values():
            s.run(5)
        for _ in range(a.rounds):
            for name, s in steps.items():
                t.setdefault(f"joint_step_{name}_ms", []).append(s.ms())
    res["timings"] = {k: {"median": med(v), "rounds": [round(x, 3) for x in v]} for k, v in t.items()}
    m = {k: v["median"] for k, v in res["timings"].items()}
    for kind, n in sizes.items():
        res.setdefault("ratios", {})[kind] = {"fused_over_plain": round(m[f"{kind}_fused_us"] / m[f"{kind}_plain_us"], 3),
                                              "separate_over_plain": round(m[f"{kind}_separate_us"] / m[f"{kind}_plain_us"], 3),
                                              "fused_extra_us": round(m[f"{kind}_fused_us"] - m[f"{kind}_plain_us"], 2),
                                              "separate_extra_us": round(m[f"{kind}_separate_us"] - m[f"{kind}_plain_us"], 2)}
        # bytes the algorithm needs (clipping active: the clipped gradient is written back), over the measured time
        res.setdefault("achieved_TB_per_s", {})[kind] = {"plain_34B": round(34.0 * n / m[f"{kind}_plain_us"] / 1e6, 2),
                                                         "fused_42B": round(42.0 * n / m[f"{kind}_fused_us"] / 1e6, 2),
                                                         "update_12B": round(12.0 * n / m[f"{kind}_update_us"] / 1e6, 2)}
    if steps is not None:
        res["joint_step_ema_over_plain"] = round(m["joint_step_ema_0.999_ms"] / m["joint_step_ema_0_ms"], 4)
    if a.kernels_csv:
        res["kernels_us"] = kernel_durations(a.kernels_csv, list(sizes))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
