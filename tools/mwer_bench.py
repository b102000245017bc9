#!/usr/bin/env python3
"""What MWER training costs per step: the CTC-only training step (BASELINE config 2: batch 32, 500 frames, vocabulary 4232, 6 layers,
bf16, no dropout) with mwer_weight 0 and 0.5 at N = 4, with and without mwer_blank_skip = 0.98, and the share of the three new entry
points (asr_mwer_errors, asr_ctc_mwer_lattice, asr_ctc_mwer_grad) in it.  One JSON object on stdout (and in --out:
profiles/mwer_bench.json).

  python tools/mwer_bench.py [--rounds 3] [--out profiles/mwer_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/mwer_bench.py --trace-run      # TRACE_STEPS steps of the MWER contender alone, to be started under rocprofv3 --kernel-trace

The logits are peaky, as a trained head's are: the freshly drawn head's weights are scaled by HEAD_SCALE (one class takes almost all of a
frame's mass) and its blank bias raised by BLANK_BIAS (that class is the blank on ~95 % of the frames).  A flat head emits a token on almost
every frame, every entry of its lists is longer than the row (2 * label width + 8) and takes part in nothing; a bias alone (the first
run of this tool: + 13, blank posterior ~0.984 on every frame) gives lists of 0.8 tokens and nothing for blank skipping to drop.
`lists` reports how many entries went through the lattices and how long they are.  Every timed block starts from the same parameters
(Step.restore): in the second run the head had drifted below the skipping threshold by the time the blocks were timed.

Contenders alternated in one process, --rounds rounds, medians.  step_ms: host wall time of STEPS eager steps between two
synchronisations, per step.  stage_us: device events around each call of the search stages and the three new entry points inside the
step (a pass of its own: the events cost host time).  kernels_us: per-kernel medians from a kernel trace of its own.

Expected, written down before the first run (none of the new kernels had been measured):
  * the device search alone measures 3.8 ms per batch of this shape (README, hotword section: beam 10) against a 3.1 ms plain step; at
    beam 4 it ranks 32 instead of 110 candidates per frame but is a chain over 500 frames all the same: 2 - 3.5 ms.  The MWER step is
    search-bound and at least twice the plain step: 6 - 8 ms.
  * blank skipping at 0.98 on peaky logits drops most frames before the search (profiles/blank_skip_bench.json: 5.4x at 95 % blank):
    the search falls below 1 ms and the MWER step to 4 - 5 ms.
  * asr_mwer_errors: 128 waves on rows of <= 52 tokens: ~10 us, launch-bound.
  * asr_ctc_mwer_lattice: the log-sum-exp pass reads the logits once (135 MB, fp64 exp per element: 60 - 120 us); the lattice is 128
    workgroups, two passes of 500 dependent steps with three fp64 exp, one log and a barrier each, ~0.5 us per step: 0.4 - 0.7 ms.  It is
    the largest of the three and latency-bound: 128 workgroups leave half of the CUs idle.
  * asr_ctc_mwer_grad (accumulate = 1): 16000 workgroups that read ~N * S = 400 f32 posteriors and touch ~40 cells each: 20 - 60 us.
  * the three together: 0.5 - 0.9 ms, 8 - 15 % of the MWER step, 20 - 30 % of what the step gains over the plain one.
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
STEPS, WARMUP, TRACE_STEPS, HEAD_SCALE, BLANK_BIAS = 20, 5, 5, 5.0, 26.0
STAGES = ("ctc_frame_topk", "ctc_blank_skip_compact", "ctc_prefix_beam", "mwer_errors", "ctc_mwer_lattice", "ctc", "ctc_mwer_grad")
NEW = ("mwer_errors", "ctc_mwer_lattice", "ctc_mwer_grad")
TRACED = ("mwer_errors_kernel", "mwer_lse_kernel", "mwer_lattice_kernel", "mwer_post_kernel", "mwer_grad_kernel", "prefix_beam", "frame_topk", "blank_skip")
EXPECTED = {"step_ms": {"plain": "~3.1", "mwer": "6 - 8, search-bound", "mwer_blank_skip": "4 - 5"},
            "stage_us": {"ctc_prefix_beam": "2000 - 3500 (below 1000 behind blank skipping)", "mwer_errors": "~10", "ctc_mwer_lattice": "400 - 700",
                         "ctc_mwer_grad": "20 - 60"},
            "new_entry_points_share_of_mwer_step": "8 - 15 %"}
CONTENDERS = {"plain": dict(mwer_weight=0.0), "mwer": dict(mwer_weight=0.5, mwer_nbest=4), "mwer_blank_skip": dict(mwer_weight=0.5, mwer_nbest=4, mwer_blank_skip=0.98)}


class Step:
    def __init__(self, **over):
        M = Models.TransformerCTC
        cfg = M.get_default_config()()
        cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, layer_num=6, ctc_weight=1.0, dtype="bf16", warm_up=4000, **over))
        torch.manual_seed(0)
        self.model = M(cfg, Vocab.synthetic(4232))
        with torch.no_grad():
            dict(self.model.named_parameters())["ctc_lo.weight"].mul_(HEAD_SCALE)
            dict(self.model.named_parameters())["ctc_lo.bias"][0] += BLANK_BIAS
        self.model = self.model.to(DEV)
        self.opt = NoamOpt(cfg.d_model, 1, cfg.warm_up, FusedAdam(self.model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
        self.pack = synthetic_pack(32, 500, 80, 4232, seed=1234, device=DEV, dtype=torch.bfloat16)
        self.p0 = None

    def restore(self):
        """Every timed block starts from the same parameters: Adam moves all 512 weights of a class by the learning rate at once, and a few
        dozen steps take the head's blank posterior from 1 - 3e-7 below 0.98 (the second run of this tool: blank skipping then drops nothing)."""
        f = self.model._flat
        if self.p0 is None:
            self.p0 = f.p.clone()
        else:
            f.p.copy_(self.p0)
            f.refresh_lowp()

    def run(self, n):
        for _ in range(n):
            self.model.iterate(self.pack, optimizer=self.opt, is_train=True)

    def ms(self, n=STEPS):
        self.restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def taking_part(self):
        last = self.model._engine.last_mwer
        if last is None:
            return None
        tok, ln, err, post, risk = last
        return {"entries": int((ln >= 0).sum()), "taking_part": int((post > 0).sum()), "row_width": int(tok.shape[2]),
                "mean_length": round(float(ln[ln >= 0].float().mean()), 1), "mean_risk": round(float(risk.mean()), 3)}


def time_stage(name):
    """Route a wrapper of kernels.py that does not time itself through kernels.timed (the engine calls it through the module)."""
    fn = getattr(K, name)
    setattr(K, name, lambda *a, **kw: K.timed(name, 0.0, lambda: fn(*a, **kw)))


def kernel_durations(path):
    """Median duration (us) and calls per step of every traced kernel, from a --trace-run under rocprofv3 --kernel-trace."""
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
    if a.trace_run:
        s = Step(**CONTENDERS["mwer"])
        s.run(TRACE_STEPS)
        torch.cuda.synchronize()
        return
    steps = {name: Step(**over) for name, over in CONTENDERS.items()}
    for s in steps.values():
        s.run(WARMUP)
    t = {}
    for _ in range(a.rounds):
        for name, s in steps.items():
            t.setdefault(name, []).append(s.ms())
    med = lambda v: round(statistics.median(v), 3)      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "expected_before_measuring": EXPECTED,
           "protocol": f"contenders alternated in one process, {a.rounds} rounds, medians; step_ms: host wall time of {STEPS} eager steps between two "
                       "synchronisations, per step; stage_us: device events around the calls inside the step, a pass of its own; kernels_us from a "
                       "kernel trace of its own",
           "workload": "TransformerCTC, batch 32, 500 frames, vocabulary 4232, 6 layers, bf16, no dropout; ctc_lo.weight *= %g, ctc_lo.bias[0] += %g" % (HEAD_SCALE, BLANK_BIAS),
           "step_ms": {k: {"median": med(v), "rounds": [round(x, 3) for x in v]} for k, v in t.items()},
           "lists": {name: s.taking_part() for name, s in steps.items()}}
    m = {k: v["median"] for k, v in res["step_ms"].items()}
    res["step_over_plain"] = {k: round(m[k] / m["plain"], 3) for k in m if k != "plain"}
    res["stage_us"] = {}
    for name in ("ctc_frame_topk", "ctc_blank_skip_compact", "ctc_prefix_beam", "mwer_errors"):
        time_stage(name)
    for name in ("mwer", "mwer_blank_skip"):
        K.TIMER = K.LaunchTimer(STAGES)
        steps[name].restore()
        steps[name].run(STEPS)
        torch.cuda.synchronize()
        summ, K.TIMER = K.TIMER.summary(), None
        per = {k: round(v["total_ms"] * 1e3 / STEPS, 2) for k, v in summ.items()}
        new = sum(per.get(k, 0.0) for k in NEW)
        res["stage_us"][name] = dict(per, new_entry_points=round(new, 2), new_share_of_step=round(new / (m[name] * 1e3), 4),
                                     new_share_of_gain_over_plain=round(new / max((m[name] - m["plain"]) * 1e3, 1e-9), 4))
    if a.kernels_csv:
        res["kernels_us"] = kernel_durations(a.kernels_csv)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
