#!/usr/bin/env python3
"""What intermediate CTC costs in the training step: the plain TransformerCTC step, the step with interctc_layers=(3,), and that step
with self-conditioning; beside them the two softmax kernels and the six products of a conditioned layer, each alone.  One JSON object on
stdout (and in --out: profiles/interctc_bench.json).

  python tools/interctc_bench.py [--rounds 3] [--out profiles/interctc_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/interctc_bench.py --trace-run      # TRACE_STEPS conditioned steps alone, to be started under rocprofv3 --kernel-trace

Shape: 32 utterances x 500 frames, V = 4232 (rows of ld = 4288), 6 layers, bf16, no dropout, w = 0.3.
Contenders alternated in one process, --rounds rounds, medians.  step_ms: host wall time of STEPS eager steps between two
synchronisations, per step.  call_us: the same for CALLS calls of one kernel or product.  kernels_us: per-kernel medians from a kernel
trace of its own (the conditioned step).

Expected, written down before the first run, from bytes and FLOPs alone (nobody had measured these):
  * softmax_rows: reads 16000 x 4232 bf16 and writes as much, ~0.27 GB: ~0.07 ms at the 3.7 - 4 TB/s the CTC and CR-CTC kernels reach.
  * softmax_bwd_add: reads p, dp and the gradient block and writes the block, ~0.55 GB: ~0.14 ms.
  * each 16000 x 4232 x 512 product is 69 GFLOP: ~0.11 ms at the rate the NT family measures on the head (94 us forward, 76 us input gradient).
  * a conditioned layer adds six such products (head forward, its input and weight gradient, the conditioning's three) and one CTC
    forward-backward (~0.25 ms): ~0.65 ms of products + 0.25 + 0.21 of softmax ~ 1.1 ms if nothing overlapped; the three weight gradients run
    on the side stream, so + 0.7 - 1.0 ms on the ~3.1 ms step.  Plain intermediate CTC adds three products and the CTC kernels: + 0.4 - 0.6 ms.
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
B, T, V, LD, D = 32, 500, 4232, 4288, 512
CALLS, STEPS, WARMUP, TRACE_STEPS, WEIGHT, LAYERS = 50, 20, 5, 10, 0.3, (3,)
TRACED = ("softmax_rows_kernel", "softmax_bwd_add_kernel")
BYTES = {"softmax_rows": 2 * B * T * V * 2, "softmax_bwd_add": 4 * B * T * V * 2}
FLOP = 2.0 * B * T * V * D
EXPECTED = {"softmax_rows_ms": "~0.07 (0.27 GB at 3.7 - 4 TB/s)", "softmax_bwd_add_ms": "~0.14 (0.55 GB)",
            "product_ms": "~0.11 each (69 GFLOP at the NT family's measured rate)",
            "step_ms": "plain + 0.4 - 0.6 (intermediate CTC), plain + 0.7 - 1.0 (conditioned: six products, one CTC forward-backward, the two softmax passes)"}


class Step:
    def __init__(self, **over):
        M = Models.TransformerCTC
        cfg = M.get_default_config()()
        cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, layer_num=6, ctc_weight=1.0, dtype="bf16", warm_up=4000, **over))
        torch.manual_seed(0)
        self.model = M(cfg, Vocab.synthetic(V)).to(DEV)
        self.opt = NoamOpt(cfg.d_model, 1, cfg.warm_up, FusedAdam(self.model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
        self.pack = synthetic_pack(B, T, 80, V, seed=1234, device=DEV, dtype=torch.bfloat16)

    def run(self, n):
        for _ in range(n):
            self.metrics, _ = self.model.iterate(self.pack, optimizer=self.opt, is_train=True)

    def ms(self, n=STEPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n


def call_us(fn, n=CALLS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def pieces(eng):
    """The kernels and products of one conditioned layer, each alone, on buffers laid out as the engine lays them out."""
    g = torch.Generator().manual_seed(7)
    h = torch.randn(B * T, D, generator=g).to(torch.bfloat16).to(DEV)
    e = torch.randn(B * T, D, generator=g).to(torch.bfloat16).to(DEV)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)      # every frame live: the byte counts above are exact
    zbuf, pbuf, dbuf, gbuf = (torch.zeros(B * T, LD, dtype=torch.bfloat16, device=DEV) for _ in range(4))
    z, p, dp, gr = (t[:, :V] for t in (zbuf, pbuf, dbuf, gbuf))
    fr = lambda t: t.view(B, T, V)      # noqa: E731
    eng.ctc_lo.fwd(h, out=z)
    out = torch.empty_like(h)
    ws = K.Workspace(DEV)
    return {
        "softmax_rows": lambda: K.softmax_rows(fr(z), lens, out=fr(p)),
        "softmax_bwd_add": lambda: K.softmax_bwd_add(fr(p), fr(dp), lens, fr(gr), accumulate=True),
        "head_fwd": lambda: eng.ctc_lo.fwd(h, out=z),
        "head_dgrad": lambda: eng.ctc_lo.dgrad(gr),
        "head_wgrad": lambda: eng.ctc_lo.wgrad(gr, h, with_bias=True, ws=ws),
        "cond_fwd": lambda: K.gemm_nt(p, eng.cond.wlp, None, out, res=h),
        "cond_dgrad": lambda: eng.cond.dgrad(e, out=dp),
        "cond_wgrad": lambda: eng.cond.wgrad(e, p, ws=ws),
    }


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
    keys = dict(interctc_weight=WEIGHT, interctc_layers=LAYERS)
    if a.trace_run:
        s = Step(interctc_condition=True, **keys)
        s.run(TRACE_STEPS)
        torch.cuda.synchronize()
        return
    steps = {"plain": Step(), "interctc": Step(**keys), "conditioned": Step(interctc_condition=True, **keys)}
    for s in steps.values():
        s.run(WARMUP)
    eng = steps["conditioned"].model._engine
    parts = pieces(eng)

    def fresh():      # the input-gradient products multiply by this step's transposed weight copies
        eng.refresh_transposes()
        eng.wait_transposes()
    fresh()
    for fn in parts.values():
        call_us(fn, 5)
    t, c = {}, {}
    for _ in range(a.rounds):
        for name, s in steps.items():
            t.setdefault(name, []).append(s.ms())
        fresh()
        for name, fn in parts.items():
            c.setdefault(name, []).append(call_us(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    cmed = {k: statistics.median(v) for k, v in c.items()}
    res = {"device": torch.cuda.get_device_name(0), "expected_before_measuring": EXPECTED,
           "protocol": f"contenders alternated in one process, {a.rounds} rounds, medians; host wall time of {STEPS} eager steps / {CALLS} calls of one "
                       f"kernel or product between two synchronisations, per step / call; kernels_us from a kernel trace of the conditioned step, a run of its own",
           "workload": f"TransformerCTC, {B} x {T} frames, V = {V} (ld = {LD}), 6 layers, bf16, no dropout, w = {WEIGHT}, layers = {list(LAYERS)}",
           "bytes": BYTES, "flop_per_product": FLOP,
           "step_ms": {k: {"median": round(med[k], 4), "rounds": [round(x, 4) for x in v]} for k, v in t.items()},
           "step_gain_ms": {k: round(med[k] - med["plain"], 4) for k in ("interctc", "conditioned")},
           "call_us": {k: {"median": round(cmed[k], 2), "rounds": [round(x, 2) for x in v]} for k, v in c.items()},
           "call_bytes_per_s": {k: round(BYTES[k] / (cmed[k] * 1e-6), 1) for k in BYTES},
           "call_flop_per_s": {k: round(FLOP / (cmed[k] * 1e-6), 1) for k in cmed if k not in BYTES},
           "loss": {k: float(s.metrics.loss) for k, s in steps.items()},
           "interctc": {k: float(s.metrics.interctc) for k, s in steps.items() if "interctc" in s.metrics}}
    if a.kernels_csv:
        res["kernels_us"] = kernel_durations(a.kernels_csv)
        for k, short in (("softmax_rows_kernel", "softmax_rows"), ("softmax_bwd_add_kernel", "softmax_bwd_add")):
            us = res["kernels_us"].get(k, {}).get("median_us")
            if us:
                res.setdefault("kernel_bytes_per_s", {})[short] = round(BYTES[short] / (us * 1e-6), 1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
