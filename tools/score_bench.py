#!/usr/bin/env python3
"""What token-level scoring costs: scoring.align_ids (asr_edit_align: one upload, one launch, one copy back) beside the only scorer the
project had, the two-row Python DP of Utils/score.py, which returns a distance and nothing else.  One JSON object on stdout (and in
--out: profiles/score_bench.json).

  python tools/score_bench.py [--rounds 3] [--out profiles/score_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/score_bench.py --trace-run      # the launches alone, in a fixed order, to be started under rocprofv3 --kernel-trace

Cases: "batch": 320 pairs of about 15 tokens (one validation batch), V = 4232, the hypothesis = the reference with ~10 % edits;
"nbest": 7176 references x 10 hypotheses (a test set's n-best lists), ops for none of them (the oracle's mode) and for all of them;
"long": one 15 000 x 15 000 pair (a stitched long-form transcript), masks in the workspace (56 MB); "lds" / "ws": one 380 x 1000 and one
390 x 1000 pair, the largest that keeps its masks in LDS and the smallest that does not.  Contenders alternated in one process, --rounds
rounds, medians; host wall time of whole calls.  The Python DP of the long pair is extrapolated from a 2000 x 2000 pair by the cell
count (x 56.25), and said so in the output.  launch_event_ms are device events around the whole wrapper call (the host's checks of
71 760 pairs sit between them: no kernel time); the kernels' own durations come from the trace with --kernels-csv.  "ops" minus "counts"
is what the mask stores and the backtrace add over a forward pass that carries counts instead.

Expected, written down before the first run (nobody had run this kernel):
  * A row step of a block is a dependent chain: an LDS read, two lane shifts, a six-step scan, two ballots, ~150 - 250 cycles, i.e.
    ~0.1 us.  A 15 x 15 pair is 15 such steps and a 15 - 20 step walk in LDS: 3 - 5 us of kernel for the batch of 320 (one wave per CU),
    and the call is all host: packing lists, one upload, one copy back, building 320 dicts - 0.3 - 0.6 ms.  The Python DP does 320 x 225
    cells at ~0.3 us: 20 - 30 ms.  So 40 - 80 x at this size, none of it due to the kernel's speed.
  * nbest: 71 760 waves of ~2 us each over 256 CUs x 8 or more resident waves: 50 - 150 us of kernel.  The host side packs 71 760 lists
    (~0.1 s) and with ops builds a million tuples (~0.5 s); the Python DP needs 5 - 7 s.  10 - 50 x, host-bound.
  * long: 235 blocks x 15 000 rows = 3.5 M row steps on ONE wave: 0.3 - 0.5 s; the walk is <= 30 000 dependent 16-byte reads from
    global memory at ~1 us: 30 ms.  The forward pass dominates by 10 x.  The Python DP: ~1 s for 2000 x 2000, so ~1 minute: ~150 x.
  * lds / ws: 380 rows x 16 blocks = 6 000 row steps, ~0.7 ms forward; the walk of ~1 100 steps costs ~0.15 ms from LDS (~130 ns a step)
    and ~1 ms from the workspace: the backtrace is a fifth of the kernel in LDS and more than half of it from global memory.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd import kernels as K  # noqa: E402
from asr_chinese_e2e_amd.scoring import align_ids  # noqa: E402
from asr_chinese_e2e_amd.Utils.score import edit_distance  # noqa: E402

DEV = "cuda"
V = 4232
TRACE_CALLS = 3
EXPECTED = {"batch_320": {"kernel_us": "3 - 5", "align_ids_ms": "0.3 - 0.6", "python_dp_ms": "20 - 30", "ratio": "40 - 80"},
            "nbest_7176x10": {"kernel_us": "50 - 150", "align_ids_s": "0.1 (counts) - 0.7 (ops)", "python_dp_s": "5 - 7", "ratio": "10 - 50"},
            "long_15000": {"kernel_s": "0.3 - 0.5", "backtrace_share": "< 0.1", "python_dp_s": "~60 (extrapolated)", "ratio": "~150"},
            "lds_vs_ws": {"forward_ms": "~0.7", "backtrace_lds_ms": "~0.15", "backtrace_ws_ms": "~1"}}


def edited(rng, ref, rate=0.1):
    h = []
    for t in ref:
        u = rng.random()
        if u < rate / 3:
            continue
        h.append(int(rng.integers(4, V)) if u < 2 * rate / 3 else t)
        if u > 1 - rate / 3:
            h.append(int(rng.integers(4, V)))
    return h


def make_cases():
    rng = np.random.default_rng(0)
    seq = lambda n: rng.integers(4, V, n).tolist()      # noqa: E731
    c = {}
    refs = [seq(int(rng.integers(10, 21))) for _ in range(320)]
    c["batch"] = dict(refs=refs, hyps=[edited(rng, r) for r in refs], ref_of=None)
    refs = [seq(int(rng.integers(10, 21))) for _ in range(7176)]
    ref_of = [u for u in range(7176) for _ in range(10)]
    c["nbest"] = dict(refs=refs, hyps=[edited(rng, refs[u]) for u in ref_of], ref_of=ref_of)
    ref = seq(15000)
    c["long"] = dict(refs=[ref], hyps=[(edited(rng, ref) + seq(1500))[:15000]], ref_of=None)
    for name, m in (("lds", 380), ("ws", 390)):
        ref = seq(m)
        c[name] = dict(refs=[ref], hyps=[(edited(rng, ref) + seq(1000))[:1000]], ref_of=None)
    ref = seq(2000)
    c["py_2000"] = dict(refs=[ref], hyps=[(edited(rng, ref) + seq(200))[:2000]], ref_of=None)
    assert K.edit_align_workspace_bytes([1000], [380], [0], 1000, 380) == 0 < K.edit_align_workspace_bytes([1000], [390], [0], 1000, 390)
    return c


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def python_dp(case):
    ro = case["ref_of"] or range(len(case["hyps"]))
    return [edit_distance(h, case["refs"][u]) for h, u in zip(case["hyps"], ro)]


class Launch:
    """A case on the device, so that the launch alone can be timed (device events) or traced."""

    def __init__(self, case):
        hyps, refs = case["hyps"], case["refs"]
        self.hl, self.rl = [len(h) for h in hyps], [len(r) for r in refs]
        self.ro = list(case["ref_of"] or range(len(hyps)))
        pad = lambda rows: torch.tensor([r + [0] * (max(map(len, rows)) - len(r)) for r in rows], dtype=torch.int32, device=DEV)      # noqa: E731
        self.hyp, self.ref = pad(hyps), pad(refs)
        self.d = [torch.tensor(x, dtype=torch.int32, device=DEV) for x in (self.hl, self.rl, self.ro)]
        self.ws = K.Workspace(DEV)
        self.out = {}

    def __call__(self, ops):
        if ops not in self.out:      # outputs allocated once: the timed call is the launch
            self.out[ops] = K.edit_align(self.hyp, self.d[0], self.ref, self.d[1], self.d[2], self.hl, self.rl, self.ro, ops=ops, ws=self.ws)
        c, o, n = self.out[ops]
        return K.edit_align(self.hyp, self.d[0], self.ref, self.d[1], self.d[2], self.hl, self.rl, self.ro, ops=ops, ws=self.ws, counts=c, ops_out=o, n_ops=n)

    def event_ms(self, ops):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        self(ops)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)


def kernel_durations(path, order):
    """The median over the trace run's calls of each (case, mode) launch, in the trace run's fixed order (us)."""
    rows = sorted((r for r in csv.DictReader(open(path, newline="")) if "edit_align_kernel" in r.get("Kernel_Name", "")), key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[-len(order) * TRACE_CALLS:]
    assert len(rows) == len(order) * TRACE_CALLS, len(rows)
    out = {}
    for i, (name, ops) in enumerate(order):
        mine = rows[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]
        assert all(("<true>" in r["Kernel_Name"] or "ILb1" in r["Kernel_Name"]) == ops for r in mine), (name, ops, mine[0]["Kernel_Name"])
        out[f"{name}_{'ops' if ops else 'counts'}"] = round(statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-csv", default="")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    cases = make_cases()
    names = ("batch", "nbest", "long", "lds", "ws")
    launches = {n: Launch(cases[n]) for n in names}
    order = [(n, ops) for n in names for ops in (True, False)]
    for n, ops in order:      # warm: code objects, the allocator, the LDS attribute
        launches[n](ops)
    torch.cuda.synchronize()
    if a.trace_run:
        for n, ops in order:
            for _ in range(TRACE_CALLS):
                launches[n](ops)
        torch.cuda.synchronize()
        return
    med = lambda v: round(statistics.median(v), 4)      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "expected_before_measuring": EXPECTED,
           "protocol": f"contenders alternated in one process, {a.rounds} rounds, medians; *_ms are host wall times of whole calls between two synchronisations, "
                       "launch_event_ms are device events around the wrapper call (outputs and workspace allocated before; the host's checks lie between them)",
           "lds_dir_bytes": K.EDIT_LDS_DIR_BYTES,
           "workspace_bytes": {n: K.edit_align_workspace_bytes(launches[n].hl, launches[n].rl, launches[n].ro, launches[n].hyp.shape[1], launches[n].ref.shape[1])
                               for n in names}}
    t = {}
    for _ in range(a.rounds):
        for n in names:
            c = cases[n]
            for ops in (True, False):
                ms, got = wall(lambda: align_ids(c["hyps"], c["refs"], ref_of=c["ref_of"], ops=ops, device=DEV))
                t.setdefault(f"{n}_align_ids_{'ops' if ops else 'counts'}_ms", []).append(ms)
                t.setdefault(f"{n}_launch_event_{'ops' if ops else 'counts'}_ms", []).append(launches[n].event_ms(ops))
            py = cases["py_2000"] if n == "long" else c
            t0 = time.perf_counter()
            want = python_dp(py)
            t.setdefault(f"{n if n != 'long' else 'py_2000'}_python_dp_ms", []).append((time.perf_counter() - t0) * 1e3)
            if n != "long":
                assert [g["distance"] for g in got] == want, n
    res["timings"] = {k: {"median": med(v), "rounds": [round(x, 4) for x in v]} for k, v in t.items()}
    m = {k: v["median"] for k, v in res["timings"].items()}
    scale = (15000 * 15000) / (2000 * 2000)
    m["long_python_dp_ms"] = round(m["py_2000_python_dp_ms"] * scale, 1)
    res["long_python_dp_note"] = f"extrapolated from the 2000 x 2000 pair by the cell count (x {scale})"
    res["python_dp_over_align_ids"] = {n: {mode: round(m[f"{n}_python_dp_ms"] / m[f"{n}_align_ids_{mode}_ms"], 2) for mode in ("ops", "counts")} for n in names}
    if a.kernels_csv:
        k = res["kernels_us"] = kernel_durations(a.kernels_csv, order)
        # what the mask stores and the backtrace add over a forward pass that carries the counts instead, as a share of the ops kernel
        res["ops_minus_counts_share_of_ops_kernel"] = {n: round((k[f"{n}_ops"] - k[f"{n}_counts"]) / k[f"{n}_ops"], 3) for n in names}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
