#!/usr/bin/env python3
"""Independent sessions: what one tick that serves 32 live callers costs, against the two ways to serve them without
model.sessions.  One JSON object on stdout (and in --out).

  python tools/sessions_bench.py [--rounds 3] [--out profiles/sessions_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/sessions_bench.py --trace-run      # a short sessions-only run, to be started under rocprofv3 --kernel-trace

The production shape of tools/stream_frontend_bench.py: C = 16, LFR 4/3, 80 mel bins, blocks of 480 ms (7680 samples), the 6-layer
bf16 joint model with a 320-wide input, 32 slots, utterances of 31 blocks.  Three contenders alternate in one process, --rounds times:
* sessions:   model.sessions(32).push_audio of one block per open slot; the slots open staggered (slot b at tick b mod 8);
* solo_x32:   32 model.stream(1) objects, push_audio called on each in turn: 32 independent callers served one by one;
* lockstep:   model.stream(32).push_audio of the block (every caller starts at the same tick and never leaves).
Host wall time per tick (a push returns ids, so it synchronises), ticks in which all 32 callers are live and past their first block.
--kernels-csv: the durations of the sessions' own kernels, read from the kernel trace of a --trace-run under the profiler.
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

DEV = "cuda"
C, LFR_M, LFR_N, N_MELS, BLOCKS, SLOTS, STAGGER = 16, 4, 3, 80, 31, 32, 8
# (asr_add_ln_slots_fwd launches add_ln_fwd_kernel itself, which the trace cannot tell from the layers' LayerNorm launches)
NEW_KERNELS = ("slot_rows_put_kernel", "slot_rows_slide_kernel", "frame_best_blank_kernel", "session_ctc_step_kernel", "ctc_prefix_beam_state_reset_kernel")


def build():
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, dropout=0.0, layer_num=6, ctc_weight=0.3, dtype="bf16", chunk_size=C))
    torch.manual_seed(0)
    model = M(cfg, Vocab.synthetic(4232)).to(DEV).eval()
    parser = AudioParser(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, device=DEV, norm="global", cmvn=(np.full(N_MELS, -1.0), np.full(N_MELS, 0.4)))
    return model, parser


def tick_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def run_sessions(model, parser, blocks, ticks):
    """-> ms of the ticks in which every slot is open and past its first block."""
    ss = model.sessions(SLOTS, parser=parser)
    block = blocks[0].shape[1]
    fed, out = [0] * SLOTS, []
    for tick in range(ticks):
        for b in range(SLOTS):
            if tick == b % STAGGER:
                ss.open(b)
        live = [ss.state[b] == "open" and fed[b] < BLOCKS for b in range(SLOTS)]
        ns = [block if l else 0 for l in live]
        fin = [l and fed[b] == BLOCKS - 1 for b, l in enumerate(live)]
        ms = tick_ms(lambda: ss.push_audio(blocks[tick % BLOCKS], ns, fin))
        if all(live) and min(fed) >= 1:
            out.append(ms)
        fed = [f + int(l) for f, l in zip(fed, live)]
    return out


def run_solo(model, parser, blocks):
    sts = [model.stream(1, parser=parser) for _ in range(SLOTS)]
    block = blocks[0].shape[1]
    rows = [[x[b:b + 1].contiguous() for b in range(SLOTS)] for x in blocks]
    out = []
    for k in range(BLOCKS):
        def serve():
            for b, st in enumerate(sts):
                st.push_audio(rows[k][b], [block], [False])
        out.append(tick_ms(serve))
    return out[1:]


def run_lockstep(model, parser, blocks):
    st = model.stream(SLOTS, parser=parser)
    block = blocks[0].shape[1]
    out = [tick_ms(lambda: st.push_audio(x, [block] * SLOTS, [False] * SLOTS)) for x in blocks]
    return out[1:]


def kernel_durations(path):
    """name -> {launches, median_us, total_us} of the sessions' kernels in a rocprofv3 kernel-trace CSV."""
    rec = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            for k in NEW_KERNELS:
                if k in name:
                    rec.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "median_us": round(statistics.median(v), 2), "total_us": round(sum(v), 1)} for k, v in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-csv", default="")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    model, parser = build()
    block = C * LFR_N * 160
    wav = torch.randn(SLOTS, block * BLOCKS, device=DEV) * 0.1
    blocks = [wav[:, k * block:(k + 1) * block].contiguous() for k in range(BLOCKS)]
    if a.trace_run:
        run_sessions(model, parser, blocks, STAGGER + 12)
        torch.cuda.synchronize()
        return
    med = lambda v: round(statistics.median(v), 3)      # noqa: E731
    run_sessions(model, parser, blocks, BLOCKS)      # warm every cache size, the allocator and the engine
    run_solo(model, parser, blocks)
    run_lockstep(model, parser, blocks)
    rounds = []
    for _ in range(a.rounds):
        s, o, l = run_sessions(model, parser, blocks, BLOCKS), run_solo(model, parser, blocks), run_lockstep(model, parser, blocks)
        rounds.append({"sessions_tick_ms": med(s), "sessions_tick_max_ms": round(max(s), 3), "solo_x32_tick_ms": med(o), "lockstep_tick_ms": med(l),
                       "ticks": [len(s), len(o), len(l)]})
    res = {"device": torch.cuda.get_device_name(0), "C": C, "lfr": [LFR_M, LFR_N], "n_mels": N_MELS, "block_samples": block, "block_audio_ms": block / 16.0,
           "slots": SLOTS, "stagger_ticks": STAGGER, "rounds": rounds,
           "median_of_rounds": {k: med([r[k] for r in rounds]) for k in ("sessions_tick_ms", "solo_x32_tick_ms", "lockstep_tick_ms")}}
    m = res["median_of_rounds"]
    res["sessions_over_lockstep"] = round(m["sessions_tick_ms"] / m["lockstep_tick_ms"], 3)
    res["solo_x32_over_sessions"] = round(m["solo_x32_tick_ms"] / m["sessions_tick_ms"], 2)
    if a.kernels_csv:
        res["kernels"] = kernel_durations(a.kernels_csv)
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
