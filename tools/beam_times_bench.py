"""Cost of token times in the CTC prefix beam search (asr_ctc_prefix_beam_timed / asr_ctc_prefix_beam_chunk_timed beside the plain entry
points), at the serving shape: beam 5, k = 10, V = 4232, random logits.

  offline:  B = 32 utterances x 500 frames in one launch
  streamed: the chunk kernel at C = 16 over 496 frames (31 calls), for B = 1 and B = 32

The plain and the timed kernels are alternated in one process over three rounds; a figure is the median round, each round the mean of
`--reps` back-to-back calls between two synchronisations (host wall time of a queue that never runs dry, so close to kernel time).
The last line is one JSON object (profiles/beam_times_bench.json): the figures, the timed / plain ratios and the tries' footprint.
--trace-only runs both contenders a few times and prints nothing: the run to wrap in `rocprofv3 --kernel-trace` for the kernels' own
durations; --summarise KERNEL_TRACE_CSV then prints them per contender as JSON (the two are told apart by their kernel names)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from asr_chinese_e2e_amd import kernels as K  # noqa: E402
from asr_chinese_e2e_amd._lib import lib  # noqa: E402

V, BEAM, TOPK, T, C = 4232, 5, 10, 500, 16
NAMES = ("plain", "timed")
TRACE_CALLS = 3      # calls of every contender in a --trace-only run


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def is_timed(kernel_name):
    """The TIMES instantiation, by its template arguments in either spelling of the trace."""
    return "true>" in kernel_name or "ELb1E" in kernel_name


def summarise(path):
    """Median kernel duration (us) per contender from the kernel trace of a --trace-only run."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = {"ctc_prefix_beam_kernel": [], "ctc_prefix_beam_chunk_kernel": []}
    for r in rows:
        for name in dur:
            if name + "<" in r["Kernel_Name"] or name + "I" in r["Kernel_Name"]:
                dur[name].append(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, is_timed(r["Kernel_Name"])))
    out = {}
    off = dur["ctc_prefix_beam_kernel"]
    out["offline_B32_T500_kernel_us"] = {n: round(statistics.median(d for d, t in off if t == (n == "timed")), 1) for n in NAMES}
    per = TRACE_CALLS * (T // C) * len(NAMES)
    ch = dur["ctc_prefix_beam_chunk_kernel"]
    assert len(ch) == 2 * per, (len(ch), per)
    for j, Bs in enumerate((1, 32)):      # the B = 1 streams run first
        part = ch[j * per:(j + 1) * per]
        out[f"stream_C16_T496_B{Bs}_kernel_us_per_chunk"] = {n: round(statistics.median(d for d, t in part if t == (n == "timed")), 1) for n in NAMES}
    for v in out.values():
        v["timed_over_plain"] = round(v["timed"] / v["plain"], 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--summarise", default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    gen = torch.Generator().manual_seed(0)
    cases = {}
    # ---- offline
    B = 32
    logits = (torch.randn(B * T, V, generator=gen) * 3.0).cuda()
    vals, ids, blank_lp = K.ctc_frame_topk(logits, TOPK, 0)
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    cases["offline_B32_T500_ms"] = {n: (lambda times=(n == "timed"): K.ctc_prefix_beam(vals, ids, blank_lp, lens, B, T, BEAM, BEAM, 0, times=times)) for n in NAMES}
    # ---- streamed: 31 chunks of 16 frames through a fresh state
    n_chunks = T // C
    for Bs in (1, 32):
        chunks = [tuple(x.view(Bs, T, -1)[:, i * C:(i + 1) * C].reshape(Bs * C, -1).contiguous() for x in (vals[:Bs * T], ids[:Bs * T], blank_lp[:Bs * T, None]))
                  for i in range(n_chunks)]
        chunks = [(v, i, b.reshape(-1)) for v, i, b in chunks]
        nv = [C] * Bs
        nv_dev = torch.tensor(nv, dtype=torch.int32, device="cuda")

        def stream(times, Bs=Bs, chunks=chunks, nv=nv, nv_dev=nv_dev):
            st = K.ctc_prefix_beam_state(Bs, BEAM, T, "cuda", times=times)
            for v, i, b in chunks:
                K.ctc_prefix_beam_chunk(st, v, i, b, nv, C, BEAM, 0, packed=True, nv_dev=nv_dev)
        cases[f"stream_C16_T496_B{Bs}_ms_per_chunk"] = {n: (lambda times=(n == "timed"), stream=stream: stream(times)) for n in NAMES}
    if args.trace_only:
        for runs in cases.values():
            for fn in runs.values():
                for _ in range(TRACE_CALLS):
                    fn()
        torch.cuda.synchronize()
        return
    from asr_chinese_e2e_amd.Models.transformer_official import PE_MAXLEN as pe_rows      # a stream's tries hold the positional table's frames
    out = {"device": torch.cuda.get_device_name(0), "shape": {"V": V, "beam": BEAM, "k": TOPK, "T": T, "C": C},
           "protocol": f"contenders alternated in one process, {args.rounds} rounds, median round; a round = mean of {args.reps} back-to-back calls",
           "trie_bytes_per_utterance": {f"T_cap={tc}_beam={bm}": {"plain": lib.asr_ctc_prefix_beam_workspace_bytes(1, tc, bm),
                                                                  "timed": lib.asr_ctc_prefix_beam_timed_workspace_bytes(1, tc, bm)}
                                        for tc, bm in ((T, BEAM), (pe_rows, BEAM), (pe_rows, 16))}}
    for case, runs in cases.items():
        rounds = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                rounds[k].append(timed(fn, args.reps))
        div = n_chunks if case.startswith("stream") else 1
        out[case] = {k: {"median_ms": round(statistics.median(v) / div, 4), "rounds_ms": [round(x / div, 4) for x in v]} for k, v in rounds.items()}
        out[case]["timed_over_plain"] = round(out[case]["timed"]["median_ms"] / out[case]["plain"]["median_ms"], 3)
        print(f"{case:36s} plain {out[case]['plain']['median_ms']:9.4f} ms   timed {out[case]['timed']['median_ms']:9.4f} ms   (x{out[case]['timed_over_plain']:.3f})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
