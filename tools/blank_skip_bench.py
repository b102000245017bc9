"""Cost and gain of blank-frame skipping (asr_ctc_blank_skip_compact in front of asr_ctc_prefix_beam / asr_ctc_prefix_beam_chunk), at the
serving shape: beam 5, k = 10, V = 4232, on synthetic peaky logits.

  offline:  B = 32 utterances x 500 frames: compaction + search in one call each
  streamed: compaction + chunk kernel at C = 16 over 496 frames (31 calls), for B = 1 and B = 32

Contenders: the plain search, and blank_skip = 0.98 on logits built so that about 0 %, 50 % and 80 % of the frames are dropped (blank runs
whose posterior is above 0.99; the 0 % row is the feature's overhead: every frame is looked at, none goes).  Every contender runs on its
own logits - also the plain search, once per logit set, so that each skip row has its own baseline ("plain_50" beside "skip_50").  The
contenders are alternated in one process over three rounds; a figure is the median round, each round the mean of `--reps` back-to-back
calls between two synchronisations (host wall time of a queue that never runs dry: the end-to-end host time of compaction + search).
Per logit set the kept-frame share is recorded, and the share of utterances whose best string with blank_skip differs from the plain
search's: an accuracy side effect on synthetic data, reported, not asserted.  The last line is one JSON object
(profiles/blank_skip_bench.json).  --trace-only runs every contender a few times and prints nothing: the run to wrap in `rocprofv3
--kernel-trace` for the kernels' own durations; --summarise KERNEL_TRACE_CSV then prints them per contender as JSON (the trace-only run
launches the contenders in a fixed order, three calls each; they are told apart by that order)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from asr_chinese_e2e_amd import kernels as K  # noqa: E402

V, BEAM, TOPK, T, C = 4232, 5, 10, 500, 16
P = 0.98
SHARES = (0, 50, 80)      # per cent of the frames that blank_skip drops


def peaky(B, share, seed):
    """Logits (B * T, V): speech segments of 1 - 6 contested frames between blank runs (p(blank) > 0.99) whose lengths are drawn so that
    about `share` per cent of the frames are dropped (every frame of a run but its head); share 0: single blank frames only."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * 1.5).astype(np.float32)
    mean_run = {0: 1.0, 50: 5.0, 80: 17.0}[share]      # dropped share = (run - 1) / (run + mean speech segment of 3.5)
    for b in range(B):
        t = 0
        while t < T:
            rows = np.arange(t, min(T, t + int(rng.integers(1, 7))))
            x[b, rows, rng.integers(4, V, len(rows))] += 9.0      # a leading token per speech frame, contested by the tail of 4232 classes
            t = int(rows[-1]) + 1
            run = 1 if share == 0 else max(1, int(rng.geometric(1.0 / mean_run)))
            x[b, t:t + run, 0] += 20.0
            t += run
    return torch.from_numpy(x.reshape(B * T, V)).cuda()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


TRACE_CALLS = 3      # calls of every contender in a --trace-only run


def contenders():
    return [f"{kind}_{s}" for s in SHARES for kind in ("plain", "skip")]


def summarise(path):
    """Median kernel durations (us) per contender from the kernel trace of a --trace-only run: the search kernel's, and for the skip rows the
    compaction kernel's alone."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = {"ctc_prefix_beam_kernel": [], "ctc_prefix_beam_chunk_kernel": [], "blank_skip_compact_kernel": []}
    for r in rows:
        for name in dur:
            if name in r["Kernel_Name"]:
                dur[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    names, skips = contenders(), [n for n in contenders() if n.startswith("skip")]
    med = lambda xs: round(statistics.median(xs), 1)      # noqa: E731
    out = {}
    n_chunks = T // C
    off = dur["ctc_prefix_beam_kernel"][-TRACE_CALLS * len(names):]      # the launches before them belong to the accuracy comparison
    comp = dur["blank_skip_compact_kernel"]
    n_off, per = TRACE_CALLS * len(skips), TRACE_CALLS * n_chunks
    assert len(comp) >= n_off + 2 * per * len(skips) and len(dur["ctc_prefix_beam_chunk_kernel"]) == 2 * per * len(names), (len(comp), len(dur["ctc_prefix_beam_chunk_kernel"]))
    comp = comp[-(n_off + 2 * per * len(skips)):]
    out["offline_B32_T500_search_kernel_us"] = {n: med(off[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]) for i, n in enumerate(names)}
    out["offline_B32_T500_compact_kernel_us"] = {n: med(comp[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]) for i, n in enumerate(skips)}
    for j, Bs in enumerate((1, 32)):
        ch = dur["ctc_prefix_beam_chunk_kernel"][j * per * len(names):(j + 1) * per * len(names)]
        cc = comp[n_off + j * per * len(skips):n_off + (j + 1) * per * len(skips)]
        out[f"stream_C16_T496_B{Bs}_search_kernel_us_per_chunk"] = {n: med(ch[i * per:(i + 1) * per]) for i, n in enumerate(names)}
        out[f"stream_C16_T496_B{Bs}_compact_kernel_us_per_chunk"] = {n: med(cc[i * per:(i + 1) * per]) for i, n in enumerate(skips)}
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
    thr = K.blank_skip_threshold(P)
    B = 32
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    cand, info = {}, {}
    for s in SHARES:
        vals, ids, blank_lp = K.ctc_frame_topk(peaky(B, s, seed=s), TOPK, 0)
        cand[s] = (vals, ids, blank_lp)
        # the kept share, and how often the best string changes (synthetic data: reported, not asserted)
        cv, ci, cb, n_kept, _ = K.ctc_blank_skip_compact(vals, ids, blank_lp, lens, thr, B, T)
        tok, ln, _ = (x.cpu() for x in K.ctc_prefix_beam(vals, ids, blank_lp, lens, B, T, BEAM, 1, 0))
        tok2, ln2, _ = (x.cpu() for x in K.ctc_prefix_beam(cv, ci, cb, n_kept, B, T, BEAM, 1, 0))
        differ = sum(tok[b, 0, :max(int(ln[b, 0]), 0)].tolist() != tok2[b, 0, :max(int(ln2[b, 0]), 0)].tolist() for b in range(B))
        info[f"skip_{s}"] = {"kept_frame_share": round(float(n_kept.sum()) / (B * T), 4), "best_string_differs_share": round(differ / B, 4),
                             "mean_best_length": round(float(ln[:, 0].float().mean()), 1)}
    cases = {}
    # ---- offline
    off = {}
    for s in SHARES:
        v, i, b = cand[s]
        off[f"plain_{s}"] = lambda v=v, i=i, b=b: K.ctc_prefix_beam(v, i, b, lens, B, T, BEAM, BEAM, 0)

        def skip(v=v, i=i, b=b):
            cv, ci, cb, n, _ = K.ctc_blank_skip_compact(v, i, b, lens, thr, B, T)
            return K.ctc_prefix_beam(cv, ci, cb, n, B, T, BEAM, BEAM, 0)
        off[f"skip_{s}"] = skip
    cases["offline_B32_T500_ms"] = off
    # ---- streamed: 31 chunks of 16 frames through a fresh state
    n_chunks = T // C
    for Bs in (1, 32):
        runs = {}
        for s in SHARES:
            vals, ids, blank_lp = cand[s]
            chunks = [tuple(x.view(B, T, -1)[:Bs, j * C:(j + 1) * C].reshape(Bs * C, -1).contiguous() for x in (vals, ids, blank_lp[:, None])) for j in range(n_chunks)]
            chunks = [(v, i, b.reshape(-1)) for v, i, b in chunks]
            nv = [C] * Bs
            nv_dev = torch.tensor(nv, dtype=torch.int32, device="cuda")

            def stream(skip, Bs=Bs, chunks=chunks, nv=nv, nv_dev=nv_dev):
                st = K.ctc_prefix_beam_state(Bs, BEAM, T, "cuda")
                sk = K.BlankSkipState(Bs, T, "cuda") if skip else None
                for v, i, b in chunks:
                    n = nv_dev
                    if skip:
                        v, i, b, n, _ = K.ctc_blank_skip_compact(v, i, b, nv_dev, thr, Bs, C, sk)
                    K.ctc_prefix_beam_chunk(st, v, i, b, nv, C, BEAM, 0, packed=True, nv_dev=n)
            runs[f"plain_{s}"] = lambda stream=stream: stream(False)
            runs[f"skip_{s}"] = lambda stream=stream: stream(True)
        cases[f"stream_C16_T496_B{Bs}_ms_per_chunk"] = runs
    if args.trace_only:
        for runs in cases.values():
            for fn in runs.values():
                for _ in range(TRACE_CALLS):
                    fn()
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "shape": {"V": V, "beam": BEAM, "k": TOPK, "T": T, "C": C, "blank_skip": P, "thr": thr},
           "logits": info,
           "protocol": f"contenders alternated in one process, {args.rounds} rounds, median round; a round = mean of {args.reps} back-to-back calls; "
                       "plain_N = the plain search on the logits of skip_N"}
    for case, runs in cases.items():
        rounds = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                rounds[k].append(timed(fn, args.reps))
        div = n_chunks if case.startswith("stream") else 1
        out[case] = {k: {"median_ms": round(statistics.median(v) / div, 4), "rounds_ms": [round(x / div, 4) for x in v]} for k, v in rounds.items()}
        for k, v in out[case].items():
            base = out[case]["plain_" + k.split("_")[1]]["median_ms"]
            print(f"{case:36s} {k:10s} {v['median_ms']:9.4f} ms   (x{v['median_ms'] / base:.3f} of its plain)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
