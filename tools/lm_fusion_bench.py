"""Cost of n-gram LM shallow fusion in the CTC prefix beam search (asr_ctc_prefix_beam_lm / asr_ctc_prefix_beam_chunk_lm beside the plain
entry points), at the serving shape: beam 5, k = 10, V = 4232, random logits.

  offline:  B = 32 utterances x 500 frames in one launch
  streamed: the chunk kernel at C = 16 over 496 frames (31 calls), for B = 1 and B = 32

Contenders: the plain search, and the search with random order-3 LMs of about 1e4, 1e5 and 1e6 n-grams (weight 0.3; every token has a
unigram, bigrams extend unigrams and trigrams extend listed bigrams, as a toolkit's file would have them), and the 1e5 one once more
with weight 0: every lookup of the LM kernel on exactly the plain search's beam, so that its time against the plain kernel's is the cost
of the fusion alone (with a weight the beam holds other, on random logits shorter, strings, and spelling them costs less).  On random logits most
extensions miss their context's arcs, so a slot typically pays one or two binary searches, the back-off terms and the indexed unigram
load: close to the longest chain an order-3 model has.  The contenders are alternated in one process over three rounds; a figure is the
median round, each round the mean of `--reps` back-to-back calls between two synchronisations (host wall time of a queue that never
runs dry, so close to kernel time).  The last line is one JSON object (profiles/lm_fusion_bench.json).  --trace-only runs every contender
a few times and prints nothing: the run to wrap in `rocprofv3 --kernel-trace` for the kernels' own durations; --summarise
KERNEL_TRACE_CSV then prints them per contender as JSON (the trace-only run launches the contenders in a fixed order, three calls each,
and the contenders of one kernel are told apart by that order).  --lm-cache DIR keeps the compiled tables (NgramLM.save) between runs:
compiling a million n-grams in Python takes about a minute."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from asr_chinese_e2e_amd import kernels as K  # noqa: E402
from asr_chinese_e2e_amd.lm import NgramLM  # noqa: E402

V, BEAM, TOPK, T, C = 4232, 5, 10, 500, 16
SIZES = (10 ** 4, 10 ** 5, 10 ** 6)
WEIGHT = 0.3


W0 = 10 ** 5      # the size that also runs with weight 0: every lookup of the LM kernel on exactly the plain search's beam


def names():
    return [f"lm_{n}" for n in SIZES] + [f"lm_{W0}_w0"]


def model(n, cache=None, seed=0, device="cuda", weight=WEIGHT):
    """A random order-3 LM of about n n-grams: V - 2 unigrams, the rest 40 % bigrams and 60 % trigrams."""
    path = os.path.join(cache, f"lm_{n}_w{weight}.npz") if cache else None
    if path and os.path.isfile(path):
        return NgramLM.load(path, device=device)
    rng = random.Random(seed)
    table = {(c,): (-1.0 - 3.0 * rng.random(), -rng.random()) for c in range(2, V)}
    rest = max(0, n - len(table))
    bigrams = []
    while len(bigrams) < int(0.4 * rest):
        g = (rng.randrange(2, V), rng.randrange(3, V))
        if g[0] != 3 and g not in table:
            table[g] = (-0.2 - 3.0 * rng.random(), -rng.random())
            bigrams.append(g)
    left = rest - len(bigrams)
    while left > 0 and bigrams:
        g = bigrams[rng.randrange(len(bigrams))] + (rng.randrange(3, V),)
        if g[1] != 3 and g not in table:
            table[g] = (-0.1 - 2.0 * rng.random(), None)
            left -= 1
    lm = NgramLM(table, 3, V, weight=weight, device=device)
    if path:
        os.makedirs(cache, exist_ok=True)
        lm.save(path)
    return lm


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


TRACE_CALLS = 3      # calls of every contender in a --trace-only run


def summarise(path):
    """Median kernel duration (us) per contender from the kernel trace of a --trace-only run."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = {"ctc_prefix_beam_kernel": [], "ctc_prefix_beam_chunk_kernel": []}
    for r in rows:
        for name in dur:
            if name + "<" in r["Kernel_Name"]:
                dur[name].append(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3, "<2>" in r["Kernel_Name"] or "ILi2E" in r["Kernel_Name"]))
    names = ["plain"] + globals()["names"]()
    out = {}
    off = dur["ctc_prefix_beam_kernel"][-TRACE_CALLS * len(names):]      # the launches before them belong to nothing timed here
    out["offline_B32_T500_kernel_us"] = {n: round(statistics.median(d for d, _ in off[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]), 1) for i, n in enumerate(names)}
    per = TRACE_CALLS * (T // C)
    ch = dur["ctc_prefix_beam_chunk_kernel"]
    assert len(ch) == 2 * per * len(names), (len(ch), per)
    for j, Bs in enumerate((1, 32)):
        part = ch[j * per * len(names):(j + 1) * per * len(names)]
        assert all(c == (i >= per) for i, (_, c) in enumerate(part)), "the plain contender comes first"
        out[f"stream_C16_T496_B{Bs}_kernel_us_per_chunk"] = {n: round(statistics.median(d for d, _ in part[i * per:(i + 1) * per]), 1) for i, n in enumerate(names)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--lm-cache", default=None)
    ap.add_argument("--build-only", action="store_true", help="compile the LMs into --lm-cache and stop")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    dev = None if args.build_only else "cuda"      # --build-only needs no GPU
    graphs = {f"lm_{n}": model(n, args.lm_cache, device=dev) for n in SIZES}
    graphs[f"lm_{W0}_w0"] = model(W0, args.lm_cache, device=dev, weight=0.0)
    if args.build_only:
        return
    tables = {name: {"ngrams": g.n_ngrams, "states": g.S, "arcs": g.A} for name, g in graphs.items()}
    gen = torch.Generator().manual_seed(0)
    cases = {}
    # ---- offline
    B = 32
    logits = (torch.randn(B * T, V, generator=gen) * 3.0).cuda()
    vals, ids, blank_lp = K.ctc_frame_topk(logits, TOPK, 0)
    lens = torch.full((B,), T, dtype=torch.int32, device="cuda")
    off = {"plain": lambda: K.ctc_prefix_beam(vals, ids, blank_lp, lens, B, T, BEAM, BEAM, 0)}
    for name, g in graphs.items():
        off[name] = lambda g=g: K.ctc_prefix_beam(vals, ids, blank_lp, lens, B, T, BEAM, BEAM, 0, lm=g)
    cases["offline_B32_T500_ms"] = off
    # ---- streamed: 31 chunks of 16 frames through a fresh state
    n_chunks = (T // C)
    for Bs in (1, 32):
        chunks = [tuple(x.view(Bs, T, -1)[:, i * C:(i + 1) * C].reshape(Bs * C, -1).contiguous() for x in (vals[:Bs * T], ids[:Bs * T], blank_lp[:Bs * T, None]))
                  for i in range(n_chunks)]
        chunks = [(v, i, b.reshape(-1)) for v, i, b in chunks]
        nv = [C] * Bs
        nv_dev = torch.tensor(nv, dtype=torch.int32, device="cuda")

        def stream(g=None, Bs=Bs, chunks=chunks, nv=nv, nv_dev=nv_dev):
            st = K.ctc_prefix_beam_state(Bs, BEAM, T, "cuda", lm=g)
            for v, i, b in chunks:
                K.ctc_prefix_beam_chunk(st, v, i, b, nv, C, BEAM, 0, packed=True, nv_dev=nv_dev)
        runs = {"plain": stream}
        for name, g in graphs.items():
            runs[name] = lambda g=g, stream=stream: stream(g)
        cases[f"stream_C16_T496_B{Bs}_ms_per_chunk"] = runs
    if args.trace_only:
        for runs in cases.values():
            for fn in runs.values():
                for _ in range(TRACE_CALLS):
                    fn()
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "shape": {"V": V, "beam": BEAM, "k": TOPK, "T": T, "C": C, "order": 3, "weight": WEIGHT}, "tables": tables,
           "protocol": f"contenders alternated in one process, {args.rounds} rounds, median round; a round = mean of {args.reps} back-to-back calls"}
    for case, runs in cases.items():
        rounds = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                rounds[k].append(timed(fn, args.reps))
        div = n_chunks if case.startswith("stream") else 1
        out[case] = {k: {"median_ms": round(statistics.median(v) / div, 4), "rounds_ms": [round(x / div, 4) for x in v]} for k, v in rounds.items()}
        for k, v in out[case].items():
            print(f"{case:36s} {k:10s} {v['median_ms']:9.4f} ms   (x{v['median_ms'] / out[case]['plain']['median_ms']:.3f} of plain)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
