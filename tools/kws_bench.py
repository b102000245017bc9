#!/usr/bin/env python3
"""What keyword spotting costs: the offline search beside asr_ctc_frame_stats on the same rows, and the sessions tick with and without
keywords=.  One JSON object on stdout (and in --out: profiles/kws_bench.json).

  python tools/kws_bench.py [--rounds 3] [--reps 5] [--out profiles/kws_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/kws_bench.py --trace-run      # a short offline-only run, to be started under rocprofv3 --kernel-trace

Offline: B = 32 utterances x 500 frames, V = 4232, bf16 rows, peaky synthetic logits; K = 1, 64 and 1000 keywords of 2 to 6 characters.
Contenders (alternated in one process, --rounds rounds, the median round; a round = the mean of --reps back-to-back calls between two
synchronisations): frame_stats alone, and asr_kws_search + asr_kws_compact at each K over a precomputed lse; and, to see what the gathers
from the 4232-wide rows cost, the K = 1000 search alone beside the same search over keywords of the same lengths that all spell one
token (every lane of a load then reads the same address).
Sessions: tools/sessions_bench.py's shape (32 slots, C = 16, the 6-layer bf16 joint model, V = 4232) - the tick without keywords, and
with a list of K = 64 and of K = 1000; host wall time of the ticks in which every slot is live, alternated in the same way.
--kernels-csv: the kernels' own durations from the trace of a --trace-run (three calls of frame_stats, search, compact per K, in a
fixed order).

Expected, written down before the first run (none of this had been timed):
  * frame_stats streams 135 MB of bf16 rows in two passes: 50 - 80 us at a few TB/s.
  * The search is a serial chain of 500 frames per wave and waits for memory once per group of frames (8 / 4 frames in the L <= 4 / 8
    buckets): ~1.5 us per group gives 100 - 200 us whatever K is, plus the selects (7 - 15 states x ~8 instructions per frame) and the
    gathers (every load instruction of a wave touches up to 64 cache lines of a 4232-wide row).  K = 1 and K = 64 are one wave per
    utterance on 32 of 256 CUs: ~150 us and ~300 us (K = 64 runs in the L <= 8 bucket).  K = 1000 is 16 waves per utterance, two per CU:
    about the same latency, up to twice the gather cost - 300 - 500 us.  So the search should cost a few times frame_stats while doing
    far fewer operations: it is latency-bound, not bandwidth-bound.
  * The tick: 16 frames per slot are 2 - 4 groups, ~10 us of search kernel, a few us of compaction, one more copy (~20 us) and the host
    side of three launches and the list's checks: +0.1 - 0.2 ms per tick at K = 64 (a few per cent of a tick of several ms), +0.2 - 0.3 ms
    at K = 1000, where the state (8.8 MB) is read and written every tick.
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
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from asr_chinese_e2e_amd import kernels as K  # noqa: E402
from asr_chinese_e2e_amd.keywords import KeywordList  # noqa: E402

DEV = "cuda"
B, T, V = 32, 500, 4232
KS = (1, 64, 1000)
TRACE_CALLS = 3
EXPECTED = {"frame_stats_us": "50 - 80", "search_kernel_us": {"K1": "~150", "K64": "~300", "K1000": "300 - 500"},
            "sessions_tick_extra_ms": {"K64": "0.1 - 0.2", "K1000": "0.2 - 0.3"}}
FRAME_SECONDS = 0.03


def keyword_list(n, seed=1):
    rng = np.random.default_rng(seed)
    return KeywordList([[int(x) for x in rng.integers(4, V, 2 + k % 5)] for k in range(n)], threshold=0.5, vocab_size=V)


def peaky(seed=0):
    """Logits (B, T, V) bf16: runs of 1 - 3 frames on one class between blank runs, contested by the tail of 4232 classes."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V)) * 1.5).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(1, 4))
            x[b, t:t + n, int(rng.integers(4, V))] += 9.0
            t += n
            n = int(rng.integers(1, 6))
            x[b, t:t + n, 0] += 12.0
            t += n
    return torch.from_numpy(x).to(DEV).bfloat16()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def offline_cases():
    logits = peaky()
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    lse = K.ctc_frame_stats(logits, lens, 0)[3]
    cases = {"frame_stats": lambda: K.ctc_frame_stats(logits, lens, 0)}
    for n in KS:
        kl = keyword_list(n)
        tabs = kl.on(DEV, FRAME_SECONDS)

        def search(kl=kl, tabs=tabs):
            cnt, rec = K.kws_search(logits, lse, lens, tabs, kl.K, kl.hits_per_keyword)
            return K.kws_compact(cnt, rec, kl.max_hits)
        cases[f"search_K{n}"] = search
    # the diagnostic for the gathers' share: the same lengths, every character the same id - all 64 lanes of a load read one address
    same = KeywordList([[7] * (2 + k % 5) for k in range(KS[-1])], threshold=0.5, vocab_size=V)
    tabs_same = same.on(DEV, FRAME_SECONDS)
    cases[f"search_K{KS[-1]}_one_token"] = lambda: K.kws_search(logits, lse, lens, tabs_same, same.K, same.hits_per_keyword)
    cases[f"search_K{KS[-1]}_no_compact"] = lambda kl=kl, tabs=tabs: K.kws_search(logits, lse, lens, tabs, kl.K, kl.hits_per_keyword)
    return cases


def run_sessions(sb, model, parser, blocks, ticks, keywords):
    """tools/sessions_bench.py's run_sessions with keywords= -> ms of the ticks in which every slot is open and past its first block."""
    ss = model.sessions(sb.SLOTS, parser=parser, keywords=keywords)
    block = blocks[0].shape[1]
    fed, out = [0] * sb.SLOTS, []
    for tick in range(ticks):
        for b in range(sb.SLOTS):
            if tick == b % sb.STAGGER:
                ss.open(b)
        live = [ss.state[b] == "open" and fed[b] < sb.BLOCKS for b in range(sb.SLOTS)]
        ns = [block if l else 0 for l in live]
        fin = [l and fed[b] == sb.BLOCKS - 1 for b, l in enumerate(live)]
        ms = sb.tick_ms(lambda: ss.push_audio(blocks[tick % sb.BLOCKS], ns, fin))
        if all(live) and min(fed) >= 1:
            out.append(ms)
        fed = [f + int(l) for f, l in zip(fed, live)]
    return out


def kernel_durations(path):
    """Per K the median over the trace run's calls of: frame_stats, the search launches summed, the compaction (us)."""
    rows = sorted(csv.DictReader(open(path, newline="")), key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        name = r.get("Kernel_Name", "")
        if "frame_stats_kernel" in name:
            calls.append({"frame_stats_us": us, "search_us": 0.0, "search_launches": 0, "compact_us": 0.0})
        elif calls and "kws_search_kernel" in name:
            calls[-1]["search_us"] += us
            calls[-1]["search_launches"] += 1
        elif calls and "kws_compact_kernel" in name:
            calls[-1]["compact_us"] += us
    calls = [c for c in calls if c["search_launches"]][-TRACE_CALLS * len(KS):]
    assert len(calls) == TRACE_CALLS * len(KS), len(calls)
    out = {}
    for i, n in enumerate(KS):
        mine = calls[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]
        out[f"K{n}"] = {k: round(statistics.median(c[k] for c in mine), 2) for k in ("frame_stats_us", "search_us", "compact_us")}
        out[f"K{n}"]["search_launches"] = mine[0]["search_launches"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-csv", default="")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--no-sessions", action="store_true")
    a = ap.parse_args()
    cases = offline_cases()
    if a.trace_run:
        for fn in cases.values():      # warm: code objects, the allocator
            fn()
        for n in KS:
            for _ in range(TRACE_CALLS):
                cases["frame_stats"]()
                cases[f"search_K{n}"]()
        torch.cuda.synchronize()
        return
    med = lambda v: round(statistics.median(v), 4)      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "expected_before_measuring": EXPECTED, "offline_shape": {"B": B, "T": T, "V": V, "dtype": "bf16", "keyword_lengths": "2..6", "K": list(KS)},
           "protocol": f"contenders alternated in one process, {a.rounds} rounds, median round; offline: a round = mean of {a.reps} back-to-back calls between "
                       "two synchronisations (host wall time); sessions: the median tick of a run of 31 blocks"}
    rounds = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, fn in cases.items():
            rounds[k].append(timed(fn, a.reps))
    res["offline_ms"] = {k: {"median_ms": med(v), "rounds_ms": [round(x, 4) for x in v]} for k, v in rounds.items()}
    if not a.no_sessions:
        import sessions_bench as sb
        model, parser = sb.build()
        block = sb.C * sb.LFR_N * 160
        wav = torch.randn(sb.SLOTS, block * sb.BLOCKS, device=DEV) * 0.1
        blocks = [wav[:, k * block:(k + 1) * block].contiguous() for k in range(sb.BLOCKS)]
        lists = {"plain": None, "keywords_K64": keyword_list(64), "keywords_K1000": keyword_list(1000)}
        for kl in lists.values():      # warm every cache size, the allocator and the engine
            run_sessions(sb, model, parser, blocks, sb.BLOCKS, kl)
        ticks = {k: [] for k in lists}
        for _ in range(a.rounds):
            for k, kl in lists.items():
                ticks[k].append(statistics.median(run_sessions(sb, model, parser, blocks, sb.BLOCKS, kl)))
        res["sessions_tick_ms"] = {k: {"median_ms": med(v), "rounds_ms": [round(x, 4) for x in v]} for k, v in ticks.items()}
        base = res["sessions_tick_ms"]["plain"]["median_ms"]
        res["sessions_tick_over_plain"] = {k: round(v["median_ms"] / base, 4) for k, v in res["sessions_tick_ms"].items()}
    if a.kernels_csv:
        res["kernels_us"] = kernel_durations(a.kernels_csv)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
