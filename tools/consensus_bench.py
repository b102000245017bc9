#!/usr/bin/env python3
"""What consensus decoding of n-best lists costs: consensus.consensus_ids (one upload, three launches, one copy back) and
consensus.consensus_packed (the launches alone, on lists that are on the device already) beside the route the project had before - all
pairs through scoring.align_ids(ops=False), the pivot alignments through align_ids(ops=True), risks and votes in Python - and beside the
pure definition (tests/consensus_ref.py).  One JSON object on stdout (and in --out: profiles/consensus_bench.json).

  python tools/consensus_bench.py [--rounds 3] [--out profiles/consensus_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/consensus_bench.py --trace-run      # the launches alone, in a fixed order, to be started under rocprofv3 --kernel-trace

Cases: "b32_n5" / "b32_n10" / "b32_n16": 32 utterances, the n-best lists of kernels.ctc_prefix_beam (beam 16, 3 candidates per frame) over
random logits of 40 frames with a blank that wins about half of them; "n64_l256": one utterance of 64 entries, edits of one 256-token
string.  Contenders alternated in one process, --rounds rounds, medians; host wall time of whole calls between two synchronisations.  The
pure definition runs once per case (the large case takes it tens of seconds).  The kernels' own durations come from a trace run of its
own with --kernels-csv; host_share = 1 - (the three kernels) / consensus_ids.  Whether the MBR entry or the consensus differs from rank 0
is counted and reported; on random logits it says nothing about accuracy and nothing is asserted about it.

Expected, written down before the first run (nobody had run these kernels):
  * pair_dist, 32 x 10: 1440 + 32 waves of ~15 dependent row steps at ~0.1 us (score.hip's measured step), 5 - 6 waves per CU: 4 - 8 us;
    n = 16 (3872 waves): 6 - 12 us; n = 5: 3 - 5 us.
  * pivot_votes, 32 x 10: 320 waves; each sums n products per lane (n dependent loads of d), runs 15 row steps with two ballots and an LDS
    store, then a ~20-step walk in LDS at ~130 ns a step: 6 - 10 us, the slowest of the three although it has the fewest waves.
  * slot_vote: 32 x 81 slots (L is the search's 40-frame capacity, of which ~31 slots are the pivot's): 2592 waves, most of which leave
    at once; the others run two n-step v_readlane sweeps: 3 - 5 us.
  * consensus_packed (three launches, no copy): 30 - 60 us of wall time, launch-bound.
  * consensus_ids, 32 x 10: packing 320 lists, one upload, one copy back, 32 result dicts of ~31 slots: 0.5 - 1.5 ms, host share above 95 %.
  * the earlier route: two align_ids calls (1440 pairs counts only, 320 with ops: 1 - 2 ms each, host-bound as the README measures), the
    risks and the votes of 320 op lists in Python (2 - 4 ms): 5 - 10 ms, 5 - 15 x consensus_ids.
  * the pure definition, 32 x 10: 32 x (90 tables + 10 alignments) of 15 x 15 at ~0.15 ms: 0.4 - 0.6 s, ~500 x consensus_ids.
  * n64_l256: pair_dist 2016 waves x 4 column blocks x 256 row steps at 0.1 us = ~100 us a wave, 8 waves per CU side by side: 100 - 200 us;
    pivot_votes 64 waves, each the same forward pass with mask stores plus a ~500-step walk (65 us) and 64 dependent loads: 200 - 300 us;
    slot_vote 513 waves of two 64-step sweeps: 4 - 8 us.  consensus_ids 1.5 - 3 ms (the 0.6 MB copy back of votes and alternatives);
    the earlier route 50 - 100 ms (2016 + 64 pairs of 256 x 256, 64 op lists of ~260 ops); the definition 4032 tables at ~4 ms: 15 - 20 s.
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
from asr_chinese_e2e_amd.consensus import _host_arrays, consensus_ids, consensus_packed, nbest_weights  # noqa: E402
from asr_chinese_e2e_amd.scoring import COR, DEL, INS, SUB, align_ids  # noqa: E402
from tests import consensus_ref as C  # noqa: E402

DEV = "cuda"
V = 4232
TRACE_CALLS = 3
KERNELS = ("nbest_pair_dist_kernel", "nbest_pivot_votes_kernel", "nbest_slot_vote_kernel")
EXPECTED = {"b32_n5": {"pair_dist_us": "3 - 5", "pivot_votes_us": "5 - 9", "slot_vote_us": "3 - 5"},
            "b32_n10": {"pair_dist_us": "4 - 8", "pivot_votes_us": "6 - 10", "slot_vote_us": "3 - 5", "consensus_packed_us": "30 - 60",
                        "consensus_ids_ms": "0.5 - 1.5", "host_share": "> 0.95", "earlier_route_ms": "5 - 10", "earlier_over_ids": "5 - 15",
                        "definition_s": "0.4 - 0.6"},
            "b32_n16": {"pair_dist_us": "6 - 12", "pivot_votes_us": "7 - 12", "slot_vote_us": "3 - 6"},
            "n64_l256": {"pair_dist_us": "100 - 200", "pivot_votes_us": "200 - 300", "slot_vote_us": "4 - 8", "consensus_ids_ms": "1.5 - 3",
                         "earlier_route_ms": "50 - 100", "definition_s": "15 - 20"}}


def search_case(rng, n):
    B, T = 32, 40
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    logits = torch.randn(B * T, V, generator=g)
    logits[:, 0] = 3.7 + 0.6 * torch.randn(B * T, generator=g)      # the largest of 4231 normals is ~3.6: the blank wins about half the frames
    vals, ids, blank_lp = K.ctc_frame_topk(logits.to(DEV), 3)
    tok, ln, scores = K.ctc_prefix_beam(vals, ids, blank_lp, torch.full((B,), T, dtype=torch.int32, device=DEV), B, T, 16, n)[:3]
    tok, ln, scores = tok.cpu().numpy(), ln.cpu().numpy(), scores.double().cpu().numpy()
    lists = [[tok[b, k, :ln[b, k]].tolist() for k in range(n) if ln[b, k] >= 0] for b in range(B)]
    return lists, [scores[b, :len(lists[b])].tolist() for b in range(B)]


def edited(rng, base, k):
    h = list(base)
    for _ in range(k):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(h) + 1))
        if kind == 0 and at < len(h):
            del h[at]
        elif kind == 1 and at < len(h):
            h[at] = int(rng.integers(4, V))
        else:
            h.insert(at, int(rng.integers(4, V)))
    return h[:C.MAX_LEN]


def make_cases():
    rng = np.random.default_rng(0)
    c = {f"b32_n{n}": search_case(rng, n) for n in (5, 10, 16)}
    base = rng.integers(4, V, 256).tolist()
    c["n64_l256"] = ([[edited(rng, base, int(rng.integers(0, 21))) for _ in range(64)]], [np.sort(rng.normal(0.0, 1.5, 64))[::-1].tolist()])
    return c


def earlier_route(lists, weights):
    """The consensus strings by what the project had before: align_ids for every pair and for the pivot alignments, the rest in Python."""
    pairs = [(u, i, k) for u, l in enumerate(lists) for i in range(len(l)) for k in range(i + 1, len(l))]
    flat = [h for l in lists for h in l]
    first = np.cumsum([0] + [len(l) for l in lists])
    dist = align_ids([lists[u][k] for u, i, k in pairs], flat, ref_of=[int(first[u]) + i for u, i, k in pairs], ops=False, device=DEV) if pairs else []
    risk = [[0] * len(l) for l in lists]
    for (u, i, k), r in zip(pairs, dist):
        risk[u][i] += weights[u][k] * r["distance"]
        risk[u][k] += weights[u][i] * r["distance"]
    pivot = [min(range(len(r)), key=lambda i: (r[i], i)) for r in risk]
    al = align_ids(flat, [lists[u][p] for u, p in enumerate(pivot)], ref_of=[u for u, l in enumerate(lists) for _ in l], ops=True, device=DEV)
    out = []
    for u, l in enumerate(lists):
        m = len(l[pivot[u]])
        votes = []
        for k, h in enumerate(l):
            v, row, run = [C.EPS] * (2 * m + 1), 0, False
            for op, ri, hj in al[int(first[u]) + k]["ops"]:
                if op == INS:
                    if not run:
                        v[2 * row] = h[hj]
                    run = True
                else:
                    if op in (COR, SUB):
                        v[2 * ri + 1] = h[hj]
                    row, run = ri + 1, False
            votes.append(v)
        top = [C.slot_alternatives([(k, votes[k][s]) for k in range(len(l))], weights[u])[0][0] for s in range(2 * m + 1)]
        out.append((pivot[u], [t for t in top if t != C.EPS]))
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class Packed:
    """A case on the device, as a search leaves it: the launches alone can be timed or traced."""

    def __init__(self, lists, weights):
        self.tok, self.ln, self.w = _host_arrays(lists, weights, None, 1.0)
        self.dev = [torch.from_numpy(x).to(DEV) for x in (self.tok, self.ln, self.w)]
        self.out = K.nbest_consensus(*self.dev, self.ln, self.w, alts=4)

    def __call__(self):
        return K.nbest_consensus(*self.dev, self.ln, self.w, alts=4, out=self.out)

    def packed(self):
        return consensus_packed(*self.dev, self.ln, self.w, alts=4)


def kernel_durations(path, names):
    """The median over the trace run's calls of each case's three kernels, in the trace run's fixed order (us)."""
    rows = sorted((r for r in csv.DictReader(open(path, newline="")) if any(k in r.get("Kernel_Name", "") for k in KERNELS)), key=lambda r: int(r["Start_Timestamp"]))
    rows = rows[-len(names) * TRACE_CALLS * 3:]
    assert len(rows) == len(names) * TRACE_CALLS * 3, len(rows)
    out = {}
    for i, name in enumerate(names):
        mine = rows[i * TRACE_CALLS * 3:(i + 1) * TRACE_CALLS * 3]
        for j, kern in enumerate(KERNELS):
            sel = mine[j::3]
            assert all(kern in r["Kernel_Name"] for r in sel), (name, kern, sel[0]["Kernel_Name"])
            out.setdefault(name, {})[kern] = round(statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sel), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-csv", default="")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    cases = make_cases()
    names = list(cases)
    weights = {n: [nbest_weights(s).tolist() for s in cases[n][1]] for n in names}
    packed = {n: Packed(cases[n][0], weights[n]) for n in names}
    torch.cuda.synchronize()
    if a.trace_run:
        for n in names:
            for _ in range(TRACE_CALLS):
                packed[n]()
        torch.cuda.synchronize()
        return
    med = lambda v: round(statistics.median(v), 4)      # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "expected_before_measuring": EXPECTED,
           "protocol": f"contenders alternated in one process, {a.rounds} rounds, medians; *_ms are host wall times of whole calls between two "
                       "synchronisations; the definition runs once per case; kernels_us from a kernel trace of its own",
           "shapes": {n: {"U": int(packed[n].tok.shape[0]), "N": int(packed[n].tok.shape[1]), "L": int(packed[n].tok.shape[2]),
                          "mean_entries": round(float(np.mean([len(l) for l in cases[n][0]])), 2),
                          "mean_tokens": round(float(np.mean([len(h) for l in cases[n][0] for h in l])), 2)} for n in names}}
    t, counts = {}, {}
    for n in names:      # warm-up of every contender, and the definition once
        lists, scores = cases[n]
        got = consensus_ids(lists, scores=scores, device=DEV)
        old = earlier_route(lists, weights[n])
        t0 = time.perf_counter()
        want = [C.consensus(l, w) for l, w in zip(lists, weights[n])]
        t[f"{n}_definition_ms"] = [(time.perf_counter() - t0) * 1e3]
        assert [(g["pivot"], g["consensus"]) for g in got] == [(w["pivot"], w["consensus"]) for w in want] == old, n
        counts[n] = {"utterances": len(lists), "mbr_not_rank0": sum(1 for g in got if g["pivot"] != 0),
                     "consensus_differs_from_rank0": sum(1 for g, l in zip(got, lists) if g["consensus"] != l[0]),
                     "consensus_in_no_entry": sum(1 for g, l in zip(got, lists) if g["consensus"] not in l),
                     "extra_insertions": sum(g["extra_insertions"] for g in got)}
    for _ in range(a.rounds):
        for n in names:
            lists, scores = cases[n]
            t.setdefault(f"{n}_consensus_ids_ms", []).append(wall(lambda: consensus_ids(lists, scores=scores, device=DEV))[0])
            t.setdefault(f"{n}_consensus_packed_ms", []).append(wall(packed[n].packed)[0])
            t.setdefault(f"{n}_launches_into_a_kept_buffer_ms", []).append(wall(packed[n])[0])
            t.setdefault(f"{n}_earlier_route_ms", []).append(wall(lambda: earlier_route(lists, weights[n]))[0])
    res["timings"] = {k: {"median": med(v), "rounds": [round(x, 4) for x in v]} for k, v in t.items()}
    m = {k: v["median"] for k, v in res["timings"].items()}
    res["earlier_route_over_consensus_ids"] = {n: round(m[f"{n}_earlier_route_ms"] / m[f"{n}_consensus_ids_ms"], 2) for n in names}
    res["definition_over_consensus_ids"] = {n: round(m[f"{n}_definition_ms"] / m[f"{n}_consensus_ids_ms"], 1) for n in names}
    res["what_the_votes_changed"] = counts
    if a.kernels_csv:
        k = res["kernels_us"] = kernel_durations(a.kernels_csv, names)
        res["host_share_of_consensus_ids"] = {n: round(1.0 - sum(k[n].values()) / 1e3 / m[f"{n}_consensus_ids_ms"], 4) for n in names}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
