#!/usr/bin/env python3
"""What rescoring n-best lists costs: rescore.lm_scores (one upload, one launch of asr_lm_score_nbest, one copy back) beside a host loop of
NgramLM.score, and the sweep of a weight grid (asr_nbest_sweep) beside the same sweep in vectorised numpy.  One JSON object on stdout (and
in --out: profiles/rescore_bench.json).

  python tools/rescore_bench.py [--rounds 3] [--lm-cache DIR] [--out profiles/rescore_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
  python tools/rescore_bench.py --trace-run [--lm-cache DIR]     # the launches alone, in a fixed order, to be started under rocprofv3 --kernel-trace
  python tools/rescore_bench.py --build-cache DIR                # compiles the two LMs on the host (no GPU needed) and saves them

LM cases: 32 x 10 and 7176 x 10 hypotheses (AISHELL-1's test set size) of 10 to 20 random tokens, under random order-3 LMs of about 1e4 and
1e6 n-grams (tools/lm_fusion_bench.py's generator, weight 1, no insertion bonus).  On random strings most lookups miss their context's arcs, so
a token typically pays one or two binary searches, the back-off terms and the indexed unigram load: close to the longest chain an order-3
model has.  Sweep case: U = 7176, N = 10, K = 4, G = 231 (att_score = 1; ctc_score 0 .. 1 by 0.5; lm 0 .. 1 by 0.1; len -1 .. 2 by 0.5),
features on a grid of eighths, errors from random edits.  Contenders alternated in one process, --rounds rounds, medians; host wall time of
whole calls between two synchronisations; the host loop over 71760 hypotheses runs once.  The kernels' own durations come from a trace run
of its own with --kernels-csv; host_share = 1 - kernel / call.

Expected, written down before the first run (nobody had run these kernels):
  * lm_score_nbest, 320 hypotheses, 1e4 n-grams: five waves, each lane ~16 tokens in series, a token ~6 - 10 dependent loads (two binary
    searches of a few steps, st_bow, st_back, the unigram pair) at 0.5 - 1 us of L2 / HBM latency: 60 - 150 us, latency-bound with nothing
    to hide it behind.  1e6 n-grams: longer arc ranges and colder tables: 100 - 250 us.
  * lm_score_nbest, 71760 hypotheses: 1122 waves, four or five per CU, all resident at once, so the same chains overlap: 100 - 300 us at
    1e4 n-grams, 200 - 600 us at 1e6 - not 224 x the small case.  If it comes out far above, the token-parallel form the design left
    open is worth a look; this script then says so.
  * lm_scores, 32 x 10: packing 320 lists, one upload, one copy back, 320 dicts: 0.3 - 0.8 ms, host share above 80 %.  The host loop: 320 x 16
    chains of Python binary searches at 3 - 5 us: 15 - 25 ms, 20 - 60 x.
  * lm_scores, 7176 x 10: the packing loop over 71760 lists (~5 us each) dominates: 0.4 - 0.7 s, host share above 99 %.  The host loop: 1.15
    million chains, 4 - 6 s: 7 - 15 x.
  * nbest_sweep: 231 x 113 waves, each 40 coalesced 512-byte loads from L2 (the 2.3 MB of features stay there), 40 multiplies and adds,
    four wave sums: ~0.5 GB of L2 reads, 80 - 250 us; the sum kernel 3 - 6 us.
  * the device sweep as a call (transposition, two uploads, two launches, one copy back of 231 x 7176 picks): 5 - 12 ms, host share above 95 %.
  * the numpy sweep: 231 grid points x (4 columns x 71760 entries with temporaries, an argmax, a gather): ~1.5 ms each, 0.25 - 0.5 s:
    25 - 80 x the device call.  rescore.sweep as a whole (asr_edit_align over 71760 entries first) is bound by that call's host packing:
    0.4 - 0.8 s."""
import argparse
import csv
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

V = 4232
LM_SIZES = (10 ** 4, 10 ** 6)
HYP_SHAPES = ((32, 10), (7176, 10))
SWEEP_SHAPE = dict(U=7176, N=10, K=4)
TRACE_CALLS = 3
EXPECTED = {"lm_score_nbest_us": {"lm_10000_32x10": "60 - 150", "lm_1000000_32x10": "100 - 250", "lm_10000_7176x10": "100 - 300", "lm_1000000_7176x10": "200 - 600"},
            "lm_scores_ms": {"32x10": "0.3 - 0.8", "7176x10": "400 - 700"}, "host_loop_ms": {"32x10": "15 - 25", "7176x10": "4000 - 6000"},
            "host_loop_over_lm_scores": {"32x10": "20 - 60", "7176x10": "7 - 15"}, "lm_scores_host_share": {"32x10": "> 0.8", "7176x10": "> 0.99"},
            "nbest_sweep_kernel_us": "80 - 250", "nbest_sweep_sum_kernel_us": "3 - 6", "device_sweep_call_ms": "5 - 12", "device_sweep_host_share": "> 0.95",
            "numpy_sweep_ms": "250 - 500", "numpy_over_device_sweep": "25 - 80", "sweep_with_edit_align_ms": "400 - 800"}


def lm_model(n, cache, device):
    from tools.lm_fusion_bench import model
    return model(n, cache=cache, device=device, weight=1.0)


def hyp_lists(U, N, seed):
    rng = np.random.default_rng(seed)
    return [[rng.integers(4, V, int(rng.integers(10, 21))).tolist() for _ in range(N)] for _ in range(U)]


def sweep_case(seed=0):
    """(f (U, N, K), lists, err (U, N, 3), grid): features on eighths, the last column a token count, errors of random size."""
    from asr_chinese_e2e_amd.rescore import Grid
    rng = np.random.default_rng(seed)
    U, N, Kc = SWEEP_SHAPE["U"], SWEEP_SHAPE["N"], SWEEP_SHAPE["K"]
    f = rng.integers(-400, 1, (U, N, Kc)).astype(np.float64) / 8.0
    f[:, :, Kc - 1] = rng.integers(10, 21, (U, N))
    f[rng.random((U, N, Kc)) < 0.01] = -math.inf
    err = rng.integers(0, 3, (U, N, 3)).astype(np.int32) * (rng.random((U, N, 1)) < 0.6)
    present = rng.random((U, N)) < 0.97
    present[:, 0] = True
    lists = [[[5] if present[u, e] else None for e in range(N)] for u in range(U)]
    grid = Grid(att_score=[1.0], ctc_score=[0.0, 0.5, 1.0], lm=[i * 0.1 for i in range(11)], len=[-1.0 + i * 0.5 for i in range(7)])
    assert len(grid) == 231
    return f, lists, err.astype(np.int32), grid.points, present


def numpy_sweep(f, present, err, grid):
    """The definition's sweep in vectorised numpy: a product, then a sum, per column; the first maximum is the lowest index."""
    U, N, Kc = f.shape
    G = grid.shape[0]
    pick, tot = np.zeros((G, U), np.int32), np.zeros((G, 4), np.int64)
    fin = np.isfinite(f)
    clean = np.where(fin, f, 0.0)
    first = np.argmax(present, axis=1)
    rows = np.arange(U)
    for g in range(G):
        total, ok = np.zeros((U, N)), present.copy()
        for k in range(Kc):
            if grid[g, k] != 0.0:
                ok &= fin[:, :, k]
                total = total + grid[g, k] * clean[:, :, k]
        p = np.argmax(np.where(ok, total, -np.inf), axis=1)
        p = np.where(ok.any(axis=1), p, first)
        e = err[rows, p].astype(np.int64)
        pick[g] = p
        tot[g] = (*e.sum(axis=0), int((e.sum(axis=1) > 0).sum()))
    return pick, tot


def kernel_durations(path):
    """Per kernel the durations (us) in launch order."""
    rows = sorted(csv.DictReader(open(path, newline="")), key=lambda r: int(r["Start_Timestamp"]))
    out = {"lm_score_nbest_kernel": [], "nbest_sweep_kernel": [], "nbest_sweep_sum_kernel": []}
    for r in rows:
        for k in out:
            if k in r.get("Kernel_Name", ""):
                out[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--lm-cache", default="")
    ap.add_argument("--build-cache", default="")
    ap.add_argument("--kernels-csv", default="")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    if a.build_cache:
        for n in LM_SIZES:
            lm = lm_model(n, a.build_cache, None)
            print(n, lm.n_ngrams, lm.S, lm.A)
        return
    import torch

    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.rescore import _device_sweep, _token_rows, entry_errors, lm_scores
    dev = "cuda"
    lms = {n: lm_model(n, a.lm_cache or None, dev) for n in LM_SIZES}
    hyps = {f"{U}x{N}": hyp_lists(U, N, seed=U) for U, N in HYP_SHAPES}
    f, lists, err, grid, present = sweep_case()
    U, N, Kc = f.shape
    G = grid.shape[0]
    # the launches alone, on inputs that are on the device already
    packed = {}
    for shape, l in hyps.items():
        tok, ln, _ = _token_rows(l, "bench")
        packed[shape] = (torch.from_numpy(tok).to(dev), torch.from_numpy(ln).to(dev), ln, torch.empty(6 * ln.shape[0], dtype=torch.int32, device=dev))
    hf, hl = np.ascontiguousarray(f.transpose(2, 1, 0)), np.ascontiguousarray(np.where(present, 0, -1).astype(np.int32).T)
    he = np.ascontiguousarray(err.transpose(2, 1, 0))
    d_sw = [torch.from_numpy(x).to(dev) for x in (hf, hl, he, grid)]
    ws = K.Workspace(torch.device(dev))
    o_pick, o_tot = torch.empty(G, U, dtype=torch.int32, device=dev), torch.empty(G, 4, dtype=torch.int64, device=dev)

    def launch_lm(n, shape):
        tok, ln, hln, out = packed[shape]
        return K.lm_score_nbest(tok, ln, hln, lms[n], out=out)

    def launch_sweep():
        return K.nbest_sweep(*d_sw, hf, hl, grid, ws=ws, out_pick=o_pick, out_tot=o_tot)
    order = [(n, shape) for n in LM_SIZES for shape in hyps]
    for n, shape in order:
        launch_lm(n, shape)
    launch_sweep()
    torch.cuda.synchronize()
    if a.trace_run:
        for n, shape in order:
            for _ in range(TRACE_CALLS):
                launch_lm(n, shape)
        for _ in range(TRACE_CALLS):
            launch_sweep()
        torch.cuda.synchronize()
        return

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def host_loop(lm, l):
        return [[lm.score(h) for h in utt] for utt in l]
    res = {"device": torch.cuda.get_device_name(0), "expected_before_measuring": EXPECTED,
           "protocol": f"contenders alternated in one process, {a.rounds} rounds, medians; *_ms are host wall times of whole calls between two synchronisations; "
                       "the host loop over 7176 x 10 hypotheses runs once; kernels_us from a kernel trace of its own",
           "lms": {str(n): {"ngrams": lm.n_ngrams, "states": lm.S, "arcs": lm.A} for n, lm in lms.items()},
           "mean_tokens": {s: round(float(np.mean([len(h) for u in l for h in u])), 2) for s, l in hyps.items()}, "sweep_shape": dict(SWEEP_SHAPE, G=G)}
    t = {}
    # agreement first (and the warm-up of every contender): the device against the host loop and against numpy
    for n, shape in order:
        got = lm_scores(hyps[shape], lms[n], device=dev)
        ms, want = wall(lambda: host_loop(lms[n], hyps[shape]))
        assert [[h["lm_score"] for h in u] for u in got] == want, (n, shape)
        if shape == "7176x10":
            t[f"lm_{n}_{shape}_host_loop_ms"] = [ms]
    pick, tot, _ = _device_sweep(f, lists, err, grid, device=dev)
    n_pick, n_tot = numpy_sweep(f, present, err, grid)
    assert np.array_equal(pick, n_pick) and np.array_equal(tot, n_tot)
    refs = [[5]] * U
    entry_errors(lists, refs, device=dev)
    for _ in range(a.rounds):
        for n, shape in order:
            t.setdefault(f"lm_{n}_{shape}_lm_scores_ms", []).append(wall(lambda: lm_scores(hyps[shape], lms[n], device=dev))[0])
            t.setdefault(f"lm_{n}_{shape}_launch_alone_ms", []).append(wall(lambda: launch_lm(n, shape))[0])
            if shape != "7176x10":
                t.setdefault(f"lm_{n}_{shape}_host_loop_ms", []).append(wall(lambda: host_loop(lms[n], hyps[shape]))[0])
        t.setdefault("device_sweep_call_ms", []).append(wall(lambda: _device_sweep(f, lists, err, grid, device=dev))[0])
        t.setdefault("sweep_launches_alone_ms", []).append(wall(launch_sweep)[0])
        t.setdefault("numpy_sweep_ms", []).append(wall(lambda: numpy_sweep(f, present, err, grid))[0])
        t.setdefault("entry_errors_edit_align_ms", []).append(wall(lambda: entry_errors(lists, refs, device=dev))[0])
    res["timings"] = {k: {"median": round(statistics.median(v), 4), "rounds": [round(x, 4) for x in v]} for k, v in t.items()}
    m = {k: v["median"] for k, v in res["timings"].items()}
    res["host_loop_over_lm_scores"] = {f"lm_{n}_{s}": round(m[f"lm_{n}_{s}_host_loop_ms"] / m[f"lm_{n}_{s}_lm_scores_ms"], 1) for n, s in order}
    res["numpy_over_device_sweep"] = round(m["numpy_sweep_ms"] / m["device_sweep_call_ms"], 2)
    res["sweep_with_edit_align_ms"] = round(m["device_sweep_call_ms"] + m["entry_errors_edit_align_ms"], 3)
    if a.kernels_csv:
        d = kernel_durations(a.kernels_csv)
        lm_d = d["lm_score_nbest_kernel"][-len(order) * TRACE_CALLS:]
        k = res["kernels_us"] = {f"lm_{n}_{s}": round(statistics.median(lm_d[i * TRACE_CALLS:(i + 1) * TRACE_CALLS]), 2) for i, (n, s) in enumerate(order)}
        k["nbest_sweep_kernel"] = round(statistics.median(d["nbest_sweep_kernel"][-TRACE_CALLS:]), 2)
        k["nbest_sweep_sum_kernel"] = round(statistics.median(d["nbest_sweep_sum_kernel"][-TRACE_CALLS:]), 2)
        res["host_share"] = {f"lm_{n}_{s}_lm_scores": round(1.0 - k[f"lm_{n}_{s}"] / 1e3 / m[f"lm_{n}_{s}_lm_scores_ms"], 4) for n, s in order}
        res["host_share"]["device_sweep_call"] = round(1.0 - (k["nbest_sweep_kernel"] + k["nbest_sweep_sum_kernel"]) / 1e3 / m["device_sweep_call_ms"], 4)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
