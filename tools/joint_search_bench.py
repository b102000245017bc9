"""One-pass joint CTC / attention search against attention-only and two-pass (rescoring) search at BASELINE configs[2] shapes:
B = 32, T = 500, V = 4232, 6 + 6 layers, bf16, beam 5, max length 32, random weights.

Two runs, because tracing slows the host and must not touch the end-to-end times:
    python tools/joint_search_bench.py --out times.json                          # ms per batch of each search, no profiler
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- \\
        python tools/joint_search_bench.py --one-pass-only                       # the same one-pass searches, traced
    python tools/joint_search_bench.py --merge times.json --kernel-stats DIR/.../p_kernel_stats.csv --out profiles/joint_search_bench.json
The merge divides each kernel's traced time by the number of one-pass searches of the traced run, and reports the prefix-scoring
kernels (asr_ctc_prefix_logprobs once per batch, asr_ctc_prefix_score + asr_ctc_prefix_gather per step) as a share of the
un-profiled one-pass time, beside the busiest kernels of the traced run (per search; the model's one-time set-up kernels are
counted in too, spread over the searches)."""
import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, V, BEAM, MAXLEN, LAM = 32, 500, 4232, 5, 32, 0.3
PREFIX_KERNELS = ("ctc_prefix_logprobs_kernel", "ctc_prefix_score_kernel", "ctc_prefix_gather_kernel")


def timed(fn, reps):
    import torch
    fn()                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def run(reps, one_pass_only):
    import torch
    from asr_chinese_e2e_amd import Models, decode
    from asr_chinese_e2e_amd.data_handler import Vocab, synthetic_pack
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, ctc_weight=LAM, cer_in_iterate=False, dtype="bf16"))
    model = M(cfg, Vocab.synthetic(V)).cuda().eval()
    pack = synthetic_pack(B, T, 80, V, device="cuda", dtype=torch.bfloat16)

    def one():
        return model.beam_search(pack, BEAM, 1, MAXLEN, ctc_weight=LAM, joint="one_pass")
    res = dict(shape=dict(B=B, T=T, V=V, layers="6+6", dtype="bf16", beam=BEAM, pre_beam=decode.default_pre_beam(BEAM), max_len=MAXLEN,
                          ctc_weight=LAM), reps=reps)
    if one_pass_only:
        res["one_pass_searches"] = reps + 1                 # the warm-up search is traced too
        res["one_pass_ms_traced"] = round(timed(one, reps), 2)
    else:
        res["attention_ms"] = round(timed(lambda: model.beam_search(pack, BEAM, 1, MAXLEN), reps), 2)
        res["two_pass_ms"] = round(timed(lambda: model.beam_search(pack, BEAM, 1, MAXLEN, ctc_weight=LAM), reps), 2)
        res["one_pass_ms"] = round(timed(one, reps), 2)
        res["one_pass_over_two_pass"] = round(res["one_pass_ms"] / res["two_pass_ms"], 3)
        res["hyps_nonempty"] = sum(1 for h in one() if h)
    return res


def merge(times, stats_csv, searches, steps):
    rows = list(csv.DictReader(open(stats_csv)))

    def short(name):
        return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
    per = {}
    for r in rows:
        n = short(r["Name"])
        if "spin_kernel" in n:              # the engine's one-time queue probe at construction (engine.py), not part of a search
            continue
        c, tot = per.get(n, (0, 0))
        per[n] = (c + int(r["Calls"]), tot + int(r["TotalDurationNs"]))
    out = dict(times)
    ms = {k: sum(tot for n, (c, tot) in per.items() if k in n) / searches / 1e6 for k in PREFIX_KERNELS}
    calls = {k: sum(c for n, (c, tot) in per.items() if k in n) for k in PREFIX_KERNELS}
    prefix = sum(ms.values())
    out.update(
        kernel_time_source="rocprofv3 --kernel-trace --stats, a run of its own; per one-pass search = traced total / searches traced",
        searches_traced=searches,
        prefix_kernels_ms_per_search={k: round(v, 3) for k, v in ms.items()},
        prefix_score_calls_per_search=calls["ctc_prefix_score_kernel"] / searches,
        prefix_score_us_per_call=round(1e3 * ms["ctc_prefix_score_kernel"] * searches / max(1, calls["ctc_prefix_score_kernel"]), 1),
        prefix_kernels_ms=round(prefix, 3),
        prefix_share_of_one_pass=round(prefix / times["one_pass_ms"], 4),
        top_kernels_ms_per_search={n: round(tot / searches / 1e6, 3)
                                   for n, (c, tot) in sorted(per.items(), key=lambda kv: -kv[1][1])[:8]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--one-pass-only", action="store_true", help="only the one-pass search (the run to trace)")
    ap.add_argument("--merge", default=None, help="JSON of an un-profiled run")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a --one-pass-only run")
    ap.add_argument("--searches", type=int, default=None, help="one-pass searches in the traced run (default: --reps + 1)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge:
        if not a.kernel_stats:
            raise SystemExit("--merge needs --kernel-stats")
        res = merge(json.load(open(a.merge)), a.kernel_stats, a.searches or a.reps + 1, MAXLEN)
    else:
        res = run(a.reps, a.one_pass_only)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
