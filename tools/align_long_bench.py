#!/usr/bin/env python3
"""Long-recording alignment: what asr_ctc_align_long costs.  One JSON object on stdout, merged into --out.

  python tools/align_long_bench.py --part kernel   [--rounds 3] [--out profiles/align_long_bench.json]
  python tools/align_long_bench.py --part versus   [--rounds 3] [--out profiles/align_long_bench.json]
  python tools/align_long_bench.py --part longform [--rounds 3] [--out profiles/align_long_bench.json]

* --part kernel: (T, L) = (20 000, 3 000) and (60 000, 8 192), V = 4232, bf16 rows of random logits, random labels.  HIP events around CALLS
  back-to-back calls, the contenders alternated in one process over --rounds rounds, medians.  The contenders per shape: the whole call,
  and the same call with lse[T - 1] = +inf, which makes the last frame impossible: the kernel runs the whole recursion, finds no path and
  returns before the backtrace, so that run is the recursion's share and the difference is the backtrace's plus the span and token passes'.
  (Four launches per call, three of them workgroups that leave at once.)
* --part versus: asr_ctc_align and asr_ctc_align_long on one shape both accept (L = 255, T = 4000, V = 4232, bf16): the per-frame cost of
  leaving the single wave (two waves, a barrier per frame, emissions gathered in the kernel instead of a materialised fp64 lattice).
* --part longform: host wall time of model.align_long on tools/long_form_bench.py's synthetic 10-minute recording (the 6-layer bf16 joint
  model, V = 4232, random weights), its transcript being the first 50 of transcribe_long's own ids of every segment, a line per segment
  (the random weights spell more than 8192 tokens in all); beside transcribe_long."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
V = 4232


def timed(torch, fn, calls):
    """ms per call: HIP events around `calls` back-to-back calls, after one warm-up call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def rounds_of(torch, contenders, rounds, calls):
    res = {k: [] for k in contenders}
    for _ in range(rounds):
        for k, fn in contenders.items():
            res[k].append(round(timed(torch, fn, calls), 4))
    return res, {k: round(statistics.median(v), 4) for k, v in res.items()}


def case(torch, np, K, T, L, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = (torch.randn(T, V, generator=g, device=DEV) * 3.0).to(torch.bfloat16)
    lab = np.random.RandomState(seed).randint(1, V, L)
    _, _, _, lse, _ = K.ctc_frame_stats(rows.view(1, T, V), None, 0)
    return rows, lse.view(T).contiguous(), lab


def part_kernel(torch, np, rounds):
    from asr_chinese_e2e_amd import kernels as K
    out = {}
    for T, L in ((20000, 3000), (60000, 8192)):
        rows, lse, lab = case(torch, np, K, T, L, L)
        dead = lse.clone()
        dead[T - 1] = float("inf")
        ws = K.Workspace(DEV)
        run = lambda l: K.ctc_align_long(rows, l, [0, T], lab, [0, L], ws=ws)      # noqa: E731
        score, score_dead = float(run(lse)[3][0]), float(run(dead)[3][0])
        res, med = rounds_of(torch, {"whole_ms": lambda: run(lse), "recursion_only_ms": lambda: run(dead)}, rounds, 3)
        rest = med["whole_ms"] - med["recursion_only_ms"]
        out[f"T{T}_L{L}"] = {"T": T, "L": L, "V": V, "dtype": "bf16", "score_finite": score == score and abs(score) != float("inf"),
                             "recursion_only_score": score_dead, "rounds": res, "median_ms": med,
                             "recursion_us_per_frame": round(1e3 * med["recursion_only_ms"] / T, 4),
                             "backtrace_and_token_passes_ms": round(rest, 4), "backtrace_and_token_passes_us_per_frame": round(1e3 * rest / T, 4),
                             "recursion_share": round(med["recursion_only_ms"] / med["whole_ms"], 4),
                             "workspace_bytes": K.ctc_align_long_workspace_bytes(1, T, L), "rows_bytes": rows.numel() * 2}
        del rows, lse, dead, ws
        torch.cuda.empty_cache()
    return out


def part_versus(torch, np, rounds):
    from asr_chinese_e2e_amd import kernels as K
    T, L = 4000, 255
    rows, lse, lab = case(torch, np, K, T, L, 5)
    logits = rows.view(1, T, V)
    il, ll = torch.tensor([T], dtype=torch.int32, device=DEV), torch.tensor([L], dtype=torch.int32, device=DEV)
    dlab = torch.from_numpy(lab.astype(np.int32)).to(DEV).view(1, L)
    ws_old, ws_new = K.Workspace(DEV), K.Workspace(DEV)
    old = lambda: K.ctc_align(logits, il, dlab, ll, ws=ws_old)      # noqa: E731
    new = lambda: K.ctc_align_long(rows, lse, [0, T], lab, [0, L], ws=ws_new)      # noqa: E731
    from tests import align_long_ref as A
    o, n = old(), new()
    differ = int((o[1][0] != n[1]).any(dim=1).sum())
    want = A.align(rows.float().cpu().numpy(), lse.cpu().numpy(), lab)
    exact = bool(np.array_equal(n[1].cpu().numpy(), want["spans"])) and float(n[3][0]) == want["score"]
    res, med = rounds_of(torch, {"ctc_align_ms": old, "ctc_align_long_ms": new}, rounds, 10)
    return {"T": T, "L": L, "V": V, "dtype": "bf16", "tokens_whose_spans_differ": differ, "ctc_align_score_f32": float(o[3][0]), "ctc_align_long_score": float(n[3][0]),
            "ctc_align_long_is_the_definition": exact, "rounds": res, "median_ms": med,
            "ctc_align_us_per_frame": round(1e3 * med["ctc_align_ms"] / T, 4), "ctc_align_long_us_per_frame": round(1e3 * med["ctc_align_long_ms"] / T, 4),
            "note": "ctc_align: softmax into an fp64 lattice, then one wave; ctc_align_long: lse given, two waves of 128 pairs, host checks and an upload of the offsets and labels per call.  The lattice is random, not peaky: over 4000 frames states fall more than e^-708 below the column maximum, which the "
                    "rescaled probability domain of ctc_align flushes to zero, so the two may take different paths; the log-domain score is the definition's"}


def part_longform(torch, np, rounds):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab
    from tools.long_form_bench import LFR_M, LFR_N, N_MELS, SECONDS, recording
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, dropout=0.0, layer_num=6, ctc_weight=0.3, dtype="bf16"))
    torch.manual_seed(0)
    model = M(cfg, Vocab.synthetic(V)).to(DEV).eval()
    parser = AudioParser(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, device=DEV)
    x = recording(np)
    wav = torch.from_numpy(x[None]).to(DEV)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    tr = lambda: model.transcribe_long(parser, wav, [len(x)], batch_size=16, beam_size=5, joint="rescore")      # noqa: E731
    _, a = wall(tr)
    lines = [[i for i in s["ids"] if i != 0][:50] for s in a[0]["segments"]]      # random weights spell more than 8192 tokens in all: 50 per segment
    al = lambda: model.align_long(parser, wav, [len(x)], [lines], batch_size=16)      # noqa: E731
    _, b = wall(al)
    res = {"align_long_s": [], "transcribe_long_s": []}
    for _ in range(rounds):
        res["align_long_s"].append(round(wall(al)[0], 4))
        res["transcribe_long_s"].append(round(wall(tr)[0], 4))
    med = {k: round(statistics.median(v), 4) for k, v in res.items()}
    score = b[0]["score"]
    return {"model": "6-layer bf16 joint, V = 4232, random weights, batch_size 16; transcribe_long with beam 5, joint='rescore'", "recording_s": SECONDS,
            "segments": len(a[0]["segments"]), "tokens": sum(len(l) for l in lines), "frames": b[0]["frames"], "feasible": score == score and abs(score) != float("inf"),
            "rounds": res, "median_s": med, "align_real_time_factor": round(med["align_long_s"] / SECONDS, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernel", "versus", "longform"], required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    fn = {"kernel": part_kernel, "versus": part_versus, "longform": part_longform}[a.part]
    res = {"device": torch.cuda.get_device_name(0), a.part: fn(torch, np, a.rounds)}
    if a.out:
        old = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                old = json.load(f)
        old.update(res)
        with open(a.out, "w") as f:
            f.write(json.dumps(old, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
