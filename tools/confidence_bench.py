#!/usr/bin/env python3
"""Token confidence and streamed token times: what they cost.  One JSON object on stdout (and in --out).

  python tools/confidence_bench.py [--rounds 3] [--out profiles/confidence_bench.json] [--kernels-csv <rocprofv3 kernel trace csv>]
                                   [--parent-json <the --plain-only output of a run over the parent commit's package>]
  python tools/confidence_bench.py --plain-only [--package-root <another checkout>]   # the timed=False tick alone
  python tools/confidence_bench.py --trace-run      # a short run of the timed tick and of transcribe(confidence=...), for rocprofv3 --kernel-trace

The shape of tools/sessions_bench.py (32 slots, C = 16, the 6-layer bf16 joint model, V = 4232, blocks of 480 ms):
* the sessions tick with timed=False and timed=True, alternated in one process over --rounds rounds, the median of the ticks in which
  all 32 callers are live; timed=False launches what the parent commit launches (asr_ctc_frame_best_blank + asr_session_ctc_step),
  timed=True asr_ctc_frame_stats + asr_session_ctc_step_tokens and the host's token bookkeeping;
  tick_timed_read_tokens_ms: the timed tick followed by tokens(b) of every slot (a random model closes a run on nearly every frame, so
  this is the most a caption display can be asked to read: every call rebuilds the slot's whole list);
* offline model.transcribe of 16 utterances of 512 encoder frames (the CTC-only twin of the model, beam 5) with and without
  confidence="post_max": two more launches behind the alignment's and one more copy to the host.
--package-root: import asr_chinese_e2e_amd from that checkout instead of this one (the parent commit's, built there): with --plain-only
the same script times the parent's tick in the same job.  The difference to this tree's timed=False tick is reported, not gated on.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("frame_stats_kernel", "token_conf_kernel", "session_ctc_step_tokens_kernel", "frame_best_blank_kernel", "session_ctc_step_kernel", "ctc_viterbi_kernel",
           "ctc_lse_gather_rows_kernel")
DEV = "cuda"
C, LFR_M, LFR_N, N_MELS, BLOCKS, SLOTS, STAGGER = 16, 4, 3, 80, 31, 32, 8


def build(torch, np):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, dropout=0.0, layer_num=6, ctc_weight=0.3, dtype="bf16", chunk_size=C))
    torch.manual_seed(0)
    model = M(cfg, Vocab.synthetic(4232)).to(DEV).eval()
    parser = AudioParser(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, device=DEV, norm="global", cmvn=(np.full(N_MELS, -1.0), np.full(N_MELS, 0.4)))
    return model, parser


def build_ctc(torch):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    M = Models.TransformerCTC
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, dropout=0.0, layer_num=6, ctc_weight=1.0, dtype="bf16"))
    torch.manual_seed(0)
    return M(cfg, Vocab.synthetic(4232)).to(DEV).eval()


def run_sessions(torch, model, parser, blocks, ticks, read_tokens=False, **kw):
    """tools/sessions_bench.py's run_sessions: ms of the ticks in which every slot is open and past its first block.  read_tokens: the
    tick also reads every slot's tokens(b), as a caption display would."""
    ss = model.sessions(SLOTS, parser=parser, **kw)
    block = blocks[0].shape[1]
    fed, out = [0] * SLOTS, []
    for tick in range(ticks):
        for b in range(SLOTS):
            if tick == b % STAGGER:
                ss.open(b)
        live = [ss.state[b] == "open" and fed[b] < BLOCKS for b in range(SLOTS)]
        ns = [block if l else 0 for l in live]
        fin = [l and fed[b] == BLOCKS - 1 for b, l in enumerate(live)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ss.push_audio(blocks[tick % BLOCKS], ns, fin)
        if read_tokens:
            for b in range(SLOTS):
                ss.tokens(b)
        ms = (time.perf_counter() - t0) * 1e3
        if all(live) and min(fed) >= 1:
            out.append(ms)
        fed = [f + int(l) for f, l in zip(fed, live)]
    return out


def run_transcribe(torch, model, pack, iters, **kw):
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.transcribe(pack, beam_size=5, **kw)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_durations(path):
    """name -> {launches, median_us, max_us, total_us} in a rocprofv3 kernel-trace CSV of a --trace-run: frame_stats_kernel runs on the
    tick's 512 frames (the median) and twice on transcribe's 8192 (the maximum)."""
    rec = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            for k in KERNELS:
                if k in name and not (k == "session_ctc_step_kernel" and "tokens" in name):
                    rec.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "median_us": round(statistics.median(v), 2), "max_us": round(max(v), 2), "total_us": round(sum(v), 1)} for k, v in rec.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-csv", default="")
    ap.add_argument("--parent-json", default="")
    ap.add_argument("--package-root", default="")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root) if a.package_root else ROOT)
    import numpy as np
    import torch
    from asr_chinese_e2e_amd.Utils import Pack
    med = lambda v: round(statistics.median(v), 3)      # noqa: E731
    model, parser = build(torch, np)
    block = C * LFR_N * 160
    wav = torch.randn(SLOTS, block * BLOCKS, device=DEV) * 0.1
    blocks = [wav[:, k * block:(k + 1) * block].contiguous() for k in range(BLOCKS)]
    if a.plain_only:
        run_sessions(torch, model, parser, blocks, BLOCKS)
        rounds = [med(run_sessions(torch, model, parser, blocks, BLOCKS)) for _ in range(a.rounds)]
        res = {"device": torch.cuda.get_device_name(0), "sessions_tick_ms_rounds": rounds, "sessions_tick_ms": med(rounds)}
    else:
        ctc = build_ctc(torch)
        pack = Pack(wave=torch.randn(16, 512, N_MELS * LFR_M, device=DEV).to(torch.bfloat16), wave_len=torch.full((16,), 512, dtype=torch.int32, device=DEV))
        if a.trace_run:
            run_sessions(torch, model, parser, blocks, STAGGER + 12, timed=True)
            run_sessions(torch, model, parser, blocks, STAGGER + 12)
            run_transcribe(torch, ctc, pack, 2, confidence="post_max")
            torch.cuda.synchronize()
            return
        run_sessions(torch, model, parser, blocks, BLOCKS)      # warm every cache size, the allocator and the engine
        run_sessions(torch, model, parser, blocks, BLOCKS, timed=True)
        run_transcribe(torch, ctc, pack, 2)
        run_transcribe(torch, ctc, pack, 2, confidence="post_max")
        rounds = []
        for _ in range(a.rounds):
            p, t = run_sessions(torch, model, parser, blocks, BLOCKS), run_sessions(torch, model, parser, blocks, BLOCKS, timed=True)
            r = run_sessions(torch, model, parser, blocks, BLOCKS, read_tokens=True, timed=True)
            o, c = run_transcribe(torch, ctc, pack, 5), run_transcribe(torch, ctc, pack, 5, confidence="post_max")
            rounds.append({"tick_ms": med(p), "tick_timed_ms": med(t), "tick_timed_read_tokens_ms": med(r), "transcribe_ms": med(o), "transcribe_confidence_ms": med(c), "ticks": [len(p), len(t)]})
        m = {k: med([r[k] for r in rounds]) for k in ("tick_ms", "tick_timed_ms", "tick_timed_read_tokens_ms", "transcribe_ms", "transcribe_confidence_ms")}
        n_tok = [len(r["tokens"]) for r in ctc.transcribe(pack, beam_size=5, confidence="post_max")]
        res = {"device": torch.cuda.get_device_name(0), "C": C, "slots": SLOTS, "V": 4232, "block_audio_ms": block / 16.0, "transcribe_shape": [16, 512],
               "transcribe_tokens_per_utterance": round(sum(n_tok) / len(n_tok), 1),
               "rounds": rounds, "median_of_rounds": m, "timed_over_plain": round(m["tick_timed_ms"] / m["tick_ms"], 3),
               "confidence_over_plain_transcribe": round(m["transcribe_confidence_ms"] / m["transcribe_ms"], 3)}
        if a.parent_json:
            with open(a.parent_json) as f:
                parent = json.load(f)
            res["parent_commit_tick_ms"] = parent["sessions_tick_ms"]
            res["plain_tick_over_parent"] = round(m["tick_ms"] / parent["sessions_tick_ms"], 3)
        if a.kernels_csv:
            res["kernels"] = kernel_durations(a.kernels_csv)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
