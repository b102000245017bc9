#!/usr/bin/env python3
"""Streaming waveform front end: what push_audio of one chunk's worth of audio costs, one JSON object on stdout.

  python tools/stream_frontend_bench.py [--reps 50] [--frontend reference|kaldi|both]

C = 16, LFR 4/3, n_mels = 80 (one chunk = 16 * 3 * 160 = 7680 samples = 0.48 s of audio), the 6-layer bf16 joint model of
tools/chunk_bench.py with a 320-wide input, B = 1 and B = 32, over a 31-chunk utterance, host wall time per call as in
tools/chunk_bench.py's stream leg (a push returns the chunk's greedy CTC ids, so it synchronises; the front end alone is
synchronised for the measurement):
* frontend_ms:   StreamingFrontEnd.push_audio of one block (append, log-mel of the new frames, normalise + stack);
* push_ms:       StreamingEncoder.push of the chunk it returned;
* push_audio_ms: StreamingEncoder.push_audio of the block, i.e. both;
* push_alone_ms: StreamingEncoder.push on precomputed features (the figure of tools/chunk_bench.py, at this model's input width);
* parse_batch_5s_us: offline AudioParser.parse_batch of B x 5 s under global CMVN (device events, median of --reps);
* rtf:           push_audio_ms / 480 ms of audio per utterance - the share of real time one session (B = 1) or 32 of them take.
--frontend kaldi measures a parser of Kaldi fbank features instead; both: one object per front end, {"reference": .., "kaldi": ..}.
"""
import argparse
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

from tools.chunk_bench import time_us  # noqa: E402

DEV = "cuda"
C, LFR_M, LFR_N, N_MELS, CHUNKS = 16, 4, 3, 80, 31


def med(v):
    return round(statistics.median(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frontend", choices=("reference", "kaldi", "both"), default="reference")
    a = ap.parse_args()
    if a.frontend == "both":
        print(json.dumps({f: run(a.reps, f) for f in ("reference", "kaldi")}))
    else:
        print(json.dumps(run(a.reps, a.frontend)))


def run(reps, frontend):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import AudioParser, StreamingFrontEnd, Vocab
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, dropout=0.0, layer_num=6, ctc_weight=0.3, dtype="bf16", chunk_size=C))
    torch.manual_seed(0)
    model = M(cfg, Vocab.synthetic(4232)).to(DEV).eval()
    parser = AudioParser(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, device=DEV, norm="global",
                         cmvn=(np.full(N_MELS, -1.0), np.full(N_MELS, 0.4)), frontend=frontend)
    block = C * LFR_N * 160
    res = {"device": torch.cuda.get_device_name(0), "C": C, "lfr": [LFR_M, LFR_N], "n_mels": N_MELS, "block_samples": block,
           "block_audio_ms": block / 16.0, "frontend": frontend}
    for B in (1, 32):
        wav = torch.randn(B, block * CHUNKS, device=DEV)
        blocks = [wav[:, k * block:(k + 1) * block].contiguous() for k in range(CHUNKS)]
        ns, open_ = [block] * B, [False] * B
        for _ in range(2):      # the first pass warms every cache size the second one meets
            fe, st = StreamingFrontEnd(parser, B, C, dtype=torch.bfloat16), model.stream(B)
            t_fe, t_push, chunks = [], [], []
            for x in blocks:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fe.push_audio(x, ns, open_)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for feats, nv in out:
                    st.push(feats, nv)
                t2 = time.perf_counter()
                t_fe.append((t1 - t0) * 1e3)
                if out:
                    t_push.append((t2 - t1) * 1e3 / len(out))
                chunks.append(len(out))
            st = model.stream(B, parser=parser)
            t_both = []
            for x in blocks:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st.push_audio(x, ns, open_)
                t_both.append((time.perf_counter() - t0) * 1e3)
            feats = torch.randn(B, C * CHUNKS, LFR_M * N_MELS, device=DEV).bfloat16()
            st = model.stream(B)
            t_alone = []
            for c0 in range(0, C * CHUNKS, C):
                x = feats[:, c0:c0 + C].contiguous()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st.push(x, [C] * B)
                t_alone.append((time.perf_counter() - t0) * 1e3)
        wav5 = torch.randn(B, 80000, device=DEV)
        wl5 = torch.full((B,), 80000, dtype=torch.int32, device=DEV)
        # the first block completes no chunk (a row needs frames past it): steady state is every block after it
        res[f"B={B}"] = {"blocks": CHUNKS, "chunks_per_block": chunks, "frontend_ms": med(t_fe[1:]), "push_ms": med(t_push), "push_audio_ms": med(t_both[1:]),
                         "push_audio_max_ms": round(max(t_both[1:]), 3), "push_alone_ms": med(t_alone),
                         "parse_batch_5s_us": round(time_us(lambda: parser.parse_batch(wav5, wl5, torch.bfloat16), reps), 2),
                         "rtf": round(statistics.median(t_both[1:]) / (block / 16.0), 5)}
    return res


if __name__ == "__main__":
    main()
