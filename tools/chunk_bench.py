#!/usr/bin/env python3
"""Chunk-masked encoder attention: what the mask costs or saves, one JSON object on stdout.

  python tools/chunk_bench.py [--reps 50] [--steps 20] [--warmup 5] [--skip-attention] [--skip-step] [--skip-stream] [--skip-stream-search]

* attention: sdpa_fwd / sdpa_bwd us at the headline head shape (B = 32, H = 8, T = 500, dk = 64, bf16, every key valid), full
  attention against chunk C = 16 with unlimited and with 4 chunks of left context (device events, median of --reps after a warm-up of
  every shape);
* step: the joint training step (bench.py's configs[2] shapes: B = 32, T = 500, 6 layers, vocab 4232, bf16, dropout 0) with
  chunk_size = 0, 16 and -1 (dynamic), the three models alternated in ONE process in rounds of --warmup untimed + --steps timed steps;
* stream: model.stream(B).push() latency per chunk of C = 16 frames at B = 1 and B = 32 (host wall time: push returns the chunk's
  greedy CTC ids, so it synchronises), unlimited left context, over a 496-frame utterance;
* stream_search: the same push with search="greedy" against search="prefix_beam" (beam 5, 10 classes per frame: asr_ctc_frame_topk +
  asr_ctc_prefix_beam_chunk instead of the argmax), the two streams alternated in ONE process, three rounds, median over the chunks of
  each round.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd import kernels as K  # noqa: E402

DEV = "cuda"


def time_us(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def attention(reps):
    B, H, T, dk = 32, 8, 500, 64
    d = H * dk
    torch.manual_seed(0)
    g = torch.randn(B * T, 3 * d, device=DEV).bfloat16()
    q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
    do = torch.randn(B * T, d, device=DEV).bfloat16()
    klen = torch.full((B,), T, dtype=torch.int32, device=DEV)
    dg = torch.empty_like(g)
    out = {}
    for name, kw in (("full", {}), ("C16_left-1", dict(chunk=16, left_chunks=-1)), ("C16_left4", dict(chunk=16, left_chunks=4))):
        o, lse = K.sdpa_fwd(q, k, v, klen, B, H, T, T, dk, **kw)
        fwd = time_us(lambda: K.sdpa_fwd(q, k, v, klen, B, H, T, T, dk, o=o, lse=lse, **kw), reps)
        bwd = time_us(lambda: K.sdpa_bwd(q, k, v, o, do, lse, klen, B, H, T, T, dk, dg[:, :d], dg[:, d:2 * d], dg[:, 2 * d:], **kw), reps)
        out[name] = {"fwd_us": round(fwd, 2), "bwd_us": round(bwd, 2)}
    return out


def joint_model(chunk, B=32, T=500, V=4232):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab, synthetic_pack
    from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, layer_num=6, ctc_weight=0.3, dtype="bf16", warm_up=4000, chunk_size=chunk))
    torch.manual_seed(0)
    model = M(cfg, Vocab.synthetic(V)).to(DEV)
    opt = NoamOpt(cfg.d_model, 1, cfg.warm_up, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
    pack = synthetic_pack(B, T, 80, V, seed=1234, device=DEV, dtype=torch.bfloat16)
    return model, opt, pack


def step(steps, warmup, rounds=3):
    runs = {c: joint_model(c) for c in (0, 16, -1)}
    times = {c: [] for c in runs}
    for _ in range(rounds):
        for c, (model, opt, pack) in runs.items():
            for _ in range(warmup):
                model.iterate(pack, optimizer=opt, is_train=True)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                model.iterate(pack, optimizer=opt, is_train=True)
            b.record()
            torch.cuda.synchronize()
            times[c].append(a.elapsed_time(b) / steps)
    names = {0: "chunk_size=0", 16: "chunk_size=16", -1: "chunk_size=-1"}
    return {names[c]: {"ms_per_step": round(statistics.median(t), 3), "rounds_ms": [round(x, 3) for x in t]} for c, t in times.items()}


def stream(C=16, T=496):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, layer_num=6, ctc_weight=0.3, dtype="bf16", chunk_size=C))
    torch.manual_seed(0)
    model = M(cfg, Vocab.synthetic(4232)).to(DEV).eval()
    out = {}
    for B in (1, 32):
        feats = torch.randn(B, T, 80, device=DEV).bfloat16()
        for _ in range(2):      # the first pass warms every cache size the second one meets
            st = model.stream(B)
            lat = []
            for c0 in range(0, T, C):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st.push(feats[:, c0:c0 + C].contiguous(), [C] * B)
                lat.append((time.perf_counter() - t0) * 1e3)
        out[f"B={B}"] = {"chunks": len(lat), "median_ms": round(statistics.median(lat), 3), "first_ms": round(lat[0], 3),
                         "last_ms": round(lat[-1], 3), "max_ms": round(max(lat), 3)}
    return out


def stream_search(C=16, T=496, rounds=3):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, layer_num=6, ctc_weight=0.3, dtype="bf16", chunk_size=C))
    torch.manual_seed(0)
    model = M(cfg, Vocab.synthetic(4232)).to(DEV).eval()
    modes = {"greedy": dict(search="greedy"), "prefix_beam": dict(search="prefix_beam", beam_size=5, frame_topk=10)}
    out = {}
    for B in (1, 32):
        feats = torch.randn(B, T, 80, device=DEV).bfloat16()
        med = {m: [] for m in modes}
        for r in range(rounds + 1):      # round 0 warms every cache size and is not reported
            for m, kw in modes.items():
                st = model.stream(B, **kw)
                lat = []
                for c0 in range(0, T, C):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    st.push(feats[:, c0:c0 + C].contiguous(), [C] * B)
                    lat.append((time.perf_counter() - t0) * 1e3)
                if r > 0:
                    med[m].append(statistics.median(lat))
        out[f"B={B}"] = {m: {"median_ms": round(statistics.median(v), 3), "rounds_ms": [round(x, 3) for x in v]} for m, v in med.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-stream", action="store_true")
    ap.add_argument("--skip-attention", action="store_true")
    ap.add_argument("--skip-stream-search", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_attention:
        res["attention_B32_H8_T500_dk64_bf16"] = attention(a.reps)
    if not a.skip_step:
        res["joint_step_B32_T500"] = step(a.steps, a.warmup)
    if not a.skip_stream:
        res["stream_push_C16"] = stream()
    if not a.skip_stream_search:
        res["stream_push_C16_search"] = stream_search()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
