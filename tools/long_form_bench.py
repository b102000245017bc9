#!/usr/bin/env python3
"""Long-form transcription: what the energy VAD, the segment gather and the stitching cost.  One JSON object on stdout, merged into --out.

  python tools/long_form_bench.py --part kernels  [--rounds 3] [--out profiles/long_form_bench.json]
  python tools/long_form_bench.py --part longform [--rounds 3] [--out profiles/long_form_bench.json]

The recording is synthetic: 10 minutes at 16 kHz, bursts of uniform noise (amplitude 0.1) of 3 s separated by 0.7 s of near-silence
(amplitude 1e-4): 162 segments of about 3.2 s under the default options.
* --part kernels: HIP events around 20 back-to-back calls of each contender, the contenders alternated in one process over --rounds rounds,
  the median of the rounds: asr_vad_energy, asr_vad_decide (its two launches), asr_segment_gather of the first 16 segments, a
  device-to-device copy of the recording's bytes (what a kernel that only moved the samples would cost), and a torch stand-in for the two
  VAD kernels (unfold, centred sum of squares, log, a cumulative-sum window count).
* --part longform: host wall time of model.transcribe_long on the 6-layer bf16 joint model (V = 4232, random weights, beam 5), beside
  model.transcribe over the same segments cut beforehand on the host; the difference is what VAD, gather and stitching cost; the
  real-time factor is wall time over the recording's duration."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SECONDS, BURST_S, PAUSE_S, CALLS = 600, 3.0, 0.7, 20
N_MELS, LFR_M, LFR_N = 80, 4, 3


def recording(np):
    rng = np.random.RandomState(0)
    n = SECONDS * 16000
    x = 1e-4 * rng.uniform(-1, 1, n)
    period, burst = int((BURST_S + PAUSE_S) * 16000), int(BURST_S * 16000)
    for a in range(int(PAUSE_S * 16000), n - burst, period):
        x[a:a + burst] = 0.1 * rng.uniform(-1, 1, burst)
    return x.astype(np.float32)


def timed(torch, fn):
    """ms per call: HIP events around CALLS back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS


def part_kernels(torch, np, rounds):
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.vad import EnergyVad, num_frames
    x = recording(np)
    wav = torch.from_numpy(x[None]).to(DEV)
    wl = torch.tensor([len(x)], dtype=torch.int32, device=DEV)
    T = num_frames(len(x))
    vad = EnergyVad()
    E = K.vad_energy(wav, wl, T)
    speech, thr = K.vad_decide(E, wl, vad.params(DEV), 0)
    segs = vad.segments(wav, wl)[0]
    part = segs[:16]
    rec, start, n = [0] * len(part), [a for a, _ in part], [b - a for a, b in part]
    out = torch.empty(len(part), max(n), device=DEV)
    dst = torch.empty_like(wav)

    def stand_in():
        f = wav[0].unfold(0, 400, 160) * 32768.0
        e = torch.log(((f - f.mean(dim=1, keepdim=True)) ** 2).sum(dim=1).clamp_min(2.0 ** -23))
        t = 5.0 + 0.5 * e.double().mean()
        c = torch.cat((torch.zeros(1, device=DEV, dtype=torch.int32), (e.double() > t).to(torch.int32).cumsum(0).to(torch.int32)))
        return (c[1:] - c[:-1]).double() >= 0.6

    agree = bool((stand_in().to(torch.uint8) == speech[0]).all())      # reported, not asserted: the stand-in sums in another order
    contenders = {
        "vad_energy_ms": lambda: K.vad_energy(wav, wl, T, E=E),
        "vad_decide_ms": lambda: K.vad_decide(E, wl, vad.params(DEV), 0, speech=speech, thr=thr),
        "segment_gather_16_ms": lambda: K.segment_gather(wav, rec, start, n, max(n), out=out),
        "copy_d2d_ms": lambda: dst.copy_(wav),
        "torch_stand_in_ms": stand_in,
    }
    res = {k: [] for k in contenders}
    for _ in range(rounds):
        for k, fn in contenders.items():
            res[k].append(round(timed(torch, fn), 5))
    med = {k: round(statistics.median(v), 5) for k, v in res.items()}
    return {"recording_s": SECONDS, "samples": len(x), "frames": T, "segments": len(segs), "stand_in_mask_equals_kernels": agree, "bytes": 4 * len(x), "calls_per_round": CALLS, "rounds": res, "median_ms": med,
            "gather_bytes": 4 * sum(n), "vad_ms_per_minute_of_audio": round((med["vad_energy_ms"] + med["vad_decide_ms"]) / (SECONDS / 60.0), 6),
            "vad_energy_over_copy": round(med["vad_energy_ms"] / med["copy_d2d_ms"], 2),
            "note": "segment_gather_16_ms includes the upload of its 48 integers (kernels.segment_gather)"}


def part_longform(torch, np, rounds):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab
    from asr_chinese_e2e_amd.Utils import Pack
    from asr_chinese_e2e_amd.vad import EnergyVad
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, dropout=0.0, layer_num=6, ctc_weight=0.3, dtype="bf16"))
    torch.manual_seed(0)
    model = M(cfg, Vocab.synthetic(4232)).to(DEV).eval()
    parser = AudioParser(n_mels=N_MELS, lfr_m=LFR_M, lfr_n=LFR_N, device=DEV)
    x = recording(np)
    wav = torch.from_numpy(x[None]).to(DEV)
    segs = EnergyVad().segments(wav, [len(x)])[0]
    kw = dict(beam_size=5, joint="rescore")

    def long():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = model.transcribe_long(parser, wav, [len(x)], batch_size=16, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def precut():
        """The same segments, cut beforehand on the host (not timed), through parse_batch and model.transcribe."""
        batches = []
        for i in range(0, len(segs), 16):
            part = segs[i:i + 16]
            b = np.zeros((len(part), max(e - a for a, e in part)), dtype=np.float32)
            for r, (a, e) in enumerate(part):
                b[r, :e - a] = x[a:e]
            batches.append((torch.from_numpy(b).to(DEV), torch.tensor([e - a for a, e in part], dtype=torch.int32, device=DEV)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = []
        for b, n in batches:
            feats, flen = parser.parse_batch(b, n)
            out += model.transcribe(Pack(wave=feats, wave_len=flen), **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    _, a = long()
    _, b = precut()
    same = [s["ids"] for s in a[0]["segments"]] == [r["ids"] for r in b]
    res = {"transcribe_long_s": [], "transcribe_precut_s": []}
    for _ in range(rounds):
        res["transcribe_long_s"].append(round(long()[0], 4))
        res["transcribe_precut_s"].append(round(precut()[0], 4))
    med = {k: round(statistics.median(v), 4) for k, v in res.items()}
    return {"model": "6-layer bf16 joint, V = 4232, random weights, beam 5, joint='rescore', batch_size 16", "segments": len(segs),
            "same_ids_as_precut": same, "rounds": res, "median_s": med,
            "vad_gather_stitch_s": round(med["transcribe_long_s"] - med["transcribe_precut_s"], 4),
            "real_time_factor": round(med["transcribe_long_s"] / SECONDS, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "longform"], required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    res = {"device": torch.cuda.get_device_name(0), a.part: (part_kernels if a.part == "kernels" else part_longform)(torch, np, a.rounds)}
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
