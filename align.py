#!/usr/bin/env python3
"""align.py - a long recording and its script in, timed lines and training utterances out.

    python align.py --model_name=TransformerOffical --ctc_weight=0.3 --ckpt=ckpt/exp/model.model --vocab_path=Predictor/vocab.t \
        --wav=lecture.wav --text=lecture.txt --out_prefix=data/lecture --part=train

Model flags are train.py's (same parser as transcribe.py); the model needs the CTC head.  Alignment flags:
  --ckpt, --vocab_path, --cmvn, --frontend, --resample, --batch_size     as transcribe.py's
  --wav            one 16-bit PCM WAV file: the whole recording
  --text           a UTF-8 file with one transcript line per text line (whitespace inside a line is removed; characters outside the
                   vocabulary become the unknown id and are counted in the line's "unk")
  --confidence     post_mean (default), post_max or post_min: the measure reported as every token's "confidence"
  --min_confidence lines with a confidence (exp of the mean log posterior over the line's frames) below it are not written (default 0.0)
  --out_prefix     PFX: every kept line's audio is written as 16-bit PCM PFX_<k>.wav (k = the line's index in --text; the file's own
                   samples at its own rate) and {"wave", "tgt"} lines are appended to PFX_<part>.json, the collector format
                   build_dataloader reads - the output can go straight into train.py.  Kept: lines with tokens whose recording could be
                   aligned and whose confidence is at least --min_confidence
  --part           train (default), dev or test: the collector file's part
  --filler         PENALTY (nats, >= 0; default: off): audio the script does not cover (a spoken title, an advertisement, an ad-lib) may
                   rest in filler frames in front of a line and behind the last one, where the blank lies more than PENALTY below the
                   frame's best class (model.align_long's filler).  One JSON line {"filler": true, "start_s", "end_s", "frames",
                   "before_line"} per run of such frames is printed after the transcript lines; the wav cuts stay a line's own tokens
  --filler_scope   lines (default: in front of every line) or tokens (in front of every token); needs --filler
  --vad_energy_threshold, --vad_energy_mean_scale, --vad_frames_context, --vad_proportion_threshold, --min_silence_s, --min_speech_s,
  --pad_s, --max_segment_s      the VAD's and the segmenter's options, as transcribe.py --long=1
The recording is cut at its pauses by the energy VAD, its segments go through the CTC head, and one launch aligns the whole script (at most
8192 tokens) to their frames (model.align_long).  One JSON line per transcript line is printed: {"file", "line", "text", "ids", "start_s",
"end_s", "start_sample", "end_sample", "logp", "frames", "confidence", "min_confidence", "unk", "kept", "tokens"}, times being the extents
of the aligned frames on the recording's axis (not frame centres) and never past its end; then the recording's summary {"file",
"duration_s", "score", "frames", "lines", "kept", "segments"}.  A script that does not fit the frames gives null times and keeps nothing.
"""
import json
import os
import sys
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab  # noqa: E402
from asr_chinese_e2e_amd.data_handler.loader import parser_norm, pcm_to_float, read_pcm  # noqa: E402
from asr_chinese_e2e_amd.data_handler import resample as resample_mod  # noqa: E402
from train import TrainConfig, get_model_class, parse_flags  # noqa: E402
from transcribe import SEGMENT_FLAGS, VAD_FLAGS, _finite, cmvn_path, load_model  # noqa: E402

CLI_KEYS = ("ckpt", "wav", "text", "cmvn", "frontend", "resample", "batch_size", "confidence", "min_confidence", "out_prefix", "part", "filler",
            "filler_scope") + tuple(VAD_FLAGS) + SEGMENT_FLAGS


def align_options(cli):
    """The flags that can be judged before a model is loaded -> (EnergyVad, the segmenter's keywords, min_confidence, confidence, part);
    SystemExit for what is missing or refused."""
    from asr_chinese_e2e_amd.confidence import BEAM_MEASURES
    from asr_chinese_e2e_amd.vad import EnergyVad, segment_frames
    for k in ("wav", "text"):
        if cli.get(k) in (None, "", False):
            raise SystemExit(f"align.py: give --{k}=<file>")
    seg = {k: cli[k] for k in SEGMENT_FLAGS if k in cli}
    try:
        vad = EnergyVad(**{VAD_FLAGS[k]: cli[k] for k in VAD_FLAGS if k in cli})
        segment_frames(**seg)
    except (TypeError, ValueError) as e:
        raise SystemExit(f"align.py: {e}") from e
    try:
        min_conf = float(cli.get("min_confidence", 0.0))
    except (TypeError, ValueError):
        min_conf = float("nan")
    if not 0.0 <= min_conf <= 1.0:
        raise SystemExit(f"align.py: --min_confidence must lie in [0, 1] (got {cli.get('min_confidence')!r})")
    conf = str(cli.get("confidence", "post_mean") or "post_mean")
    if conf not in BEAM_MEASURES:
        raise SystemExit(f"align.py: --confidence must be one of {', '.join(BEAM_MEASURES)} (got {conf!r})")
    part = str(cli.get("part", "train") or "train")
    if part not in ("train", "dev", "test"):
        raise SystemExit(f"align.py: --part must be train, dev or test (got {part!r})")
    return vad, seg, min_conf, conf, part


def filler_options(cli):
    """--filler / --filler_scope -> the keywords model.align_long takes for them ({} when the filler is off); SystemExit naming the flag
    for a penalty that is no finite number >= 0, an unknown scope, or a scope without a penalty."""
    from asr_chinese_e2e_amd.align_long import FILLER_SCOPES
    filler, scope = cli.get("filler"), cli.get("filler_scope")
    if scope is not None and scope not in FILLER_SCOPES:
        raise SystemExit(f"align.py: --filler_scope must be one of {', '.join(FILLER_SCOPES)} (got {scope!r})")
    if filler is None:
        if scope is not None:
            raise SystemExit(f"align.py: --filler_scope={scope} needs --filler=PENALTY")
        return {}
    if isinstance(filler, bool) or not isinstance(filler, (int, float)) or not np.isfinite(filler) or filler < 0:
        raise SystemExit(f"align.py: --filler must be a finite penalty >= 0 in nats (got {filler!r})")
    return {"filler": float(filler), "filler_scope": scope or "lines"}


def filler_lines(res):
    """One JSON line per filler run of align_long's result (none without --filler), times never past the recording's end."""
    return [{"filler": True, "start_s": min(f["start_s"], res["duration_s"]), "end_s": min(f["end_s"], res["duration_s"]), "frames": f["frames"],
             "before_line": f["before_line"]} for f in res.get("fillers", ())]


def read_lines(path):
    """The transcript: one line per text line, empty lines dropped."""
    with open(path, encoding="utf-8") as f:
        return [l.strip() for l in f if l.strip()]


def result_lines(path, n_samples, sr, res, min_conf):
    """The JSON lines of one recording from align_long's result: one per transcript line, then the summary.  A line is kept when it has
    times and its confidence is at least min_conf; its samples are [start_sample, end_sample) of the file at its own rate sr."""
    lines, at, kept = [], 0, 0
    for k, l in enumerate(res["lines"]):
        toks = res["tokens"][at:at + len(l["ids"])]
        at += len(l["ids"])
        line = {"file": path, "line": k}
        line.update({key: _finite(v) for key, v in l.items()})
        line.update(start_sample=None, end_sample=None, kept=False, tokens=toks)
        if l["start_s"] is not None:
            a, b = min(int(round(l["start_s"] * sr)), n_samples), min(int(round(l["end_s"] * sr)), n_samples)
            line.update(start_sample=a, end_sample=b, end_s=min(l["end_s"], res["duration_s"]), kept=bool(b > a and l["confidence"] >= min_conf))
            for t in toks:
                t["end_s"] = min(t["end_s"], res["duration_s"])
        kept += line["kept"]
        lines.append(line)
    return lines + [{"file": path, "duration_s": res["duration_s"], "score": _finite(res["score"]), "frames": res["frames"], "lines": len(res["lines"]),
                     "kept": kept, "segments": [list(s) for s in res["segments"]]}]


def write_collector(out_prefix, part, lines, pcm, ch, sr):
    """Every kept line's samples as PFX_<k>.wav (16-bit PCM, the file's channels and rate) and its {"wave", "tgt"} line appended to
    PFX_<part>.json.  pcm: the file's interleaved int16 samples.  Returns the wav paths."""
    paths = []
    d = os.path.dirname(out_prefix)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(f"{out_prefix}_{part}.json", "a", encoding="utf-8") as man:
        for l in lines:
            if not l.get("kept"):
                continue
            p = f"{out_prefix}_{l['line']}.wav"
            with wave.open(p, "wb") as w:
                w.setnchannels(ch)
                w.setsampwidth(2)
                w.setframerate(sr)
                w.writeframes(np.ascontiguousarray(pcm[l["start_sample"] * ch:l["end_sample"] * ch], dtype="<i2").tobytes())
            man.write(json.dumps({"wave": p, "tgt": l["text"]}, ensure_ascii=False) + "\n")
            paths.append(p)
    return paths


def align_file(model, parser, path, texts, vad, seg_kw, bs, resample, sample_rate, conf, min_conf, out_prefix, part, fill_kw=None):
    pcm, ch, sr = read_pcm(path)
    if sr != sample_rate:
        if not resample:
            raise SystemExit(f"align.py: {path}: sample rate {sr}, the model expects {sample_rate}")
        try:
            resample_mod.plan(sr)
        except ValueError as e:
            raise SystemExit(f"align.py: {path}: {e}") from e
    n = pcm.size // ch
    x = np.empty(n, dtype=np.float32)
    pcm_to_float(pcm, ch, x)
    wav = torch.from_numpy(x.reshape(1, -1)) if n else torch.zeros(1, 1)
    try:
        res = model.align_long(parser, wav, [n], [texts], vad=vad, batch_size=bs, source_rate=sr if sr != sample_rate else None, confidence=conf, **seg_kw,
                               **(fill_kw or {}))[0]
    except ValueError as e:
        raise SystemExit(f"align.py: {e}") from e
    lines = result_lines(path, n, sr, res, min_conf)
    for line in lines[:-1] + filler_lines(res) + lines[-1:]:      # the transcript lines, the filler runs, the summary
        print(json.dumps(line, ensure_ascii=False), flush=True)
    if out_prefix:
        write_collector(str(out_prefix), part, lines[:-1], pcm, ch, sr)
    return lines


def align(**flags):
    cli = {k: flags.pop(k) for k in CLI_KEYS if k in flags}
    vad, seg_kw, min_conf, conf, part = align_options(cli)
    fill_kw = filler_options(cli)
    texts = read_lines(str(cli["text"]))
    config = TrainConfig()
    config.fn_build(flags)
    Model, ModelConfig = get_model_class(config.model_name)
    config.fn_combine(ModelConfig())
    config.fn_build(flags)
    if not torch.cuda.is_available():
        raise SystemExit("align.py needs an MI355X: the alignment path has no CPU fallback")
    vocab = Vocab.load(config.vocab_path)
    model = load_model(config, vocab, cli.get("ckpt"))
    if not model.use_ctc:
        raise SystemExit("align.py: the model has no CTC head (--ctc_weight=0): alignment comes from it")
    parser = AudioParser(sample_rate=config.sample_rate, n_mels=config.n_mels, window_size=config.window_size,
                         lfr_m=config.lfr_m, lfr_n=config.lfr_n, frontend=str(cli.get("frontend", "reference")), **parser_norm(cmvn_path(cli)))
    out_prefix = cli.get("out_prefix") if cli.get("out_prefix") not in (None, "", False) else None
    align_file(model, parser, str(cli["wav"]), texts, vad, seg_kw, max(1, int(cli.get("batch_size", 16))), bool(int(cli.get("resample", 0) or 0)),
               config.sample_rate, conf, min_conf, out_prefix, part, fill_kw)


if __name__ == "__main__":
    align(**parse_flags(sys.argv[1:]))
