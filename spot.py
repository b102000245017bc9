#!/usr/bin/env python3
"""spot.py - audio files and a list of phrases in, one JSON line per place a phrase is spoken out.

    python spot.py --model_name=TransformerOffical --ctc_weight=0.3 --ckpt=ckpt/exp/model.model --vocab_path=Predictor/vocab.t \
        --keywords=phrases.txt --wavs=a.wav,b.wav

Model flags are train.py's (same parser as transcribe.py); the model needs the CTC head.  Spotting flags:
  --ckpt, --vocab_path, --cmvn, --frontend, --resample, --batch_size, --wavs, --manifest     as transcribe.py's
  --keywords       a UTF-8 file with one phrase per line (1 to 16 characters of the vocabulary; whitespace inside a phrase is removed),
                   optionally a tab and the phrase's own threshold behind it; duplicate lines are kept
  --threshold      the default threshold p in (0, 1] (0.5): a phrase is reported where the geometric mean of its characters' posteriors
                   along its best alignment reaches p
  --max_token_s    a match may last at most this long per character (0.5)
  --hits           the hits kept per file (or segment) and phrase (8); what is found beyond is counted in the file's "dropped"
  --long           1 = the files are whole recordings: each is cut at its pauses by the energy VAD (model.spot_long) and the hits carry
                   times on the recording's axis and their "segment"; the VAD's and the segmenter's flags as transcribe.py --long=1
One JSON line per hit is printed, in the order of the hits' ends: {"file", "keyword", "phrase", "ids", "start_s", "end_s", "start_frame",
"end_frame", "score", "confidence"} - start_s is the END of the first character's frames (the search enters a phrase on the last frame
of its first character), end_s the end of the frame the last character's score peaked on, never past the audio's end; then the file's
summary {"file", "duration_s", "hits", "dropped"}.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab, load_wav  # noqa: E402
from asr_chinese_e2e_amd.data_handler.loader import parser_norm  # noqa: E402
from asr_chinese_e2e_amd.data_handler import resample as resample_mod  # noqa: E402
from asr_chinese_e2e_amd.Utils import Pack  # noqa: E402
from train import TrainConfig, get_model_class, parse_flags  # noqa: E402
from transcribe import SEGMENT_FLAGS, VAD_FLAGS, audio_files, cmvn_path, load_model  # noqa: E402

CLI_KEYS = ("ckpt", "wavs", "manifest", "keywords", "threshold", "max_token_s", "hits", "long", "cmvn", "frontend", "resample", "batch_size") + tuple(VAD_FLAGS) + SEGMENT_FLAGS


def spot_options(cli):
    """The flags that can be judged before a model is loaded -> (keyword list arguments, None or (EnergyVad, the segmenter's keywords));
    SystemExit for what is missing or refused."""
    if cli.get("keywords") in (None, "", False, True):
        raise SystemExit("spot.py: give --keywords=<file with one phrase per line>")
    if not cli.get("wavs") and not cli.get("manifest"):
        raise SystemExit("spot.py: give --wavs=a.wav,b.wav or --manifest=<collector json>")
    kw = {}
    for flag, name, default in (("threshold", "threshold", 0.5), ("max_token_s", "max_token_s", 0.5), ("hits", "hits_per_keyword", 8)):
        v = cli.get(flag, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
            raise SystemExit(f"spot.py: --{flag} must be a number (got {v!r})")
        kw[name] = v
    if not 0.0 < kw["threshold"] <= 1.0:
        raise SystemExit(f"spot.py: --threshold must be a probability in (0, 1] (got {kw['threshold']!r})")
    if not kw["max_token_s"] > 0.0:
        raise SystemExit(f"spot.py: --max_token_s must be positive (got {kw['max_token_s']!r})")
    if int(kw["hits_per_keyword"]) != kw["hits_per_keyword"] or not 1 <= kw["hits_per_keyword"] <= 64:
        raise SystemExit(f"spot.py: --hits must be an integer in [1, 64] (got {kw['hits_per_keyword']!r})")
    kw["hits_per_keyword"] = int(kw["hits_per_keyword"])
    long_form = bool(int(cli.get("long", 0) or 0))
    given = [k for k in tuple(VAD_FLAGS) + SEGMENT_FLAGS if k in cli]
    if not long_form:
        if given:
            raise SystemExit(f"spot.py: --{given[0]} applies to --long=1")
        return kw, None
    from asr_chinese_e2e_amd.vad import EnergyVad, segment_frames
    seg = {k: cli[k] for k in SEGMENT_FLAGS if k in cli}
    try:
        vad = EnergyVad(**{VAD_FLAGS[k]: cli[k] for k in VAD_FLAGS if k in cli})
        segment_frames(**seg)
    except (TypeError, ValueError) as e:
        raise SystemExit(f"spot.py: {e}") from e
    return kw, (vad, seg)


def hit_lines(path, duration_s, res):
    """The JSON lines of one file from spot_keywords' / spot_long's result for it: one per hit, then the summary."""
    lines = [dict({"file": path}, **dict(h, end_s=min(h["end_s"], duration_s))) for h in res["hits"]]
    return lines + [{"file": path, "duration_s": duration_s, "hits": len(res["hits"]), "dropped": res["dropped"]}]


def read_checked(path, sample_rate, resample):
    pcm, sr = load_wav(path)
    if sr != sample_rate:
        if not resample:
            raise SystemExit(f"spot.py: {path}: sample rate {sr}, the model expects {sample_rate}")
        try:
            resample_mod.plan(sr)
        except ValueError as e:
            raise SystemExit(f"spot.py: {path}: {e}") from e
    return pcm, sr


def spot_files(model, parser, files, keywords, bs, resample, sample_rate, long_form=None):
    """Prints every file's lines; utterances go --batch_size at a time through model.spot_keywords, recordings one by one through
    model.spot_long."""
    for i in range(0, len(files), 1 if long_form else bs):
        chunk = files[i:i + (1 if long_form else bs)]
        loaded = [read_checked(p, sample_rate, resample) for p in chunk]
        waves, rates = [w for w, _ in loaded], [r for _, r in loaded]
        S = max(1, max(len(w) for w in waves))
        wav = np.zeros((len(waves), S), dtype=np.float32)
        for b, w in enumerate(waves):
            wav[b, : len(w)] = w
        wav, wav_len = torch.from_numpy(wav), [len(w) for w in waves]
        if long_form:
            try:
                out = model.spot_long(parser, wav, wav_len, keywords, vad=long_form[0], batch_size=bs, source_rate=rates[0] if rates[0] != sample_rate else None,
                                      **long_form[1])
            except ValueError as e:
                raise SystemExit(f"spot.py: --long=1: {e}") from e
        else:
            wav_len = torch.tensor(wav_len, dtype=torch.int32)
            if any(r != sample_rate for r in rates):
                wav, wav_len, _ = resample_mod.resample_batch(wav.cuda(), wav_len.tolist(), rates)
            feats, flen = parser.parse_batch(wav.cuda(), torch.as_tensor(wav_len, dtype=torch.int32).cuda())
            out = model.spot_keywords(Pack(wave=feats, wave_len=flen), keywords)
        for path, w, sr, r in zip(chunk, waves, rates, out):
            for line in hit_lines(path, len(w) / float(sr), r):
                print(json.dumps(line, ensure_ascii=False), flush=True)


def spot(**flags):
    cli = {k: flags.pop(k) for k in CLI_KEYS if k in flags}
    kw, long_form = spot_options(cli)
    config = TrainConfig()
    config.fn_build(flags)
    Model, ModelConfig = get_model_class(config.model_name)
    config.fn_combine(ModelConfig())
    config.fn_build(flags)
    vocab = Vocab.load(config.vocab_path)
    from asr_chinese_e2e_amd.keywords import KeywordList
    try:
        keywords = KeywordList.from_file(str(cli["keywords"]), vocab, **kw)
    except (OSError, ValueError) as e:
        raise SystemExit(f"spot.py: --keywords: {e}") from e
    if not torch.cuda.is_available():
        raise SystemExit("spot.py needs an MI355X: the search has no CPU fallback")
    model = load_model(config, vocab, cli.get("ckpt"))
    if not model.use_ctc:
        raise SystemExit("spot.py: the model has no CTC head (--ctc_weight=0): the posteriors come from it")
    parser = AudioParser(sample_rate=config.sample_rate, n_mels=config.n_mels, window_size=config.window_size,
                         lfr_m=config.lfr_m, lfr_n=config.lfr_n, frontend=str(cli.get("frontend", "reference")), **parser_norm(cmvn_path(cli)))
    spot_files(model, parser, audio_files(cli), keywords, max(1, int(cli.get("batch_size", 16))), bool(int(cli.get("resample", 0) or 0)),
               config.sample_rate, long_form)


if __name__ == "__main__":
    spot(**parse_flags(sys.argv[1:]))
