#!/usr/bin/env python3
"""transcribe.py - audio in, text out: the inference entry point the reference's Predictor/predictor.py was meant to be.

    python transcribe.py --model_name=TransformerOffical --ctc_weight=0.3 --ckpt=ckpt/exp/model.model \
        --vocab_path=Predictor/vocab.t --wavs=a.wav,b.wav

Model flags are train.py's (same parser, same TrainConfig / ModelConfig merge, same get_model_class), so the flags a model was
trained with rebuild it.  Inference flags:
  --ckpt         state dict as BaseModel.save writes it (required; a missing file or missing keys are errors);
                 several files, --ckpt=a.model,b.model,c.model, are averaged in memory (average.py writes such a mean to a file)
  --vocab_path   the vocabulary the model was trained with (Vocab.save)
  --wavs         comma-separated 16-bit PCM WAV files, or
  --manifest     a collector manifest (one JSON object {"wave": path, ...} per line)
  --beam_size    beam of the search (default 5)
  --ctc_weight   joint models: weight of the CTC score in the search (default: the model's ctc_weight)
  --joint        joint models: rescore (default; CTC re-ranks the attention beam's n-best list), one_pass (CTC prefix scores
                 take part in every step of the search) or ctc_rescore (the CTC prefix beam search's n-best list re-ranked by one
                 teacher-forced decoder pass)
  --batch_size   utterances per batch (default 16)
  --timestamps   per-character times from the CTC head (default: on when the model has one)
  --stream       1 = run the encoder chunk by chunk (model.stream) under the decoding chunk mask (--decoding_chunk_size /
                 --decoding_left_chunks, or the model's static --chunk_size / --left_chunks): one JSON line
                 {"file", "chunk", "partial"} of greedy CTC text per chunk, then the final line as without it.  With --cmvn the
                 samples themselves are streamed (push_audio, in blocks of --stream_block_samples, default one chunk's worth of
                 audio): the live-audio path.  Without it the features are normalised over the whole utterance first and only
                 the encoder streams: that emulates streaming over files.
  --stream_search  with --stream=1: greedy (default) or prefix_beam - a CTC prefix beam search of --beam_size over the --frame_topk
                 (default 10) best classes of each frame runs with the audio; the per-chunk line becomes {"file", "chunk", "partial",
                 "stable"}: the best hypothesis now (revisable) and the part of it no later chunk can change.  The final line then
                 comes from finish(joint="ctc_rescore"): the decoder re-ranks the streamed n-best (a CTC-only model keeps the CTC best)
  --frontend     reference (default: the reference's log-mel) or kaldi (Kaldi fbank, the features of the Kaldi / WeNet / ESPnet / k2
                 recipes: for models trained with train.py --frontend=kaldi, and CMVN files of those features); token times are frame
                 centres, which for kaldi lie 12.5 ms later than the reference's for the same frame index.
  --cmvn         global CMVN statistics (tools/compute_cmvn.py) the model was trained with (train.py --cmvn); empty = the
                 per-utterance normalisation
  --resample     1 = files at 8, 11.025, 12, 22.05, 24, 32, 44.1, 48, 88.2 or 96 kHz are converted to 16 kHz on the GPU (one launch per
                 batch; with --stream=1 --cmvn a batch whose files share one rate is converted as it streams) and their JSON line
                 gains "source_rate"; 0 (default) = a file at another rate ends the run
  --sessions     N (with --stream=1 and --cmvn): the files go through N independent slots of one batch (model.sessions) instead of
                 batches that advance in lock-step - each file streams at its own pace, and when one finishes the next file takes
                 its slot in the same tick loop.  The same per-chunk lines ("chunk" counts the file's own chunks), the final lines in
                 order of completion.  16 kHz files only.
  --endpoint     1 (with --sessions): the per-chunk lines gain "endpoint": null, or the CTC endpoint rule that fires for the file now
                 (silence_start, silence_after_speech, max_length - WeNet's rules); it only reports, the file streams on
  --context      a UTF-8 file of hotwords, one phrase per line (every character must be in the vocabulary): the CTC prefix beam search
                 prefers hypotheses that spell them (context.ContextGraph, one graph for all files), and the final lines gain "bias".
                 Offline it needs a search that runs the prefix beam search (a CTC-only model, or --joint=ctc_rescore); with --stream=1
                 (--sessions=N included) it needs --stream_search=prefix_beam
  --context_score  the bonus per matched hotword token (default 3.0, WeNet's context_score)
  --lm           an n-gram language model in ARPA format over the vocabulary's characters (orders 1 to 5; lm.NgramLM.from_arpa), or the
                 .npz that NgramLM.save wrote (its weights are the saved ones): shallow fusion in the CTC prefix beam search, and the
                 final lines gain "lm_score".  The same searches as --context admits; not together with --context
  --lm_weight    the LM weight (default 0.3)
  --lm_ins       the bonus per token of a hypothesis (default 0.0)
  --blank_skip   a probability in (0, 1], e.g. 0.98: blank-frame skipping in front of the CTC prefix beam search - a frame whose blank
                 posterior is above it, and whose predecessor's is too, is dropped before the search (the head of every such run stays);
                 scores then sum over the kept frames.  The same searches as --context admits: offline, --long=1, and --stream=1
                 --stream_search=prefix_beam (--sessions=N included)
  --confidence   post_max (WeNet's measure), post_min, post_mean, ent_mean or ent_min: every token of the final lines gains "confidence"
                 (that measure over the token's frames) and "measures" (all five), the line "confidence" (the mean over its tokens);
                 from the CTC posteriors, so it needs the CTC head and timestamps
  --timed        1 (with --stream=1, --sessions=N included; greedy search only): the per-chunk lines gain "tokens", the characters so
                 far with frames, times and confidence (the measure of --confidence, default post_max); the last one may still be
                 open ("final": false)
  --beam_times   1 (with --stream=1 --stream_search=prefix_beam, --sessions=N included; not with --context or --lm): the per-chunk lines
                 gain "tokens", the characters of the best hypothesis now with frames, times and confidence over its best single
                 alignment (the measure of --confidence: post_max, post_min or post_mean); "final": true marks those that can no
                 longer change
  --long         1 = the files are whole recordings (a meeting, a lecture) rather than utterances: each is cut at its pauses by the energy
                 VAD on the GPU (Kaldi's compute-vad-energy; model.transcribe_long), its segments are transcribed in time order,
                 --batch_size at a time, by the search the other flags choose, and one JSON line per segment is printed: {"file",
                 "segment", "start_s", "end_s", "text", "ids", "score", "tokens", ...} with token times on the recording's axis (frame
                 centres, as the final lines'), then the file's final line {"file", "duration_s", "text", "ids", "segments"} with the
                 joined text.  Not with --stream=1: long streaming is what --sessions is for.  --resample=1 as above
  --vad_energy_threshold, --vad_energy_mean_scale, --vad_frames_context, --vad_proportion_threshold
                 the VAD's options under Kaldi's names (defaults 5.0, 0.5, 0, 0.6); with --long=1 only
  --min_silence_s, --min_speech_s, --pad_s, --max_segment_s
                 the segmenter's: pauses shorter than min_silence_s (0.3) do not cut, speech shorter than min_speech_s (0.1) is dropped,
                 every segment is widened by pad_s (0.1) on both sides, a segment longer than max_segment_s (20.0) is cut at the longest
                 pause in its second half; with --long=1 only
Audio goes through load_wav -> AudioParser.parse_batch on the device -> model.transcribe; one JSON line per file is printed:
{"file", "duration_s", "text", "ids", "score", "tokens": [{"id", "token", "start_frame", "end_frame", "start_s", "end_s", "logp"}]}.
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab, load_wav  # noqa: E402
from asr_chinese_e2e_amd.data_handler.loader import parser_norm  # noqa: E402
from asr_chinese_e2e_amd.Utils import Pack  # noqa: E402
from asr_chinese_e2e_amd.data_handler import resample as resample_mod  # noqa: E402
from train import TrainConfig, get_model_class, parse_flags  # noqa: E402

CLI_KEYS = ("ckpt", "wavs", "manifest", "beam_size", "batch_size", "timestamps", "joint", "stream", "cmvn", "stream_block_samples", "resample", "stream_search", "frame_topk", "frontend", "sessions", "endpoint", "context", "context_score", "lm", "lm_weight", "lm_ins", "blank_skip", "confidence", "timed", "beam_times", "long", "vad_energy_threshold", "vad_energy_mean_scale", "vad_frames_context", "vad_proportion_threshold", "min_silence_s", "min_speech_s", "pad_s", "max_segment_s")
VAD_FLAGS = {"vad_energy_threshold": "energy_threshold", "vad_energy_mean_scale": "energy_mean_scale", "vad_frames_context": "frames_context",
             "vad_proportion_threshold": "proportion_threshold"}
SEGMENT_FLAGS = ("min_silence_s", "min_speech_s", "pad_s", "max_segment_s")


def _finite(x):
    return None if isinstance(x, float) and not math.isfinite(x) else x


def load_model(config, vocab, ckpt, device="cuda"):
    """Model of config.model_name with the checkpoint's weights; a missing file or missing keys raise.  `ckpt` may name several files,
    `a.model,b.model,c.model` (or a list): their mean (asr_chinese_e2e_amd.averaging.average_state_dicts), taken in memory."""
    Model, _ = get_model_class(config.model_name)
    paths = [p for p in (ckpt if isinstance(ckpt, (list, tuple)) else str(ckpt or "").split(",")) if p]
    for p in paths or [ckpt]:
        if not p or not os.path.isfile(p):
            raise SystemExit(f"transcribe.py: checkpoint not found: {p!r}")
    if len(paths) > 1:
        from asr_chinese_e2e_amd.averaging import average_state_dicts
        state, ckpt = average_state_dicts(paths), ",".join(paths)
    else:
        ckpt = paths[0]
        state = torch.load(ckpt, map_location="cpu", weights_only=True)
    model = Model(config, vocab)
    missing, unexpected = model.load_state_dict(state, strict=False)
    if missing:
        raise SystemExit(f"transcribe.py: {ckpt} lacks {len(missing)} parameters of {config.model_name} "
                         f"(model flags differ from the training run?): {missing[:5]}")
    if unexpected:
        print(f"transcribe.py: ignoring {len(unexpected)} unexpected keys of {ckpt}: {unexpected[:5]}", file=sys.stderr)
    return model.to(device).eval()


def audio_files(flags):
    if flags.get("wavs"):
        w = flags["wavs"]
        return [p for p in (w if isinstance(w, (list, tuple)) else str(w).split(",")) if p]
    if flags.get("manifest"):
        with open(flags["manifest"], encoding="utf-8") as f:
            return [json.loads(line)["wave"] for line in f if line.strip()]
    raise SystemExit("transcribe.py: give --wavs=a.wav,b.wav or --manifest=<collector json>")


def _shifted(tokens, shift_s):
    """A timed stream's tokens with their times moved to frame centres, as the final lines' are."""
    for t in tokens:
        t["start_s"], t["end_s"] = t["start_s"] + shift_s, t["end_s"] + shift_s
    return tokens


def _chunk_lines(st, files, nv, ids, text, chunk, id2tok, shift_s=0.0):
    """The per-chunk JSON lines of the files that got frames: greedy = the text so far; prefix beam = the best hypothesis now and its
    stable part."""
    part = st.partial() if st.search == "prefix_beam" else None
    spell = lambda seq: "".join(id2tok[t] for t in seq if part is None or t not in (0, 2, 3))      # noqa: E731  (beam mode: as the final text, without pad / sos / eos)
    timed = st.tokens() if st.timed or st.beam_times else None
    for b in range(len(files)):
        if nv[b] <= 0:
            continue
        text[b] += spell(ids[b])
        line = {"file": files[b], "chunk": chunk, "partial": text[b]}
        if part is not None:
            line.update(partial=spell(part[b]["ids"]), stable=text[b])
        if timed is not None:
            line["tokens"] = _shifted(timed[b], shift_s)
        print(json.dumps(line, ensure_ascii=False), flush=True)


def stream_batch(model, files, feats, flen, id2tok, stream_kw=None, shift_s=0.0, **search):
    """model.stream over a batch of feature sequences in chunks of the decoding chunk size: prints the partial text of every
    file after every chunk, returns what model.transcribe returns (finish()).  stream_kw: model.stream's search arguments."""
    B, T, F = feats.shape
    C = model.decoding_chunk_size
    lens = [int(x) for x in flen.tolist()]
    st = model.stream(B, **(stream_kw or {}))
    text = [""] * B
    for i, c0 in enumerate(range(0, T, C)):
        x = feats[:, c0:c0 + C]
        if x.shape[1] < C:
            x = torch.nn.functional.pad(x, (0, 0, 0, C - x.shape[1]))
        nv = [max(0, min(C, n - c0)) for n in lens]
        _chunk_lines(st, files, nv, st.push(x.contiguous(), nv), text, i, id2tok, shift_s)
    return st.finish(**search)


def stream_audio_batch(model, parser, files, wav, wav_len, id2tok, block, source_rate=None, stream_kw=None, shift_s=0.0, **search):
    """model.stream fed with the samples themselves, `block` at a time (wav (B, S) f32 on the host, wav_len list): the same lines as
    stream_batch prints, the same result.  source_rate: the rate of wav when it is not 16 kHz (converted as it streams)."""
    B, S = wav.shape
    st = model.stream(B, parser=parser, source_rate=source_rate, **(stream_kw or {}))
    text, chunk = [""] * B, 0
    for s0 in range(0, max(S, 1), block):
        n = [max(0, min(block, l - s0)) for l in wav_len]
        final = [l <= s0 + block for l in wav_len]
        for nv, ids in st.push_audio_chunks(wav[:, s0:s0 + block].contiguous(), n, final):
            _chunk_lines(st, files, nv, ids, text, chunk, id2tok, shift_s)
            chunk += 1
    return st.finish(**search)


def final_line(path, n_samples, sr, r, shift_s, sample_rate):
    """The JSON line of one finished file from its result dict r (token times moved to frame centres, never past the audio's end)."""
    dur = n_samples / float(sr)
    for t in r["tokens"] or ():          # the last encoder frame may reach past the end of the audio
        for k in ("start_s", "end_s"):
            if t[k] is not None:
                t[k] = min(t[k] + shift_s, dur)
    line = {"file": path, "duration_s": dur, "text": r["text"], "ids": r["ids"],
            "score": _finite(r["score"]), "tokens": r["tokens"]}
    if "bias" in r:
        line["bias"] = r["bias"]
    if "lm_score" in r:
        line["lm_score"] = r["lm_score"]
    if "confidence" in r:
        line["confidence"] = r["confidence"]
    if sr != sample_rate:
        line["source_rate"] = sr
    return line


def stream_sessions(model, parser, files, n_slots, id2tok, block, shift_s, sample_rate, endpoint=False, stream_kw=None, **search):
    """The files through n_slots independent sessions (model.sessions): every tick feeds each open slot its file's next `block`
    samples; a slot whose file has ended is finished, its final line printed, and the next file takes it in the same loop."""
    ss = model.sessions(n_slots, parser=parser, endpoint={} if endpoint else None, **(stream_kw or {}))
    beam_mode = ss.search == "prefix_beam"
    spell = lambda seq: "".join(id2tok[t] for t in seq if not beam_mode or t not in (0, 2, 3))      # noqa: E731  (as _chunk_lines)
    queue = list(files)
    slot = [None] * n_slots      # per slot: {"file", "pcm", "pos", "text", "chunk"}
    while queue or any(slot):
        for b in range(n_slots):
            if slot[b] is None and queue:
                path = queue.pop(0)
                pcm, sr = load_wav(path)
                if sr != sample_rate:
                    raise SystemExit(f"transcribe.py: {path}: sample rate {sr}; --sessions streams {sample_rate} Hz files only")
                slot[b] = dict(file=path, pcm=torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.float32)), pos=0, text="", chunk=0)
                ss.open(b)
        n, final = [0] * n_slots, [False] * n_slots
        wav = torch.zeros(n_slots, block)
        for b, f in enumerate(slot):
            if f is not None:
                n[b] = max(0, min(block, len(f["pcm"]) - f["pos"]))
                wav[b, :n[b]] = f["pcm"][f["pos"]:f["pos"] + n[b]]
                f["pos"] += n[b]
                final[b] = f["pos"] >= len(f["pcm"])
        for nv, ids in ss.push_audio_chunks(wav, n, final):
            ends = ss.endpoints() if endpoint else None
            for b, f in enumerate(slot):
                if f is None or nv[b] <= 0:
                    continue
                f["text"] += spell(ids[b])
                line = {"file": f["file"], "chunk": f["chunk"], "partial": f["text"]}
                if beam_mode:
                    line.update(partial=spell(ss.partial(b)["ids"]), stable=f["text"])
                if endpoint:
                    line["endpoint"] = ends[b]
                if ss.timed or ss.beam_times:
                    line["tokens"] = _shifted(ss.tokens(b), shift_s)
                f["chunk"] += 1
                print(json.dumps(line, ensure_ascii=False), flush=True)
        for b, f in enumerate(slot):
            if f is not None and ss.status(b)["state"] == "ended":
                r = ss.finish(b, **search)
                print(json.dumps(final_line(f["file"], len(f["pcm"]), sample_rate, r, shift_s, sample_rate), ensure_ascii=False), flush=True)
                slot[b] = None


def long_options(cli):
    """--long and its flags -> None without --long=1, else (EnergyVad, the segmenter's keywords).  SystemExit for --long=1 with a streaming
    flag, for a VAD or segmenter flag without --long=1, and for values the VAD or the segmenter refuses - before any model is loaded."""
    from asr_chinese_e2e_amd.vad import EnergyVad, segment_frames
    given = [k for k in tuple(VAD_FLAGS) + SEGMENT_FLAGS if k in cli]
    if not bool(int(cli.get("long", 0) or 0)):
        if given:
            raise SystemExit(f"transcribe.py: --{given[0]} applies to --long=1")
        return None
    for k in ("stream", "sessions"):
        if bool(int(cli.get(k, 0) or 0)):
            raise SystemExit(f"transcribe.py: --long=1 cannot be combined with --{k}: it segments whole recordings offline, long streaming is what "
                             "--stream=1 --sessions=N is for")
    seg = {k: cli[k] for k in SEGMENT_FLAGS if k in cli}
    try:
        vad = EnergyVad(**{VAD_FLAGS[k]: cli[k] for k in VAD_FLAGS if k in cli})
        segment_frames(**seg)
    except (TypeError, ValueError) as e:
        raise SystemExit(f"transcribe.py: --long=1: {e}") from e
    return vad, seg


def segment_lines(path, n_samples, sr, res, shift_s, sample_rate):
    """The JSON lines of one recording from transcribe_long's result: one per segment (token times moved to frame centres, never past the
    recording's end), then the file's final line."""
    lines = []
    for i, seg in enumerate(res["segments"]):
        for t in seg["tokens"] or ():
            for k in ("start_s", "end_s"):
                if t[k] is not None:
                    t[k] = min(t[k] + shift_s, res["duration_s"])
        line = {"file": path, "segment": i}
        line.update({k: (_finite(v) if k == "score" else v) for k, v in seg.items()})
        lines.append(line)
    final = {"file": path, "duration_s": res["duration_s"], "text": res["text"], "ids": res["ids"], "segments": len(res["segments"])}
    if sr != sample_rate:
        final["source_rate"] = sr
    return lines + [final]


def transcribe_long_files(model, parser, files, vad, seg_kw, bs, resample, shift_s, sample_rate, **search):
    """--long=1: every file through model.transcribe_long (which moves the samples to the parser's device), a file at a time."""
    for path in files:
        pcm, sr = load_wav(path)
        if sr != sample_rate:
            if not resample:
                raise SystemExit(f"transcribe.py: {path}: sample rate {sr}, the model expects {sample_rate}")
            try:
                resample_mod.plan(sr)
            except ValueError as e:
                raise SystemExit(f"transcribe.py: {path}: {e}") from e
        wav = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.float32).reshape(1, -1))
        if wav.shape[1] == 0:
            wav = torch.zeros(1, 1)
        try:
            res = model.transcribe_long(parser, wav, [len(pcm)], vad=vad, batch_size=bs, source_rate=sr if sr != sample_rate else None, **seg_kw, **search)[0]
        except ValueError as e:
            raise SystemExit(f"transcribe.py: --long=1: {e}") from e
        for line in segment_lines(path, len(pcm), sr, res, shift_s, sample_rate):
            print(json.dumps(line, ensure_ascii=False), flush=True)


def cmvn_path(cli):
    """The value of --cmvn as a path, or None (absent / empty: per-utterance normalisation)."""
    v = cli.get("cmvn")
    return str(v) if v not in (None, "", False) else None


def transcribe(**flags):
    cli = {k: flags.pop(k) for k in CLI_KEYS if k in flags}
    ctc_weight = flags.get("ctc_weight")          # model flag and decoding weight: the search uses the model's unless given
    long_form = long_options(cli)
    config = TrainConfig()
    config.fn_build(flags)
    Model, ModelConfig = get_model_class(config.model_name)
    config.fn_combine(ModelConfig())
    config.fn_build(flags)
    if not torch.cuda.is_available():
        raise SystemExit("transcribe.py needs an MI355X: the inference path has no CPU fallback")
    vocab = Vocab.load(config.vocab_path)
    model = load_model(config, vocab, cli.get("ckpt"))
    files = audio_files(cli)
    parser = AudioParser(sample_rate=config.sample_rate, n_mels=config.n_mels, window_size=config.window_size,
                         lfr_m=config.lfr_m, lfr_n=config.lfr_n, frontend=str(cli.get("frontend", "reference")), **parser_norm(cmvn_path(cli)))
    shift_s = parser.frame_centre_sample(0) / float(config.sample_rate)      # token times are frame centres: a Kaldi frame's lies 12.5 ms later
    beam = int(cli.get("beam_size", 5))
    bs = max(1, int(cli.get("batch_size", 16)))
    timestamps = bool(cli.get("timestamps", model.use_ctc))
    joint = str(cli.get("joint", "rescore"))
    if joint not in ("rescore", "one_pass", "ctc_rescore"):
        raise SystemExit(f"transcribe.py: --joint must be rescore, one_pass or ctc_rescore (got {joint!r})")
    stream = bool(int(cli.get("stream", 0)))
    stream_search = str(cli.get("stream_search", "greedy"))
    if stream_search not in ("greedy", "prefix_beam"):
        raise SystemExit(f"transcribe.py: --stream_search must be greedy or prefix_beam (got {stream_search!r})")
    if stream_search == "prefix_beam" and not stream:
        raise SystemExit("transcribe.py: --stream_search=prefix_beam applies to --stream=1")
    if stream_search == "prefix_beam" and not model.use_ctc:
        raise SystemExit("transcribe.py: --stream_search=prefix_beam needs a model with the CTC head")
    beam_stream = stream_search == "prefix_beam"
    stream_kw = dict(search="prefix_beam", beam_size=beam, frame_topk=int(cli.get("frame_topk", 10))) if beam_stream else {}
    confidence = cli.get("confidence") if cli.get("confidence") not in (None, "", False, 0) else None
    if confidence is not None:
        from asr_chinese_e2e_amd.confidence import MEASURES
        if str(confidence) not in MEASURES:
            raise SystemExit(f"transcribe.py: --confidence must be one of {', '.join(MEASURES)} (got {confidence!r})")
        confidence = str(confidence)
        if not model.use_ctc or not timestamps:
            raise SystemExit("transcribe.py: --confidence needs a model with the CTC head and timestamps: it is taken over the frames of the CTC alignment")
    if bool(int(cli.get("timed", 0) or 0)):
        if not stream or beam_stream or not model.use_ctc:
            raise SystemExit("transcribe.py: --timed=1 applies to --stream=1 with the greedy search of a model with the CTC head")
        stream_kw.update(timed=True, confidence=confidence or "post_max")
    if bool(int(cli.get("beam_times", 0) or 0)):
        from asr_chinese_e2e_amd.confidence import BEAM_MEASURES
        if not stream or not beam_stream:
            raise SystemExit("transcribe.py: --beam_times=1 applies to --stream=1 --stream_search=prefix_beam")
        if cli.get("context") not in (None, "", False) or cli.get("lm") not in (None, "", False):
            raise SystemExit("transcribe.py: --beam_times=1 is not combined with --context or --lm: only the plain prefix beam search carries times")
        if (confidence or "post_max") not in BEAM_MEASURES:
            raise SystemExit(f"transcribe.py: --beam_times=1 reports {', '.join(BEAM_MEASURES)}: the entropy measures need full posterior rows")
        stream_kw.update(beam_times=True, confidence=confidence or "post_max")
    context = None
    if cli.get("context") not in (None, "", False):
        from asr_chinese_e2e_amd.context import ContextGraph
        if stream and stream_search != "prefix_beam":
            raise SystemExit("transcribe.py: --context with --stream=1 needs --stream_search=prefix_beam (hotwords bias the CTC prefix beam search)")
        if not stream and model.use_decoder and joint != "ctc_rescore":
            raise SystemExit("transcribe.py: --context needs a search that runs the CTC prefix beam search: a CTC-only model or --joint=ctc_rescore")
        try:
            context = ContextGraph.from_file(str(cli["context"]), vocab, score=float(cli.get("context_score", 3.0)), device="cuda")
        except (OSError, ValueError) as e:
            raise SystemExit(f"transcribe.py: --context: {e}") from e
        if stream:
            stream_kw["context"] = context
    lm = None
    if cli.get("lm") not in (None, "", False):
        from asr_chinese_e2e_amd.lm import NgramLM
        if context is not None:
            raise SystemExit("transcribe.py: --lm and --context cannot be combined: the search runs one of the two")
        if stream and stream_search != "prefix_beam":
            raise SystemExit("transcribe.py: --lm with --stream=1 needs --stream_search=prefix_beam (the LM is fused into the CTC prefix beam search)")
        if not stream and model.use_decoder and joint != "ctc_rescore":
            raise SystemExit("transcribe.py: --lm needs a search that runs the CTC prefix beam search: a CTC-only model or --joint=ctc_rescore")
        try:
            if str(cli["lm"]).endswith(".npz"):
                lm = NgramLM.load(str(cli["lm"]), device="cuda")
            else:
                lm = NgramLM.from_arpa(str(cli["lm"]), vocab, weight=float(cli.get("lm_weight", 0.3)), ins=float(cli.get("lm_ins", 0.0)), device="cuda")
            lm.check_vocab(model.V)
        except (OSError, ValueError) as e:
            raise SystemExit(f"transcribe.py: --lm: {e}") from e
        if stream:
            stream_kw["lm"] = lm
    blank_skip = None
    if cli.get("blank_skip") is not None and cli["blank_skip"] != "":      # 0 is a value, and a refused one
        from asr_chinese_e2e_amd.kernels import blank_skip_threshold
        try:
            if isinstance(cli["blank_skip"], bool):
                raise ValueError("a flag without a value")
            blank_skip = float(cli["blank_skip"])
            blank_skip_threshold(blank_skip)
        except (TypeError, ValueError) as e:
            raise SystemExit(f"transcribe.py: --blank_skip must be a probability in (0, 1] (got {cli['blank_skip']!r})") from e
        if stream and stream_search != "prefix_beam":
            raise SystemExit("transcribe.py: --blank_skip with --stream=1 needs --stream_search=prefix_beam (frames are dropped in front of the CTC prefix beam search)")
        if not stream and model.use_decoder and joint != "ctc_rescore":
            raise SystemExit("transcribe.py: --blank_skip needs a search that runs the CTC prefix beam search: a CTC-only model or --joint=ctc_rescore")
        if stream:
            stream_kw["blank_skip"] = blank_skip
    resample = bool(int(cli.get("resample", 0)))      # --resample=1: files at another rate are converted on the GPU instead of ending the run
    if stream and model.decoding_chunk_size <= 0:
        raise SystemExit("transcribe.py: --stream=1 needs a decoding chunk (--decoding_chunk_size, or a static --chunk_size)")
    id2tok = vocab._id2token
    n_sessions = int(cli.get("sessions", 0) or 0)
    if bool(int(cli.get("endpoint", 0) or 0)) and not n_sessions:
        raise SystemExit("transcribe.py: --endpoint=1 applies to --sessions=N")
    if n_sessions:
        if not stream or parser.norm != "global":
            raise SystemExit("transcribe.py: --sessions=N needs --stream=1 and --cmvn (the samples themselves are streamed)")
        if not model.use_ctc:
            raise SystemExit("transcribe.py: --sessions=N needs a model with the CTC head")
        search = dict(ctc_weight=ctc_weight, timestamps=timestamps, joint="ctc_rescore") if beam_stream else dict(beam_size=beam, ctc_weight=ctc_weight, timestamps=timestamps, joint=joint)
        if confidence is not None:
            search["confidence"] = confidence
        block = int(cli.get("stream_block_samples", 0)) or model.decoding_chunk_size * config.lfr_n * 160
        stream_sessions(model, parser, files, n_sessions, id2tok, block, shift_s, config.sample_rate, endpoint=bool(int(cli.get("endpoint", 0) or 0)),
                        stream_kw=stream_kw, **search)
        return
    if long_form is not None:
        search = dict(beam_size=beam, ctc_weight=ctc_weight, timestamps=timestamps, joint=joint)
        if context is not None:
            search["context"] = context
        if lm is not None:
            search["lm"] = lm
        if blank_skip is not None:
            search["blank_skip"] = blank_skip
        if confidence is not None:
            search["confidence"] = confidence
        transcribe_long_files(model, parser, files, long_form[0], long_form[1], bs, resample, shift_s, config.sample_rate, **search)
        return
    for i in range(0, len(files), bs):
        chunk = files[i:i + bs]
        waves, rates = [], []
        for path in chunk:
            pcm, sr = load_wav(path)
            if sr != config.sample_rate:
                if not resample:
                    raise SystemExit(f"transcribe.py: {path}: sample rate {sr}, the model expects {config.sample_rate}")
                try:
                    resample_mod.plan(sr)
                except ValueError as e:
                    raise SystemExit(f"transcribe.py: {path}: {e}") from e
            waves.append(pcm)
            rates.append(sr)
        S = max(1, max(len(w) for w in waves))
        wav = np.zeros((len(waves), S), dtype=np.float32)
        for b, w in enumerate(waves):
            wav[b, : len(w)] = w
        wav_len = torch.tensor([len(w) for w in waves], dtype=torch.int32)
        wav = torch.from_numpy(wav)
        stream_rate = None      # the batch streams at its source rate when every file shares it; otherwise it is converted first
        if any(r != config.sample_rate for r in rates):
            if stream and parser.norm == "global" and len(set(rates)) == 1:
                stream_rate = rates[0]
            else:      # one launch for the batch, whatever rates it mixes
                wav, wav_len, _ = resample_mod.resample_batch(wav.cuda(), wav_len.tolist(), rates)
        search = dict(beam_size=beam, ctc_weight=ctc_weight, timestamps=timestamps, joint=joint)
        if context is not None and not stream:
            search["context"] = context
        if lm is not None and not stream:
            search["lm"] = lm
        if blank_skip is not None and not stream:
            search["blank_skip"] = blank_skip
        if beam_stream:      # the streamed search's own n-best, re-ranked by the decoder
            search = dict(ctc_weight=ctc_weight, timestamps=timestamps, joint="ctc_rescore")
        if confidence is not None:
            search["confidence"] = confidence
        if stream and parser.norm == "global":      # the samples stream: blocks of one chunk's worth of audio unless told otherwise
            block = int(cli.get("stream_block_samples", 0)) or model.decoding_chunk_size * config.lfr_n * 160 * (stream_rate or 16000) // 16000
            out = stream_audio_batch(model, parser, chunk, wav, wav_len.tolist(), id2tok, block, source_rate=stream_rate, stream_kw=stream_kw, shift_s=shift_s, **search)
        else:
            feats, flen = parser.parse_batch(wav.cuda(), wav_len.cuda())
            if stream:
                out = stream_batch(model, chunk, feats, flen, id2tok, stream_kw=stream_kw, shift_s=shift_s, **search)
            else:
                out = model.transcribe(Pack(wave=feats, wave_len=flen), **search)
        for path, w, sr, r in zip(chunk, waves, rates, out):
            print(json.dumps(final_line(path, len(w), sr, r, shift_s, config.sample_rate), ensure_ascii=False), flush=True)


if __name__ == "__main__":
    transcribe(**parse_flags(sys.argv[1:]))
