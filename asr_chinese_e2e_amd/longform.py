"""Transcribing recordings that are longer than an utterance: the energy VAD (vad.py) cuts each recording at its pauses, the segments
go through model.transcribe in batches, and the results are stitched back onto the recording's time axis.  Every search transcribe has
(attention, joint, ctc_rescore, hotwords, LM, confidence, timestamps) runs unchanged on the pieces.

Out of scope: a neural VAD, segmenting by the model's own blank posteriors, streaming VAD, overlapping windows with text merging for
recordings without pauses (the hard cut at max_segment_s is the fallback), speaker turns, length-sorted batching - the segments of a
recording are batched in time order, which keeps the result a function of the recording and batch_size alone."""
from . import kernels as K
from .vad import FLEN, HOP, SR, EnergyVad, segment_frames


def encoder_rows(parser, max_frames):
    """Encoder frames (rows after low-frame-rate stacking) of a segment of max_frames VAD frames, the longest the segmenter emits."""
    frames = parser.num_frames(HOP * (max_frames - 1) + FLEN)
    return -(-frames // parser.lfr_n)


def check_max_segment(parser, table, max_frames, max_segment_s):
    """ValueError when a segment of max_frames frames would pass the positional-encoding table of `table` encoder frames; the message
    names the largest max_segment_s that fits."""
    if encoder_rows(parser, max_frames) <= table:
        return
    lo, hi = 0, max_frames                                     # encoder_rows is monotone: the largest admissible count by bisection
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if encoder_rows(parser, mid) <= table else (lo, mid)
    raise ValueError(f"max_segment_s = {max_segment_s}: a segment of {max_frames} frames is {encoder_rows(parser, max_frames)} encoder frames, past the "
                     f"positional-encoding table ({table} frames); the largest admissible max_segment_s is {lo / 100.0}")


def stitch(results, segs, duration_s):
    """One recording's result from transcribe's result dicts of its segments (in time order) and their (start_sample, end_sample):
    token times move by the segment's start, frames stay relative to the segment, text / ids are joined in order."""
    out = []
    for r, (s0, s1) in zip(results, segs):
        off = s0 / float(SR)
        seg = dict(r)
        seg.update(start_s=off, end_s=s1 / float(SR), start_sample=int(s0))
        if r.get("tokens") is not None:
            seg["tokens"] = [dict(t, start_s=None if t.get("start_s") is None else t["start_s"] + off,
                                  end_s=None if t.get("end_s") is None else t["end_s"] + off) for t in r["tokens"]]
        out.append(seg)
    return {"text": "".join(s["text"] for s in out), "ids": [i for s in out for i in s["ids"]], "duration_s": duration_s, "segments": out}


class Plan:
    """What the loop over a batch of recordings needs: the 16 kHz samples on the device, the VAD's segments per recording as
    (start_sample, end_sample), the recordings' durations, the batch size."""

    def __init__(self, wav, segs, duration, batch_size):
        self.wav, self.segs, self.duration, self.batch_size = wav, segs, duration, batch_size


def plan(model, parser, wav, wav_len, vad, batch_size, source_rate, min_silence_s, min_speech_s, pad_s, max_segment_s, what):
    """The checks, the resampling and the segmentation every long-form call shares (transcribe_long, keywords.spot_long); `what` names
    the caller in the messages.  Everything is refused before any launch."""
    import torch
    opts = segment_frames(min_silence_s, min_speech_s, pad_s, max_segment_s)
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or int(batch_size) < 1:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    batch_size = int(batch_size)
    vad = EnergyVad() if vad is None else vad
    if wav.dim() != 2:
        raise ValueError(f"{what}: wav must be (B, S), got {tuple(wav.shape)}")
    B = wav.shape[0]
    lens = [int(v) for v in (wav_len.tolist() if torch.is_tensor(wav_len) else wav_len)]
    if len(lens) != B or any(l < 0 or l > wav.shape[1] for l in lens):
        raise ValueError(f"{what}: wav_len must hold {B} lengths in [0, {wav.shape[1]}], got {lens}")
    device = parser.window.device
    check_max_segment(parser, model._ensure_engine(device).pe.shape[0], opts[3], max_segment_s)
    rate = SR if source_rate is None else source_rate
    duration = [l / float(rate) for l in lens]
    wav = wav.to(device=device, dtype=torch.float32)
    if rate != SR:
        from .data_handler.resample import resample_batch
        wav, _, lens = resample_batch(wav.contiguous(), lens, [rate] * B)
    wav = wav.contiguous()
    return Plan(wav, vad.segments(wav, lens, min_silence_s, min_speech_s, pad_s, max_segment_s), duration, batch_size)


def batches(p, parser, b):
    """Recording b's segments in time order, batch_size at a time: (the segments of the batch, their features as a Pack) - one
    asr_segment_gather and one parser.parse_batch per batch."""
    import torch
    from .Utils import Pack
    device = parser.window.device
    for i in range(0, len(p.segs[b]), p.batch_size):
        part = p.segs[b][i:i + p.batch_size]
        n = [s1 - s0 for s0, s1 in part]
        batch = K.segment_gather(p.wav, [b] * len(part), [s0 for s0, _ in part], n, max(1, max(n)))
        feats, flen = parser.parse_batch(batch, torch.tensor(n, dtype=torch.int32).to(device))
        yield part, Pack(wave=feats, wave_len=flen)


def transcribe_long(model, parser, wav, wav_len, vad=None, batch_size=16, source_rate=None, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1,
                    max_segment_s=20.0, **transcribe_kw):
    """wav (B, S) f32: B whole recordings (at source_rate when given, else 16 kHz), wav_len their lengths -> per recording
    {"text", "ids", "duration_s", "segments": [{"start_s", "end_s", "start_sample", "text", "ids", "score", "tokens", ...}]}: what
    model.transcribe(**transcribe_kw) returns for every segment the VAD finds, on the recording's time axis (token start_s / end_s
    absolute, start_frame / end_frame relative to the segment, start_sample the segment's first sample at 16 kHz).  The segments of a
    recording go in time order into batches of batch_size: one asr_segment_gather, parser.parse_batch and model.transcribe per batch.
    A recording without speech gives segments [] and text "".  vad: an EnergyVad (None: Kaldi's defaults).  context_ids, if given, holds
    one graph index per recording.  Refused with ValueError before any launch: a max_segment_s whose encoder frames pass the
    positional-encoding table, 2 pad_s > min_silence_s, non-finite or negative options, a batch_size below 1."""
    context_ids = transcribe_kw.pop("context_ids", None)
    if context_ids is not None and wav.dim() == 2 and len(context_ids) != wav.shape[0]:
        raise ValueError(f"transcribe_long: context_ids holds {len(context_ids)} entries for {wav.shape[0]} recordings")
    p = plan(model, parser, wav, wav_len, vad, batch_size, source_rate, min_silence_s, min_speech_s, pad_s, max_segment_s, "transcribe_long")
    B = len(p.segs)
    out = []
    for b in range(B):
        results = []
        for part, pack in batches(p, parser, b):
            kw = dict(transcribe_kw)
            if context_ids is not None:
                kw["context_ids"] = [context_ids[b]] * len(part)
            results += model.transcribe(pack, **kw)
        out.append(stitch(results, p.segs[b], p.duration[b]))
    return out
