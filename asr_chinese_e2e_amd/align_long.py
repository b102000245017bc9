"""Aligning a whole recording to its transcript: the energy VAD (vad.py) cuts the recording at its pauses, the segments go through the
encoder and the CTC head in time order, their valid rows are laid end to end on the device, and ONE asr_ctc_align_long launch finds the
best single CTC path of the whole transcript (up to 8192 tokens) through all of them.  Tokens and transcript lines come back with times
on the recording's axis, log-probabilities and confidences: what a corpus builder needs to cut a lecture into training utterances
(align.py writes them in the collector format build_dataloader reads).

Audio the transcript does not cover (a spoken title, an advertisement, an ad-lib): with filler = a penalty in nats, the blank states in
front of every line (or of every token) and behind the last token are wide (asr_ctc_align_long_filler, tests/align_filler_ref.py): on a
frame whose blank lies more than the penalty below the frame's best class they emit best - penalty instead, so such frames neither pay
the blank's price nor push a neighbouring character over the foreign audio.  The runs of such frames come back as "fillers".

Out of scope: script lines that were never spoken (the per-line confidence remains the flag for those), filler in the one-wave
asr_ctc_align, per-gap penalties, a learned garbage model, more than 8192 tokens per recording, pruned or banded search, alignment by
the attention decoder, units other than the vocabulary's, text normalisation beyond removing whitespace, aligning inside the silences
the VAD removed, streaming."""
import math

from . import kernels as K
from ._lib import ALIGN_LONG_MAX_LABELS
from .confidence import BEAM_MEASURES, measure
from .longform import check_max_segment
from .vad import SR, EnergyVad, segment_frames


def text_ids(vocab, V, blank, texts, B):
    """texts[b] = a string, a list of lines (strings) or a list of id lists -> per recording (lines [{"text", "ids", "unk"}], ids, the
    line of every id).  Strings become ids with vocab.convert_str (no bos / eos) after whitespace is removed; characters outside the
    vocabulary become the unknown id and are counted per line.  ValueError: len(texts) != B, a label equal to the blank or outside
    [0, V), more than ALIGN_LONG_MAX_LABELS tokens in a recording."""
    if len(texts) != B:
        raise ValueError(f"align_long: {len(texts)} transcripts for {B} recordings")
    unk = vocab._token2id[vocab.UNK]
    id2tok = vocab._id2token
    out = []
    for b, t in enumerate(texts):
        lines = []
        for item in ([t] if isinstance(t, str) else list(t)):
            if isinstance(item, str):
                chars = "".join(item.split())
                ids = [int(x) for x in vocab.convert_str(chars, use_bos=False, use_eos=False)]
                n_unk = sum(1 for c, x in zip(vocab._tokenize_fn(chars), ids) if x == unk and c != vocab.UNK)
                lines.append({"text": chars, "ids": ids, "unk": n_unk})
            else:
                ids = [int(x) for x in item]
                lines.append({"text": "".join(id2tok[x] if 0 <= x < len(id2tok) else "" for x in ids), "ids": ids, "unk": sum(1 for x in ids if x == unk)})
        ids = [x for l in lines for x in l["ids"]]
        for x in ids:
            if x == blank or x < 0 or x >= V:
                raise ValueError(f"align_long: recording {b}: label {x}: labels are ids in [0, {V}) other than the blank ({blank})")
        if len(ids) > ALIGN_LONG_MAX_LABELS:
            raise ValueError(f"align_long: recording {b}: {len(ids)} tokens, the limit is {ALIGN_LONG_MAX_LABELS} per recording: split the script at a known anchor")
        out.append((lines, ids, [k for k, l in enumerate(lines) for _ in l["ids"]]))
    return out


def segment_rows(parser, n_samples):
    """Encoder frames (rows after low-frame-rate stacking) of a segment of n_samples samples: parse_batch's feature length."""
    return -(-parser.num_frames(int(n_samples)) // parser.lfr_n)


def stitch_alignment(lines, ids, line_of, segs, seg_rows, score, spans, tok, frame_seconds, id2tok, which, duration_s):
    """One recording's result from the kernel's outputs.  segs: [(start_sample, end_sample)] in time order, seg_rows: the rows each
    contributed to the concatenated frames; spans (L, 2) / tok (L, 3) / score as asr_ctc_align_long writes them (host lists).  A frame's
    time comes from the segment the frame lies in, as stitch's: start = segment start + frame * d, end = segment start + (frame + 1) * d."""
    d = float(frame_seconds)
    first = [0]
    for n in seg_rows:
        first.append(first[-1] + int(n))
    feasible = score != float("-inf") and score == score

    def seg_of(f):
        lo, hi = 0, len(seg_rows) - 1
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if first[mid] <= f else (lo, mid - 1)
        return lo

    tokens = []
    for i, x in enumerate(ids):
        t = {"id": x, "token": id2tok[x] if 0 <= x < len(id2tok) else None, "line": line_of[i], "start_s": None, "end_s": None, "segment": None,
             "start_frame": None, "end_frame": None, "logp": None, "measures": None, "confidence": None}
        if feasible:
            f0, f1 = int(spans[i][0]), int(spans[i][1])
            s0, s1 = seg_of(f0), seg_of(f1)
            sm, mx, mn = (float(v) for v in tok[i])
            m = {"post_max": math.exp(mx), "post_min": math.exp(mn), "post_mean": math.exp(sm / (f1 - f0 + 1))}
            t.update(start_s=segs[s0][0] / float(SR) + (f0 - first[s0]) * d, end_s=segs[s1][0] / float(SR) + (f1 - first[s1] + 1) * d, segment=s0,
                     start_frame=f0, end_frame=f1, logp=sm, measures=m, confidence=m[which])
        tokens.append(t)
    out_lines, at = [], 0
    for l in lines:
        mine = tokens[at:at + len(l["ids"])]
        at += len(l["ids"])
        line = {"text": l["text"], "ids": l["ids"], "start_s": None, "end_s": None, "logp": None, "frames": None, "confidence": None,
                "min_confidence": None, "unk": l["unk"]}
        if mine and feasible:
            logp = 0.0
            for t in mine:
                logp += t["logp"]
            frames = sum(t["end_frame"] - t["start_frame"] + 1 for t in mine)
            line.update(start_s=mine[0]["start_s"], end_s=mine[-1]["end_s"], logp=logp, frames=frames, confidence=math.exp(logp / frames),
                        min_confidence=min(t["measures"]["post_mean"] for t in mine))
        out_lines.append(line)
    return {"score": float(score), "duration_s": duration_s, "frames": first[-1], "tokens": tokens, "lines": out_lines,
            "segments": [(s0 / float(SR), s1 / float(SR)) for s0, s1 in segs]}


FILLER_SCOPES = ("lines", "tokens")


def filler_penalty(filler, filler_scope):
    """The checked options of align_long's filler: None (off) or the penalty as a float.  ValueError: a penalty that is a bool, no
    number, NaN, infinite or negative, an unknown scope, a scope other than the default while the filler is off."""
    if filler_scope not in FILLER_SCOPES:
        raise ValueError(f"align_long: filler_scope must be one of {', '.join(FILLER_SCOPES)} (got {filler_scope!r})")
    if filler is None:
        if filler_scope != "lines":
            raise ValueError(f"align_long: filler_scope = {filler_scope!r} without a filler penalty (filler is None: the feature is off)")
        return None
    if isinstance(filler, bool) or not isinstance(filler, (int, float)) or not math.isfinite(filler) or filler < 0:
        raise ValueError(f"align_long: filler must be None or a finite penalty >= 0 in nats (got {filler!r})")
    return float(filler)


def filler_gaps(lines, n_ids, scope):
    """gap flags of one recording (one per token): "lines" marks the first token of every line that has tokens, "tokens" every token.
    (The tail is always wide.)"""
    if scope == "tokens":
        return [1] * n_ids
    gap, at = [0] * n_ids, 0
    for l in lines:
        if l["ids"]:
            gap[at] = 1
        at += len(l["ids"])
    return gap


def stitch_fillers(path, line_of, n_lines, segs, seg_rows, frame_seconds, feasible=True):
    """The filler runs of one recording from the kernel's path (host list, one value per concatenated frame: a token index, -1 on a blank
    frame, -2 on a filler frame) -> (the count of filler frames, [{"start_frame", "end_frame", "frames", "start_s", "end_s", "segment",
    "before_token", "before_line"}] for every maximal run of -2).  Times as stitch_alignment's: the start on the clock of the segment
    that holds the first frame, the end on the clock of the segment that holds the last.  before_token: the token whose gap the run lies
    in (the one after the last token seen), len(line_of) for the tail; before_line: that token's line, n_lines for the tail."""
    d = float(frame_seconds)
    first = [0]
    for n in seg_rows:
        first.append(first[-1] + int(n))
    L = len(line_of)

    def seg_of(f):
        k = 0
        while k + 1 < len(seg_rows) and first[k + 1] <= f:
            k += 1
        return k

    runs, count, last, t, T = [], 0, -1, 0, len(path) if feasible else 0
    while t < T:
        v = int(path[t])
        if v >= 0:
            last = v
        if v != -2:
            t += 1
            continue
        e = t
        while e + 1 < T and int(path[e + 1]) == -2:
            e += 1
        s0, s1, bt = seg_of(t), seg_of(e), last + 1
        runs.append({"start_frame": t, "end_frame": e, "frames": e - t + 1, "start_s": segs[s0][0] / float(SR) + (t - first[s0]) * d,
                     "end_s": segs[s1][0] / float(SR) + (e - first[s1] + 1) * d, "segment": s0, "before_token": bt,
                     "before_line": line_of[bt] if bt < L else n_lines})
        count += e - t + 1
        t = e + 1
    return count, runs


def align_long(model, parser, wav, wav_len, texts, vad=None, batch_size=16, source_rate=None, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1,
               max_segment_s=20.0, confidence="post_mean", max_bytes=4 << 30, filler=None, filler_scope="lines"):
    """wav (B, S) f32: B whole recordings (at source_rate when given, else 16 kHz), wav_len their lengths, texts their transcripts (a
    string, a list of lines or a list of id lists each) -> per recording {"score", "duration_s", "frames", "tokens": [{"id", "token",
    "line", "start_s", "end_s", "segment", "start_frame", "end_frame", "logp", "measures", "confidence"}], "lines": [{"text", "ids",
    "start_s", "end_s", "logp", "frames", "confidence", "min_confidence", "unk"}], "segments": [(start_s, end_s)]}.  Frames count the
    recording's concatenated encoder frames (the VAD's segments end to end); a token's logp is the sum of its log posteriors over its
    run, a line's the float64 sum of its tokens', its confidence exp(logp / frames), its min_confidence the smallest post_mean of its
    tokens.  A line without tokens, and everything of a recording whose transcript does not fit its frames (score -inf), carries None.
    confidence: post_max, post_min or post_mean (confidence.py's); the entropy measures need full rows per token and are refused.
    filler: None (off: the call and the result are exactly those without the argument) or a penalty >= 0 in nats.  Then the blank in
    front of the first token of every line (filler_scope "lines") or of every token ("tokens"), and the one behind the last token, are
    wide (asr_ctc_align_long_filler): on a frame whose blank lies more than `filler` below the frame's best class, such a state emits
    best - filler instead of the blank.  Each result gains "filler_frames", the count of such frames on the path, and "fillers", their
    maximal runs [{"start_frame", "end_frame", "frames", "start_s", "end_s", "segment", "before_token", "before_line"}] (stitch_fillers);
    "score" includes the filler emissions.  Refused before any launch or VAD: a filler that is a bool, NaN, infinite or negative, an
    unknown filler_scope, a filler_scope other than "lines" while filler is None.
    Refused with ValueError before any launch: a model without CTC head, a label equal to the blank or outside [0, V), more than 8192
    tokens in a recording, len(texts) != B, and what transcribe_long refuses about its options; after the VAD and before the encoder
    runs: a recording whose rows plus workspace exceed max_bytes."""
    import torch
    from .Utils import Pack
    if not getattr(model, "use_ctc", False):
        raise ValueError("align_long aligns with the CTC head, and this model has none (config.ctc_weight = 0)")
    filler = filler_penalty(filler, filler_scope)
    which = measure(confidence) or "post_mean"
    if which not in BEAM_MEASURES:
        raise ValueError(f"align_long reports {BEAM_MEASURES}: the entropy measures need full posterior rows per token (got {which!r})")
    opts = segment_frames(min_silence_s, min_speech_s, pad_s, max_segment_s)
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or int(batch_size) < 1:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    batch_size = int(batch_size)
    if wav.dim() != 2:
        raise ValueError(f"align_long: wav must be (B, S), got {tuple(wav.shape)}")
    B = wav.shape[0]
    lens = [int(v) for v in (wav_len.tolist() if torch.is_tensor(wav_len) else wav_len)]
    if len(lens) != B or any(l < 0 or l > wav.shape[1] for l in lens):
        raise ValueError(f"align_long: wav_len must hold {B} lengths in [0, {wav.shape[1]}], got {lens}")
    V, blank = int(model.V), 0
    parsed = text_ids(model.vocab, V, blank, texts, B)
    vad = EnergyVad() if vad is None else vad
    device = parser.window.device
    eng = model._ensure_engine(device)
    check_max_segment(parser, eng.pe.shape[0], opts[3], max_segment_s)
    rate = SR if source_rate is None else source_rate
    duration = [l / float(rate) for l in lens]
    wav = wav.to(device=device, dtype=torch.float32)
    if rate != SR:
        from .data_handler.resample import resample_batch
        wav, _, lens = resample_batch(wav.contiguous(), lens, [rate] * B)
    wav = wav.contiguous()
    segs = vad.segments(wav, lens, min_silence_s, min_speech_s, pad_s, max_segment_s)
    seg_rows = [[segment_rows(parser, s1 - s0) for s0, s1 in segs[b]] for b in range(B)]
    ld = int(getattr(eng, "ld_v", V) or V)
    esize = 2 if getattr(eng, "dtype", torch.float32) == torch.bfloat16 else 4
    for b in range(B):
        T_b, L_b = sum(seg_rows[b]), len(parsed[b][1])
        rows_b, ws_b = T_b * ld * esize, K.ctc_align_long_workspace_bytes(1, T_b, L_b)
        if rows_b + ws_b > max_bytes:
            raise ValueError(f"align_long: recording {b}: {T_b} frames of logits ({rows_b} bytes) plus {ws_b} bytes of back-pointers for {L_b} tokens exceed "
                             f"max_bytes = {max_bytes}")
    rows = lse = best = None
    at = 0
    for b in range(B):
        for i in range(0, len(segs[b]), batch_size):
            part = segs[b][i:i + batch_size]
            n = [s1 - s0 for s0, s1 in part]
            batch = K.segment_gather(wav, [b] * len(part), [s0 for s0, _ in part], n, max(1, max(n)))
            feats, flen = parser.parse_batch(batch, torch.tensor(n, dtype=torch.int32).to(device))
            logits = model._ctc_logits(Pack(wave=feats, wave_len=flen))
            _, seg_best, _, seg_lse, _ = K.ctc_frame_stats(logits, flen.to(torch.int32), blank)
            if rows is None:      # the first logits say how the rows are laid out
                total = sum(sum(r) for r in seg_rows)
                rows = torch.zeros(max(total, 1), K._frame_rows(logits), dtype=logits.dtype, device=device)[:, :V]
                lse = torch.zeros(max(total, 1), dtype=torch.float32, device=device)
                best = torch.zeros(max(total, 1), dtype=torch.float32, device=device) if filler is not None else None
            for k, want in enumerate(seg_rows[b][i:i + batch_size]):      # device-to-device: a segment's valid rows behind the ones before
                if want > logits.shape[1]:
                    raise RuntimeError(f"align_long: a segment of {want} encoder frames came back with {logits.shape[1]}")
                rows[at:at + want].copy_(logits[k, :want])
                lse[at:at + want].copy_(seg_lse[k, :want])
                if best is not None:
                    best[at:at + want].copy_(seg_best[k, :want])
                at += want
    if rows is None:      # no recording has speech
        rows, lse = torch.zeros(1, V, dtype=torch.float32, device=device), torch.zeros(1, dtype=torch.float32, device=device)
        best = torch.zeros(1, dtype=torch.float32, device=device) if filler is not None else None
    T_of = [sum(r) for r in seg_rows]
    row_off, lab_off = [0], [0]
    for b in range(B):
        row_off.append(row_off[-1] + T_of[b])
        lab_off.append(lab_off[-1] + len(parsed[b][1]))
    labels = [x for p in parsed for x in p[1]]
    path = None
    if filler is None:
        _, spans, tok, score = K.ctc_align_long(rows[:row_off[-1]], lse[:row_off[-1]], row_off, labels, lab_off, blank=blank, ws=getattr(eng, "ws", None))
    else:
        star = best[:row_off[-1]] - filler      # star[t] = the frame's best log posterior - the penalty: one f32 op
        gap = [g for p in parsed for g in filler_gaps(p[0], len(p[1]), filler_scope)]
        path, spans, tok, score = K.ctc_align_long_filler(rows[:row_off[-1]], lse[:row_off[-1]], star, row_off, labels, lab_off, gap, [1] * B, blank=blank,
                                                          ws=getattr(eng, "ws", None))
        path = path.cpu().tolist()
    spans, tok, score = spans.cpu().tolist(), tok.cpu().tolist(), score.cpu().tolist()
    d = model.frame_seconds()
    id2tok = model.vocab._id2token
    out = [stitch_alignment(parsed[b][0], parsed[b][1], parsed[b][2], segs[b], seg_rows[b], score[b], spans[lab_off[b]:lab_off[b + 1]],
                            tok[lab_off[b]:lab_off[b + 1]], d, id2tok, which, duration[b]) for b in range(B)]
    if path is not None:
        for b, res in enumerate(out):
            feasible = score[b] != float("-inf") and score[b] == score[b]
            res["filler_frames"], res["fillers"] = stitch_fillers(path[row_off[b]:row_off[b + 1]], parsed[b][2], len(parsed[b][0]), segs[b], seg_rows[b], d, feasible)
    return out
