"""Keyword spotting on the CTC posteriors: where in the audio is one of these phrases spoken, and how sure is the model?

The search (csrc/kws.hip; the definition: tests/kws_ref.py, restated in include/asr_hip.h) runs every phrase of a KeywordList against every
frame of every utterance with a free start and a free end: H_t = the largest log-probability of a CTC alignment of the phrase that ends on
frame t.  A frame is a candidate when exp(H_t / L), the geometric mean per character, reaches the phrase's threshold and the match is no
longer than L * max_token_s; a maximal run of candidate frames is one hit, placed on the run's best frame.  A hit's start_frame is the LAST
frame of the first character's run (the search enters the first character afresh on every frame), its end_frame the frame the last
character's score peaked on: times follow ctc_align's convention, start_s = start_frame * d and end_s = (end_frame + 1) * d.

    kl = KeywordList.from_file("phrases.txt", model.vocab, threshold=0.5)
    model.spot_keywords(batch, kl)          -> per utterance {"hits": [...], "dropped": n}
    model.spot_long(parser, wav, wav_len, kl)     whole recordings, cut at their pauses by the energy VAD

Out of scope: per-utterance lists, a per-gap limit in place of the span cap, a filler / garbage model, phrases of more than 16 tokens,
wildcards, spotting inside the silences the VAD removed, blank-frame skipping in front of the search (it reads every frame)."""
import ctypes
import math

import numpy as np
import torch

from . import kernels as K
from ._lib import KWS_MAX_CAP, KWS_MAX_KEYWORDS, KWS_MAX_LEN

BLANK = 0
DEFAULT_THRESHOLD, DEFAULT_MAX_TOKEN_S, DEFAULT_HITS = 0.5, 0.5, 8
MAX_HITS = 1024      # rows of one utterance's hit list on the device, unless the list asks for another number


class KwsTables(ctypes.Structure):
    """asr_kws_list of include/asr_hip.h (same field order)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("tok", "len", "thr", "span", "index", "host_tok", "host_len", "host_index")] + [("K", ctypes.c_int)]


def threshold_lp(L, p):
    """thr = float32(L ln p), the product in float64."""
    return float(np.float32(int(L) * math.log(float(p))))


def max_token_frames(max_token_s, frame_seconds):
    return max(1, int(math.floor(float(max_token_s) / float(frame_seconds) + 1e-9)))


def _bucket(L):
    return 4 if L <= 4 else 8 if L <= 8 else 16


class KeywordList:
    def __init__(self, phrases, threshold=DEFAULT_THRESHOLD, max_token_s=DEFAULT_MAX_TOKEN_S, vocab_size=None, hits_per_keyword=DEFAULT_HITS, max_hits=None,
                 texts=None):
        """phrases: a list of token id lists, or of (ids, threshold) pairs; ids in [1, vocab_size), 1 to 16 of them (0 is the CTC
        blank).  threshold p in (0, 1]: a phrase is reported where the geometric mean of its characters' posteriors along the best
        alignment reaches p.  max_token_s: a match may span at most L * max(1, floor(max_token_s / frame_seconds)) frames (blank frames
        are almost free: without the cap two characters a long silence apart would still match).  hits_per_keyword: the records kept per
        (utterance, keyword) and call; max_hits: the rows of an utterance's list (None: min(K * hits_per_keyword, 1024)); what does not
        fit is counted in "dropped".  Duplicate phrases are kept, each under its own index."""
        phrases = list(phrases) if phrases is not None else []
        if not phrases:
            raise ValueError("KeywordList: no phrase given")
        if len(phrases) > KWS_MAX_KEYWORDS:
            raise ValueError(f"KeywordList: {len(phrases)} phrases (at most {KWS_MAX_KEYWORDS})")
        V = None if vocab_size is None else int(vocab_size)
        ids, ps = [], []
        for i, ph in enumerate(phrases):
            p = threshold
            if isinstance(ph, (tuple, list)) and len(ph) == 2 and isinstance(ph[0], (tuple, list)):
                ph, p = ph
            ph = [int(t) for t in ph]
            if not ph:
                raise ValueError(f"KeywordList: phrase {i} is empty")
            if len(ph) > KWS_MAX_LEN:
                raise ValueError(f"KeywordList: phrase {i} has {len(ph)} tokens (at most {KWS_MAX_LEN})")
            for t in ph:
                if t == BLANK:
                    raise ValueError(f"KeywordList: phrase {i} holds the CTC blank (id {BLANK})")
                if t < 0 or (V is not None and t >= V):
                    raise ValueError(f"KeywordList: phrase {i}: token {t} outside [1, {'V' if V is None else V})")
            try:
                p = float(p)
            except (TypeError, ValueError):
                raise ValueError(f"KeywordList: phrase {i}: threshold {p!r} is not a number")
            if not (p > 0.0 and p <= 1.0):      # a NaN fails both
                raise ValueError(f"KeywordList: phrase {i}: threshold {p} outside (0, 1]")
            ids.append(ph)
            ps.append(p)
        mts = float(max_token_s)
        if not (mts > 0.0 and mts < float("inf")):
            raise ValueError(f"KeywordList: max_token_s must be positive and finite (got {max_token_s})")
        cap = int(hits_per_keyword)
        if isinstance(hits_per_keyword, bool) or cap != hits_per_keyword or not 1 <= cap <= KWS_MAX_CAP:
            raise ValueError(f"KeywordList: hits_per_keyword must be an integer in [1, {KWS_MAX_CAP}] (got {hits_per_keyword!r})")
        Kn = len(ids)
        mh = min(Kn * cap, MAX_HITS) if max_hits is None else int(max_hits)
        if mh < 1:
            raise ValueError(f"KeywordList: max_hits must be positive (got {max_hits!r})")
        if texts is not None and len(texts) != Kn:
            raise ValueError(f"KeywordList: {len(texts)} texts for {Kn} phrases")
        # table rows: the phrases sorted by length bucket (stable), so that the 64 keywords of a wave share a kernel
        order = sorted(range(Kn), key=lambda k: _bucket(len(ids[k])))
        tok = torch.zeros(Kn, KWS_MAX_LEN, dtype=torch.int32)
        for j, k in enumerate(order):
            tok[j, : len(ids[k])] = torch.tensor(ids[k], dtype=torch.int32)
        self._ids, self._ps, self._V, self._mts, self._cap, self._mh = tuple(tuple(p) for p in ids), tuple(ps), V, mts, cap, mh
        self._texts = None if texts is None else tuple(texts)
        self._order = tuple(order)
        self._host = (tok, torch.tensor([len(ids[k]) for k in order], dtype=torch.int32),
                      torch.tensor([threshold_lp(len(ids[k]), ps[k]) for k in order], dtype=torch.float32), torch.tensor(order, dtype=torch.int32))
        self._dev = {}

    def __setattr__(self, name, value):
        if name.startswith("_") and name not in self.__dict__:
            object.__setattr__(self, name, value)
        else:
            raise AttributeError("KeywordList is immutable")

    K = property(lambda self: len(self._ids))
    ids = property(lambda self: self._ids)
    thresholds = property(lambda self: self._ps)
    texts = property(lambda self: self._texts)
    vocab_size = property(lambda self: self._V)
    max_token_s = property(lambda self: self._mts)
    hits_per_keyword = property(lambda self: self._cap)
    max_hits = property(lambda self: self._mh)
    order = property(lambda self: self._order)
    thr = property(lambda self: [threshold_lp(len(i), p) for i, p in zip(self._ids, self._ps)])

    def spans(self, frame_seconds):
        """Per phrase, the longest match in frames: L * max(1, floor(max_token_s / frame_seconds + 1e-9))."""
        m = max_token_frames(self._mts, frame_seconds)
        return [len(i) * m for i in self._ids]

    def check_vocab(self, V):
        """Raises unless every token is below V (for a list built without vocab_size)."""
        top = max(max(p) for p in self._ids)
        if top >= int(V):
            raise ValueError(f"KeywordList: token {top} outside [1, {int(V)})")

    def on(self, device, frame_seconds):
        """The asr_kws_list struct the entry points take, its tables on `device`, the span caps for frames of frame_seconds; kept."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, float(frame_seconds))
        got = self._dev.get(key)
        if got is None:
            sp = self.spans(frame_seconds)
            span = torch.tensor([sp[k] for k in self._order], dtype=torch.int32)
            tabs = tuple(t.to(device) for t in (self._host[0], self._host[1], self._host[2], span, self._host[3]))
            struct = KwsTables(*[t.data_ptr() for t in tabs], self._host[0].data_ptr(), self._host[1].data_ptr(), self._host[3].data_ptr(), len(self._ids))
            got = self._dev[key] = (struct, tabs)
        return got[0]

    def decode(self, flat, B, max_hits, frame_seconds, id2tok=None):
        """flat: kernels.kws_compact's buffer on the host -> per utterance {"hits": [...], "dropped": n}, the hits sorted by
        (end_frame, keyword)."""
        count, dropped, rows = (t.numpy() for t in K.kws_unpack(flat, B, max_hits))
        d = float(frame_seconds)
        out = []
        for b in range(B):
            hs = [self.hit(k, s, e, float(np.array([w], dtype=np.int32).view(np.float32)[0]), d, id2tok) for k, s, e, w in rows[b, :int(count[b])].tolist()]
            hs.sort(key=lambda h: (h["end_frame"], h["keyword"]))
            out.append({"hits": hs, "dropped": int(dropped[b])})
        return out

    def hit(self, k, start, end, score, d, id2tok=None):
        ids = list(self._ids[k])
        text = self._texts[k] if self._texts is not None else None if id2tok is None else "".join(id2tok[x] for x in ids)
        return {"keyword": k, "phrase": text, "ids": ids, "start_frame": start, "end_frame": end, "start_s": start * d, "end_s": (end + 1) * d,
                "score": score, "confidence": math.exp(score / len(ids))}

    @classmethod
    def from_file(cls, path, vocab, threshold=DEFAULT_THRESHOLD, max_token_s=DEFAULT_MAX_TOKEN_S, hits_per_keyword=DEFAULT_HITS, max_hits=None):
        """A list from a UTF-8 file: one phrase per line (ContextGraph.from_file's convention), optionally a tab and the phrase's own
        threshold behind it; every character is looked up in `vocab` (data_handler.vocab.Vocab, or a token -> id mapping); blank lines
        are skipped, duplicate lines kept; a line with an unknown character or a bad threshold raises and names the line."""
        t2i = getattr(vocab, "_token2id", vocab)
        size = len(getattr(vocab, "_id2token", t2i))
        phrases, texts = [], []
        with open(path, encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                head, tab, tail = line.rstrip("\r\n").partition("\t")
                text = "".join(head.split())
                if not text and not tail.strip():
                    continue
                if not text:
                    raise ValueError(f"{path}, line {no}: a threshold without a phrase")
                p = threshold
                if tab and tail.strip():
                    try:
                        p = float(tail.strip())
                    except ValueError:
                        raise ValueError(f"{path}, line {no}: threshold {tail.strip()!r} is not a number")
                    if not (p > 0.0 and p <= 1.0):
                        raise ValueError(f"{path}, line {no}: threshold {p} outside (0, 1]")
                ids = []
                for ch in text:
                    if ch not in t2i:
                        raise ValueError(f"{path}, line {no}: character {ch!r} is not in the vocabulary")
                    ids.append(int(t2i[ch]))
                if len(ids) > KWS_MAX_LEN:
                    raise ValueError(f"{path}, line {no}: {len(ids)} characters (at most {KWS_MAX_LEN})")
                if BLANK in ids:
                    raise ValueError(f"{path}, line {no}: the phrase holds the CTC blank")
                phrases.append((ids, p))
                texts.append(text)
        if not phrases:
            raise ValueError(f"{path}: no phrase")
        return cls(phrases, threshold=threshold, max_token_s=max_token_s, vocab_size=size, hits_per_keyword=hits_per_keyword, max_hits=max_hits, texts=texts)


def _check(model, keywords):
    if not isinstance(keywords, KeywordList):
        raise ValueError(f"keywords must be a keywords.KeywordList, got {type(keywords).__name__}")
    if not model.use_ctc:
        raise ValueError("keyword spotting reads the CTC head's posteriors, and this model has none (config.ctc_weight = 0)")
    keywords.check_vocab(model.V)


def spot_logits(keywords, logits, in_len, frame_seconds, id2tok=None):
    """The search over given CTC logits (B, T, V) f32 / bf16 with in_len (B) int32 on the device: asr_ctc_frame_stats for lse,
    asr_kws_search, asr_kws_compact, one copy to the host.  -> per utterance {"hits", "dropped"}."""
    _, _, _, lse, _ = K.ctc_frame_stats(logits, in_len, BLANK)
    cnt, rec = K.kws_search(logits, lse, in_len, keywords.on(logits.device, frame_seconds), keywords.K, keywords.hits_per_keyword, BLANK)
    flat = torch.empty(logits.shape[0] * (2 + 4 * keywords.max_hits), dtype=torch.int32, device=logits.device)
    K.kws_compact(cnt, rec, keywords.max_hits, out=flat)
    return keywords.decode(flat.cpu(), logits.shape[0], keywords.max_hits, frame_seconds, id2tok)


def spot_keywords(model, input, keywords):
    """model.spot_keywords: the encoder and the CTC projection as ctc_align runs them, then spot_logits."""
    _check(model, keywords)
    logits = model._ctc_logits(input)
    return spot_logits(keywords, logits, input.wave_len.to(torch.int32).contiguous(), model.frame_seconds(), model.vocab._id2token)


def stitch_hits(results, segs):
    """One recording's hits from spot_keywords' results of its segments (in time order) and their (start_sample, end_sample): times
    move by the segment's start, frames stay relative to the segment, every hit gains "segment".  -> {"hits", "dropped"}."""
    from .vad import SR
    hits, dropped = [], 0
    for i, (r, (s0, _)) in enumerate(zip(results, segs)):
        off = s0 / float(SR)
        hits += [dict(h, start_s=h["start_s"] + off, end_s=h["end_s"] + off, segment=i) for h in r["hits"]]
        dropped += r["dropped"]
    return {"hits": hits, "dropped": dropped}


def spot_long(model, parser, wav, wav_len, keywords, vad=None, batch_size=16, source_rate=None, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1,
              max_segment_s=20.0):
    """model.spot_long: longform.transcribe_long's loop with spot_keywords in place of transcribe - the same options, refusals, segments
    and batches.  -> per recording {"hits": [...], "dropped", "duration_s", "segments": [(start_s, end_s)]}; a recording without speech
    has no hits.  A phrase the VAD cut in two, or spoken inside a removed silence, is not found."""
    from . import longform
    from .vad import SR
    _check(model, keywords)
    plan = longform.plan(model, parser, wav, wav_len, vad, batch_size, source_rate, min_silence_s, min_speech_s, pad_s, max_segment_s, "spot_long")
    out = []
    for b in range(len(plan.segs)):
        results = []
        for _, pack in longform.batches(plan, parser, b):
            results += spot_keywords(model, pack, keywords)
        r = stitch_hits(results, plan.segs[b])
        r.update(duration_s=plan.duration[b], segments=[(s0 / float(SR), s1 / float(SR)) for s0, s1 in plan.segs[b]])
        out.append(r)
    return out
