"""Token confidence and streamed token times from the CTC posteriors: the host side of csrc/confidence.hip.

Five measures per token, from the frames s..e it occupies (lp_t = log p_t[token], ent_t = 1 - H(p_t) / ln V):
    post_max  = exp(max lp_t)        the largest frame posterior along the path (WeNet's measure; the default)
    post_min  = exp(min lp_t)
    post_mean = exp(sum lp_t / n)    the geometric mean; agrees with ctc_align's logp
    ent_mean  = sum ent_t / n        entropy-based frame confidences (NeMo's family: Shannon entropy, linear normalisation), averaged
    ent_min   = min ent_t
The utterance's confidence is the arithmetic mean of the chosen measure over the tokens that have one (float64 on the host).

Offline (ctc_align / transcribe / finish with confidence=...) a token's frames are its span of the Viterbi alignment.  Streamed in greedy
mode (model.stream / model.sessions with timed=True) they are the run of equal best classes the CTC collapse turns into the token, known
the moment the run closes: TokenLog keeps each slot's list from the records asr_session_ctc_step_tokens hands out per tick."""
import math

from . import kernels as K

MEASURES = ("post_max", "post_min", "post_mean", "ent_mean", "ent_min")


def measure(confidence):
    """None -> None (off), True -> "post_max", or one of MEASURES."""
    if confidence is None or confidence is False:
        return None
    if confidence is True:
        return "post_max"
    if confidence not in MEASURES:
        raise ValueError(f"confidence must be None, True or one of {MEASURES} (got {confidence!r})")
    return confidence


BEAM_MEASURES = MEASURES[:3]      # what the prefix beam search can report: it sees a token's own posteriors, never a full row


def beam_times_check(search, use_ctc, context, lm, confidence):
    """The refusals of beam_times=True (token times of prefix beam hypotheses), before anything is launched; returns the measure."""
    if search != "prefix_beam":
        raise ValueError("beam_times=True needs search='prefix_beam': the greedy path reports times with timed=True")
    if context is not None or lm is not None:
        raise ValueError("beam_times=True is not combined with a hotword context or an n-gram LM: only the plain prefix beam search carries times")
    which = measure(confidence) or "post_max"
    if which not in BEAM_MEASURES:
        raise ValueError(f"beam_times=True reports {BEAM_MEASURES}: the entropy measures need full posterior rows, which the search never sees (got {which!r})")
    if not use_ctc:
        raise ValueError("beam_times=True needs a model with the CTC head (config.ctc_weight > 0): times and confidence come from it")
    return which


def beam_tokens(ids, start, end, mx, mn, sm, which, id2tok, frame_seconds, n_final=None, real=None):
    """The tokens of one prefix beam hypothesis from its records (asr_ctc_prefix_beam_timed: per token the first and last frame of its run
    in the hypothesis' best single alignment, the largest, smallest and summed log-posterior over the run): {"id", "token", "start_frame",
    "end_frame", "start_s", "end_s", "measures", "confidence"} as TokenLog's, the three measures of BEAM_MEASURES.  n_final (streams): the
    first n_final entries get "final": True, the others False.  A hypothesis longer than its record row keeps the tokens that have one.
    real (a search behind blank-frame skipping): (start, end) in real frames (asr_frame_index_remap) - they are what is reported, while the
    mean stays over the rows the search saw, whose count start / end give."""
    out, d = [], float(frame_seconds)
    for i in range(min(len(ids), len(start))):
        x, st, en = int(ids[i]), int(start[i]), int(end[i])
        m = {"post_max": math.exp(float(mx[i])), "post_min": math.exp(float(mn[i])), "post_mean": math.exp(float(sm[i]) / (en - st + 1))}
        if real is not None:
            st, en = int(real[0][i]), int(real[1][i])
        t = {"id": x, "token": id2tok[x] if 0 <= x < len(id2tok) else None, "start_frame": st, "end_frame": en, "start_s": st * d,
             "end_s": (en + 1) * d, "measures": m, "confidence": m[which]}
        if n_final is not None:
            t["final"] = i < n_final
        out.append(t)
    return out


def measures_dict(five):
    """{measure: value} of a token's five values; None when the token has none (NaN: its utterance could not be aligned)."""
    if five[0] != five[0]:      # the kernel writes NaN to all five or to none
        return None
    return dict(zip(MEASURES, five))


def utterance(values):
    """The arithmetic mean of the tokens' values that are not None; None when there is none."""
    vals = [float(v) for v in values if v is not None]
    return math.fsum(vals) / len(vals) if vals else None


class TokenLog:
    """Per slot the timed tokens of a greedy stream: the closed runs (final) and, last, the run still open (final=False: its end and
    measures may still move)."""

    def __init__(self, slots, which, id2tok, frame_seconds):
        self.which, self.id2tok, self.d = measure(which) or "post_max", id2tok, float(frame_seconds)
        self.raw = [[] for _ in range(slots)]         # closed runs as the kernel's records: ([id, first, last], [8 words as floats])
        self.closed = [[] for _ in range(slots)]      # ... as dicts, built when tokens() asks (never more of them than raw holds)
        self.open = [None] * slots

    def reset(self, b):
        self.raw[b], self.closed[b], self.open[b] = [], [], None

    def _entry(self, rec_i, rec_f, final):
        x, st, en = int(rec_i[0]), int(rec_i[1]), int(rec_i[2])
        m = measures_dict(rec_f[3:8])
        return {"id": x, "token": self.id2tok[x] if 0 <= x < len(self.id2tok) else None, "start_frame": st, "end_frame": en,
                "start_s": st * self.d, "end_s": (en + 1) * self.d, "measures": m, "confidence": m[self.which] if m else None, "final": final}

    def ingest(self, buf, C, slots):
        """buf: asr_session_ctc_step_tokens' (slots, 13 + 9 C) int32 buffer on the host; slots: those the tick touched.  The tick keeps
        the records as words; they become dicts when tokens() asks."""
        R = K.STEP_TOKENS_REC
        ints = buf.numpy()
        flts = ints.view("float32")
        n_closed = ints[:, 4 + C].tolist()
        base, lo_open = 5 + C, 5 + C + C * R
        has_open = (ints[:, lo_open] >= 0).tolist()
        for b in slots:
            if n_closed[b]:
                hi = base + n_closed[b] * R
                self.raw[b] += zip(ints[b, base:hi].reshape(-1, R)[:, :3].tolist(), flts[b, base:hi].reshape(-1, R).tolist())
            self.open[b] = (ints[b, lo_open:lo_open + 3].tolist(), flts[b, lo_open:lo_open + R].tolist()) if has_open[b] else None

    def close(self, b):
        """The slot's input has ended: the open run is a token like the others."""
        if self.open[b] is not None:
            self.raw[b].append(self.open[b])
            self.open[b] = None

    def tokens(self, b):
        done = self.closed[b]
        done += [self._entry(i, f, True) for i, f in self.raw[b][len(done):]]
        return [dict(t) for t in done] + ([self._entry(*self.open[b], False)] if self.open[b] is not None else [])
