"""Definitions the independent-sessions kernels and rules are checked against (numpy float64 / integers, no GPU).

frame_best_blank   per frame: the best class (first maximum wins) and log p(blank) = log_softmax(logits)[blank] in float64
ctc_step           one tick of a slot's CTC bookkeeping: the collapse with the carried last class, the run of trailing silent
                   frames, the frames consumed, "decoded" - asr_session_ctc_step's contract (include/asr_hip.h)
endpoint_rule      WeNet's CTC endpoint rules, restated literally (wenet/runtime/core/decoder/ctc_endpoint.cc, which no binary here
                   pins): a rule fires when (decoded or not must_have_decoded) and trailing silence >= min_trailing_silence and
                   length >= min_length; the first that fires is reported.  Times are whole microseconds: frames * frame_us against
                   milliseconds * 1000, so no float rounding decides the frame at which a rule fires.
"""
import numpy as np

DEFAULT_RULES = (("silence_start", False, 5000, 0), ("silence_after_speech", True, 1000, 0), ("max_length", False, 0, 20000))


def frame_best_blank(logits, blank=0):
    """logits (R, V) -> (path (R,) int, blank_lp (R,) float64)."""
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(x - m).sum(axis=1))
    return x.argmax(axis=1), x[:, blank] - lse      # numpy's argmax returns the first maximum


def ctc_step(path, blank_lp, n_valid, reset, state, silence_lp, blank=0):
    """One slot, one tick.  path: the chunk's classes (None: beam sessions, nothing is emitted), blank_lp: its log p(blank) as float32
    values, n_valid: frames to consume, reset: start from the fresh state, state: (last, trailing, frames, decoded).
    -> (ids emitted, new state).  A frame is silent iff float32(blank_lp) > float32(silence_lp)."""
    last, trailing, frames, decoded = (blank, 0, 0, 0) if reset else state
    thr = np.float32(silence_lp)
    ids = []
    for t in range(n_valid):
        if path is not None:
            c = int(path[t])
            if c != blank and c != last:
                ids.append(c)
            last = c
        trailing = trailing + 1 if np.float32(blank_lp[t]) > thr else 0
    frames += n_valid
    if ids:
        decoded = 1
    return ids, (last, trailing, frames, decoded)


def endpoint_rule(trailing, frames, decoded, frame_us, rules=DEFAULT_RULES):
    trailing_us, length_us = trailing * frame_us, frames * frame_us
    for name, must_have_decoded, min_trailing_silence_ms, min_length_ms in rules:
        if must_have_decoded and not decoded:
            continue
        if trailing_us < min_trailing_silence_ms * 1000:
            continue
        if length_us < min_length_ms * 1000:
            continue
        return name
    return None
