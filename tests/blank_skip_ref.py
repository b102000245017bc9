"""Blank-frame skipping in front of the CTC prefix beam search: the definition, in plain Python.  Everything else - the compaction
kernel, the host loop, the streamed and the sessions searches - is tested against this file.

blank_skip = p with 0 < p <= 1.  thr = float32(log(float32(p))), computed once on the host.
Frame t of an utterance is HIGH iff blank_lp[t] > thr: float32 against float32, strict, so a NaN is not high.
Frame t is DROPPED iff it is high and frame t - 1 of the same utterance exists and is high: the head of every run of high frames is kept.
  - one blank still separates "A _ _ _ A" from "A A": a doubled character survives, in every hypothesis;
  - the rule is causal: across a chunk boundary one bit travels (the last consumed frame was high), so any cutting gives the same set.
The search with blank_skip = p is by definition the search on the kept rows, in order, with the kept count as its length."""
import numpy as np


def threshold(p):
    return np.float32(np.log(np.float32(p)))


def is_high(lp, thr):
    return bool(np.float32(lp) > np.float32(thr))


def kept_frames(blank_lp, thr, carry=False):
    """(the kept frame indices of one utterance in order, the carry bit behind its last frame).  carry: the frame in front of frame 0
    was high (a chunk in the middle of a stream); False at the start of an utterance."""
    kept = []
    for t in range(len(blank_lp)):
        high = is_high(blank_lp[t], thr)
        if not (high and carry):
            kept.append(t)
        carry = high
    return kept, carry


def kept_frames_chunked(blank_lp, cuts, thr):
    """The same set from chunks: cuts = the chunk lengths (zeros allowed, summing to the frame count); indices are absolute."""
    kept, carry, t0 = [], False, 0
    for n in cuts:
        k, carry = kept_frames(blank_lp[t0:t0 + n], thr, carry)
        kept += [t0 + t for t in k]
        t0 += n
    assert t0 == len(blank_lp)
    return kept


def kept_frames_drop_every_high(blank_lp, thr):
    """NOT the definition: the variant that drops every high frame, which merges a doubled character (tests show why the head stays)."""
    return [t for t in range(len(blank_lp)) if not is_high(blank_lp[t], thr)]


def compact(vals, ids, blank_lp, in_len, thr):
    """vals / ids (B, T, k), blank_lp (B, T) numpy, in_len (B): (vals, ids, blank_lp of the same shapes with the kept rows first and zeros
    behind them, out_len (B), out_frame (B, T) = the frame of every kept row, zeros behind them).  Rows at and past in_len are not read."""
    B, T = blank_lp.shape
    ov, oi, ob = np.zeros_like(vals), np.zeros_like(ids), np.zeros_like(blank_lp)
    out_len, out_frame = np.zeros(B, dtype=np.int32), np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        kept, _ = kept_frames(blank_lp[b, :int(in_len[b])], thr)
        n = out_len[b] = len(kept)
        ov[b, :n], oi[b, :n], ob[b, :n], out_frame[b, :n] = vals[b, kept], ids[b, kept], blank_lp[b, kept], kept
    return ov, oi, ob, out_len, out_frame
