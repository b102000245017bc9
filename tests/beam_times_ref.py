"""Token times and confidence of CTC prefix beam hypotheses: the definition (TEST INFRASTRUCTURE, float64, plain Python).

A dict-of-prefixes restatement of oracle/decode_ref.py::ctc_prefix_beam_search - the same candidates, the same merge rule, the same
ranking (a stable sort of the same insertion order) - in which every prefix also carries its best single alignment:

    vb, vnb   the fp64 log-probability of the best alignment that ends in blank / in non-blank
    hb, hnb   that alignment's records, one per token of the prefix: (start, end, mx, mn, sm) = the first and last absolute frame of the
              token's run, the largest and smallest log-posterior of the token over the run (float32) and their float32 sum, added one
              frame at a time in ascending t from the first value

At frame t, for a beam entry with last token e, tot = logadd(pb, pnb) and (v, h) = best(vb, vnb, hb, hnb):
    blank                 the same prefix:   vb'  <- v + lb,      hb'  <- h
    candidate c == e      the same prefix:   vnb' <- vnb + lp,    hnb' <- ext(hnb, t, lp)          (the repeat)
                          prefix + (c,):     vnb' <- vb + lp,     hnb' <- hb + (rec(t, lp),)
    candidate c != e      prefix + (c,):     vnb' <- v + lp,      hnb' <- h + (rec(t, lp),)
A contribution whose value is -inf is ignored.  Only the non-blank slot of a prefix that is already in the beam has two sources, its own
repeat and the extension of its parent: the larger value wins, the repeat on equality.  Every sum is v + float(lp) in that order.

Final records.  S = parent(h) over every non-empty hb / hnb of every live entry with a finite value, parent = the list without its last
record.  Every list of a later frame is a copy of one of these lists, an ext of one (the same parent) or an append to one (the list itself
becomes the parent), so it descends from a member of S: what all members of S share can never change, and the shared part can only
grow.  A record belongs to a token: two lists share a leading record only where their prefixes share the token it belongs to.  The final
count is the length of the longest leading part common to all members of S, none if one of those lists is empty.

Nothing of WeNet's is pinned here (its binaries are not available): this file is the definition the kernels are tested against, bit for
bit, and tests/test_beam_times_cpu.py pins it in turn to the oracle's strings and scores and to brute force over every alignment.
"""
import itertools
import math

import numpy as np

from oracle.decode_ref import NEG, logadd

f32 = np.float32


def rec(t, lp):
    lp = f32(lp)
    return (t, t, lp, lp, lp)


def ext(h, t, lp):
    s, e, mx, mn, sm = h[-1]
    lp = f32(lp)
    return h[:-1] + ((s, t, max(mx, lp), min(mn, lp), f32(sm + lp)),)


def best(vb, vnb, hb, hnb):
    return (vnb, hnb) if vnb > vb else (vb, hb)


class _Entry:
    __slots__ = ("pb", "pnb", "vb", "vnb", "hb", "hnb", "rep")

    def __init__(self, pb=NEG, pnb=NEG, vb=NEG, vnb=NEG, hb=(), hnb=()):
        self.pb, self.pnb, self.vb, self.vnb, self.hb, self.hnb = pb, pnb, vb, vnb, hb, hnb
        self.rep = False      # vnb came from the prefix's own repeat

    def total(self):
        return logadd(self.pb, self.pnb)


class BeamTimes:
    """The search, one frame at a time: step(lb, cands) with lb = the blank's log-posterior and cands = [(class, log-posterior)] of the
    frame (blank entries are skipped); hyps() and final_count() at any point."""

    def __init__(self, beam_size, blank=0):
        self.beam_size, self.blank, self.t = int(beam_size), blank, 0
        self.beam = {(): _Entry(pb=0.0, vb=0.0)}

    def step(self, lb, cands):
        t, nxt = self.t, {}

        def slot(prefix):
            if prefix not in nxt:
                nxt[prefix] = _Entry()
            return nxt[prefix]

        def acc_b(prefix, p, v, h):
            cur = slot(prefix)
            cur.pb = logadd(cur.pb, p)
            if v != NEG and v > cur.vb:
                cur.vb, cur.hb = v, h

        def acc_nb(prefix, p, v, h, rep):
            cur = slot(prefix)
            cur.pnb = logadd(cur.pnb, p)
            if v != NEG and (v > cur.vnb or (v == cur.vnb and rep and not cur.rep)):
                cur.vnb, cur.hnb, cur.rep = v, h, rep

        lb = float(lb)
        for prefix, en in self.beam.items():
            v, h = best(en.vb, en.vnb, en.hb, en.hnb)
            acc_b(prefix, en.total() + lb, v + lb, h)
            for c, lp in cands:
                c, lpd = int(c), float(lp)
                if c == self.blank:
                    continue
                if prefix and c == prefix[-1]:
                    acc_nb(prefix, en.pnb + lpd, en.vnb + lpd, ext(en.hnb, t, lp) if en.vnb != NEG else (), True)
                    acc_nb(prefix + (c,), en.pb + lpd, en.vb + lpd, en.hb + (rec(t, lp),), False)
                else:
                    acc_nb(prefix + (c,), en.total() + lpd, v + lpd, h + (rec(t, lp),), False)
        ranked = sorted(nxt.items(), key=lambda kv: kv[1].total(), reverse=True)[:self.beam_size]
        self.beam = dict(ranked)
        self.t += 1

    def hyps(self):
        """Best first, entries of zero probability left out: {"prefix", "score", "viterbi_score", "records"}."""
        out = []
        for prefix, en in sorted(self.beam.items(), key=lambda kv: kv[1].total(), reverse=True):
            if en.total() == NEG:
                continue
            v, h = best(en.vb, en.vnb, en.hb, en.hnb)
            out.append({"prefix": prefix, "score": en.total(), "viterbi_score": v, "records": h})
        return out

    def final_count(self):
        members = []
        for prefix, en in self.beam.items():
            if en.total() == NEG:
                continue
            for v, h in ((en.vb, en.hb), (en.vnb, en.hnb)):
                if v == NEG:
                    continue
                if not h:
                    return 0
                members.append(tuple(zip(prefix[:-1], h[:-1])))
        n = 0
        for col in zip(*members):
            if any(x != col[0] for x in col):
                break
            n += 1
        return n if members else 0


def frames_of(logp, blank=0, candidates=None):
    """The frames of a (T, V) array of log-posteriors as step() takes them (candidates as the oracle's: None = every class)."""
    T, V = logp.shape
    return [(logp[t, blank], [(int(c), logp[t, int(c)]) for c in (range(V) if candidates is None else candidates[t])]) for t in range(T)]


def search(frames, beam_size, blank=0):
    s = BeamTimes(beam_size, blank)
    for lb, cands in frames:
        s.step(lb, cands)
    return s


def measures(record):
    s, e, mx, mn, sm = record
    return {"post_max": math.exp(mx), "post_min": math.exp(mn), "post_mean": math.exp(float(sm) / (e - s + 1))}


def viterbi_bruteforce(logp, labels, blank=0):
    """max over the alignments that spell `labels` of their log-probability, summed in ascending t from 0.0 (tiny T and V only)."""
    T, V = logp.shape
    top = NEG
    for path in itertools.product(range(V), repeat=T):
        col, prev = [], None
        for c in path:
            if c != prev and c != blank:
                col.append(c)
            prev = c
        if tuple(col) == tuple(labels):
            v = 0.0
            for t, c in enumerate(path):
                v = v + float(logp[t, c])
            top = max(top, v)
    return top
