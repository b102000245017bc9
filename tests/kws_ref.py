"""Keyword spotting on the CTC posteriors: the definition (include/asr_hip.h, csrc/kws.hip), in plain numpy float32, and a float64
brute force over every alignment.  The kernels agree with this file bit for bit; wekws / WeNet were not on hand, the definition is ours.

A frame's emissions are lp_t(v) = float32(logits[t, v]) - lse[t], one float32 subtraction (lse: asr_ctc_frame_stats over the same rows).
A keyword w_0 .. w_{L-1} (1 <= L <= 16, no blank) has the states s = 0 .. 2L-2: even s = 2i emits lp_t(w_i), odd s emits lp_t(blank), the
optional blank between w_i and w_{i+1}.  No leading and no trailing blank: a match begins on w_0 and ends on w_{L-1}.

    D_{-1}(s) = -inf, start_{-1}(s) = -1.  At frame t:
      s = 0:   best = 0.0, bs = t                      (a match may begin on any frame; every continued path has D <= 0)
      s >= 1:  best = D_{t-1}(s), bs = start_{t-1}(s);
               those of s-1 iff D_{t-1}(s-1) > best    (strict)
               for even s >= 2 with w_{s/2} != w_{s/2-1}: those of s-2 iff D_{t-1}(s-2) > best    (strict, after the step above)
      D_t(s) = best + e_t(s)                           (one float32 addition)
      start_t(s) = bs if best > -inf else -1
    H_t = D_t(2L-2), hs_t = start_t(2L-2)

Frame t is a candidate iff H_t >= thr and hs_t >= 0 and t - hs_t + 1 <= span.  A maximal run of candidate frames is one hit: end = the
frame of the run's largest H (the first on ties), start = that frame's hs, score = its H.  A run closes on the first frame that is no
candidate, or behind the last frame.  Per (utterance, keyword) and call the first `cap` hits are kept, the count keeps counting."""
import itertools
import math

import numpy as np

MAX_LEN = 16
NEG = np.float32(-np.inf)


def threshold(L, p):
    """thr = float32(L ln p): exp(H / L), the geometric mean per character, is compared with p."""
    return np.float32(int(L) * math.log(float(p)))


def max_token_frames(max_token_s, frame_seconds):
    return max(1, int(math.floor(float(max_token_s) / float(frame_seconds) + 1e-9)))


def span_cap(L, max_token_s, frame_seconds):
    return int(L) * max_token_frames(max_token_s, frame_seconds)


def emissions(logits, lse):
    """logits (T, V) of any float dtype whose values float32 holds exactly, lse (T) float32 -> lp (T, V) float32."""
    with np.errstate(invalid="ignore"):
        return np.asarray(logits, dtype=np.float32) - np.asarray(lse, dtype=np.float32)[:, None]


# ------------------------------------------------------------------------------------------------ the recursion, one keyword, loops
def new_state(L):
    S = 2 * L - 1
    return [NEG] * S, [-1] * S


def frame_step(D, st, lp_t, kw, t, blank=0):
    """One frame, as the docstring says it: (D, start) of frame t - 1 -> those of frame t (new lists)."""
    L = len(kw)
    nD, nst = [None] * (2 * L - 1), [None] * (2 * L - 1)
    for s in range(2 * L - 1):
        if s == 0:
            best, bs = np.float32(0.0), t
        else:
            best, bs = D[s], st[s]
            if D[s - 1] > best:
                best, bs = D[s - 1], st[s - 1]
            if s % 2 == 0 and kw[s // 2] != kw[s // 2 - 1] and D[s - 2] > best:
                best, bs = D[s - 2], st[s - 2]
        e = np.float32(lp_t[kw[s // 2] if s % 2 == 0 else blank])
        nD[s] = np.float32(best + e)
        nst[s] = bs if best > NEG else -1
    return nD, nst


def scan_loops(lp, kw, blank=0):
    """lp (T, V) float32 -> (H (T) float32, hs (T) int) of one keyword."""
    D, st = new_state(len(kw))
    H, hs = [], []
    for t in range(len(lp)):
        D, st = frame_step(D, st, lp[t], kw, t, blank)
        H.append(D[-1])
        hs.append(st[-1])
    return np.array(H, dtype=np.float32).reshape(-1), np.array(hs, dtype=np.int64).reshape(-1)


# ------------------------------------------------------------------------------------------------ the same over a list of keywords
class Scanner:
    """The recursion for K keywords at once (arrays (K, S), S = 2 max L - 1; a keyword's states past 2L-2 are computed and never read:
    a state depends on lower states only).  Resumable: step(lp_t) takes the frames one at a time, t counts from the first."""

    def __init__(self, keywords, blank=0):
        self.kws = [[int(x) for x in k] for k in keywords]
        K, Lm = len(self.kws), max(len(k) for k in self.kws)
        S = 2 * Lm - 1
        self.sym = np.full((K, S), blank, dtype=np.int64)
        self.skip = np.zeros((K, S), dtype=bool)
        self.last = np.array([2 * len(k) - 2 for k in self.kws])
        for i, k in enumerate(self.kws):
            for s in range(0, 2 * len(k) - 1, 2):
                self.sym[i, s] = k[s // 2]
                self.skip[i, s] = s >= 2 and k[s // 2] != k[s // 2 - 1]
        self.rows = np.arange(K)
        self.reset()

    def reset(self):
        K, S = self.sym.shape
        self.D = np.full((K, S), NEG, dtype=np.float32)
        self.st = np.full((K, S), -1, dtype=np.int64)
        self.t = 0

    def step(self, lp_t):
        """-> (H (K) float32, hs (K) int) of this frame."""
        D, st = self.D, self.st
        K = D.shape[0]
        best, bs = D.copy(), st.copy()
        D1 = np.concatenate([np.full((K, 1), NEG, dtype=np.float32), D[:, :-1]], 1)
        s1 = np.concatenate([np.full((K, 1), -1, dtype=np.int64), st[:, :-1]], 1)
        m = D1 > best
        best, bs = np.where(m, D1, best), np.where(m, s1, bs)
        D2 = np.concatenate([np.full((K, 2), NEG, dtype=np.float32), D[:, :-2]], 1)[:, :D.shape[1]]
        s2 = np.concatenate([np.full((K, 2), -1, dtype=np.int64), st[:, :-2]], 1)[:, :D.shape[1]]
        m = self.skip & (D2 > best)
        best, bs = np.where(m, D2, best), np.where(m, s2, bs)
        best[:, 0], bs[:, 0] = np.float32(0.0), self.t
        with np.errstate(invalid="ignore"):
            self.D = (best + np.asarray(lp_t, dtype=np.float32)[self.sym]).astype(np.float32)
        self.st = np.where(best > NEG, bs, -1)
        self.t += 1
        return self.D[self.rows, self.last].copy(), self.st[self.rows, self.last].copy()


def scan(lp, keywords, blank=0):
    """lp (T, V) float32 -> (H (T, K) float32, hs (T, K) int)."""
    sc = Scanner(keywords, blank)
    K = len(sc.kws)
    H, hs = np.zeros((len(lp), K), dtype=np.float32), np.zeros((len(lp), K), dtype=np.int64)
    for t in range(len(lp)):
        H[t], hs[t] = sc.step(lp[t])
    return H, hs


# ------------------------------------------------------------------------------------------------ candidates, runs, hits
def is_candidate(H, hs, t, thr, span):
    return bool(H >= thr) and hs >= 0 and t - hs + 1 <= span


class Runs:
    """The open run of one (utterance, keyword): feed(t, H, hs) returns the hit a frame closes (or None), close() the open one."""

    def __init__(self, thr, span):
        self.thr, self.span, self.open = np.float32(thr), int(span), None

    def feed(self, t, H, hs):
        if is_candidate(H, hs, t, self.thr, self.span):
            if self.open is None or H > self.open[2]:      # strict: the first frame of equal H keeps the run
                self.open = (int(hs), int(t), np.float32(H))
            return None
        return self.close()

    def close(self):
        hit, self.open = self.open, None
        return hit


def hits_of(H, hs, thr, span):
    """One (utterance, keyword): H, hs (T) -> every hit (start, end, score float32), in order; an open run closes behind the last frame."""
    r, out = Runs(thr, span), []
    for t in range(len(H)):
        h = r.feed(t, H[t], hs[t])
        if h is not None:
            out.append(h)
    h = r.close()
    if h is not None:
        out.append(h)
    return out


def search(lp_list, keywords, thr, span, blank=0):
    """lp_list: per utterance lp (T_b, V) float32 (T_b may be 0).  -> per utterance, per keyword: the list of hits (uncapped)."""
    out = []
    for lp in lp_list:
        if len(lp) == 0:
            out.append([[] for _ in keywords])
            continue
        H, hs = scan(lp, keywords, blank)
        out.append([hits_of(H[:, k], hs[:, k], thr[k], span[k]) for k in range(len(keywords))])
    return out


def bits(x):
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


def capped(per_keyword, cap):
    """asr_kws_search's outputs for one utterance: (count (K), records (K, cap, 3) int32 {start, end, score bits}, 0 behind)."""
    K = len(per_keyword)
    cnt, rec = np.zeros(K, dtype=np.int32), np.zeros((K, cap, 3), dtype=np.int32)
    for k, hits in enumerate(per_keyword):
        cnt[k] = len(hits)
        for i, (s, e, sc) in enumerate(hits[:cap]):
            rec[k, i] = (s, e, bits(sc))
    return cnt, rec


def compact(per_keyword, cap, max_hits):
    """asr_kws_compact's outputs for one utterance: (count, dropped, hits (max_hits, 4) int32 {keyword, start, end, score bits}), the
    order keyword ascending, then end ascending; dropped = every hit found and not written."""
    rows = [(k, s, e, bits(sc)) for k, hits in enumerate(per_keyword) for (s, e, sc) in hits[:cap]]
    found = sum(len(h) for h in per_keyword)
    out = np.zeros((max_hits, 4), dtype=np.int32)
    n = min(len(rows), max_hits)
    if n:
        out[:n] = np.array(rows[:n], dtype=np.int64).astype(np.int32)
    return n, found - n, out


class Stream:
    """The resumable form for one slot: push(lp (n, V), final) -> per keyword the hits closed by these frames (frames count from the
    slot's first frame); final closes the open runs.  Any cutting of the frames gives the hits of search() over all of them."""

    def __init__(self, keywords, thr, span, blank=0):
        self.sc = Scanner(keywords, blank)
        self.runs = [Runs(thr[k], span[k]) for k in range(len(self.sc.kws))]

    def push(self, lp, final=False):
        out = [[] for _ in self.runs]
        for row in lp:
            t = self.sc.t
            H, hs = self.sc.step(row)
            for k, r in enumerate(self.runs):
                h = r.feed(t, H[k], hs[k])
                if h is not None:
                    out[k].append(h)
        if final:
            for k, r in enumerate(self.runs):
                h = r.close()
                if h is not None:
                    out[k].append(h)
        return out


# ------------------------------------------------------------------------------------------------ float64 brute force
def brute_force(lp, kw, blank=0):
    """H_t in float64 by enumeration: the largest sum of lp over every path of states that begins in state 0 on some frame s, ends in
    state 2L-2 on frame t, and moves by 0, +1, or +2 (onto an even state whose character differs from the one before).  -> (H (T) float64,
    starts: per t the set of s that reach the maximum; empty where no alignment exists)."""
    T, L = len(lp), len(kw)
    S = 2 * L - 1
    lp = np.asarray(lp, dtype=np.float64)
    H = np.full(T, -np.inf)
    starts = [set() for _ in range(T)]
    for s0 in range(T):
        for t in range(s0, T):
            n = t - s0 + 1
            for moves in itertools.product((0, 1, 2), repeat=n - 1):
                if sum(moves) != S - 1:
                    continue
                s, tot, ok = 0, lp[s0][kw[0]], True
                for i, m in enumerate(moves):
                    s += m
                    if m == 2 and (s % 2 == 1 or kw[s // 2] == kw[s // 2 - 1]):
                        ok = False
                        break
                    tot += lp[s0 + 1 + i][kw[s // 2] if s % 2 == 0 else blank]
                if not ok or tot == -np.inf:
                    continue
                if tot > H[t]:
                    H[t], starts[t] = tot, {s0}
                elif tot == H[t]:
                    starts[t].add(s0)
    return H, starts
