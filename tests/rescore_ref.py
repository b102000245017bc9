"""Rescoring of n-best lists: the definition (include/asr_hip.h: asr_lm_score_nbest, asr_nbest_sweep), in plain Python and numpy, fp64.

The LM part restates nothing: NgramLM's host methods (asr_chinese_e2e_amd/lm.py: score, walk) are the statement.
    lm_scores(lm, lists)[u][e] = (lm.score(tokens), bias, state, len(tokens)) with (state, bias) = lm.walk(tokens); an absent entry
                                 (None) gives (0.0, 0.0, -1, 0)

An utterance is a list of N entries (None = absent: it keeps its index and takes part in nothing) with K <= 8 features each, finite or
-inf; a weight vector w has K finite values.
    total(f, w)   = t after: t = 0.0; for k ascending: if w[k] != 0.0: t = t + (w[k] * f[k]) - the product is rounded, then the sum
                    (Python floats: no fused multiply-add); a term of weight 0.0 is skipped, so 0 * -inf never happens
    unscorable    = some f[k] with w[k] != 0.0 is not finite; the total is then not formed
    pick          = the present, scorable entry of greatest total, the lowest index on ties (the search's own order); the present entry
                    of lowest index if none is scorable; an utterance with no present entry is refused
    order         = the scorable entries by descending total, then ascending index; then the unscorable ones by ascending index
    sweep         = for every grid point g the picks, tot[g] = (sum sub, sum del, sum ins, utterances whose pick has sub + del + ins > 0)
                    over the picks' error counts, cer[g] = (sub + del + ins) / ref_tokens; best = the fewest errors, then the fewest
                    wrong utterances, then the lowest grid index"""
import math

import numpy as np

MAX_N, MAX_K, MAX_G = 64, 8, 65536


def lm_scores(lm, lists):
    out = []
    for utt in lists:
        row = []
        for h in utt:
            if h is None:
                row.append((0.0, 0.0, -1, 0))
                continue
            h = [int(c) for c in h]
            state, bias = lm.walk(h)
            row.append((lm.score(h), bias, state, len(h)))
        out.append(row)
    return out


def _check_weights(w):
    w = [float(x) for x in w]
    if not 1 <= len(w) <= MAX_K or not all(math.isfinite(x) for x in w):
        raise ValueError(f"a weight vector has 1 to {MAX_K} finite values (got {w})")
    return w


def total(f, w):
    """(scorable, total) of one entry's features under w; total is None when the entry is unscorable."""
    t = 0.0
    for k in range(len(w)):
        if w[k] != 0.0:
            x = float(f[k])
            if x != x or x == math.inf:
                raise ValueError("a feature is NaN or +inf")
            if x == -math.inf:
                return False, None
            p = w[k] * x
            t = t + p
    return True, t


def totals(feats, present, w):
    """Per entry the total, None for an absent or unscorable one."""
    w = _check_weights(w)
    if len(feats) > MAX_N:
        raise ValueError(f"a list of {len(feats)} entries, the limit is {MAX_N}")
    if not any(present):
        raise ValueError("an utterance with no present entry")
    out = []
    for f, on in zip(feats, present):
        ok, t = total(f, w) if on else (False, None)
        out.append(t if ok else None)
    return out


def pick(feats, present, w):
    tot = totals(feats, present, w)
    best = None
    for e, t in enumerate(tot):
        if t is not None and (best is None or t > tot[best]):
            best = e
    return best if best is not None else [bool(p) for p in present].index(True)


def order(feats, present, w):
    """The present entries' indices: scorable ones by descending total then ascending index, then the unscorable ones by index."""
    tot = totals(feats, present, w)
    good = sorted((e for e, t in enumerate(tot) if t is not None), key=lambda e: (-tot[e], e))
    return good + [e for e, t in enumerate(tot) if t is None and present[e]]


def sweep(feats, present, err, grid, ref_len):
    """feats[u][e][k], present[u][e], err[u][e] = (sub, del, ins), grid[g][k], ref_len[u].  Returns {"pick" (G, U) int32, "tot" (G, 4)
    int64, "cer" (G) float64, "best"}."""
    G, U = len(grid), len(feats)
    if not 1 <= G <= MAX_G:
        raise ValueError(f"a grid of {G} points, between 1 and {MAX_G}")
    picks, tot = np.zeros((G, U), dtype=np.int32), np.zeros((G, 4), dtype=np.int64)
    for g, w in enumerate(grid):
        for u in range(U):
            p = pick(feats[u], present[u], w)
            picks[g, u] = p
            s, d, i = (int(x) for x in err[u][p])
            tot[g] += (s, d, i, int(s + d + i > 0))
    ref_tokens = int(sum(int(n) for n in ref_len))
    errs = tot[:, :3].sum(axis=1)
    cer = np.asarray([int(e) / ref_tokens if ref_tokens else (math.inf if e else 0.0) for e in errs], dtype=np.float64)
    best = min(range(G), key=lambda g: (int(errs[g]), int(tot[g, 3]), g))
    return {"pick": picks, "tot": tot, "cer": cer, "best": best, "ref_tokens": ref_tokens}
