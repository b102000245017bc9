"""The definition asr_ctc_align_long_filler is compared with bit for bit: tests/align_long_ref.py's best single CTC path, with some of its
blank states marked WIDE.  float64, plain numpy.

No state is added and the topology does not change.  gap[i] (i < L) marks the blank state 2i in front of label i, gap_tail the last state
2L.  The caller gives one float32 per frame, star[t]: the log-probability of "anything".  With eb = lp(t, blank) (float32, as today), a
wide blank state emits on frame t
    star[t] if star[t] > eb, else eb                (strict: the blank wins ties; the chosen float32 is converted to float64 as today)
at t = 0 (v[0]) too, and in the L = 0 sum.  The recursion max(v[s], v[s-1], v[s-2]), the tie order, the choice of the end state and the
float32 token sums are align_long_ref's.  path[t] gains the value -2: frame t sits in a wide blank state and star[t] > eb (a filler
frame); a plain blank frame stays -1.

By construction: with every flag 0, or with star = -inf everywhere, every output has align_long_ref.align's bits; and a wide blank stays
optional and skippable like any blank, so a script that matches its audio (the blank being the best class of its gap frames, star at most
the best class) aligns exactly as without, score included.

brute(): every alignment, for T <= 7 and L <= 3, with the wide emission."""
import numpy as np

from tests.align_long_ref import emissions

NEG = -np.inf


def wide_states(L, gap, gap_tail):
    """(2L + 1,) bool: the states that are wide blanks."""
    w = np.zeros(2 * L + 1, bool)
    w[0:2 * L:2] = np.asarray(gap, dtype=np.uint8).reshape(-1)[:L] != 0
    w[2 * L] = bool(gap_tail)
    return w


def align(rows, lse, star, labels, gap, gap_tail, blank=0):
    """-> dict(score float64, path (T,) int64 with -2 on filler frames, spans (L, 2) int64, tok (L, 3) float32 = sm, mx, mn)."""
    lp = emissions(rows, lse)
    star = np.asarray(star, dtype=np.float32).reshape(-1)
    T, lab = lp.shape[0], np.asarray(labels, dtype=np.int64).reshape(-1)
    L = lab.shape[0]
    S = 2 * L + 1
    assert star.shape[0] == T and np.asarray(gap).reshape(-1).shape[0] == L and not np.isnan(star).any()
    out = dict(score=NEG, path=np.full(T, -1, np.int64), spans=np.full((L, 2), -1, np.int64), tok=np.full((L, 3), NEG, np.float32))
    if T == 0:
        out["score"] = 0.0 if L == 0 else NEG
        return out
    wide = wide_states(L, gap, gap_tail)
    sym = np.full(S, blank, np.int64)
    sym[1::2] = lab
    skip = np.zeros(S, bool)
    skip[3::2] = lab[1:] != lab[:-1]
    fill = star > lp[:, blank]      # (T,): a wide blank state emits star[t] on these frames (strict >)

    wide_at = np.flatnonzero(wide)

    def emit(t):      # (S,) float64: the float32 each state emits on frame t, converted
        e = lp[t].take(sym)
        if fill[t]:
            e[wide_at] = star[t]
        return e.astype(np.float64)

    v = np.full(S, NEG)
    v[:min(2, S)] = emit(0)[:min(2, S)]
    bp = np.zeros((T, S), np.int8)
    a1, a2 = np.full(S, NEG), np.full(S, NEG)
    for t in range(1, T):      # align_long_ref's step: s, then s-1, then (where the skip exists) s-2, each only if strictly larger
        a1[1:] = v[:-1]
        a2[2:] = v[:-2]
        m1 = a1 > v
        best = np.where(m1, a1, v)
        m2 = skip & (a2 > best)
        best = np.where(m2, a2, best)
        with np.errstate(invalid="ignore"):
            v = best + emit(t)
        bp[t] = np.where(m2, 2, m1)
    s = 2 * L
    if L and v[2 * L - 1] > v[2 * L]:
        s = 2 * L - 1
    if not v[s] > NEG:
        return out
    out["score"] = float(v[s])
    states = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    odd = states % 2 == 1
    out["path"] = np.where(odd, states // 2, np.where(wide[states] & fill, -2, -1))
    for i in range(L):
        ts = np.flatnonzero(states == 2 * i + 1)
        out["spans"][i] = (ts[0], ts[-1])
        x = lp[ts[0]:ts[-1] + 1, lab[i]]
        sm = np.float32(0.0)
        for e in x:
            sm = np.float32(sm + e)
        out["tok"][i] = (sm, x.max(), x.min())
    return out


def brute(rows, lse, star, labels, gap, gap_tail, blank=0):
    """(best score, [state sequences that reach it exactly]) over every alignment the CTC topology allows, scored as align() scores
    (float64 sums of the float32 emissions in ascending t, wide blanks emitting the larger of star and the blank, the blank on ties);
    (-inf, []) when there is none.  T <= 7, L <= 3."""
    lp = emissions(rows, lse)
    star = np.asarray(star, dtype=np.float32).reshape(-1)
    T, L = lp.shape[0], len(labels)
    assert T <= 7 and L <= 3
    S = 2 * L + 1
    ext = [blank if s % 2 == 0 else labels[s // 2] for s in range(S)]
    wide = wide_states(L, gap, gap_tail)
    if T == 0:
        return (0.0, [[]]) if L == 0 else (NEG, [])

    def e(t, s):
        x = lp[t, ext[s]]
        if wide[s] and star[t] > lp[t, blank]:
            x = star[t]
        return np.float64(x)

    best, paths = NEG, []

    def walk(seq, sc):      # every continuation the topology allows, depth first
        nonlocal best, paths
        t, a = len(seq), seq[-1]
        if t == T:
            if a >= 2 * L - 1:
                if sc > best:
                    best, paths = float(sc), [list(seq)]
                elif sc == best:
                    paths.append(list(seq))
            return
        for b in (a, a + 1, a + 2):
            if b >= S or (b - a == 2 and (b % 2 == 0 or ext[b] == ext[a])):
                continue
            walk(seq + [b], sc + e(t, b))

    for s0 in range(min(2, S)):
        walk([s0], e(0, s0))
    return best, paths


def states_of(path, T):
    """The state sequence of an align() result: blank and filler frames take the even state after the last token."""
    out, last = [], -1
    for t in range(T):
        if path[t] >= 0:
            last = int(path[t])
            out.append(2 * last + 1)
        else:
            out.append(2 * (last + 1))
    return out


def toy(penalty, seed=0):
    """The script [1, 2 | 3, 4] over frames peaked 1 _ 2 _ 5 5 5 _ 5 _ 3 _ 4 _ (class 5 is in no label; peak + 6 on small noise), gaps at
    the line starts and the tail, star = max_c lp - penalty -> (rows, lse, star, labels, gap, gap_tail, peaked class per frame)."""
    from tests.align_long_ref import lse_of
    peaked = np.array([1, 0, 2, 0, 5, 5, 5, 0, 5, 0, 3, 0, 4, 0])
    rows = np.random.RandomState(seed).normal(0.0, 0.5, (len(peaked), 6)).astype(np.float32)
    rows[np.arange(len(peaked)), peaked] += np.float32(6.0)
    lse = lse_of(rows)
    star = (emissions(rows, lse).max(-1) - np.float32(penalty)).astype(np.float32)
    return rows, lse, star, np.array([1, 2, 3, 4]), np.array([1, 0, 1, 0], np.uint8), 1, peaked


def filler_case(L, V, seed, flagged, unflagged=(), tail_frames=3, run=2, peak=5.0, blank=0):
    """Inputs in the manner of align_long_ref.peaky_case with foreign audio: class V - 1 is kept out of the labels and peaked on `run`
    frames inserted in front of every pair in `flagged` (whose gap flag is set) and in `unflagged` (whose flag is not, unless it is in
    `flagged` too) and on `tail_frames` frames after the last token; every token is peaked on one frame with a blank-peaked frame behind
    it.  star = max_c lp - 1 on the inserted frames and on every third frame (below the blank where the blank is the best class, above it
    elsewhere), -inf on the rest.
    -> (rows (T, V) float32, lse, star, labels, gap (L,) uint8, gap_tail = 1)."""
    from tests.align_long_ref import lse_of
    rng = np.random.RandomState(seed)
    labels = 1 + rng.randint(0, V - 2, L)      # classes 1 .. V - 2
    flagged = sorted(set(int(i) for i in flagged if 0 <= int(i) < L))
    insert = set(flagged) | set(int(i) for i in unflagged if 0 <= int(i) < L)
    sym, foreign = [], []
    for i in range(L):
        if i in insert:
            foreign += list(range(len(sym), len(sym) + run))
            sym += [V - 1] * run
        sym += [int(labels[i]), blank]
    foreign += list(range(len(sym), len(sym) + tail_frames))
    sym += [V - 1] * tail_frames + [blank]
    T = len(sym)
    rows = rng.normal(0.0, 1.0, (T, V)).astype(np.float32)
    rows[np.arange(T), np.array(sym)] += np.float32(peak)
    lse = lse_of(rows)
    star = np.full(T, NEG, np.float32)
    on = np.zeros(T, bool)
    on[foreign] = True
    on[::3] = True
    star[on] = (emissions(rows, lse).max(-1) - np.float32(1.0)).astype(np.float32)[on]
    gap = np.zeros(L, np.uint8)
    gap[flagged] = 1
    return rows, lse, star, labels, gap, 1
