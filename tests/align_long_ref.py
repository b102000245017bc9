"""The definition asr_ctc_align_long is compared with bit for bit: the best single CTC path of labels[0..L) through T frames in the
log domain, float64, plain numpy (one vectorised step per frame).

Emission: lp(t, c) = float32(logit[t, c]) - lse[t], ONE float32 subtraction (bf16 -> float32 is exact).
States s = 0 .. 2L, blanks at even s, label (s - 1) / 2 at odd s.
    v[0] = float64(lp(0, blank)), v[1] = float64(lp(0, lab[0])), the rest -inf
    v'[s] = best + float64(lp(t, sym(s))), best = the maximum of v[s], v[s-1] and - for odd s >= 3 with lab[i] != lab[i-1] - v[s-2]
    ties prefer s, then s-1, then s-2 (strict >); the end is the larger of v[2L] and v[2L-1], the blank on ties
    T = 0 is feasible iff L = 0 (score 0.0); an infeasible pair has score -inf, spans -1, tok -inf and a path of -1
Per token i on its run [s_i, e_i]: sm = the float32 sum from 0.f of lp(t, lab[i]) in ascending t (confidence.py's convention), mx / mn
the largest / smallest such lp.  Every operation is a named IEEE operation on named operands in a named order, so no tolerance exists.

brute(): every alignment, for T <= 7 and L <= 3.  margin(): the smallest gap between the winning and the runner-up finite predecessor
over all cells - used only where a result is compared with asr_ctc_align, which works in a rescaled probability domain and may break
a near tie differently."""
import numpy as np

NEG = -np.inf


def emissions(rows, lse):
    """lp (T, V) float32 from rows (T, >= V) float32 (bf16 rows: converted exactly by the caller) and lse (T,) float32."""
    rows, lse = np.asarray(rows, dtype=np.float32), np.asarray(lse, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (rows - lse[:, None]).astype(np.float32)


def align(rows, lse, labels, blank=0, want_margin=False):
    """-> dict(score float64, path (T,) int64, spans (L, 2) int64, tok (L, 3) float32 = sm, mx, mn[, margin float64])."""
    lp = emissions(rows, lse)
    T, lab = lp.shape[0], np.asarray(labels, dtype=np.int64).reshape(-1)
    L = lab.shape[0]
    S = 2 * L + 1
    out = dict(score=NEG, path=np.full(T, -1, np.int64), spans=np.full((L, 2), -1, np.int64), tok=np.full((L, 3), NEG, np.float32))
    if want_margin:
        out["margin"] = np.inf
    if T == 0:
        out["score"] = 0.0 if L == 0 else NEG
        return out
    sym = np.full(S, blank, np.int64)
    sym[1::2] = lab
    skip = np.zeros(S, bool)
    skip[3::2] = lab[1:] != lab[:-1]
    v = np.full(S, NEG)
    v[0] = np.float64(lp[0, blank])
    if L:
        v[1] = np.float64(lp[0, lab[0]])
    bp = np.zeros((T, S), np.int8)
    mg = np.inf
    for t in range(1, T):
        a1, a2 = np.full(S, NEG), np.full(S, NEG)
        a1[1:] = v[:-1]
        a2[2:] = v[:-2]
        a2[~skip] = NEG
        best, code = v.copy(), np.zeros(S, np.int8)
        m = a1 > best
        best[m], code[m] = a1[m], 1
        m = a2 > best
        best[m], code[m] = a2[m], 2
        if want_margin:
            c = np.sort(np.stack((v, a1, a2)), axis=0)
            both = np.isfinite(c[1])
            if both.any():
                mg = min(mg, float((c[2][both] - c[1][both]).min()))
        with np.errstate(invalid="ignore"):
            v = best + lp[t, sym].astype(np.float64)
        bp[t] = code
    if want_margin:
        if L and np.isfinite(v[2 * L]) and np.isfinite(v[2 * L - 1]):
            mg = min(mg, abs(float(v[2 * L] - v[2 * L - 1])))
        out["margin"] = mg
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
    out["path"] = np.where(odd, states // 2, -1)
    for i in range(L):
        ts = np.flatnonzero(states == 2 * i + 1)
        out["spans"][i] = (ts[0], ts[-1])
        x = lp[ts[0]:ts[-1] + 1, lab[i]]
        sm = np.float32(0.0)
        for e in x:
            sm = np.float32(sm + e)
        out["tok"][i] = (sm, x.max(), x.min())
    return out


def brute(rows, lse, labels, blank=0):
    """(best score, [state sequences that reach it exactly]) over every alignment the CTC topology allows, scored as align() scores
    (float64 sums of the float32 emissions in ascending t); (-inf, []) when there is none.  T <= 7, L <= 3."""
    lp = emissions(rows, lse)
    T, L = lp.shape[0], len(labels)
    assert T <= 7 and L <= 3
    S = 2 * L + 1
    ext = [blank if s % 2 == 0 else labels[s // 2] for s in range(S)]
    if T == 0:
        return (0.0, [[]]) if L == 0 else (NEG, [])
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
            walk(seq + [b], sc + np.float64(lp[t, ext[b]]))

    for s0 in range(min(2, S)):
        walk([s0], np.float64(lp[0, ext[s0]]))
    return best, paths


def states_of(path, spans, T):
    """The state sequence of an align() result (path of token indices): blanks between tokens take the even state after the last token."""
    out, last = [], -1
    for t in range(T):
        if path[t] >= 0:
            last = int(path[t])
            out.append(2 * last + 1)
        else:
            out.append(2 * (last + 1))
    return out


def repeats(labels):
    lab = np.asarray(labels).reshape(-1)
    return int((lab[1:] == lab[:-1]).sum())


def peaky_case(T, L, V, peak, seed, blank=0):
    """(rows (T, V) float32, lse (T,) float32, labels): random logits with `peak` added along one alignment (every token on one even
    frame, blanks elsewhere; T >= 2 L), so the lattice has a clear winner almost everywhere."""
    rng = np.random.RandomState(seed)
    labels = (blank + 1 + rng.randint(0, V - 1, L)) % V
    assert T >= 2 * L
    rows = rng.normal(0.0, 1.0, (T, V)).astype(np.float32)
    frame_sym = np.full(T, blank)
    frame_sym[2 * np.sort(rng.choice(T // 2, L, replace=False))] = labels
    rows[np.arange(T), frame_sym] += np.float32(peak)
    return rows, lse_of(rows), labels


def lse_of(rows):
    x = np.asarray(rows, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = x.max(-1, keepdims=True)
        return (m[:, 0] + np.log(np.exp(x - m).sum(-1))).astype(np.float32)
