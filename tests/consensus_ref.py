"""Consensus decoding of n-best lists: the definition (include/asr_hip.h: asr_nbest_consensus), in plain Python and numpy integers on top
of tests/score_ref.py.

An utterance is a list of hypotheses h_0 .. h_{N-1} (id lists, best first; None = absent: it keeps its index and takes part in nothing)
with integer weights w_k >= 0.
    d[i][k]   = the edit distance of h_i and h_k (score_ref.table), 0 where a side is absent
    risk[i]   = sum_k w_k * d[i][k] over the present k; pivot = the present i with the least risk, the lowest i on ties; W = sum_k w_k
    alignment = score_ref.align(ref=h_pivot, hyp=h_k) for every present k: the pivot is the row side
    slots     = 2 m + 1 for m = len(h_pivot): slot 2 i + 1 is pivot position i, slot 2 g the gap in front of position g (g = m: the end)
    vote[k][2 i + 1] = h_k's token of the COR / SUB op at ref_pos i, EPS for a DEL
    vote[k][2 g]     = the FIRST token h_k inserts in gap g, EPS when it inserts none; the later tokens of an insertion run vote nowhere and
                       are counted in extra[k]
    alternatives of a slot = its distinct votes (EPS is one), weight(a) = the w_k of the entries voting a, first(a) = the lowest such k,
                       ordered by weight descending, then first ascending
    consensus = the top alternative of every slot in slot order, EPS skipped; mbr = h_pivot
    confidence[i] = weight(h_pivot[i] at slot 2 i + 1) / W, expected_errors[i] = risk[i] / W (float64 divisions; 0.0 when W == 0)
The weights of scores: nbest_weights."""
import numpy as np

from tests import score_ref as R

EPS = -1
WEIGHT_ONE = 1 << 20
MAX_N, MAX_LEN, MAX_ALTS, MAX_WEIGHT_SUM = 64, 256, 8, 1 << 30


def nbest_weights(scores, scale=1.0):
    """int32 weights of one utterance's scores: q_k = softmax(scale * s_k) over the finite scores in float64, w_k = floor(q_k * 2**20 +
    0.5); a score of -inf gives 0."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1) * float(scale)
    w = np.zeros(s.shape[0], dtype=np.int32)
    fin = np.isfinite(s)
    if fin.any():
        e = np.exp(s[fin] - s[fin].max())
        w[fin] = np.floor(e / e.sum() * WEIGHT_ONE + 0.5).astype(np.int32)
    return w


def distances(hyps):
    N = len(hyps)
    d = np.zeros((N, N), dtype=np.int64)
    for i in range(N):
        for k in range(N):
            if i != k and hyps[i] is not None and hyps[k] is not None:
                d[i, k] = R.table(hyps[i], hyps[k])[-1, -1]
    assert (d == d.T).all() and (np.diag(d) == 0).all()
    return d


def votes_of(pivot_ids, hyp):
    """(votes over the 2 m + 1 slots, extra insertions) of one hypothesis aligned to the pivot."""
    m = len(pivot_ids)
    v = [EPS] * (2 * m + 1)
    extra, row, run = 0, 0, False      # row: pivot tokens consumed so far = the gap an insertion falls into
    for op, ri, hj in R.align(pivot_ids, hyp)["ops"]:
        if op == R.INS:
            if run:
                extra += 1
            else:
                v[2 * row] = int(hyp[hj])
            run = True
        else:
            if op != R.DEL:
                v[2 * ri + 1] = int(hyp[hj])
            row, run = ri + 1, False
    return v, extra


def slot_alternatives(values, weights):
    """[(token, weight, first)] of one slot, ordered: values / weights of the present entries in index order as (k, value) / {k: w}."""
    acc = {}
    for k, a in values:
        if a in acc:
            acc[a][0] += int(weights[k])
        else:
            acc[a] = [int(weights[k]), k]
    return sorted(((a, w, f) for a, (w, f) in acc.items()), key=lambda t: (-t[1], t[2]))


def consensus(hyps, weights, alts=4):
    """The whole definition for one utterance.  hyps: id lists or None (absent); weights: ints.  Returns a dict of plain integers and
    lists: d, risk, pivot, W, votes (N rows of 2 m + 1; an absent entry's row is all EPS), extra (N), slots [{"alts": [(token, weight)]
    top `alts`, "n_alts", "pivot_weight"}], consensus, mbr, confidence, expected_errors, extra_insertions."""
    N = len(hyps)
    w = [int(x) for x in weights]
    assert len(w) == N and 1 <= N <= MAX_N and 1 <= alts <= MAX_ALTS and all(x >= 0 for x in w)
    present = [k for k in range(N) if hyps[k] is not None]
    assert present and all(len(hyps[k]) <= MAX_LEN and all(int(t) >= 0 for t in hyps[k]) for k in present)
    W = sum(w[k] for k in present)
    assert W <= MAX_WEIGHT_SUM
    d = distances(hyps)
    risk = [sum(w[k] * int(d[i, k]) for k in present) if i in present else 0 for i in range(N)]
    pivot = min(present, key=lambda i: (risk[i], i))
    piv = [int(t) for t in hyps[pivot]]
    m = len(piv)
    votes, extra = [[EPS] * (2 * m + 1) for _ in range(N)], [0] * N
    for k in present:
        votes[k], extra[k] = votes_of(piv, hyps[k])
    assert votes[pivot] == [piv[s // 2] if s & 1 else EPS for s in range(2 * m + 1)] and extra[pivot] == 0
    slots = []
    for s in range(2 * m + 1):
        al = slot_alternatives([(k, votes[k][s]) for k in present], w)
        slots.append({"alts": [(a, x) for a, x, _ in al[:alts]], "n_alts": len(al), "pivot_weight": [x for a, x, _ in al if a == votes[pivot][s]][0]})
    return {"d": d.tolist(), "risk": risk, "pivot": pivot, "W": W, "votes": votes, "extra": extra, "slots": slots,
            "consensus": [sl["alts"][0][0] for sl in slots if sl["alts"][0][0] != EPS], "mbr": piv,
            "confidence": [slots[2 * i + 1]["pivot_weight"] / W if W else 0.0 for i in range(m)],
            "expected_errors": [risk[i] / W if W else 0.0 for i in range(N)], "extra_insertions": sum(extra)}
