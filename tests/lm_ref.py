"""The definition of n-gram LM shallow fusion in the CTC prefix beam search, restated in fp64 (TEST INFRASTRUCTURE).

KenLM is not available, so the feature is parity unpinned by KenLM: this file is the definition the kernels and
asr_chinese_e2e_amd/lm.py are tested against.  It shares no code with either: the model is a dict keyed by id tuples, the query is the
recursive ARPA back-off rule written literally, and the search is oracle/decode_ref.py::ctc_prefix_beam_search restated with the bias
(with no LM it returns decode_ref's lists, asserted in tests/test_lm_cpu.py).

table: {tuple of ids: (log10p, log10bow or None)}.  log10 p(w | h) = log10p(h.w) if h.w is listed, otherwise bow(h) + log10 p(w | h[1:]);
bow(h) = 0 if h is not listed or has no back-off column; at the empty history a token without a unigram scores <unk>'s unigram if there
is one, otherwise unk_log10; h is first cut to its last order - 1 tokens; a hypothesis starts from (<s>) if <s> is listed, else from ().
Every value enters as the fp64 term weight * (log10value * math.log(10.0)).  Appending a token does bias = bias + term once per back-off
weight met, in chain order, then once for the probability found, then bias = bias + ins.  Candidates of a frame are ranked by
logadd(pb, pnb) + bias; nothing else of the search changes.  A result reports ctc_score = log p, lm_score = bias + term(</s> | history)
(the end term is 0.0 if </s> is not listed) and score = ctc_score + lm_score; the list is ordered by score (a stable sort of the rank order)."""
import math
import random

from oracle.decode_ref import NEG, logadd

UNK, BOS, EOS = 1, 2, 3

# the kinds of back-off chain a query can take (Model.kinds collects the ones met)
TRIGRAM_HIT, BACKOFF_ONE, BACKOFF_TWO, CONTEXT_NOT_LISTED, CONTEXT_WITHOUT_BOW, UNK_TERM, HIT_THEN_SHORTER_STATE = range(7)


class Model:
    def __init__(self, table, order, weight=0.3, ins=0.0, unk_log10=-10.0):
        self.table, self.order = dict(table), int(order)
        self.weight, self.ins, self.unk_log10 = float(weight), float(ins), float(unk_log10)
        self.kinds = set()

    def term(self, log10value):
        return self.weight * (log10value * math.log(10.0))

    def cut(self, h):
        n = self.order - 1
        return tuple(h[len(h) - n:]) if n > 0 and len(h) > n else (tuple(h) if n > 0 else ())

    def add(self, h, w, bias, top=None):
        """bias after the terms of log10 p(w | h) have been added in chain order (h already cut)."""
        top = len(h) if top is None else top
        if h + (w,) in self.table:
            if len(h) == 2 and top == 2:
                self.kinds.add(TRIGRAM_HIT)
                if self.order == 3 and (h + (w,))[1:] not in self.table and not any(g[:2] == (h + (w,))[1:] for g in self.table):
                    self.kinds.add(HIT_THEN_SHORTER_STATE)
            if top == 2 and len(h) == 1:
                self.kinds.add(BACKOFF_ONE)
            if top == 2 and len(h) == 0:
                self.kinds.add(BACKOFF_TWO)
            return bias + self.term(self.table[h + (w,)][0])
        if not h:
            self.kinds.add(UNK_TERM)
            return bias + self.term(self.table[(UNK,)][0] if (UNK,) in self.table else self.unk_log10)
        if h not in self.table:
            self.kinds.add(CONTEXT_NOT_LISTED)
        elif self.table[h][1] is None:
            self.kinds.add(CONTEXT_WITHOUT_BOW)
        else:
            bias = bias + self.term(self.table[h][1])
        return self.add(h[1:], w, bias, top)

    def log10p(self, h, w):
        """The plain query, unweighted: log10 p(w | h)."""
        h = self.cut(h)
        if h + (w,) in self.table:
            return self.table[h + (w,)][0]
        if not h:
            return self.table[(UNK,)][0] if (UNK,) in self.table else self.unk_log10
        bow = self.table[h][1] if h in self.table and self.table[h][1] is not None else 0.0
        return bow + self.log10p(h[1:], w)

    def start(self):
        return (BOS,) if (BOS,) in self.table else ()

    def biases(self, tokens):
        """The bias after every token of the string."""
        hist, bias, out = self.start(), 0.0, []
        for c in tokens:
            bias = self.add(self.cut(hist), int(c), bias)
            bias = bias + self.ins
            hist = hist + (int(c),)
            out.append(bias)
        return out

    def bias(self, tokens):
        b = self.biases(tokens)
        return b[-1] if b else 0.0

    def lm_score(self, tokens):
        """bias + term(</s> | history); the end term is 0.0 if </s> is not listed."""
        bias = self.bias(tokens)
        if (EOS,) not in self.table:
            return bias
        return self.add(self.cut(self.start() + tuple(int(c) for c in tokens)), EOS, bias)


def ctc_prefix_beam_search(logp, beam_size, blank=0, candidates=None, lm=None):
    """decode_ref.ctc_prefix_beam_search with rank = logadd(pb, pnb) + bias(prefix).  Returns (list, gap): list = [(prefix, score,
    ctc_score, lm_score)] ordered by score, for the whole beam (lm=None: lm_score 0.0, score = ctc_score); gap = the smallest difference
    between two adjacent ranked candidates over all frames (inf when no frame has two) - a ranking can only differ from this one where the
    gap is within the other side's rounding."""
    T, V = logp.shape
    beam = {(): (0.0, NEG)}
    walked = {}

    def bias_of(prefix):
        if lm is None:
            return 0.0
        if prefix not in walked:
            walked[prefix] = lm.bias(prefix)
        return walked[prefix]

    def rank(kv):
        tot = logadd(*kv[1])
        return tot + bias_of(kv[0]) if tot != NEG else NEG

    gap = math.inf
    for t in range(T):
        nxt = {}

        def acc(prefix, idx, val):
            cur = nxt.setdefault(prefix, [NEG, NEG])
            cur[idx] = logadd(cur[idx], val)

        cand = range(V) if candidates is None else candidates[t]
        for prefix, (pb, pnb) in beam.items():
            acc(prefix, 0, logadd(pb, pnb) + logp[t, blank])
            for c in cand:
                c = int(c)
                if c == blank:
                    continue
                lp = logp[t, c]
                if prefix and c == prefix[-1]:
                    acc(prefix, 1, pnb + lp)
                    acc(prefix + (c,), 1, pb + lp)
                else:
                    acc(prefix + (c,), 1, logadd(pb, pnb) + lp)
        ranked = sorted(nxt.items(), key=rank, reverse=True)
        keys = [rank(kv) for kv in ranked]
        for a, b in zip(keys, keys[1:]):
            if b != NEG:
                gap = min(gap, a - b)
        beam = {k: tuple(v) for k, v in ranked[:beam_size]}
    out = []
    for prefix, v in sorted(beam.items(), key=rank, reverse=True):
        ctc = logadd(*v)
        lms = lm.lm_score(prefix) if lm is not None else 0.0
        out.append((prefix, ctc + lms, ctc, lms))
    out.sort(key=lambda h: h[1], reverse=True)
    return out, gap


# ---- the LM of the tests: order 3 over V = 12 (0 = blank, 1 = <unk>, 2 = <s>, 3 = </s>, 4 .. 11 = characters), drawn once from a fixed
# stream of random.Random(12).random() values (that method's stream is the same in every Python 3).  It has holes on purpose: token 11
# has no unigram (the unk term; <unk> itself has none either, so unk_log10 is used), about a third of the listed contexts have no
# back-off column, most bigrams are not listed (a context that is not listed: bow 0), trigrams are listed whether or not their bigram
# prefix is, and most listed trigrams a b c have no state (b, c), so the hit is followed by a shorter state.
V = 12
ORDER = 3


def _draw():
    rng = random.Random(12)
    table = {}
    for a in range(2, 11):                       # unigrams: <s>, </s>, 4 .. 10; not 1 (<unk>) and not 11
        table[(a,)] = (-0.5 - 2.0 * rng.random(), None if rng.random() < 0.3 else -1.5 * rng.random())
    for a in range(2, V):
        for b in range(3, V):
            if a != EOS and rng.random() < 0.3:
                table[(a, b)] = (-0.1 - 2.0 * rng.random(), None if rng.random() < 0.35 else -1.2 * rng.random())
    for a in range(2, V):
        for b in range(4, V):
            for c in range(3, V):
                if a != EOS and rng.random() < 0.08:
                    table[(a, b, c)] = (-0.05 - 1.5 * rng.random(), None)
    return table


TABLE = _draw()


def table(with_bos=True):
    """The test LM; with_bos=False: without the unigram <s>, so that a hypothesis starts from the empty history."""
    return {g: v for g, v in TABLE.items() if with_bos or g != (BOS,)}


def lattice(seed, T, peak):
    """A random (T, V) fp64 log-probability lattice: log_softmax of peak * N(0, 1)."""
    import numpy as np
    x = np.random.RandomState(seed).randn(T, V) * peak
    x = x - x.max(axis=1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=1, keepdims=True))


def topk_candidates(logp, k):
    """Per frame the k best classes, descending, ties by ascending index (asr_ctc_frame_topk's order)."""
    import numpy as np
    return [list(np.lexsort((np.arange(logp.shape[1]), -logp[t]))[:k]) for t in range(logp.shape[0])]
