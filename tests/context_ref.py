"""The definition of hotword (context) biasing in the CTC prefix beam search, restated in fp64 (TEST INFRASTRUCTURE).

WeNet's binaries are not available, so the feature is parity unpinned by WeNet: this file is the definition the kernels and
asr_chinese_e2e_amd/context.py are tested against.  It shares no code with either: the trie is a dict of dicts, and the search is
oracle/decode_ref.py::ctc_prefix_beam_search restated with the bonus (with no graph it returns decode_ref's lists, asserted in
tests/test_context_cpu.py).

A graph = a set of phrases (non-empty lists of token ids in [1, V)) and one per-token bonus w.  Trie: root of depth 0; a node is final if
a phrase ends on it; sec(n) = depth of the deepest final node on the path root..n (n included; 0: none); held(n) = w * (depth(n) - sec(n)).
A hypothesis carries (n, bias) from (root, 0.0).  Appending token c:
  1. n has a child m on c: bias += w, n = m; if m is final and has no children, n = root (the bonus stays).
  2. otherwise: bias -= held(n), n = root, then rule 1 is tried once from the root (no child there: the state stays at the root).
Candidates of a frame are ranked by logadd(pb, pnb) + bias; nothing else of the search changes.  A result reports ctc_score = log p,
bias = bias - held(n) and score = ctc_score + bias; the list is ordered by score (a stable sort of the beam's rank order)."""
import math

from oracle.decode_ref import NEG, logadd


class Trie:
    """The naive trie of one graph: nodes are dicts {"kids": {token: node}, "final", "depth", "sec", "path"}."""

    def __init__(self, phrases, w=3.0):
        self.w = float(w)
        self.root = {"kids": {}, "final": False, "depth": 0, "sec": 0, "path": ()}
        for ph in phrases:
            assert len(ph) > 0
            n = self.root
            for t in ph:
                n = n["kids"].setdefault(int(t), {"kids": {}, "final": False, "depth": n["depth"] + 1, "sec": 0, "path": n["path"] + (int(t),)})
            n["final"] = True
        self._sec(self.root, 0)

    def _sec(self, n, sec):
        n["sec"] = n["depth"] if n["final"] else sec
        for kid in n["kids"].values():
            self._sec(kid, n["sec"])

    def held(self, n):
        return self.w * (n["depth"] - n["sec"])

    def step(self, n, bias, c):
        m = n["kids"].get(int(c))
        if m is None:
            bias = bias - self.held(n)
            n = self.root
            m = n["kids"].get(int(c))
            if m is None:
                return n, bias
        bias = bias + self.w
        return (self.root if m["final"] and not m["kids"] else m), bias

    def walk(self, tokens):
        """(node, raw bias) of the string."""
        n, bias = self.root, 0.0
        for c in tokens:
            n, bias = self.step(n, bias, c)
        return n, bias


def ctc_prefix_beam_search(logp, beam_size, blank=0, candidates=None, trie=None):
    """decode_ref.ctc_prefix_beam_search with the bonus.  Returns (list, gap): list = [(prefix, score, ctc_score, bias)] ordered by
    score, for the whole beam (trie=None: bias 0.0, score = ctc_score); gap = the smallest difference between two adjacent ranked
    candidates over all frames (inf when no frame has two) - a ranking can only differ from this one where the gap is within the other
    side's rounding."""
    T, V = logp.shape
    beam = {(): (0.0, NEG)}
    walked = {}

    def bias_of(prefix):
        if trie is None:
            return 0.0
        if prefix not in walked:
            walked[prefix] = trie.walk(prefix)
        return walked[prefix][1]

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
        bias = 0.0
        if trie is not None:
            n, raw = trie.walk(prefix)
            bias = raw - trie.held(n)
        out.append((prefix, ctc + bias, ctc, bias))
    out.sort(key=lambda h: h[1], reverse=True)
    return out, gap


# the graphs of the tests, over V = 12: phrases of length 1 to 4, a repeated token (3, 3), a phrase that is a prefix of another
# ((3, 3) and (3, 3, 7)), a single token (5,); two graphs packed into one ContextGraph
V = 12
GRAPHS = [
    [(1, 2, 6), (3, 3), (3, 3, 7), (5,), (8, 9, 10, 11)],
    [(4,), (2, 2, 2, 9), (10, 1), (7, 11, 3)],
]


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
