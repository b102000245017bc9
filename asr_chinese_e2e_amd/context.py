"""Hotword (context) biasing of the CTC prefix beam search: the phrase lists compiled into one flat automaton.

A graph is a set of phrases (token id lists) and one per-token bonus w (WeNet's context_score, 3.0).  Its trie has a root of depth 0;
a node is final if a phrase ends on it; sec(n) = the depth of the deepest final node on the path root..n (0: none);
held(n) = w * (depth(n) - sec(n)) = the bonus handed out for a phrase that has begun and not finished.
A hypothesis carries (n, bias), starting at (root, 0.0).  Appending token c:
    1. n has a child m on c: bias += w, n = m; a final m without children sends n back to the root (the bonus stays);
    2. otherwise: bias -= held(n), n = root, and rule 1 is tried once from the root.
(n, bias) is a function of the token string alone, computed by the same fp64 additions on the host (walk) and in the kernels
(csrc/prefix_beam.hip, pb_ctx_advance) - so the two agree bit for bit.  A result reports bias - held(n): an unfinished phrase earns nothing.

The tables (all graphs in one object, states numbered graph after graph, breadth first):
    st_off   int32 [S + 1]  arcs of state s = [st_off[s], st_off[s + 1])
    arc_tok  int32 [A]      ascending within a state
    arc_next int32 [A]      the state the arc leads to; an arc onto a final leaf leads to its graph's root (the leaf is no state)
    st_held  fp64  [S]      held(s)
    st_root  int32 [S]      the root of the state's graph
    root_of_graph           host list, one root per graph
This class is the only producer of the tables and validates what the kernels would otherwise read out of bounds."""
import ctypes

import torch

DEFAULT_SCORE = 3.0


class ContextTables(ctypes.Structure):
    """asr_context_graph of include/asr_hip.h (same field order): device pointers, sizes and w."""
    _fields_ = [("st_off", ctypes.c_void_p), ("arc_tok", ctypes.c_void_p), ("arc_next", ctypes.c_void_p), ("st_held", ctypes.c_void_p),
                ("S", ctypes.c_int), ("A", ctypes.c_int), ("w", ctypes.c_double)]


class ContextGraph:
    def __init__(self, graphs, score=DEFAULT_SCORE, device=None, vocab_size=None):
        """graphs: a list of graphs, each a list of phrases, each a non-empty list of token ids in [1, vocab_size).  score: the
        per-token bonus w.  device: where the tables are put at once (None: on first use, on(device))."""
        w = float(score)
        if w != w or w in (float("inf"), float("-inf")):
            raise ValueError(f"ContextGraph: score must be finite (got {score})")
        graphs = [list(g) for g in graphs] if graphs is not None else []
        if not graphs:
            raise ValueError("ContextGraph: no graph given (an empty phrase list)")
        V = None if vocab_size is None else int(vocab_size)
        st_off, arc_tok, arc_next, st_held, st_root, roots, index = [0], [], [], [], [], [], []
        for gi, phrases in enumerate(graphs):
            if not phrases:
                raise ValueError(f"ContextGraph: graph {gi} has no phrase")
            trie = {"kids": {}, "final": False}
            for pi, ph in enumerate(phrases):
                ph = [int(t) for t in ph]
                if not ph:
                    raise ValueError(f"ContextGraph: graph {gi}, phrase {pi} is empty")
                node = trie
                for t in ph:
                    if t < 1 or (V is not None and t >= V):
                        raise ValueError(f"ContextGraph: graph {gi}, phrase {pi}: token {t} outside [1, {'V' if V is None else V}) "
                                         "(0 is the CTC blank)")
                    node = node["kids"].setdefault(t, {"kids": {}, "final": False})
                node["final"] = True
            # breadth first: every node but a final leaf becomes a state
            root = len(st_held)
            roots.append(root)
            order, paths = [(trie, 0, 0, ())], {(): root}
            i = 0
            while i < len(order):
                node = order[i][0]
                for t in sorted(node["kids"]):
                    kid = node["kids"][t]
                    if kid["kids"]:
                        depth = order[i][1] + 1
                        paths[order[i][3] + (t,)] = root + len(order)
                        order.append((kid, depth, depth if kid["final"] else order[i][2], order[i][3] + (t,)))
                i += 1
            for node, depth, sec, path in order:
                for t in sorted(node["kids"]):
                    kid = node["kids"][t]
                    arc_tok.append(t)
                    arc_next.append(paths[path + (t,)] if kid["kids"] else root)
                st_off.append(len(arc_tok))
                st_held.append(w * (depth - sec))
                st_root.append(root)
            index.append(paths)
        S, A = len(st_held), len(arc_tok)
        if S >= 2 ** 31 or A >= 2 ** 31:
            raise ValueError(f"ContextGraph: {S} states / {A} arcs do not fit an int32")
        # what a kernel would read out of bounds otherwise
        assert len(st_off) == S + 1 and st_off[0] == 0 and st_off[-1] == A
        for s in range(S):
            lo, hi = st_off[s], st_off[s + 1]
            assert 0 <= lo <= hi <= A
            assert all(arc_tok[a] < arc_tok[a + 1] for a in range(lo, hi - 1)), "arcs sorted and unique"
        assert all(0 <= n < S for n in arc_next)
        self._w, self._S, self._A, self._V = w, S, A, V
        self._roots = tuple(roots)
        self._index = tuple(index)
        self._host = (torch.tensor(st_off, dtype=torch.int32), torch.tensor(arc_tok, dtype=torch.int32),
                      torch.tensor(arc_next, dtype=torch.int32), torch.tensor(st_held, dtype=torch.float64),
                      torch.tensor(st_root, dtype=torch.int32))
        self._lists = (st_off, arc_tok, arc_next, st_held, st_root)
        self._dev = {}
        if device is not None:
            self.on(device)

    def __setattr__(self, name, value):
        if name.startswith("_") and name not in self.__dict__:
            object.__setattr__(self, name, value)
        else:
            raise AttributeError("ContextGraph is immutable")

    # ------------------------------------------------------------------ the tables
    w = property(lambda self: self._w)
    S = property(lambda self: self._S)
    A = property(lambda self: self._A)
    vocab_size = property(lambda self: self._V)
    n_graphs = property(lambda self: len(self._roots))
    root_of_graph = property(lambda self: self._roots)
    st_off = property(lambda self: self._host[0])
    arc_tok = property(lambda self: self._host[1])
    arc_next = property(lambda self: self._host[2])
    st_held = property(lambda self: self._host[3])
    st_root = property(lambda self: self._host[4])

    def on(self, device):
        """(tables on `device`: st_off, arc_tok, arc_next, st_held, st_root; the ContextTables struct the entry points take)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        got = self._dev.get(device)
        if got is None:
            tabs = tuple(t.to(device) for t in self._host)
            # an empty arc table still needs an address
            arcs = [t if t.numel() else torch.zeros(1, dtype=torch.int32, device=device) for t in tabs[1:3]]
            struct = ContextTables(tabs[0].data_ptr(), arcs[0].data_ptr(), arcs[1].data_ptr(), tabs[3].data_ptr(), self._S, self._A, self._w)
            got = self._dev[device] = (tabs, struct, arcs)
        return got[0], got[1]

    def check_vocab(self, V):
        """Raises unless every token is below V (for a graph built without vocab_size)."""
        top = max(self._lists[1]) if self._lists[1] else 0
        if top >= int(V):
            raise ValueError(f"ContextGraph: token {top} outside [1, {int(V)})")

    def roots(self, context_ids, B):
        """Per-utterance roots for `context_ids` (None: graph 0 for all; -1: unbiased), as a list of B ints."""
        ids = [0] * B if context_ids is None else [int(x) for x in context_ids]
        if len(ids) != B:
            raise ValueError(f"context_ids must hold {B} graph indices, got {len(ids)}")
        return [self.root(g) for g in ids]

    def root(self, graph):
        graph = int(graph)
        if graph == -1:
            return -1
        if not 0 <= graph < len(self._roots):
            raise ValueError(f"context graph {graph} of {len(self._roots)} (-1: unbiased)")
        return self._roots[graph]

    def state_of(self, graph, tokens):
        """The state reached from graph's root by spelling `tokens` inside the trie (KeyError if they leave it or end on a final leaf)."""
        return self._index[int(graph)][tuple(int(t) for t in tokens)]

    def held(self, state):
        """held(state): the bonus a hypothesis standing on `state` has been handed for a phrase not finished (0.0 for state -1)."""
        state = int(state)
        if state == -1:
            return 0.0
        if not 0 <= state < self._S:
            raise ValueError(f"state {state} of {self._S}")
        return self._lists[3][state]

    def _find(self, state, c):
        st_off, arc_tok, arc_next = self._lists[0], self._lists[1], self._lists[2]
        lo, hi = st_off[state], st_off[state + 1]
        end = hi
        while lo < hi:
            mid = (lo + hi) >> 1
            if arc_tok[mid] < c:
                lo = mid + 1
            else:
                hi = mid
        return arc_next[lo] if lo < end and arc_tok[lo] == c else -1

    def advance(self, root, state, bias, c):
        """One token: (state, bias) -> (state, bias) over the flat tables, the statements of the kernels' pb_ctx_advance."""
        if root < 0:
            return state, bias
        m = self._find(state, c)
        if m >= 0:
            return m, bias + self._w
        bias = bias - self._lists[3][state]
        m = self._find(root, c)
        if m >= 0:
            return m, bias + self._w
        return root, bias

    def walk(self, graph, tokens):
        """(state, bias) of a hypothesis that spells `tokens` under graph `graph` (-1: (-1, 0.0)); bias is the raw value, before
        held(state) is taken off."""
        root = self.root(graph)
        state, bias = root, 0.0
        for c in tokens:
            state, bias = self.advance(root, state, bias, int(c))
        return state, bias

    @classmethod
    def from_file(cls, path, vocab, score=DEFAULT_SCORE, device=None):
        """One graph from a UTF-8 file: one phrase per line, every character looked up in `vocab` (data_handler.vocab.Vocab, or a
        token -> id mapping); blank lines are skipped; a line with an unknown character raises and names the line."""
        t2i = getattr(vocab, "_token2id", vocab)
        size = len(getattr(vocab, "_id2token", t2i))
        phrases = []
        with open(path, encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                text = "".join(line.split())
                if not text:
                    continue
                ids = []
                for ch in text:
                    if ch not in t2i:
                        raise ValueError(f"{path}, line {no}: character {ch!r} is not in the vocabulary")
                    ids.append(int(t2i[ch]))
                phrases.append(ids)
        if not phrases:
            raise ValueError(f"{path}: no phrase")
        return cls([phrases], score=score, device=device, vocab_size=size)
