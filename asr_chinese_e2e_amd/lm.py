"""N-gram LM shallow fusion in the CTC prefix beam search: a back-off n-gram model (ARPA) compiled into one flat automaton.

The query is the ARPA back-off rule, what KenLM and SRILM answer:
    log10 p(w | h) = log10p(h.w) if the n-gram h.w is listed, otherwise bow(h) + log10 p(w | h[1:]),
bow(h) = 0 if h is not listed or has no back-off column; at the empty history a token without a unigram scores <unk>'s unigram if
there is one, otherwise unk_log10; a history longer than order - 1 is first cut to its last order - 1 tokens; a hypothesis starts from
the history (<s>) if <s> is listed, otherwise from the empty history.

Weights are folded in here: every table entry is the fp64 TERM weight * (log10value * math.log(10.0)).  A hypothesis carries
(state, bias) from (start, 0.0).  Appending token c does bias = bias + term once per back-off weight met on the chain, in chain
order, then once for the probability found, then bias = bias + ins.  Nothing but these fp64 additions touches the bias on the host
(advance) or on the device (csrc/prefix_beam.hip, pb_lm_advance) - so the two agree bit for bit.  A reported hypothesis carries lm_score =
bias + term(</s> | its state) (final); the end term is 0.0 if </s> is not listed.  The search ranks by log p + bias without it.

States: 0 is the empty history; the others are the prefixes of 1 .. order - 1 tokens of the listed n-grams (every context a listed
n-gram can be reached from; no minimisation).  The state of a history is its longest suffix that is a state.  The tables:
    st_off   int32 [S + 1]  arcs of state s = [st_off[s], st_off[s + 1]); state 0 has none
    arc_tok  int32 [A]      ascending within a state
    arc_next int32 [A]      the state of s.c; ~state when s.c is not listed itself (it is only a context of longer n-grams): such an arc
                            fixes the next state and the chain goes on
    arc_term fp64  [A]      term(log10p(s.c)); 0.0 on an unlisted arc (never added)
    st_back  int32 [S]      the state of the longest proper suffix of s that is a state
    st_bow   fp64  [S]      term(bow(s)); 0.0 if s is not listed or has no back-off column
    uni_term fp64  [V]      the unigram level, dense over the tokens: the unigram's term, the unk term where there is none
    uni_next int32 [V]      the state (c,), 0 if it is none
so every chain ends in one indexed load and never in a search or a miss.  This class is the only producer of the tables and validates
what the kernels would otherwise read out of bounds."""
import ctypes
import math

import numpy as np
import torch

UNK_ID, BOS_ID, EOS_ID = 1, 2, 3      # data_handler/vocab.py: ids 0-3 are PAD, UNK, BOS, EOS
MAX_ORDER = 5
_TABLES = ("st_off", "arc_tok", "arc_next", "arc_term", "st_back", "st_bow", "uni_term", "uni_next")
_F64 = ("arc_term", "st_bow", "uni_term")


class LmTables(ctypes.Structure):
    """asr_ngram_lm of include/asr_hip.h (same field order): device pointers, sizes, start state and ins."""
    _fields_ = [(n, ctypes.c_void_p) for n in _TABLES] + [(n, ctypes.c_int) for n in ("S", "A", "V", "order", "start")] + [("ins", ctypes.c_double)]


def _finite(x):
    return x == x and x not in (math.inf, -math.inf)


class NgramLM:
    def __init__(self, ngrams, order, vocab_size, weight=0.3, ins=0.0, unk_log10=-10.0, device=None, bos=BOS_ID, eos=EOS_ID, unk=UNK_ID, dropped=0):
        """ngrams: {tuple of token ids: (log10p, log10bow or None)} - the listed n-grams of 1 .. order tokens, ids in [0, vocab_size).
        weight / ins: the LM weight and the per-token insertion bonus (natural-log units, as the CTC score).  bos / eos / unk: the ids
        of <s>, </s> and <unk>.  device: where the tables are put at once (None: on first use, on(device))."""
        order, V = int(order), int(vocab_size)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"NgramLM: orders 1 to {MAX_ORDER} are supported (got {order})")
        if V < 1:
            raise ValueError(f"NgramLM: vocab_size {vocab_size}")
        w, ins, unk_log10 = float(weight), float(ins), float(unk_log10)
        if not (_finite(w) and _finite(ins) and _finite(unk_log10)):
            raise ValueError(f"NgramLM: weight, ins and unk_log10 must be finite (got {weight}, {ins}, {unk_log10})")
        ln10 = math.log(10.0)

        def term(x):
            return w * (x * ln10)

        listed = {}
        for g, val in ngrams.items():
            g = tuple(int(t) for t in g)
            if not 1 <= len(g) <= order:
                raise ValueError(f"NgramLM: n-gram {g} has {len(g)} tokens, the order is {order}")
            if any(t < 0 or t >= V for t in g):
                raise ValueError(f"NgramLM: n-gram {g} holds a token outside [0, {V})")
            p, bow = val
            p = float(p)
            bow = None if bow is None else float(bow)
            if not _finite(p) or (bow is not None and not _finite(bow)):
                raise ValueError(f"NgramLM: n-gram {g} has a non-finite value {val}")
            listed[g] = (p, bow)
        # states: the empty history, then every prefix of 1 .. order - 1 tokens of a listed n-gram, shorter ones first
        ctxs = set()
        for g in listed:
            for j in range(1, min(len(g), order - 1) + 1):
                ctxs.add(g[:j])
        ctxs = sorted(ctxs, key=lambda h: (len(h), h))
        sid = {(): 0}
        for h in ctxs:
            sid[h] = len(sid)
        S = len(sid)

        def state_of(h):
            """The longest suffix of h (cut to order - 1 tokens) that is a state."""
            h = h[len(h) - (order - 1):] if len(h) > order - 1 else h
            for i in range(len(h) + 1):
                if h[i:] in sid:
                    return sid[h[i:]]
            return 0

        arcs = [None] * S      # per state {token: listed?}
        for g in listed:
            if len(g) >= 2:
                s = sid[g[:-1]]
                if arcs[s] is None:
                    arcs[s] = {}
                arcs[s][g[-1]] = True
        for h in ctxs:
            if len(h) >= 2:
                s = sid[h[:-1]]
                if arcs[s] is None:
                    arcs[s] = {}
                arcs[s].setdefault(h[-1], False)
        st_off, arc_tok, arc_next, arc_term = [0, 0], [], [], []
        st_back, st_bow = [0], [0.0]
        for h in ctxs:
            a = arcs[sid[h]]
            for c in sorted(a) if a else ():
                nx = state_of(h + (c,))
                arc_tok.append(c)
                arc_next.append(nx if a[c] else ~nx)
                arc_term.append(term(listed[h + (c,)][0]) if a[c] else 0.0)
            st_off.append(len(arc_tok))
            st_back.append(state_of(h[1:]))
            bow = listed[h][1] if h in listed else None
            st_bow.append(0.0 if bow is None else term(bow))
        unk_term = term(listed[(unk,)][0]) if (unk,) in listed else term(unk_log10)
        uni_term = [term(listed[(c,)][0]) if (c,) in listed else unk_term for c in range(V)]
        uni_next = [sid.get((c,), 0) for c in range(V)]
        start = sid.get((bos,), 0) if (bos,) in listed else 0
        tabs = dict(st_off=st_off, arc_tok=arc_tok, arc_next=arc_next, arc_term=arc_term, st_back=st_back, st_bow=st_bow, uni_term=uni_term,
                    uni_next=uni_next)
        arrays = {n: np.asarray(tabs[n], dtype=np.float64 if n in _F64 else np.int32) for n in _TABLES}
        meta = dict(order=order, V=V, start=start, ins=ins, weight=w, unk_log10=unk_log10, bos=int(bos), eos=int(eos), unk=int(unk),
                    has_eos=(int(eos),) in listed, n_ngrams=len(listed), dropped=int(dropped))
        self._set(arrays, meta, device)

    # ------------------------------------------------------------------ construction from compiled tables (the constructor, load)
    def _set(self, arrays, meta, device=None):
        order, V, start = int(meta["order"]), int(meta["V"]), int(meta["start"])
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"NgramLM: orders 1 to {MAX_ORDER} are supported (got {order})")
        for n in _TABLES:
            want = np.float64 if n in _F64 else np.int32
            if arrays[n].dtype != want or arrays[n].ndim != 1:
                raise ValueError(f"NgramLM: table {n} must be a flat {np.dtype(want).name} array")
        S, A = int(arrays["st_back"].shape[0]), int(arrays["arc_tok"].shape[0])
        if S >= 2 ** 31 - 1 or A >= 2 ** 31 - 1:
            raise ValueError(f"NgramLM: {S} states / {A} arcs do not fit an int32")
        off, tok, nxt = arrays["st_off"], arrays["arc_tok"], arrays["arc_next"]
        # what a kernel would read out of bounds otherwise
        ok = (S >= 1 and V >= 1 and off.shape[0] == S + 1 and arrays["st_bow"].shape[0] == S and arrays["arc_next"].shape[0] == A and
              arrays["arc_term"].shape[0] == A and arrays["uni_term"].shape[0] == V and arrays["uni_next"].shape[0] == V and 0 <= start < S)
        ok = ok and int(off[0]) == 0 and int(off[1]) == 0 and int(off[-1]) == A and bool((np.diff(off) >= 0).all())
        if ok and A:
            first = np.zeros(A, dtype=bool)
            first[off[:-1][np.diff(off) > 0]] = True                     # the first arc of every state that has any
            ok = bool(((np.diff(tok) > 0) | first[1:]).all())             # ascending and unique within a state
            ok = ok and int(tok.min()) >= 0 and int(tok.max()) < V
            real = np.where(nxt >= 0, nxt, ~nxt)
            ok = ok and int(real.min()) >= 0 and int(real.max()) < S
        ok = ok and int(arrays["st_back"].min()) >= 0 and int(arrays["st_back"].max()) < S and int(arrays["st_back"][0]) == 0
        ok = ok and int(arrays["uni_next"].min()) >= 0 and int(arrays["uni_next"].max()) < S
        if not ok:
            raise ValueError("NgramLM: inconsistent tables (offsets, arc order, or an index outside its table)")
        if not all(bool(np.isfinite(arrays[n]).all()) for n in _F64) or not (_finite(float(meta["ins"])) and _finite(float(meta["weight"]))):
            raise ValueError("NgramLM: weight, ins and every table value must be finite")
        self._arrays = {n: arrays[n] for n in _TABLES}
        self._meta = dict(meta)
        self._S, self._A = S, A
        self._lists = None
        self._dev = {}
        if device is not None:
            self.on(device)

    def __setattr__(self, name, value):
        if name.startswith("_") and (name not in self.__dict__ or name == "_lists"):
            object.__setattr__(self, name, value)
        else:
            raise AttributeError("NgramLM is immutable")

    # ------------------------------------------------------------------ the tables
    S = property(lambda self: self._S)
    A = property(lambda self: self._A)
    order = property(lambda self: self._meta["order"])
    vocab_size = property(lambda self: self._meta["V"])
    start = property(lambda self: self._meta["start"])
    weight = property(lambda self: self._meta["weight"])
    ins = property(lambda self: self._meta["ins"])
    eos = property(lambda self: self._meta["eos"])
    has_eos = property(lambda self: bool(self._meta["has_eos"]))
    n_ngrams = property(lambda self: self._meta["n_ngrams"])
    dropped = property(lambda self: self._meta["dropped"])

    def table(self, name):
        """One of the compiled tables as a host tensor (st_off, arc_tok, arc_next, arc_term, st_back, st_bow, uni_term, uni_next)."""
        return torch.from_numpy(self._arrays[name])

    def on(self, device):
        """(tables on `device` in the order of LmTables, the LmTables struct the entry points take)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        got = self._dev.get(device)
        if got is None:
            tabs = []
            for n in _TABLES:
                a = self._arrays[n]
                # an empty arc table still needs an address
                tabs.append(torch.from_numpy(a).to(device) if a.shape[0] else torch.zeros(1, dtype=torch.float64 if n in _F64 else torch.int32, device=device))
            m = self._meta
            struct = LmTables(*[t.data_ptr() for t in tabs], self._S, self._A, m["V"], m["order"], m["start"], m["ins"])
            got = self._dev[device] = (tuple(tabs), struct)
        return got

    def check_vocab(self, V):
        """Raises unless the LM was compiled for a vocabulary of V tokens."""
        if int(V) != self._meta["V"]:
            raise ValueError(f"NgramLM: compiled for a vocabulary of {self._meta['V']} tokens, the model has {int(V)}")

    # ------------------------------------------------------------------ the query on the host: the statements of the kernels' pb_lm_advance
    def _chain(self, state, bias, c):
        if self._lists is None:
            self._lists = {n: self._arrays[n].tolist() for n in _TABLES}
        L = self._lists
        st_off, arc_tok, arc_next = L["st_off"], L["arc_tok"], L["arc_next"]
        st = state if 0 <= state < self._S else 0
        nx = -1
        for _ in range(1, self._meta["order"]):
            if st == 0:
                break
            lo, hi = st_off[st], st_off[st + 1]
            end = hi
            while lo < hi:
                mid = (lo + hi) >> 1
                if arc_tok[mid] < c:
                    lo = mid + 1
                else:
                    hi = mid
            if lo < end and arc_tok[lo] == c:
                raw = arc_next[lo]
                if nx < 0:
                    nx = raw if raw >= 0 else ~raw
                if raw >= 0:
                    return nx, bias + L["arc_term"][lo]
            bias = bias + L["st_bow"][st]
            st = L["st_back"][st]
        cc = min(max(c, 0), self._meta["V"] - 1)
        bias = bias + L["uni_term"][cc]
        if nx < 0:
            nx = L["uni_next"][cc]
        return nx, bias

    def advance(self, state, bias, c):
        """One token: (state, bias) -> (state, bias)."""
        state, bias = self._chain(int(state), bias, int(c))
        return state, bias + self._meta["ins"]

    def walk(self, tokens):
        """(state, bias) of a hypothesis that spells `tokens`; the end-of-sentence term is not in it."""
        state, bias = self._meta["start"], 0.0
        for c in tokens:
            state, bias = self.advance(state, bias, c)
        return state, bias

    def final(self, state, bias):
        """lm_score of a reported hypothesis: bias + term(</s> | state), the chain's additions onto bias (no ins); bias itself if </s>
        is not listed.  state -1 (no entry): bias."""
        if not self._meta["has_eos"] or int(state) < 0:
            return bias
        return self._chain(int(state), bias, self._meta["eos"])[1]

    def score(self, tokens):
        """lm_score of the finished string `tokens`."""
        return self.final(*self.walk(tokens))

    # ------------------------------------------------------------------ files
    def save(self, path):
        """The compiled tables as an .npz (parsing a multi-million-line ARPA file in Python takes a while)."""
        m = self._meta
        with open(path, "wb") as f:
            np.savez(f, **self._arrays, meta_int=np.asarray([m[k] for k in ("order", "V", "start", "bos", "eos", "unk", "has_eos", "n_ngrams", "dropped")], dtype=np.int64),
                     meta_f64=np.asarray([m["ins"], m["weight"], m["unk_log10"]], dtype=np.float64))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            missing = [n for n in _TABLES + ("meta_int", "meta_f64") if n not in z.files]
            if missing:
                raise ValueError(f"{path}: not a saved NgramLM (no {missing[0]})")
            arrays = {n: np.ascontiguousarray(z[n]) for n in _TABLES}
            mi, mf = z["meta_int"].tolist(), z["meta_f64"].tolist()
        meta = dict(zip(("order", "V", "start", "bos", "eos", "unk", "has_eos", "n_ngrams", "dropped"), mi))
        meta["has_eos"] = bool(meta["has_eos"])
        meta.update(ins=mf[0], weight=mf[1], unk_log10=mf[2])
        obj = cls.__new__(cls)
        obj._set(arrays, meta, device)
        return obj

    @classmethod
    def from_arpa(cls, path, vocab, weight=0.3, ins=0.0, unk_log10=-10.0, device=None):
        """A standard ARPA file: \\data\\ with `ngram N=count` lines, one \\N-grams: section per order (lines `log10p w1 .. wN [log10bow]`,
        fields separated by tabs or blanks) and \\end\\.  Words are looked up in `vocab` (data_handler.vocab.Vocab, or a token -> id
        mapping); <s>, </s> and <unk> are recognised by name.  An n-gram with any other word outside the vocabulary is dropped and
        counted (lm.dropped).  A count that does not match its section, a missing \\end\\ or an order above 5 raises."""
        t2i = getattr(vocab, "_token2id", vocab)
        i2t = getattr(vocab, "_id2token", None)
        size = len(i2t) if i2t is not None else max(list(t2i.values()) + [EOS_ID]) + 1
        special = {"<s>": BOS_ID, "</s>": EOS_ID, "<unk>": UNK_ID, "<UNK>": UNK_ID}
        counts, seen, ngrams, dropped = {}, {}, {}, 0
        section, in_data, ended = 0, False, False
        with open(path, encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                line = line.strip()
                if not line:
                    continue
                if ended:
                    raise ValueError(f"{path}, line {no}: text after \\end\\")
                if line.startswith("\\"):
                    if line == "\\data\\":
                        if in_data or section:
                            raise ValueError(f"{path}, line {no}: a second \\data\\")
                        in_data = True
                    elif line == "\\end\\":
                        ended = True
                    elif line.endswith("-grams:") and line[1:-7].isdigit():
                        n = int(line[1:-7])
                        if n != section + 1 or n not in counts:
                            raise ValueError(f"{path}, line {no}: section {line} out of order or without a count in \\data\\")
                        section, in_data = n, False
                        seen[n] = 0
                    else:
                        raise ValueError(f"{path}, line {no}: unknown section {line}")
                    continue
                if in_data:
                    if not line.startswith("ngram ") or "=" not in line:
                        raise ValueError(f"{path}, line {no}: expected `ngram N=count`")
                    n, cnt = line[6:].split("=", 1)
                    n, cnt = int(n), int(cnt)
                    if n > MAX_ORDER:
                        raise ValueError(f"{path}, line {no}: order {n}: orders 1 to {MAX_ORDER} are supported")
                    if n != len(counts) + 1 or cnt < 0:
                        raise ValueError(f"{path}, line {no}: orders must be listed 1, 2, ... with counts >= 0")
                    counts[n] = cnt
                    continue
                if not section:
                    raise ValueError(f"{path}, line {no}: text before \\data\\")
                fields = line.split()
                if len(fields) not in (section + 1, section + 2):
                    raise ValueError(f"{path}, line {no}: a {section}-gram line has {section + 1} or {section + 2} fields, got {len(fields)}")
                try:
                    p = float(fields[0])
                    bow = float(fields[section + 1]) if len(fields) == section + 2 else None
                except ValueError:
                    raise ValueError(f"{path}, line {no}: not a number") from None
                seen[section] += 1
                ids = []
                for wd in fields[1:section + 1]:
                    i = special.get(wd, t2i.get(wd))
                    if i is None:
                        break
                    ids.append(int(i))
                if len(ids) < section:
                    dropped += 1
                    continue
                ngrams[tuple(ids)] = (p, bow)
        if not counts:
            raise ValueError(f"{path}: no \\data\\ section")
        if not ended:
            raise ValueError(f"{path}: no \\end\\")
        for n, cnt in counts.items():
            if seen.get(n) != cnt:
                raise ValueError(f"{path}: \\data\\ announces {cnt} {n}-grams, the file holds {seen.get(n, 0)}")
        return cls(ngrams, len(counts), size, weight=weight, ins=ins, unk_log10=unk_log10, device=device, dropped=dropped)
