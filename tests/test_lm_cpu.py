"""N-gram LM shallow fusion without a GPU: the ARPA reader on a file written by hand, the compiled automaton of lm.NgramLM against the
recursive definition of tests/lm_ref.py bit for bit, the definition on a constructed lattice (through lm_ref and through the host loop of
decode.ctc_prefix_beam_search), weight 0, the refusals that need no launch, and the new entry points in the binding."""
import math
import random
import types

import numpy as np
import pytest
import torch

from oracle import decode_ref as D
from tests import lm_ref as R
from asr_chinese_e2e_amd.lm import NgramLM

LN10 = math.log(10.0)

ARPA = """\\data\\
ngram 1=4
ngram 2=2

\\1-grams:
-1.0\t<s>\t-0.5
-0.7\ta\t-0.3
-0.9\tb
-1.2\t</s>

\\2-grams:
-0.2\t<s> a
-0.4\ta b

\\end\\
"""
VOCAB = {"$": 0, "%": 1, "^": 2, "&": 3, "a": 4, "b": 5}
A_, B_ = 4, 5


# ---------------------------------------------------------------------------------------------- 1. ARPA by hand
def test_arpa_by_hand_gives_the_back_off_values(tmp_path):
    path = tmp_path / "hand.arpa"
    path.write_text(ARPA, encoding="utf-8")
    lm = NgramLM.from_arpa(str(path), VOCAB, weight=1.0, ins=0.0)
    assert lm.order == 2 and lm.vocab_size == 6 and lm.dropped == 0 and lm.n_ngrams == 6 and lm.has_eos
    assert lm.start != 0      # <s> is listed: a hypothesis starts from the history (<s>)
    s_bos = lm.start
    s_a, _ = lm.advance(s_bos, 0.0, A_)
    s_b, _ = lm.advance(s_bos, 0.0, B_)
    # (state, token) -> the log10 values added in chain order
    cases = [(s_bos, A_, [-0.2]),            # p(a | <s>): bigram hit
             (s_bos, B_, [-0.5, -0.9]),      # p(b | <s>) = -1.4
             (s_a, B_, [-0.4]),              # p(b | a): bigram hit
             (s_a, A_, [-0.3, -0.7]),        # p(a | a) = -1.0
             (s_b, A_, [-0.7]),              # p(a | b): b has no back-off column
             (s_a, 3, [-0.3, -1.2]),         # p(</s> | a) = -1.5
             (s_b, 3, [-1.2])]               # p(</s> | b): unigram
    log10 = [-0.2, -1.4, -0.4, -1.0, -0.7, -1.5, -1.2]
    for (st, c, chain), total in zip(cases, log10):
        want = 0.0
        for x in chain:
            want = want + 1.0 * (x * LN10)
        got = lm.advance(st, 0.0, c)[1]
        assert got == want, (st, c, got, want)      # exactly: the same fp64 additions
        assert abs(got / LN10 - total) < 1e-12, (st, c, got / LN10, total)
    # the end term through final(), and a whole string
    assert lm.final(s_a, 0.0) == 0.0 + (-0.3 * LN10) + (-1.2 * LN10) and lm.final(s_b, 0.0) == -1.2 * LN10
    assert lm.score([A_, B_]) == ((0.0 + -0.2 * LN10) + -0.4 * LN10) + -1.2 * LN10
    # the weight and the insertion bonus are folded in on the host
    lm2 = NgramLM.from_arpa(str(path), VOCAB, weight=0.3, ins=0.25)
    assert lm2.advance(lm2.start, 0.0, B_)[1] == ((0.0 + 0.3 * (-0.5 * LN10)) + 0.3 * (-0.9 * LN10)) + 0.25
    # the definition agrees
    ref = R.Model({(2,): (-1.0, -0.5), (A_,): (-0.7, -0.3), (B_,): (-0.9, None), (3,): (-1.2, None), (2, A_): (-0.2, None), (A_, B_): (-0.4, None)}, 2, 1.0)
    for h, w, total in [((2,), A_, -0.2), ((2,), B_, -1.4), ((A_,), B_, -0.4), ((A_,), A_, -1.0), ((B_,), A_, -0.7), ((A_,), 3, -1.5), ((B_,), 3, -1.2)]:
        assert abs(ref.log10p(h, w) - total) < 1e-12


def test_arpa_drops_words_outside_the_vocabulary_and_refuses_malformed_files(tmp_path):
    def load(text):
        p = tmp_path / "x.arpa"
        p.write_text(text, encoding="utf-8")
        return NgramLM.from_arpa(str(p), VOCAB, weight=1.0)
    more = ARPA.replace("ngram 1=4", "ngram 1=5").replace("ngram 2=2", "ngram 2=3").replace("-1.2\t</s>\n", "-1.2\t</s>\n-2.0\tq\t-0.1\n").replace(
        "-0.4\ta b\n", "-0.4\ta b\n-0.3\tq a\n")
    lm = load(more)
    assert lm.dropped == 2 and lm.n_ngrams == 6
    assert lm.score([A_, B_, A_]) == load(ARPA).score([A_, B_, A_])
    with pytest.raises(ValueError, match="announces 4 1-grams"):
        load(ARPA.replace("-0.9\tb\n", ""))                           # a count mismatch
    with pytest.raises(ValueError, match="announces 2 2-grams"):
        load(ARPA.replace("\\end\\", "-0.1\tb a\n\\end\\"))
    with pytest.raises(ValueError, match=r"no \\end\\"):
        load(ARPA.replace("\\end\\\n", ""))
    with pytest.raises(ValueError, match="order 6"):
        load(ARPA.replace("ngram 2=2\n", "ngram 2=2\nngram 3=0\nngram 4=0\nngram 5=0\nngram 6=1\n"))
    with pytest.raises(ValueError, match="fields"):
        load(ARPA.replace("-0.4\ta b\n", "-0.4\ta b a -0.1 7\n"))
    with pytest.raises(ValueError, match="not a number"):
        load(ARPA.replace("-0.4\ta b\n", "x\ta b\n"))
    with pytest.raises(ValueError, match="non-finite"):
        load(ARPA.replace("-0.4\ta b\n", "-inf\ta b\n"))
    # <unk> is recognised by name and serves the tokens without a unigram
    with_unk = load(ARPA.replace("ngram 1=4", "ngram 1=5").replace("-1.2\t</s>\n", "-1.2\t</s>\n-3.0\t<unk>\n"))
    assert with_unk.advance(0, 0.0, 0)[1] == -3.0 * LN10 and load(ARPA).advance(0, 0.0, 0)[1] == -10.0 * LN10


# ---------------------------------------------------------------------------------------------- 2. the automaton against the definition
def _random_strings(n, seed, table):
    """Token strings over [1, V): uniform ones, and ones stitched from the listed n-grams (so that high-order hits happen and break off)."""
    rng = random.Random(seed)
    grams = sorted(table)
    out = [[]]
    while len(out) < n:
        if rng.random() < 0.5:
            out.append([1 + int(rng.random() * (R.V - 1)) for _ in range(1 + int(rng.random() * 9))])
        else:
            s = []
            for _ in range(1 + int(rng.random() * 4)):
                s += [t for t in grams[int(rng.random() * len(grams))] if t != R.BOS] if rng.random() < 0.8 else [1 + int(rng.random() * (R.V - 1))]
            out.append(s)
    return out


@pytest.mark.parametrize("with_bos", [True, False], ids=["bos", "no_bos"])
@pytest.mark.parametrize("weight,ins", [(0.3, 0.0), (0.7, 0.4), (1.0, -0.2)])
def test_automaton_equals_the_recursive_definition_bit_for_bit(weight, ins, with_bos):
    table = R.table(with_bos)
    ref = R.Model(table, R.ORDER, weight, ins)
    lm = NgramLM(table, R.ORDER, R.V, weight=weight, ins=ins)
    assert (lm.start != 0) == with_bos
    for s in _random_strings(400, 7, table):
        want = ref.biases(s)
        st, bias = lm.start, 0.0
        for i, c in enumerate(s):
            st, bias = lm.advance(st, bias, c)
            assert bias == want[i] and type(bias) is float, (s, i, bias, want[i])      # exactly: the same fp64 additions
            assert 0 <= st < lm.S
        assert lm.walk(s) == (st, bias)
        assert lm.score(s) == ref.lm_score(s), s
    # every kind of chain occurred
    assert ref.kinds == {R.TRIGRAM_HIT, R.BACKOFF_ONE, R.BACKOFF_TWO, R.CONTEXT_NOT_LISTED, R.CONTEXT_WITHOUT_BOW, R.UNK_TERM, R.HIT_THEN_SHORTER_STATE}


def test_tables_are_consistent_and_survive_save_and_load(tmp_path):
    lm = NgramLM(R.table(), R.ORDER, R.V, weight=0.3, ins=0.1)
    S, A = lm.S, lm.A
    off, tok, nxt = lm.table("st_off").tolist(), lm.table("arc_tok").tolist(), lm.table("arc_next").tolist()
    assert len(off) == S + 1 and off[0] == off[1] == 0 and off[-1] == A      # state 0 has no arc range
    for s in range(S):
        assert tok[off[s]:off[s + 1]] == sorted(set(tok[off[s]:off[s + 1]]))      # ascending and unique within a state
    assert all(0 <= (n if n >= 0 else ~n) < S for n in nxt) and any(n < 0 for n in nxt)      # the test LM has contexts that are not listed
    assert all(0 <= b < S for b in lm.table("st_back").tolist()) and lm.table("uni_term").numel() == R.V
    # a trigram whose bigram prefix is not listed is still found from that context
    hole = next(g for g in sorted(R.TABLE) if len(g) == 3 and g[:2] not in R.TABLE and g[0] != R.BOS)
    ref = R.Model(R.table(), R.ORDER, 0.3, 0.1)
    assert lm.walk(hole)[1] == ref.bias(hole)
    path = tmp_path / "lm.npz"
    lm.save(str(path))
    back = NgramLM.load(str(path))
    for name in ("st_off", "arc_tok", "arc_next", "arc_term", "st_back", "st_bow", "uni_term", "uni_next"):
        assert torch.equal(lm.table(name), back.table(name)) and lm.table(name).dtype == back.table(name).dtype, name
    assert (back.S, back.A, back.order, back.vocab_size, back.start, back.ins, back.weight, back.has_eos, back.dropped) == \
           (lm.S, lm.A, lm.order, lm.vocab_size, lm.start, lm.ins, lm.weight, lm.has_eos, lm.dropped)
    assert back.score([4, 5, 6, 11, 7]) == lm.score([4, 5, 6, 11, 7])
    with pytest.raises(AttributeError):
        lm.weight = 1.0
    np.savez(str(tmp_path / "other.npz"), x=np.zeros(3))
    with pytest.raises(ValueError, match="not a saved NgramLM"):
        NgramLM.load(str(tmp_path / "other.npz"))


def test_orders_one_to_five_and_no_higher():
    rng = random.Random(3)
    for order in range(1, 6):
        table = {(c,): (-1.0 - rng.random(), -rng.random()) for c in range(2, 9)}
        for n in range(2, order + 1):
            for _ in range(30):
                g = tuple(4 + int(rng.random() * 5) for _ in range(n))
                table[g] = (-rng.random(), None if n == order or rng.random() < 0.3 else -rng.random())
        ref = R.Model(table, order, 0.5, 0.05)
        lm = NgramLM(table, order, 10, weight=0.5, ins=0.05)
        for _ in range(200):
            s = [1 + int(rng.random() * 9) for _ in range(1 + int(rng.random() * 8))]
            assert lm.walk(s)[1] == ref.bias(s) and lm.score(s) == ref.lm_score(s), (order, s)
    with pytest.raises(ValueError, match="orders 1 to 5"):
        NgramLM({(4,): (-1.0, None)}, 6, 10)
    with pytest.raises(ValueError, match="the order is 2"):
        NgramLM({(4, 5, 6): (-1.0, None)}, 2, 10)


# ---------------------------------------------------------------------------------------------- 3. / 4. the definition on lattices
def _frames(rows):
    """(T, V) log-probabilities from per-frame {class: probability}; the rest of each frame's mass is spread over the other classes."""
    out = np.zeros((len(rows), R.V))
    for t, row in enumerate(rows):
        rest = (1.0 - sum(row.values())) / (R.V - len(row))
        for c in range(R.V):
            out[t, c] = math.log(row.get(c, rest))
    return out


class _HostModel:
    """What decode.ctc_prefix_beam_search(on_device=False) needs of a model, without a GPU: the CTC head's output is given."""
    V = R.V

    def __init__(self, logp):
        self.logits = torch.from_numpy(np.asarray(logp)).float()[None]
        self.eng = types.SimpleNamespace(use_ctc=True, training=False)

    def _ensure_engine(self, device):
        return self.eng

    def forward(self, input):
        return types.SimpleNamespace(ctc_logits=self.logits)

    def input(self):
        return types.SimpleNamespace(wave=types.SimpleNamespace(device="cpu"), wave_len=torch.tensor([self.logits.shape[1]]))


def _host_topk(logits, k, blank=0):
    """asr_ctc_frame_topk on the host: log_softmax, the k best classes per frame (ties: smaller index first), the blank's value."""
    lsm = torch.log_softmax(logits.double(), -1)
    order = np.stack([np.lexsort((np.arange(lsm.shape[1]), -lsm[r].numpy()))[:k] for r in range(lsm.shape[0])])
    ids = torch.from_numpy(order.astype(np.int32))
    return lsm.gather(1, ids.long()).float(), ids, lsm[:, blank].float()


def _host_search(monkeypatch, logp, beam, nbest, k, lm=None):
    from asr_chinese_e2e_amd import decode
    monkeypatch.setattr(decode.K, "ctc_frame_topk", _host_topk)
    m = _HostModel(logp)
    return decode.ctc_prefix_beam_search(m, m.input(), beam, nbest, k, on_device=False, lm=lm)[0]


def _pick_reversal():
    """Tokens (x, y1, y2, z) of the test LM, drawn from it: the LM (weight 1) prefers x y2 z to x y1 z by more than 1.5 nats."""
    ref = R.Model(R.table(), R.ORDER, 1.0)
    best = None
    for x in range(4, 11):
        for z in range(4, 11):
            for y1 in range(4, 11):
                for y2 in range(4, 11):
                    if len({x, y1, y2, z}) == 4:
                        d = ref.lm_score((x, y2, z)) - ref.lm_score((x, y1, z))
                        if best is None or d > best[0]:
                            best = (d, x, y1, y2, z)
    assert best[0] > 1.5, best
    return best[1:]


def test_the_lm_changes_the_answer(monkeypatch):
    x, y1, y2, z = _pick_reversal()
    # x, blank, y1 (0.50) or y2 (0.40), blank, z, blank: "x y1 z" beats "x y2 z" by log 1.25 = 0.22 nats acoustically
    logp = _frames([{x: 0.95, 0: 0.03}, {0: 0.95, x: 0.03}, {y1: 0.50, y2: 0.40}, {0: 0.95, y1: 0.03}, {z: 0.95, 0: 0.03}, {0: 0.95, z: 0.03}])
    table = R.table()
    # weight 0.3: the LM's preference is worth more than 0.45 nats, and a dropped token would cost log (0.95 / 0.03) = 3.5
    ref, lm = R.Model(table, R.ORDER, 0.3), NgramLM(table, R.ORDER, R.V, weight=0.3)
    cand = R.topk_candidates(logp, 2)
    plain, _ = R.ctc_prefix_beam_search(logp, 8, candidates=cand)
    fused, gap = R.ctc_prefix_beam_search(logp, 8, candidates=cand, lm=ref)
    assert plain[0][0] == (x, y1, z) and plain[1][0] == (x, y2, z)
    assert fused[0][0] == (x, y2, z) and gap > 1e-9
    by = {h[0]: h for h in fused}
    pl = {h[0]: h for h in plain}
    for p in ((x, y1, z), (x, y2, z)):
        assert by[p][3] == ref.lm_score(p) == lm.score(p) and by[p][1] == by[p][2] + by[p][3]
        assert abs(by[p][2] - pl[p][2]) < 1e-12      # ctc_score stays the pure log-probability
    # the host loop of the product applies the same definition through NgramLM.walk (float32 candidates: close, and the same order)
    host_plain = _host_search(monkeypatch, logp, 8, 8, 2)
    host = _host_search(monkeypatch, logp, 8, 8, 2, lm=lm)
    assert host_plain[0]["yseq"] == [x, y1, z] and set(host_plain[0]) == {"yseq", "score"}
    assert host[0]["yseq"] == [x, y2, z] and set(host[0]) == {"yseq", "score", "ctc_score", "lm_score"}
    assert [tuple(h["yseq"]) for h in host] == [h[0] for h in fused]
    for h, w in zip(host, fused):
        assert h["lm_score"] == w[3] and h["score"] == h["ctc_score"] + h["lm_score"] and abs(h["ctc_score"] - w[2]) < 1e-5


@pytest.mark.parametrize("peak", [3.0, 1.0, 0.3])
def test_no_lm_and_weight_zero_reproduce_the_oracle(monkeypatch, peak):
    table = R.table()
    zero_ref, zero = R.Model(table, R.ORDER, 0.0, 0.0), NgramLM(table, R.ORDER, R.V, weight=0.0, ins=0.0)
    for seed in range(3):
        logp = R.lattice(seed, 48, peak)
        cand = R.topk_candidates(logp, 5)
        want = D.ctc_prefix_beam_search(logp, 4, candidates=cand)
        plain, gap = R.ctc_prefix_beam_search(logp, 4, candidates=cand)
        assert [(p, s) for p, s, _, _ in plain] == want and gap > 0.0      # with no LM, decode_ref's lists
        off, _ = R.ctc_prefix_beam_search(logp, 4, candidates=cand, lm=zero_ref)
        assert [(p, s) for p, s, _, _ in off] == want
        assert all(l == 0.0 and math.copysign(1.0, l) == 1.0 and sc == ctc for _, sc, ctc, l in off)
        fused, gap = R.ctc_prefix_beam_search(logp, 4, candidates=cand, lm=R.Model(table, R.ORDER, 0.5, 0.1))
        assert gap > 1e-9 and [h[1] for h in fused] == sorted((h[1] for h in fused), reverse=True)
        assert [h[0] for h in fused] != [h[0] for h in plain] or seed
    logp = R.lattice(0, 24, peak)
    host_plain = _host_search(monkeypatch, logp, 4, 4, 5)
    host = _host_search(monkeypatch, logp, 4, 4, 5, lm=zero)
    assert [h["yseq"] for h in host] == [h["yseq"] for h in host_plain]
    for h, p in zip(host, host_plain):
        assert h["lm_score"] == 0.0 and math.copysign(1.0, h["lm_score"]) == 1.0 and h["score"] == h["ctc_score"] == p["score"]
    for s in ([], [4, 5, 11, 1, 6]):
        st, b = zero.walk(s)
        assert b == 0.0 and math.copysign(1.0, b) == 1.0 and math.copysign(1.0, zero.final(st, b)) == 1.0


# ---------------------------------------------------------------------------------------------- 5. refusals that need no launch
def test_refusals_before_any_launch():
    from asr_chinese_e2e_amd import Models, decode, kernels
    from asr_chinese_e2e_amd.context import ContextGraph
    from asr_chinese_e2e_amd.sessions import Sessions
    from asr_chinese_e2e_amd.stream import StreamingEncoder
    lm = NgramLM(R.table(), R.ORDER, R.V)
    cg = ContextGraph([[(4, 5)]], vocab_size=R.V)
    t = torch.zeros(4, 2)
    # an LM together with a context
    with pytest.raises(ValueError, match="cannot be combined"):
        kernels.ctc_prefix_beam(t, t.int(), t[:, 0], None, 1, 4, 2, 2, lm=lm, context=cg)
    with pytest.raises(ValueError, match="cannot be combined"):
        kernels.ctc_prefix_beam_state(1, 2, 4, "cpu", lm=lm, context=cg)
    m = _HostModel(R.lattice(0, 4, 1.0))
    with pytest.raises(ValueError, match="cannot be combined"):
        decode.ctc_prefix_beam_search(m, m.input(), 2, 1, lm=lm, context=cg)
    with pytest.raises(ValueError, match="cannot be combined"):
        decode.ctc_rescore_search(m, m.input(), 2, 1, lm=lm, context=cg)
    with pytest.raises(TypeError):
        decode.ctc_prefix_beam_search(m, m.input(), 2, 1, lm=R.table())
    # an LM whose vocabulary size differs from the model's
    m.V = R.V + 1
    with pytest.raises(ValueError, match="vocabulary of 12 tokens, the model has 13"):
        decode.ctc_prefix_beam_search(m, m.input(), 2, 1, lm=lm)
    m.V = R.V
    # searches without a prefix beam
    M = Models.TransformerOffical
    for kw in (dict(joint="one_pass", ctc_weight=0.3), dict(joint="rescore", ctc_weight=0.3), dict(joint="rescore", ctc_weight=0.0)):
        with pytest.raises(ValueError, match="ctc_rescore"):
            M.beam_search(m, m.input(), beam_size=3, lm=lm, **kw)
    m.decoding_chunk_size, m.decoding_left_chunks, m.use_ctc = 4, -1, True
    for cls in (StreamingEncoder, Sessions):
        with pytest.raises(ValueError, match="prefix_beam"):
            cls(m, 2, search="greedy", lm=lm)
        with pytest.raises(ValueError, match="prefix_beam"):
            cls(m, 2, lm=lm)
        with pytest.raises(ValueError, match="cannot be combined"):
            cls(m, 2, search="prefix_beam", beam_size=4, frame_topk=5, lm=lm, context=cg)
    # non-finite weight, ins or table values
    for kw in (dict(weight=float("inf")), dict(weight=float("nan")), dict(ins=float("-inf")), dict(unk_log10=float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            NgramLM(R.table(), R.ORDER, R.V, **kw)
    with pytest.raises(ValueError, match="non-finite"):
        NgramLM({(4,): (float("-inf"), None)}, 1, R.V)
    with pytest.raises(ValueError, match="non-finite"):
        NgramLM({(4,): (-1.0, float("nan"))}, 2, R.V)
    with pytest.raises(ValueError, match="finite"):
        NgramLM({(4,): (-1e308, None)}, 1, R.V, weight=1e10)      # the folded term overflows
    with pytest.raises(ValueError, match="outside"):
        NgramLM({(4, R.V): (-1.0, None)}, 2, R.V)


def test_the_new_entry_points_are_bound_and_the_abi_is_unchanged():
    from asr_chinese_e2e_amd import _lib
    for name in ("asr_ctc_prefix_beam_lm", "asr_ctc_prefix_beam_lm_workspace_bytes", "asr_ctc_prefix_beam_lm_state_bytes", "asr_ctc_prefix_beam_lm_state_init",
                 "asr_ctc_prefix_beam_lm_state_reset", "asr_ctc_prefix_beam_chunk_lm"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name), name
    assert _lib.lib.asr_abi_version() == _lib.ABI_VERSION == 10
    # the LM state: the plain one, then fp64 bias[beam], int32 st[beam], padded to 8 bytes
    for B, beam in ((1, 1), (3, 4), (2, 5), (7, 16)):
        plain = _lib.lib.asr_ctc_prefix_beam_state_bytes(B, beam)
        got = _lib.lib.asr_ctc_prefix_beam_lm_state_bytes(B, beam)
        assert got == plain + B * (8 * beam + (4 * beam + 7) // 8 * 8) and got % 8 == 0
        assert _lib.lib.asr_ctc_prefix_beam_lm_workspace_bytes(B, 50, beam) == 2 * _lib.lib.asr_ctc_prefix_beam_workspace_bytes(B, 50, beam)
    from asr_chinese_e2e_amd.lm import LmTables
    import ctypes
    assert ctypes.sizeof(LmTables) == 8 * 8 + 5 * 4 + 4 + 8      # asr_ngram_lm: 8 pointers, 5 ints, a pad word, ins
