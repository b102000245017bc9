"""Hotword biasing without a GPU: the compiled tables of context.ContextGraph against the naive trie of tests/context_ref.py, the
validation errors, the definition on two constructed lattices, w = 0, and the new entry points in the binding."""
import math
import random

import numpy as np
import pytest

from oracle import decode_ref as D
from tests import context_ref as CR
from asr_chinese_e2e_amd.context import ContextGraph


def _random_strings(n, seed):
    """Token strings over [1, V): uniform ones, and ones stitched from the graphs' phrases and their prefixes (so that phrases are
    begun, finished, broken off and chained)."""
    rng = random.Random(seed)
    pieces = [ph[:i] for g in CR.GRAPHS for ph in g for i in range(1, len(ph) + 1)]
    out = [[]]
    while len(out) < n:
        if rng.random() < 0.4:
            out.append([rng.randrange(1, CR.V) for _ in range(rng.randrange(1, 9))])
        else:
            s = []
            for _ in range(rng.randrange(1, 5)):
                s += list(rng.choice(pieces)) if rng.random() < 0.8 else [rng.randrange(1, CR.V)]
            out.append(s)
    return out


@pytest.mark.parametrize("w", [3.0, 0.7, 0.0])
def test_compiled_tables_walk_as_the_naive_trie(w):
    cg = ContextGraph(CR.GRAPHS, score=w, vocab_size=CR.V)
    assert cg.n_graphs == 2 and len(cg.root_of_graph) == 2 and cg.w == w
    S, A = cg.S, cg.A
    assert cg.st_off.tolist()[0] == 0 and cg.st_off.tolist()[-1] == A and cg.st_off.numel() == S + 1
    assert cg.arc_tok.numel() == cg.arc_next.numel() == A and cg.st_held.numel() == cg.st_root.numel() == S
    assert all(0 <= n < S for n in cg.arc_next.tolist()) and all(1 <= t < CR.V for t in cg.arc_tok.tolist())
    off, tok = cg.st_off.tolist(), cg.arc_tok.tolist()
    for s in range(S):
        assert tok[off[s]:off[s + 1]] == sorted(set(tok[off[s]:off[s + 1]]))      # ascending and unique within a state
    for gi, phrases in enumerate(CR.GRAPHS):
        trie = CR.Trie(phrases, w)
        assert cg.st_root.tolist()[cg.root_of_graph[gi]] == cg.root_of_graph[gi]
        for s in _random_strings(2000, 100 + gi):
            node, bias = trie.walk(s)
            state, got = cg.walk(gi, s)
            assert got == bias and type(got) is float, (gi, s, got, bias)      # exactly: the same fp64 additions
            assert state == cg.state_of(gi, node["path"]), (gi, s, state, node["path"])
            assert cg.held(state) == trie.held(node)
            assert cg.st_root.tolist()[state] == cg.root_of_graph[gi]
    assert cg.walk(-1, [3, 3, 7]) == (-1, 0.0) and cg.held(-1) == 0.0
    # a final leaf is no state: its arc already points at the root
    assert cg.walk(0, [5]) == (cg.root_of_graph[0], w) and cg.walk(1, [4, 4]) == (cg.root_of_graph[1], 2 * w)
    # (3, 3) is final and a prefix of (3, 3, 7): nothing is held on it, and the longer phrase goes on from it
    st, b = cg.walk(0, [3, 3])
    assert st != cg.root_of_graph[0] and b == 2 * w and cg.held(st) == 0.0
    assert cg.walk(0, [3, 3, 7]) == (cg.root_of_graph[0], 3 * w)
    st, b = cg.walk(0, [8, 9, 10])
    assert cg.held(st) == 3 * w and b - cg.held(st) == 0.0


def test_context_graph_is_immutable_and_validates():
    cg = ContextGraph(CR.GRAPHS, vocab_size=CR.V)
    with pytest.raises(AttributeError):
        cg.w = 1.0
    with pytest.raises(AttributeError):
        cg._w = 1.0
    with pytest.raises(ValueError, match="token 0"):
        ContextGraph([[(1, 0, 2)]], vocab_size=CR.V)
    with pytest.raises(ValueError, match="token 12"):
        ContextGraph([[(1, 12)]], vocab_size=CR.V)
    with pytest.raises(ValueError, match="token 12"):
        ContextGraph([[(1, 12)]]).check_vocab(CR.V)
    with pytest.raises(ValueError, match="empty"):
        ContextGraph([[(1, 2), ()]], vocab_size=CR.V)
    with pytest.raises(ValueError, match="graph 1 has no phrase"):
        ContextGraph([[(1, 2)], []], vocab_size=CR.V)
    with pytest.raises(ValueError, match="no graph"):
        ContextGraph([], vocab_size=CR.V)
    with pytest.raises(ValueError, match="finite"):
        ContextGraph(CR.GRAPHS, score=float("inf"))
    with pytest.raises(ValueError, match="graph 2 of 2"):
        cg.walk(2, [1])
    with pytest.raises(ValueError):
        cg.roots([0, 1], 3)
    assert cg.roots(None, 3) == [cg.root_of_graph[0]] * 3 and cg.roots([1, -1, 0], 3) == [cg.root_of_graph[1], -1, cg.root_of_graph[0]]


def test_from_file_reads_phrases_and_names_the_bad_line(tmp_path):
    from asr_chinese_e2e_amd.data_handler import Vocab
    vocab = Vocab.synthetic(40)
    a, b, c = (chr(0x4E00 + i) for i in range(3))
    good = tmp_path / "hot.txt"
    good.write_text(f"{a}{b}\n\n  \n{c}\n{a}{b}{c}\n", encoding="utf-8")
    cg = ContextGraph.from_file(str(good), vocab, score=2.0)
    ref = CR.Trie([(4, 5), (6,), (4, 5, 6)], 2.0)
    assert cg.n_graphs == 1 and cg.w == 2.0 and cg.vocab_size == 40
    for s in ([4, 5, 6], [4, 5, 7], [6, 6], [4, 4, 5]):
        assert cg.walk(0, s)[1] == ref.walk(s)[1]
    bad = tmp_path / "bad.txt"
    bad.write_text(f"{a}{b}\n\n{a}x{c}\n", encoding="utf-8")
    with pytest.raises(ValueError, match=r"bad\.txt, line 3: character 'x'"):
        ContextGraph.from_file(str(bad), vocab)
    empty = tmp_path / "empty.txt"
    empty.write_text("\n\n", encoding="utf-8")
    with pytest.raises(ValueError, match="no phrase"):
        ContextGraph.from_file(str(empty), vocab)


# ---------------------------------------------------------------------------------------------- the definition on constructed lattices
A_, B_, C_, D_, E_ = 1, 2, 3, 4, 5


def _frames(rows):
    """(T, 6) log-probabilities from per-frame {class: probability}; the rest of each frame's mass is spread over the other classes."""
    out = np.zeros((len(rows), 6))
    for t, row in enumerate(rows):
        rest = (1.0 - sum(row.values())) / (6 - len(row))
        for c in range(6):
            out[t, c] = math.log(row.get(c, rest))
    return out


def _as_dict(lst):
    return {p: (sc, ctc, bias) for p, sc, ctc, bias in lst}


def _five_frames(last):
    """A, blank, D (0.62) or B (0.31), blank, `last` - each frame with a clear second candidate, so that top-2 pruning is unambiguous."""
    return _frames([{A_: 0.95, 0: 0.03}, {0: 0.95, A_: 0.03}, {D_: 0.62, B_: 0.31}, {0: 0.95, D_: 0.03}, {last: 0.95, 0: 0.03}])


def test_a_finished_phrase_wins_and_an_unfinished_one_pays_back():
    trie = CR.Trie([(A_, B_, C_)], 3.0)
    cg = ContextGraph([[(A_, B_, C_)]], vocab_size=6)
    wide = 10 ** 4      # a beam that never prunes here: every ctc_score is the exact sum over the candidates, biased or not
    # "A D C" beats "A B C" by log 2 = 0.69 nats: the middle frame gives D twice B's probability
    logp = _five_frames(C_)
    cand = CR.topk_candidates(logp, 2)      # biasing re-ranks what the acoustic model proposes: the two best classes of each frame
    assert [sorted(c) for c in cand] == [[0, A_], [0, A_], [B_, D_], [0, D_], [0, C_]]
    plain, _ = CR.ctc_prefix_beam_search(logp, wide, candidates=cand)
    assert [(p, s) for p, s, _, _ in plain] == D.ctc_prefix_beam_search(logp, wide, candidates=cand)
    pd = _as_dict(plain)
    assert plain[0][0] == (A_, D_, C_) and abs(pd[(A_, D_, C_)][0] - pd[(A_, B_, C_)][0] - math.log(2.0)) < 0.05      # plus what the D of frame 3 adds to "A D C"
    biased, _ = CR.ctc_prefix_beam_search(logp, wide, candidates=cand, trie=trie)
    assert biased[0][0] == (A_, B_, C_) and biased[0][3] == 9.0
    assert abs(biased[0][2] - pd[(A_, B_, C_)][1]) < 1e-12 and biased[0][1] == biased[0][2] + 9.0
    bd = _as_dict(biased)
    assert set(bd) == set(pd)
    assert bd[(A_, D_, C_)][2] == 0.0 and abs(bd[(A_, D_, C_)][1] - pd[(A_, D_, C_)][1]) < 1e-12
    for p, (sc, ctc, bias) in bd.items():      # the tables agree with the definition on every hypothesis of the list
        st, raw = cg.walk(0, p)
        assert raw - cg.held(st) == bias, p
    # "A B E": the 6.0 handed out for "A B" is paid back - the result equals the unbiased one, with bias 0.0
    logp = _five_frames(E_)
    cand = CR.topk_candidates(logp, 2)
    plain, _ = CR.ctc_prefix_beam_search(logp, wide, candidates=cand)
    biased, _ = CR.ctc_prefix_beam_search(logp, wide, candidates=cand, trie=trie)
    assert plain[0][0] == (A_, D_, E_) and (A_, B_, E_) in _as_dict(plain)
    assert [p for p, _, _, _ in biased] == [p for p, _, _, _ in plain]
    for (p, sc, ctc, bias), (_, psc, pctc, _) in zip(biased, plain):
        assert bias == 0.0 and sc == ctc and (ctc == pctc or abs(ctc - pctc) < 1e-12), p
    assert cg.walk(0, (A_, B_))[1] == 6.0 and cg.walk(0, (A_, B_, E_)) == (cg.root_of_graph[0], 0.0)
    # a phrase begun at the end of the string earns nothing either
    st, raw = cg.walk(0, (D_, A_, B_))
    assert raw == 6.0 and raw - cg.held(st) == 0.0


@pytest.mark.parametrize("peak", [3.0, 1.0, 0.3])
def test_no_graph_and_w_zero_reproduce_the_oracle(peak):
    for seed in range(3):
        logp = CR.lattice(seed, 48, peak)
        cand = CR.topk_candidates(logp, 5)
        want = D.ctc_prefix_beam_search(logp, 4, candidates=cand)
        plain, gap = CR.ctc_prefix_beam_search(logp, 4, candidates=cand)
        assert [(p, s) for p, s, _, _ in plain] == want and gap > 0.0
        for gi, phrases in enumerate(CR.GRAPHS):
            zero, _ = CR.ctc_prefix_beam_search(logp, 4, candidates=cand, trie=CR.Trie(phrases, 0.0))
            assert [(p, s) for p, s, _, _ in zero] == want
            assert all(bias == 0.0 and sc == ctc for _, sc, ctc, bias in zero)
            biased, gap = CR.ctc_prefix_beam_search(logp, 4, candidates=cand, trie=CR.Trie(phrases, 3.0))
            assert gap > 1e-9
            assert [h[1] for h in biased] == sorted((h[1] for h in biased), reverse=True)
            assert all(bias >= 0.0 for _, _, _, bias in biased)


def test_the_new_entry_points_are_bound_and_the_abi_is_unchanged():
    from asr_chinese_e2e_amd import _lib
    for name in ("asr_ctc_prefix_beam_ctx", "asr_ctc_prefix_beam_ctx_state_bytes", "asr_ctc_prefix_beam_ctx_state_init",
                 "asr_ctc_prefix_beam_ctx_state_reset", "asr_ctc_prefix_beam_chunk_ctx"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name), name
    assert _lib.lib.asr_abi_version() == _lib.ABI_VERSION == 10
    # the context state: the plain one, then fp64 bias[beam], int32 ctx[beam], int32 root, padded to 8 bytes
    for B, beam in ((1, 1), (3, 4), (2, 5), (7, 16)):
        plain = _lib.lib.asr_ctc_prefix_beam_state_bytes(B, beam)
        ctx = _lib.lib.asr_ctc_prefix_beam_ctx_state_bytes(B, beam)
        assert ctx == plain + B * (8 * beam + (4 * beam + 4 + 7) // 8 * 8) and ctx % 8 == 0
