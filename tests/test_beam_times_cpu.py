"""Token times of CTC prefix beam hypotheses without a GPU: the definition (tests/beam_times_ref.py) against the oracle's search and
against brute force over every alignment, its invariants, the final records, and the refusals of the Python surface."""
import math
import os
import re
import types

import numpy as np
import pytest

from oracle import decode_ref as D
from tests import beam_times_ref as BT
from tests.helpers import ROOT

NAMES = ("asr_ctc_prefix_beam_timed", "asr_ctc_prefix_beam_timed_state_init", "asr_ctc_prefix_beam_timed_state_reset", "asr_ctc_prefix_beam_chunk_timed")


def _logp(T, V, seed, peak=2.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, V)) * peak
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


def _cands(logp, k):
    return [list(np.argsort(-row, kind="stable")[:k]) for row in logp]


CASES = [(12, 6, 3, 6, 0), (20, 9, 4, 5, 1), (17, 7, 1, 7, 2), (25, 12, 8, 4, 3), (9, 5, 16, 3, 4)]      # T, V, beam, k, seed


@pytest.mark.parametrize("T,V,beam,k,seed", CASES)
def test_strings_and_scores_are_the_oracles_and_the_invariants_hold(T, V, beam, k, seed):
    for peak in (3.0, 0.3):
        logp = _logp(T, V, seed, peak)
        cand = _cands(logp, k)
        got = BT.search(BT.frames_of(logp, 0, cand), beam).hyps()
        want = [(p, s) for p, s in D.ctc_prefix_beam_search(logp, beam, 0, cand) if s != D.NEG]
        assert [(h["prefix"], h["score"]) for h in got] == want      # the same additions in the same order: equal, not close
        for h in got:
            recs = h["records"]
            assert len(recs) == len(h["prefix"])                                     # one record per token
            assert all(s <= e for s, e, *_ in recs)                                  # start <= end
            assert all(a[1] < b[0] for a, b in zip(recs, recs[1:]))                  # strictly ascending, no overlap
            assert all(0 <= s and e < T for s, e, *_ in recs)
            for (s, e, mx, mn, sm), c in zip(recs, h["prefix"]):                     # the measures are the token's posteriors over the run
                run = [np.float32(logp[t, c]) for t in range(s, e + 1)]
                acc = run[0]
                for x in run[1:]:
                    acc = np.float32(acc + x)
                assert (mx, mn, sm) == (max(run), min(run), acc)
                m = BT.measures((s, e, mx, mn, sm))
                assert m["post_min"] <= m["post_mean"] * (1 + 1e-6) and m["post_mean"] <= m["post_max"] * (1 + 1e-6) <= 1 + 1e-6
            # the alignment the records describe has the stated log-probability: tokens over their runs, blanks elsewhere
            if h["viterbi_score"] != D.NEG:
                path = [0] * T
                for (s, e, *_), c in zip(recs, h["prefix"]):
                    path[s:e + 1] = [c] * (e - s + 1)
                v = 0.0
                for t, c in enumerate(path):
                    v = v + float(logp[t, c])
                assert v == h["viterbi_score"] <= h["score"] + 1e-12


@pytest.mark.parametrize("T,V,seed", [(1, 2, 0), (3, 3, 1), (5, 3, 2), (6, 4, 3), (6, 3, 4), (4, 4, 5)])
def test_viterbi_score_is_the_brute_force_maximum(T, V, seed):
    """Every class a candidate and a beam wider than the number of prefixes: nothing is pruned, so the carried alignment is the best one."""
    logp = _logp(T, V, seed, 1.5)
    n_prefixes = sum((V - 1) ** n for n in range(T + 1))
    got = BT.search(BT.frames_of(logp), n_prefixes + 1).hyps()
    assert len(got) > 1
    for h in got:
        assert h["viterbi_score"] == BT.viterbi_bruteforce(logp, h["prefix"]), h


def test_repeat_wins_the_tie_against_the_parents_extension():
    """Two frames with equal posteriors: prefix (1,) reaches its non-blank alignment 1 1 (the repeat) and blank 1 (its parent's extension)
    with the same value; the extension is met first (the empty prefix
    ranks first) and the repeat still wins: its run covers both frames."""
    lp = math.log(0.5)
    logp = np.full((2, 2), lp)
    en = BT.search(BT.frames_of(logp), 4).beam[(1,)]
    assert en.vnb == lp + lp and en.rep and [(r[0], r[1]) for r in en.hnb] == [(0, 1)]
    assert en.vb == en.vnb and [(r[0], r[1]) for r in en.hb] == [(0, 0)]      # 1 blank ties as well: best() reports the blank one on equality


@pytest.mark.parametrize("T,V,beam,k,seed", CASES)
def test_final_records_only_grow_and_never_change(T, V, beam, k, seed):
    for peak in (3.0, 0.3):
        logp = _logp(T, V, seed, peak)
        s = BT.BeamTimes(beam)
        last, fixed = 0, ()
        for lb, cands in BT.frames_of(logp, 0, _cands(logp, k)):
            s.step(lb, cands)
            n = s.final_count()
            assert n >= last
            for h in s.hyps():      # every hypothesis, not the best alone, starts with the records that were final before
                assert tuple(zip(h["prefix"], h["records"]))[:len(fixed)] == fixed
            best = s.hyps()[0]
            assert n <= len(best["prefix"])
            last, fixed = n, tuple(zip(best["prefix"], best["records"]))[:n]
        if beam == 1 and last:
            assert last >= len(s.hyps()[0]["prefix"]) - 1      # one entry: all but the token still open


class _Model:
    decoding_chunk_size, decoding_left_chunks, use_ctc, V = 8, -1, True, 30
    vocab = types.SimpleNamespace(_id2token=[str(i) for i in range(30)])

    def frame_seconds(self):
        return 0.03


class _NoCtc(_Model):
    use_ctc = False


def test_python_surface_refuses_before_any_launch():
    from asr_chinese_e2e_amd import Models, kernels
    from asr_chinese_e2e_amd.sessions import Sessions
    from asr_chinese_e2e_amd.stream import StreamingEncoder
    for make in (lambda m=_Model, **kw: Sessions(m(), 2, **kw), lambda m=_Model, **kw: StreamingEncoder(m(), 2, **kw)):
        with pytest.raises(ValueError, match="beam_times=True needs search='prefix_beam'"):
            make(beam_times=True)
        with pytest.raises(ValueError, match="beam_times=True needs search='prefix_beam'"):
            make(beam_times=True, search="greedy")
        with pytest.raises(ValueError, match="hotword context or an n-gram LM"):
            make(beam_times=True, search="prefix_beam", context=object())
        with pytest.raises(ValueError, match="hotword context or an n-gram LM"):
            make(beam_times=True, search="prefix_beam", lm=object())
        for which in ("ent_mean", "ent_min"):
            with pytest.raises(ValueError, match="entropy measures"):
                make(beam_times=True, search="prefix_beam", confidence=which)
        with pytest.raises(ValueError, match="confidence must be"):
            make(beam_times=True, search="prefix_beam", confidence="best")
        with pytest.raises(ValueError, match="CTC head"):
            make(_NoCtc, beam_times=True, search="prefix_beam")
        with pytest.raises(ValueError, match="timed=True needs search='greedy'"):      # as before
            make(timed=True, search="prefix_beam", beam_times=True)
        ok = make(beam_times=True, search="prefix_beam", confidence="post_min")
        assert ok.which == "post_min" and ok.beam_times
        assert not make(search="prefix_beam").beam_times
    st = StreamingEncoder(_Model(), 2, search="prefix_beam", beam_times=True)
    assert st.tokens() == [[], []] and st.partial()[0]["tokens"] == [] and "tokens" not in st.nbest()[0][0]
    ss = Sessions(_Model(), 2, search="prefix_beam", beam_times=True)
    ss.open(1)
    assert ss.tokens(1) == [] and ss.partial(1)["tokens"] == []
    T = Models.TransformerCTC
    ctc = types.SimpleNamespace(use_ctc=True, use_decoder=False)
    with pytest.raises(ValueError, match="hotword context or an n-gram LM"):
        T.ctc_prefix_beam_search(ctc, None, beam_times=True, lm=object())
    with pytest.raises(ValueError, match="hotword context or an n-gram LM"):
        T.ctc_prefix_beam_search(ctc, None, beam_times=True, context=object())
    with pytest.raises(ValueError, match="entropy measures"):
        T.ctc_prefix_beam_search(ctc, None, beam_times=True, confidence="ent_mean")
    with pytest.raises(ValueError, match="CTC head"):
        T.ctc_prefix_beam_search(types.SimpleNamespace(use_ctc=False, use_decoder=True), None, beam_times=True)
    with pytest.raises(ValueError, match="device search only"):
        T.ctc_prefix_beam_search(ctc, None, beam_times=True, on_device=False)
    with pytest.raises(ValueError, match="hotword context or an n-gram LM"):
        kernels.ctc_prefix_beam_state(1, 2, 8, "cpu", lm=object(), times=True)


def test_beam_tokens_spell_the_records():
    from asr_chinese_e2e_amd.confidence import BEAM_MEASURES, beam_tokens
    f = np.float32
    mx, mn, sm = [f(-0.1), f(-0.5)], [f(-0.7), f(-0.5)], [f(-1.2), f(-0.5)]
    got = beam_tokens([7, 40], [2, 6], [4, 6], mx, mn, sm, "post_mean", [str(i) for i in range(30)], 0.03, n_final=1)
    assert [(t["id"], t["token"], t["start_frame"], t["end_frame"], t["final"]) for t in got] == [(7, "7", 2, 4, True), (40, None, 6, 6, False)]
    assert got[0]["start_s"] == 2 * 0.03 and got[0]["end_s"] == 5 * 0.03 and tuple(got[0]["measures"]) == BEAM_MEASURES
    assert got[0]["measures"] == BT.measures((2, 4, mx[0], mn[0], sm[0])) and got[0]["confidence"] == math.exp(float(sm[0]) / 3)
    assert "final" not in beam_tokens([7], [2], [4], mx, mn, sm, "post_max", ["a"] * 8, 0.03)[0]
    assert len(beam_tokens([7, 8, 9], [2, 6], [4, 6], mx, mn, sm, "post_max", ["a"] * 10, 0.03)) == 2      # a row shorter than the hypothesis


# ------------------------------------------------------------------------------------------------ the C ABI
def test_library_header_and_binding_agree_on_the_new_symbols():
    from asr_chinese_e2e_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asr_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n) and hasattr(_lib.fast, n), n
        decl = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{n} is not declared in include/asr_hip.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        kinds = [_lib.Z if p.startswith("size_t") else _lib.P if "*" in p else _lib.I for p in params]
        assert kinds == _lib.SIGNATURES[n][1], n
    for n in ("asr_ctc_prefix_beam_timed_workspace_bytes", "asr_ctc_prefix_beam_timed_state_bytes"):
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert _lib.lib.asr_abi_version() == 10      # additive: the ABI version stays
    lib = _lib.lib
    # both tries: 2 + 8 words per node; the state: the plain one, then 2 fp64 and 2 int32 per entry and the node counter, padded to 8
    assert lib.asr_ctc_prefix_beam_timed_workspace_bytes(3, 10, 4) == 3 * 10 * 41 * 4 == lib.asr_ctc_prefix_beam_workspace_bytes(3, 10, 4) * 5
    for beam in (1, 2, 5, 16):
        per = lib.asr_ctc_prefix_beam_timed_state_bytes(3, beam) // 3
        assert per % 8 == 0 and per == lib.asr_ctc_prefix_beam_state_bytes(1, beam) + 16 * beam + ((8 * beam + 4 + 7) // 8) * 8
    assert lib.asr_ctc_prefix_beam_timed_workspace_bytes(0, 10, 4) == 0 and lib.asr_ctc_prefix_beam_timed_state_bytes(1, 0) == 0


def test_argument_checks_run_before_any_launch():
    """Every refusal comes from the host-side checks with fake, never dereferenced pointers."""
    from asr_chinese_e2e_amd import _lib
    f = _lib.fast
    off = dict(vals=1024, ids=2048, blank_lp=4096, in_len=8192, ws=1 << 20, ws_bytes=3 * 10 * 41 * 4, out_tok=1 << 14, out_len=1 << 15, out_score=1 << 16,
               out_vit=1 << 17, out_start=1 << 18, out_end=1 << 19, out_mx=3 << 19, out_mn=5 << 19, out_sm=7 << 19, B=3, T=10, k=5, beam=4, nbest=4, Lcap=10,
               blank=0, stream=None)

    def call(fn, base, **over):
        a = dict(base)
        a.update(over)
        return fn(*a.values())
    for name in ("vals", "ids", "blank_lp", "ws", "out_tok", "out_len", "out_score", "out_vit", "out_start", "out_end", "out_mx", "out_mn", "out_sm"):
        assert call(f.asr_ctc_prefix_beam_timed, off, **{name: None}) == -1 and "null pointer" in _lib.last_error(), name
    for over in (dict(B=0), dict(T=0), dict(k=0), dict(beam=17), dict(k=16), dict(nbest=5), dict(Lcap=0), dict(out_vit=(1 << 17) + 4), dict(out_start=(1 << 18) + 2),
                 dict(out_sm=(7 << 19) + 1)):
        assert call(f.asr_ctc_prefix_beam_timed, off, **over) == -1, over
    assert call(f.asr_ctc_prefix_beam_timed, off, ws_bytes=3 * 10 * 41 * 4 - 1) not in (0, -1) and "workspace" in _lib.last_error()
    ch = dict(vals=1024, ids=2048, blank_lp=4096, n_valid=8192, state=1 << 13, ws=1 << 20, ws_bytes=3 * 10 * 41 * 4, out_tok=1 << 14, out_len=1 << 15,
              out_score=1 << 16, out_vit=1 << 17, out_start=1 << 18, out_end=1 << 19, out_mx=3 << 19, out_mn=5 << 19, out_sm=7 << 19, out_stable=9 << 19,
              out_final=11 << 19, B=3, C=4, k=5, beam=4, nbest=4, Lcap=10, T_cap=10, blank=0, stream=None)
    for name in ("vals", "ids", "blank_lp", "n_valid", "state", "ws", "out_tok", "out_vit", "out_sm", "out_stable", "out_final"):
        assert call(f.asr_ctc_prefix_beam_chunk_timed, ch, **{name: None}) == -1 and "null pointer" in _lib.last_error(), name
    for over in (dict(B=0), dict(C=0), dict(T_cap=0), dict(beam=17), dict(k=16), dict(nbest=5), dict(state=(1 << 13) + 4), dict(out_vit=(1 << 17) + 4),
                 dict(out_final=(11 << 19) + 2)):
        assert call(f.asr_ctc_prefix_beam_chunk_timed, ch, **over) == -1, over
    assert call(f.asr_ctc_prefix_beam_chunk_timed, ch, ws_bytes=8) not in (0, -1) and "workspace" in _lib.last_error()
    si = dict(state=1 << 13, ws=1 << 20, B=3, beam=4, T_cap=10, stream=None)
    for over in (dict(state=None), dict(ws=None), dict(B=0), dict(beam=17), dict(T_cap=0), dict(state=(1 << 13) + 4), dict(ws=(1 << 20) + 4)):
        assert call(f.asr_ctc_prefix_beam_timed_state_init, si, **over) == -1, over
    sr = dict(state=1 << 13, ws=1 << 20, flags=1 << 12, B=3, beam=4, T_cap=10, stream=None)
    for over in (dict(flags=None), dict(flags=(1 << 12) + 2), dict(beam=0)):
        assert call(f.asr_ctc_prefix_beam_timed_state_reset, sr, **over) == -1, over
