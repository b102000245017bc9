"""The fp64 restatement of CTC prefix scoring (tests/joint_ref.py) against brute-force enumeration of every frame path on tiny
lattices: psi(h) = total probability of the paths whose collapse begins with h, and the eos score = log p_ctc(h) of
oracle/decode_ref.ctc_label_logprob_bruteforce.  No GPU."""
import itertools
import math

import numpy as np
import pytest

from oracle.decode_ref import ctc_label_logprob_bruteforce
from tests import joint_ref as J


def _paths(logp, blank=0):
    T, V = logp.shape
    for path in itertools.product(range(V), repeat=T):
        col, prev = [], None
        for c in path:
            if c != prev and c != blank:
                col.append(c)
            prev = c
        yield tuple(col), sum(logp[t, c] for t, c in enumerate(path))


def _brute_prefix(logp, prefix, blank=0):
    tot = -math.inf
    n = len(prefix)
    for col, lp in _paths(logp, blank):
        if col[:n] == tuple(prefix):
            tot = np.logaddexp(tot, lp)
    return float(tot)


def _lattice(T, V, seed):
    rng = np.random.default_rng(seed)
    return J.log_softmax(rng.normal(0.0, 1.5, size=(T, V)))


@pytest.mark.parametrize("T,V,seed", [(1, 3, 0), (3, 4, 1), (5, 3, 2), (6, 4, 3), (7, 3, 4)])
def test_prefix_probability_matches_enumeration(T, V, seed):
    logp = _lattice(T, V, seed)
    for n in range(0, 4):
        for prefix in itertools.product(range(1, V), repeat=n):     # repeated tokens included ([1, 1], [2, 2, 1], ...)
            want = _brute_prefix(logp, prefix)
            got = J.prefix_logprob(logp, prefix)
            if want == -math.inf:
                assert got == -math.inf, (prefix, got)
            else:
                assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (prefix, got, want)


def test_empty_prefix_has_probability_one():
    logp = _lattice(5, 4, 7)
    assert J.prefix_logprob(logp, ()) == 0.0
    assert abs(_brute_prefix(logp, ())) < 1e-12


@pytest.mark.parametrize("T,V,seed", [(3, 3, 5), (5, 4, 6), (6, 3, 8)])
def test_eos_score_is_full_sequence_probability(T, V, seed):
    logp = _lattice(T, V, seed)
    # [sos] itself: the empty labelling
    assert abs(J.full_logprob(J.sos_state(logp), True) - ctc_label_logprob_bruteforce(logp, [])) < 1e-9
    for n in range(1, 4):
        for prefix in itertools.product(range(1, V), repeat=n):
            _, st = J.prefix_state(logp, prefix)
            want = ctc_label_logprob_bruteforce(logp, list(prefix))
            got = J.full_logprob(st)
            if want == -math.inf:
                assert got == -math.inf, (prefix, got)
            else:
                assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (prefix, got, want)


def test_blank_candidate_and_too_long_prefix_are_impossible():
    logp = _lattice(4, 4, 9)
    psi, st = J.prefix_state(logp, (2,))
    assert J.extend(logp, st, 2, 0, False)[0] == -math.inf            # the blank is never a label
    assert J.prefix_logprob(logp, (1, 2, 3, 1)) > -math.inf           # four labels fit four frames
    assert J.prefix_logprob(logp, (1, 2, 3, 1, 2)) == -math.inf       # five do not
    assert J.prefix_logprob(logp, (1, 1, 2)) > -math.inf              # a repeat needs a blank between: 4 frames
    assert J.prefix_logprob(logp, (1, 1, 1)) == -math.inf             # 5 frames needed
    assert _brute_prefix(logp, (1, 1, 1)) == -math.inf


def test_search_with_ctc_weight_one_finds_best_labelling():
    """ctc_weight = 1 and a uniform attention model: the one-pass search ranks by CTC alone and, with a beam wide enough for the
    tiny vocabulary, returns the best labelling of brute-force enumeration with its probability."""
    from oracle.decode_ref import best_labelling_bruteforce
    T, V, sos, eos = 5, 5, 2, 3
    logp = _lattice(T, V, 11)
    logp[:, sos] = logp[:, eos] = -30.0                      # sos / eos are CTC classes too; keep them out of the best labelling
    logp = J.log_softmax(logp)
    flat = np.zeros(V)
    hyp = J.one_pass_search(lambda seq: flat, logp, beam=5, pre_beam=5, maxlen=T + 1, ctc_weight=1.0, sos=sos, eos=eos, nbest=3)
    best, score = best_labelling_bruteforce(logp)[0]
    assert hyp[0]["yseq"] == [sos] + list(best) + [eos], (hyp, best)
    assert abs(hyp[0]["score"] - score) < 1e-9 and abs(hyp[0]["ctc_score"] - score) < 1e-9
    assert all(abs(h["score"] - h["ctc_score"]) < 1e-12 for h in hyp)
