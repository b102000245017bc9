"""The beam-merge restatement (tests/beam_ref.py) that asr_beam_step is tested against, pinned on hand-worked cases: the tie rule,
eos retirement, the forced end at maxlen - 1, an exhausted maxlen and dead slots; and against the reference's own form of the merge
(sorted(...)[:beam] after every hypothesis, oracle/ref_model.beam_search) on random candidates with many ties.  No GPU."""
import numpy as np
import pytest

from tests import beam_ref as BR

EOS = 9
NEG = -np.inf


def f32(x):
    return np.float32(x)


def run(vals, ids, score, alive, maxlen, step, last_tok=None):
    vals = np.asarray(vals, dtype=np.float32)
    B, beam = vals.shape[0], vals.shape[1]
    last_tok = np.full((B, beam), 77, np.int32) if last_tok is None else last_tok
    return BR.beam_step(vals, np.asarray(ids, np.int32), np.asarray(score, np.float32), np.asarray(alive, np.int32), last_tok,
                        np.asarray(maxlen, np.int32), step, EOS)


def test_equal_scores_keep_first_come_order():
    # sums: (h0, j0) = -2, (h0, j1) = -4, (h1, j0) = -2, (h1, j1) = -2.5: the two -2 survive with h0's first
    o = run([[[-1, -3], [0, -0.5]]], [[[3, 4], [5, 6]]], [[-1, -2]], [[1, 1]], [10], 2)
    assert o["parent"].tolist() == [[0, 1]] and o["last_tok"].tolist() == [[3, 5]]
    assert o["rec_score"].tolist() == [[-2.0, -2.0]] and o["rec_end"].tolist() == [[0, 0]]
    assert o["alive"].tolist() == [[1, 1]] and o["n_alive"] == 2
    # a tie within one hypothesis: the smaller candidate index j first
    o = run([[[-1, -1], [-5, -5]]], [[[4, 3], [1, 2]]], [[0, 0]], [[1, 1]], [10], 2)
    assert o["last_tok"].tolist() == [[4, 3]] and o["parent"].tolist() == [[0, 0]]


def test_eos_retires_the_hypothesis_and_dead_slots_do_not_compete():
    vals = [[[-0.5, -1, -4], [-0.1, -3, -5], [0, 0, 0]]]
    ids = [[[EOS, 2, 3], [4, EOS, 1], [1, 1, 1]]]
    o = run(vals, ids, [[0, -1, 7]], [[1, 1, 0]], [5], 1)      # slot 2 is dead: its high score is never a candidate
    assert o["rec_tok"].tolist() == [[EOS, 2, 4]] and o["rec_par"].tolist() == [[0, 0, 1]]
    assert o["rec_end"].tolist() == [[1, 0, 0]] and o["alive"].tolist() == [[0, 1, 1]] and o["n_alive"] == 2
    assert o["rec_score"][0].tolist() == [f32(-0.5), f32(-1), f32(-1) + f32(-0.1)]
    assert o["score"][0].tolist() == o["rec_score"][0].tolist()


def test_last_step_appends_eos_to_every_survivor():
    o = run([[[-1, -2], [-1.5, -3]]], [[[EOS, 5], [6, 7]]], [[0, 0]], [[1, 1]], [4], 3)
    assert o["rec_tok"].tolist() == [[EOS, 6]] and o["rec_par"].tolist() == [[0, 1]]
    assert o["rec_end"].tolist() == [[2, 2]]                    # end = 2 also after an eos of its own
    assert o["alive"].tolist() == [[0, 0]] and o["n_alive"] == 0


def test_exhausted_maxlen_has_no_candidates():
    last_tok = np.array([[11, 12], [13, 14]], np.int32)
    o = run([[[-1, -2], [-3, -4]], [[-1, -2], [-3, -4]]], [[[1, 2], [3, 4]], [[5, 6], [7, 8]]], [[-0.25, -0.5], [0, 0]], [[1, 1], [1, 0]],
            [3, 10], 3, last_tok)
    # utterance 0: step 3 >= maxlen 3 - every slot dead, score and last token left as they were
    assert o["alive"][0].tolist() == [0, 0] and o["parent"][0].tolist() == [0, 1]
    assert o["rec_tok"][0].tolist() == [0, 0] and o["rec_par"][0].tolist() == [0, 0] and o["rec_end"][0].tolist() == [0, 0]
    assert o["rec_score"][0].tolist() == [NEG, NEG]
    assert o["score"][0].tolist() == [-0.25, -0.5] and o["last_tok"][0].tolist() == [11, 12]
    # utterance 1: only slot 0 alive, its two candidates fill the beam
    assert o["rec_tok"][1].tolist() == [5, 6] and o["parent"][1].tolist() == [0, 0] and o["n_alive"] == 2


def test_minus_inf_candidates_fill_the_beam_in_order():
    o = run([[[-0.2, NEG, NEG], [0, 0, 0], [0, 0, 0]]], [[[1, 2, 3], [4, 4, 4], [5, 5, 5]]], [[0, 0, 0]], [[1, 0, 0]], [6], 0)
    assert o["rec_tok"].tolist() == [[1, 2, 3]] and o["rec_score"][0].tolist() == [f32(-0.2), NEG, NEG]
    assert o["alive"].tolist() == [[1, 1, 1]] and o["n_alive"] == 3


def _reference_merge(vals, ids, score, alive, beam):
    """oracle/ref_model.beam_search's merge for one utterance: keep the best `beam` after every hypothesis."""
    kept = []
    for h in range(beam):
        if not alive[h]:
            continue
        for j in range(beam):
            kept.append((float(np.float32(score[h]) + np.float32(vals[h][j])), h, int(ids[h][j])))
        kept = sorted(kept, key=lambda c: c[0], reverse=True)[:beam]
    return kept


@pytest.mark.parametrize("beam", [1, 2, 5, 8])
def test_one_stable_sort_equals_the_reference_incremental_merge(beam):
    rng = np.random.default_rng(beam)
    for trial in range(200):
        vals = -rng.integers(0, 4, size=(1, beam, beam)).astype(np.float32)          # few distinct values: many exact ties
        score = -rng.integers(0, 3, size=(1, beam)).astype(np.float32)
        ids = rng.integers(0, 12, size=(1, beam, beam)).astype(np.int32)
        alive = (rng.random((1, beam)) < 0.7).astype(np.int32)
        alive[0, trial % beam] = 1
        o = run(vals, ids, score, alive, [100], 5)
        want = _reference_merge(vals[0], ids[0], score[0], alive[0], beam)
        n = len(want)
        assert o["rec_score"][0, :n].tolist() == [c[0] for c in want]
        assert o["rec_par"][0, :n].tolist() == [c[1] for c in want]
        assert o["rec_tok"][0, :n].tolist() == [c[2] for c in want]
        assert (o["rec_score"][0, n:] == NEG).all()
