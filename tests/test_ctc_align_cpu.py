"""CTC forced alignment without a GPU: the fp64 Viterbi restatement the device kernel (asr_ctc_align) is tested against, pinned by
brute-force enumeration of every alignment on tiny cases, and the host-side argument validation of the entry point."""
import itertools
import math

import numpy as np
import pytest

NEG = -math.inf


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def viterbi_ref(logp, labels, blank=0):
    """Best CTC path of `labels` through frames logp (Tb, V) (log-softmax, fp64): the max-product form of ctc_loss.
    Ties: predecessor s before s-1 before s-2; at the end 2L before 2L-1.
    Returns (score, states (Tb,) of the blank-augmented sequence, or None when infeasible)."""
    Tb, L = logp.shape[0], len(labels)
    S = 2 * L + 1
    if Tb == 0:
        return (0.0, []) if L == 0 else (NEG, None)
    ext = [blank if s % 2 == 0 else labels[s // 2] for s in range(S)]
    delta = [NEG] * S
    delta[0] = logp[0, blank]
    if L > 0:
        delta[1] = logp[0, labels[0]]
    bp = np.zeros((Tb, S), dtype=np.int64)
    for t in range(1, Tb):
        new = [NEG] * S
        for s in range(S):
            best, arg = delta[s], s
            if s >= 1 and delta[s - 1] > best:
                best, arg = delta[s - 1], s - 1
            if s >= 2 and s % 2 == 1 and ext[s] != ext[s - 2] and delta[s - 2] > best:
                best, arg = delta[s - 2], s - 2
            new[s] = best + logp[t, ext[s]] if best > NEG else NEG
            bp[t, s] = arg
        delta = new
    end = 2 * L
    if L > 0 and delta[2 * L - 1] > delta[2 * L]:
        end = 2 * L - 1
    if delta[end] == NEG:
        return NEG, None
    states = [end]
    for t in range(Tb - 1, 0, -1):
        states.append(int(bp[t, states[-1]]))
    return float(delta[end]), states[::-1]


def align_outputs(logp, labels, T, blank=0, Lmax=None):
    """The outputs asr_ctc_align defines, from viterbi_ref: (path (T,), spans (Lmax, 2), token_logp (Lmax,), score)."""
    Tb, L = logp.shape[0], len(labels)
    Lmax = L if Lmax is None else Lmax
    score, states = viterbi_ref(logp, labels, blank)
    path = np.full(T, -1, dtype=np.int64)
    spans = np.full((Lmax, 2), -1, dtype=np.int64)
    tlp = np.zeros(Lmax)
    if states is None:
        path[:Tb] = blank
        tlp[:L] = NEG
        return path, spans, tlp, score
    for t, s in enumerate(states):
        if s % 2:
            i = s // 2
            path[t] = labels[i]
            if spans[i, 0] < 0:
                spans[i, 0] = t
            spans[i, 1] = t
            tlp[i] += logp[t, labels[i]]
        else:
            path[t] = blank
    return path, spans, tlp, score


def rescore(logp, path, blank=0):
    """fp64 log-probability of a frame-wise path (token ids per frame)."""
    return float(sum(logp[t, c] for t, c in enumerate(path) if c >= 0))


def collapse(seq, blank=0):
    out, prev = [], None
    for c in seq:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def _brute(logp, labels, blank=0):
    """Every state sequence the CTC topology allows (start in 0 / 1, end in 2L / 2L-1, steps of 0, 1 or an allowed 2)."""
    Tb, L = logp.shape[0], len(labels)
    S = 2 * L + 1
    ext = [blank if s % 2 == 0 else labels[s // 2] for s in range(S)]
    best, paths = NEG, []
    for seq in itertools.product(range(S), repeat=Tb):
        if seq[0] > 1 or seq[-1] < 2 * L - 1:
            continue
        ok = True
        for a, b in zip(seq, seq[1:]):
            d = b - a
            if d < 0 or d > 2 or (d == 2 and (b % 2 == 0 or ext[b] == ext[a])):
                ok = False
                break
        if not ok:
            continue
        assert collapse([ext[s] for s in seq], blank) == list(labels)
        sc = float(sum(logp[t, ext[s]] for t, s in enumerate(seq)))
        if sc > best + 1e-12:
            best, paths = sc, [list(seq)]
        elif abs(sc - best) <= 1e-12:
            paths.append(list(seq))
    return best, paths


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("labels", [[1], [1, 2], [2, 2], [1, 1, 1], [3, 1, 3], [1, 2, 1]])
@pytest.mark.parametrize("T", [1, 3, 5, 7])
def test_viterbi_ref_matches_brute_force(seed, labels, T):
    rng = np.random.default_rng(seed * 131 + T)
    logp = log_softmax(rng.normal(0, 2.0, (T, 4)))
    score, states = viterbi_ref(logp, labels)
    best, paths = _brute(logp, labels)
    if not paths:
        assert states is None and score == NEG
        reps = sum(a == b for a, b in zip(labels, labels[1:]))
        assert T < len(labels) + reps            # infeasible exactly when the frames are too few
        return
    assert abs(score - best) < 1e-12
    assert states in paths
    path, spans, tlp, sc2 = align_outputs(logp, labels, T)
    assert collapse(path.tolist()) == labels
    assert abs(rescore(logp, path) - best) < 1e-12
    blank_lp = sum(logp[t, 0] for t in range(T) if path[t] == 0)
    assert abs(tlp.sum() + blank_lp - best) < 1e-12
    assert all(spans[i, 0] <= spans[i, 1] < spans[i + 1, 0] for i in range(len(labels) - 1))


def test_viterbi_ref_edge_cases():
    logp = log_softmax(np.random.default_rng(3).normal(0, 1, (4, 3)))
    # L = 0: every frame blank
    score, states = viterbi_ref(logp, [])
    assert states == [0] * 4 and abs(score - logp[:, 0].sum()) < 1e-12
    # in_len = 0
    assert viterbi_ref(logp[:0], []) == (0.0, [])
    assert viterbi_ref(logp[:0], [1]) == (NEG, None)
    path, spans, tlp, score = align_outputs(logp[:0], [], 5)
    assert (path == -1).all() and score == 0.0
    # infeasible: 'aa' needs 3 frames
    path, spans, tlp, score = align_outputs(logp[:2], [1, 1], 4, Lmax=3)
    assert score == NEG and path.tolist() == [0, 0, -1, -1] and (spans == -1).all() and tlp.tolist() == [NEG, NEG, 0.0]
    # exactly enough frames: the only path
    score, states = viterbi_ref(logp[:3], [1, 1])
    assert states == [1, 2, 3]


def test_viterbi_ref_tie_rules():
    # uniform posteriors: every alignment ties.  Preferring the state itself over s-1 over s-2 walks back through the final
    # blank as long as it was reachable, so the labels come as EARLY as possible, each on one frame, blank-separated only when repeated
    T = 7
    logp = log_softmax(np.zeros((T, 4)))
    _, states = viterbi_ref(logp, [1, 2, 3])
    assert states == [1, 3, 5, 6, 6, 6, 6]
    _, states = viterbi_ref(logp, [1, 1])
    assert states == [1, 2, 3, 4, 4, 4, 4]
    # end tie: 2L before 2L-1
    _, states = viterbi_ref(logp[:2], [2])
    assert states[-1] == 2
    # stay before s-1: frame 1 is blank or the label with equal probability, so the final blank at frame 2 has two equal
    # predecessors (itself at frame 1, or the label at frame 1); the rule keeps the blank
    x = np.full((3, 3), -5.0)
    x[0, 1] = 0.0
    x[1, 0] = x[1, 1] = 0.0
    x[2, 0] = 0.0
    _, states = viterbi_ref(log_softmax(x), [1])
    assert states == [1, 2, 2]
    # s-1 before s-2: label 2 at frame 2 reached from the blank after label 1 or directly from label 1, equally likely
    x = np.full((3, 4), -5.0)
    x[0, 1] = 0.0
    x[1, 0] = x[1, 1] = 0.0
    x[2, 2] = 0.0
    _, states = viterbi_ref(log_softmax(x), [1, 2])
    assert states == [1, 2, 3]


def _args(**over):
    a = dict(logits=16, in_len=16, labels=16, lab_len=16, path=16, spans=16, token_logp=16, score=16, B=2, T=10, V=8, ld=8, Lmax=3,
             blank=0, ws=16, ws_bytes=1 << 30, dtype=0, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("fast", [False, True])
def test_ctc_align_host_validation(fast):
    """Arguments are checked on the host before any launch (callable without a GPU), through ctypes and the fastcall trampolines."""
    from asr_chinese_e2e_amd import _lib
    f = _lib.fast if fast else _lib.lib
    for name in ("logits", "labels", "path", "spans", "token_logp", "score", "ws"):
        assert f.asr_ctc_align(*_args(**{name: None})) == -1
        assert "asr_ctc_align: null pointer" in _lib.last_error()
    assert f.asr_ctc_align(*_args(Lmax=256)) == -1
    assert "Lmax = 256" in _lib.last_error()
    need = _lib.lib.asr_ctc_align_workspace_bytes(2, 10, 3)
    assert f.asr_ctc_align(*_args(ws_bytes=need - 1)) == -1
    assert "workspace" in _lib.last_error()
    assert f.asr_ctc_align(*_args(ld=7)) == -1
    assert "row stride" in _lib.last_error()
    assert f.asr_ctc_align(*_args(dtype=7)) == -2


def test_ctc_align_workspace_bytes():
    from asr_chinese_e2e_amd import _lib
    for args in [(32, 500, 22), (1, 1, 1), (4, 2000, 255), (3, 7, 64)]:
        assert _lib.fast.asr_ctc_align_workspace_bytes(*args) == _lib.lib.asr_ctc_align_workspace_bytes(*args)
    W = 32    # Lmax = 22: 32 (blank, label) pairs per frame
    n = 32 * 500
    assert _lib.lib.asr_ctc_align_workspace_bytes(32, 500, 22) == n * 2 * W * 8 + n * W + n * 4
