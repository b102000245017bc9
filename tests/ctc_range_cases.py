"""Inputs of the CTC dynamic-range tests (tests/test_ctc_range_cpu.py, tests/test_ctc_range_gpu.py).

Blank-dominated posteriors: seeded `randn` logits (B, T, V) with a constant added to the blank column, on every frame or on the first half
of the frames only - the state of a CTC head early in training (blank ~ 0.99, every label ~ 1e-5).  The all-blank prefix then carries
the maximum of every lattice column and the final states sit (p_label / p_blank)^L below it: past the fp64 range for long labels.
Labels are drawn as tests/test_kernels_gpu.py::ctc_case draws them.  tests/test_ctc_range_cpu.py shows from the oracle alone which
utterances are past the range (`hazard`) and which are inside it.

Also the batches that pin the lattice row widths (Lmax = 31 .. 255) and the tails of the recursion's prefetch (in_len around the chunk
boundaries) on plain random logits."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

# hazard, per utterance: True (final states and frame posteriors past the range), "frames" (the frame posteriors only), False, None (infeasible)
Case = namedtuple("Case", "name logits in_len labels lab_len hazard")


def repeats(labels):
    """Adjacent equal labels: each needs a blank in between, so an alignment needs len(labels) + repeats(labels) frames."""
    return int(sum(int(a) == int(b) for a, b in zip(labels[:-1], labels[1:])))


def round_to(logits, dtype):
    """float32 array -> the values the kernel reads in `dtype`, as float32."""
    return torch.from_numpy(logits).to(dtype).float().numpy()


def _labels(rng, B, V, Lmax, lab_len, repeat):
    labels = rng.randint(1, V, size=(B, Lmax))
    if repeat:
        labels[:, 1::2] = labels[:, 0::2][:, : labels[:, 1::2].shape[1]]
    return np.where(np.arange(Lmax)[None] < np.asarray(lab_len)[:, None], labels, 0)


def boosted(name, seed, T, V, Lmax, boost, lab_len, in_len, hazard, half=False, repeat=False, dtype=torch.float32, exact=(), late=False):
    """`exact`: utterances whose in_len becomes len + repeats of their labels (the only alignments are the tightest ones).
    `late`: the second half of the frames is dominated by the utterance's last label."""
    B = len(lab_len)
    rng = np.random.RandomState(seed)
    logits = rng.randn(B, T, V).astype(np.float32)
    logits[:, : (T // 2 if half else T), 0] += boost
    labels = _labels(rng, B, V, Lmax, lab_len, repeat)
    for b in range(B if late else 0):      # the last label is class V - 1 and occurs nowhere else in the sequence
        if lab_len[b] > 0:
            labels[b, : lab_len[b]] = np.where(labels[b, : lab_len[b]] == V - 1, V - 2, labels[b, : lab_len[b]])
            labels[b, lab_len[b] - 1] = V - 1
            logits[b, T // 2:, V - 1] += boost
    in_len = np.array(in_len)
    for b in exact:
        in_len[b] = lab_len[b] + repeats(labels[b, : lab_len[b]])
    assert in_len.max() <= T
    return Case(name, round_to(logits, dtype), in_len, labels, np.array(lab_len), tuple(hazard))


L_E = 90    # batch E: the label length at which the real vocabulary's posteriors leave the fp64 range (test_ctc_range_cpu.py)


@lru_cache(maxsize=None)
def range_case(name, dtype=torch.float32):
    """The batches of the issue.  Every batch but A carries a short utterance as a control in the same launch."""
    if name == "A":      # long label, short label, empty label, truly infeasible (100 labels in 40 frames)
        return boosted("A", 100, 250, 64, 100, 12.0, [100, 12, 0, 100], [250, 250, 250, 40], [True, False, False, None], dtype=dtype)
    if name == "A50":    # batch A on the generic kernels (V % 8 != 0)
        return boosted("A50", 101, 250, 50, 100, 12.0, [100, 12, 0, 100], [250, 250, 250, 40], [True, False, False, None], dtype=dtype)
    if name == "B":      # labels repeated pairwise, exactly feasible: T = L + repeats = 96
        c = boosted("B", 102, 96, 64, 64, 12.0, [64, 10], [96, 60], [True, False], repeat=True, dtype=dtype, exact=(0,))
        assert c.in_len[0] == 96, c.in_len
        return c
    if name == "C":      # a full row of the widest lattice
        return boosted("C", 103, 600, 64, 255, 12.0, [255, 10], [600, 431], [True, False], dtype=dtype)
    if name == "D":      # non-stationary: blank-dominated on the first half only; inside the range
        return boosted("D", 104, 300, 64, 110, 14.0, [110, 10], [300, 211], [False, False], half=True, dtype=dtype)
    if name == "E":      # the real vocabulary
        return boosted("E", 105, 400, 4232, L_E, 12.0, [L_E, 10], [400, 317], [True, False], dtype=dtype)
    if name == "F":
        # The first half of the frames is dominated by the blank, the second by the last label.  alpha is largest in the all-blank prefix,
        # beta in "stay in the last label", and the final state carries the last alpha column's maximum, so the loss tail is in range; but
        # the states where alpha * beta peaks in the middle frames lie ~L/2 improbable labels below BOTH column maxima: only the frame
        # posteriors leave the range.  No single tilt per utterance brings both ends back.
        return boosted("F", 106, 250, 64, 100, 12.0, [100, 10], [250, 250], ["frames", False], half=True, late=True, dtype=dtype)
    raise KeyError(name)


RANGE_NAMES = ("A", "A50", "B", "C", "D", "E", "F")
WIDTH_LMAX = (31, 32, 63, 64, 127, 128, 255)
TAIL_LMAX = (31, 63, 127, 255)                                        # one batch per row width 32, 64, 128, 256
TAIL_IN_LEN = (1, 2, 8, 9, 10, 24, 25, 26, 56, 57, 58, 64, 65, 130)    # around nsteps % 8 and the 2 NB - 1 chunk boundary, NB = 4 and 2


def _random(name, seed, T, V, Lmax, lab_len, in_len, labels, dtype):
    rng = np.random.RandomState(seed)
    logits = (rng.randn(len(lab_len), T, V) * 2).astype(np.float32)
    return Case(name, round_to(logits, dtype), np.array(in_len), labels, np.array(lab_len), (False,) * len(lab_len))


@lru_cache(maxsize=None)
def width_case(Lmax, V, dtype):
    """L = Lmax, L = Lmax - 1, L = 1, pairwise repeated labels in exactly L + repeats frames, and the same utterance with one frame more."""
    rng = np.random.RandomState(1000 + Lmax)
    lab_len = [Lmax, Lmax - 1, 1, Lmax, Lmax]
    labels = _labels(rng, 5, V, Lmax, lab_len, False)
    labels[3, 1::2] = labels[3, 0::2][: labels[3, 1::2].shape[0]]
    labels[4] = labels[3]
    need = Lmax + repeats(labels[3])
    T = max(need + 1, Lmax + repeats(labels[0]) + 3)
    in_len = [T, T - 1, T - 2, need, need + 1]
    assert all(in_len[b] >= lab_len[b] + repeats(labels[b, : lab_len[b]]) for b in range(5))
    return _random(f"width{Lmax}", 2000 + Lmax, T, V, Lmax, lab_len, in_len, labels, dtype)


@lru_cache(maxsize=None)
def tail_case(Lmax, V, dtype):
    rng = np.random.RandomState(3000 + Lmax)
    lab_len = [min(Lmax, t // 2) for t in TAIL_IN_LEN]
    labels = _labels(rng, len(TAIL_IN_LEN), V, Lmax, lab_len, False)
    assert all(t >= l + repeats(labels[b, :l]) for b, (t, l) in enumerate(zip(TAIL_IN_LEN, lab_len)))
    return _random(f"tail{Lmax}", 4000 + Lmax, max(TAIL_IN_LEN), V, Lmax, lab_len, TAIL_IN_LEN, labels, dtype)


def margins(logits, labels, blank=0):
    """From the log-domain oracle alone: how far below the column maxima a scaled linear lattice must reach for one utterance.
    Returns (nll, tail, frame): tail = log of (final states / maximum of the last alpha column); frame = the smallest over the frames
    of log of (largest alpha beta / y of the frame / (column maximum of alpha * column maximum of beta))."""
    from oracle import ctc_ref
    nll, _, la, lb = ctc_ref.ctc_one(np.asarray(logits, dtype=np.float64), np.asarray(labels), blank)
    if not np.isfinite(nll):
        return nll, -np.inf, -np.inf
    lp = ctc_ref.log_softmax(np.asarray(logits, dtype=np.float64))
    ext = np.full(2 * len(labels) + 1, blank, dtype=np.int64)
    ext[1::2] = labels
    tail = (np.logaddexp(la[-1, -1], la[-1, -2]) if len(labels) else la[-1, -1]) - la[-1].max()
    with np.errstate(invalid="ignore"):
        post = np.where(np.isneginf(la) | np.isneginf(lb), -np.inf, la + lb - lp[:, ext])
    frame = (post.max(1) - (la.max(1) + lb.max(1))).min()
    return float(nll), float(tail), float(frame)
