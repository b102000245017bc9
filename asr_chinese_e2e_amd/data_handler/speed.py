"""Host side of the waveform speed perturbation (sox / Kaldi `speed`; the reference has no waveform-side augmentation: parity unpinned by
the reference).  A factor is a rational p/q read from the decimal text of the user's number; an utterance of n samples becomes
ceil(n q / p) samples, y[n] = sum_k x[k] h(n p/q - k), with h a Hann-windowed sinc of width Z = 6 zero crossings and roll-off 0.99
(torchaudio's resampler defaults), the cutoff lowered by q/p when the utterance is sped up.  The kernel (csrc/speed.hip) evaluates the
polyphase form with the tables built here; tests/speed_ref.py restates the definition in float64."""
import math
import random
from fractions import Fraction

import numpy as np

Z = 6                               # zero crossings of the sinc on each side
ROLLOFF = Fraction(99, 100)
PQ_MAX = 20


def parse_factor(s):
    """0.9 -> (9, 10), 1.1 -> (11, 10), "0.95" -> (19, 20): the fraction the decimal TEXT of the number spells, 1 <= p, q <= 20."""
    try:
        fr = Fraction(str(s).strip())
    except (ValueError, ZeroDivisionError) as e:
        raise ValueError(f"speed factor {s!r} is not a number") from e
    p, q = fr.numerator, fr.denominator
    if not (1 <= p <= PQ_MAX and 1 <= q <= PQ_MAX):
        raise ValueError(f"speed factor {s!r} = {p}/{q}: numerator and denominator must lie in 1 .. {PQ_MAX}")
    return p, q


def perturbed_len(n, p, q):
    """Samples of an n-sample utterance at speed p/q: the number of output indices m with m p / q < n.  THE length formula: the
    loader's buckets, the kernel's out_len and the tests all go through it."""
    n, p, q = int(n), int(p), int(q)
    return (n * q + p - 1) // p


def cutoff(p, q):
    return ROLLOFF * min(Fraction(1), Fraction(q, p))


def half_width(p, q):
    """W: the filter h(t) vanishes for |t| >= Z / c, so taps j = -W .. W around the input position cover it."""
    return math.ceil(Z / cutoff(p, q))


def phase_table(p, q):
    """H (q, 2 W + 1) float64: H[r][j + W] = h(r/q - j), h(t) = c sinc(c t) 0.5 (1 + cos(pi t c / Z)) for |t| < Z / c, else 0."""
    c, W = float(cutoff(p, q)), half_width(p, q)
    t = np.arange(q, dtype=np.float64)[:, None] / q - np.arange(-W, W + 1, dtype=np.float64)[None, :]
    h = c * np.sinc(c * t) * 0.5 * (1.0 + np.cos(np.pi * t * c / Z))
    return np.where(np.abs(t) < Z / c, h, 0.0)


def build_tables(factors):
    """factors: sequence of numbers / strings -> (pq (F, 2) int32, taps (F, qmax, ntaps) float32).  Each table is computed in float64 and
    rounded once; narrower filters are centred in the common width, unused rows and the rows of factor 1 (never read) are 0."""
    pq = [parse_factor(s) for s in factors]
    if not pq:
        raise ValueError("no speed factors")
    qmax = max(q for _, q in pq)
    Wmax = max(half_width(p, q) for p, q in pq if p != q) if any(p != q for p, q in pq) else 0
    taps = np.zeros((len(pq), qmax, 2 * Wmax + 1), dtype=np.float32)
    for f, (p, q) in enumerate(pq):
        if p != q:
            W = half_width(p, q)
            taps[f, :q, Wmax - W:Wmax + W + 1] = phase_table(p, q).astype(np.float32)
    return np.asarray(pq, dtype=np.int32).reshape(-1, 2), taps


def draw_factors(seed, epoch, n, n_factors):
    """Factor index of every utterance 0 .. n-1 of the data set: a pure function of (seed, epoch, utterance index) - one generator seeded
    from (seed, epoch), consumed in index order - so every data-parallel rank, and a rerun with the same seed, draws the same factors."""
    rng = random.Random(f"speed_perturb/{int(seed)}/{int(epoch)}")
    return [rng.randrange(n_factors) for _ in range(n)]
