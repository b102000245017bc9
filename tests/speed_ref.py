"""Float64 reference of the waveform speed perturbation (sox / Kaldi `speed`; the reference project has nothing of the kind, so this file
IS the definition the kernel is held to).

A factor is a rational s = p/q read from the decimal text of the number (0.9 -> 9/10, 1.1 -> 11/10), 1 <= p, q <= 20.  For an
utterance x of n_in samples
    n_out = ceil(n_in q / p)                      (the number of n with n p / q < n_in)
    y[n]  = sum_k x[k] h(n p / q - k),            x[k] = 0 outside [0, n_in)
    h(t)  = c sinc(c t) 0.5 (1 + cos(pi t c / Z)) for |t| < Z / c, else 0,      Z = 6,  c = 0.99 min(1, q / p)
(a Hann-windowed sinc with torchaudio's default width and roll-off; the cutoff drops for s > 1 so that speeding up does not alias).
p == q is the identity.  perturb() evaluates the sum directly - h at the exact offsets, no table; table() is the polyphase table
H[r][j + W] = h(r/q - j), W = ceil(Z / c), which the tests use for the error bound and the table properties."""
import math
from fractions import Fraction

import numpy as np

Z = 6
ROLLOFF = 0.99


def factor(s):
    fr = Fraction(str(s))
    p, q = fr.numerator, fr.denominator
    if not (1 <= p <= 20 and 1 <= q <= 20):
        raise ValueError(f"speed factor {s!r} = {p}/{q} outside 1 .. 20")
    return p, q


def n_out(n_in, p, q):
    return (n_in * q + p - 1) // p


def cutoff(p, q):
    return ROLLOFF * min(1.0, q / p)


def half_width(p, q):
    return math.ceil(Z / cutoff(p, q))


def h(t, p, q):
    c = cutoff(p, q)
    t = np.asarray(t, dtype=np.float64)
    return np.where(np.abs(t) < Z / c, c * np.sinc(c * t) * 0.5 * (1.0 + np.cos(np.pi * t * c / Z)), 0.0)


def table(p, q):
    W = half_width(p, q)
    return h(np.arange(q)[:, None] / q - np.arange(-W, W + 1)[None, :], p, q)


def perturb(x, p, q):
    """x (n_in,) -> y (n_out,) float64."""
    x = np.asarray(x, dtype=np.float64)
    if p == q:
        return x.copy()
    n_in, W = x.size, half_width(p, q)
    n = np.arange(n_out(n_in, p, q), dtype=np.int64)
    k = (n * p // q)[:, None] + np.arange(-W, W + 1, dtype=np.int64)[None, :]      # every k with |n p/q - k| < Z/c lies in here
    t = ((n * p)[:, None] - k * q) / q                                               # exact numerator, one rounding
    xk = np.where((k >= 0) & (k < n_in), x[np.clip(k, 0, max(n_in - 1, 0))] if n_in else 0.0, 0.0)
    return (xk * h(t, p, q)).sum(axis=1)
