"""Float64 reference of the sample-rate conversion to 16 kHz (the reference project has no resampler, so this file IS the definition the
kernel is held to: parity unpinned by the reference).

For a source rate fs, p/q = fs/16000 in lowest terms.  For an utterance x of n_in samples
    n_out = ceil(n_in q / p)
    y[n]  = sum_k x[k] h(n p / q - k),            x[k] = 0 outside [0, n_in)
    h(t)  = c sinc(c t) w(t c / Z),               c = ROLLOFF min(1, q / p)
    w(u)  = I0(BETA sqrt(1 - u^2)) / I0(BETA) for |u| < 1, else 0
    Z = 64, ROLLOFF = 0.9475937167399596, BETA = 14.769656459379492
(a Kaiser-windowed sinc with the constants of the common "kaiser_best" resamplers).  p == q is the identity.  resample() evaluates the sum
directly - h at the exact offsets, no table; table() is the polyphase table H[r][j + W] = h(r/q - j), W = ceil(Z / c), which the tests use
for the error bound and the table properties.  Rates whose q passes 640 or whose 2 W + 1 passes 1023 are refused."""
import math

import numpy as np
from scipy.special import i0

TARGET = 16000
Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492


def plan(fs):
    """-> (p, q, W)."""
    g = math.gcd(int(fs), TARGET)
    p, q = int(fs) // g, TARGET // g
    W = 0 if p == q else math.ceil(Z / cutoff(p, q))
    if int(fs) != fs or fs < 1 or q > 640 or 2 * W + 1 > 1023:
        raise ValueError(f"sample rate {fs} = {p}/{q} x 16000 is not supported")
    return p, q, W


def n_out(n_in, p, q):
    return (n_in * q + p - 1) // p


def cutoff(p, q):
    return ROLLOFF * min(1.0, q / p)


def h(t, p, q):
    c = cutoff(p, q)
    t = np.asarray(t, dtype=np.float64)
    u = t * c / Z
    inside = np.abs(u) < 1.0
    w = i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / i0(BETA)
    return np.where(inside, c * np.sinc(c * t) * w, 0.0)


def table(fs):
    p, q, W = plan(fs)
    return h(np.arange(q)[:, None] / q - np.arange(-W, W + 1)[None, :], p, q)


def resample(x, fs):
    """x (n_in,) at fs -> y (n_out,) float64 at 16 kHz."""
    x = np.asarray(x, dtype=np.float64)
    p, q, W = plan(fs)
    if p == q:
        return x.copy()
    n_in = x.size
    y = np.empty(n_out(n_in, p, q), dtype=np.float64)
    j = np.arange(-W, W + 1, dtype=np.int64)[None, :]
    for s in range(0, y.size, 4096):                                                    # in pieces: (n_out, ntaps) float64 at once is large
        n = np.arange(s, min(s + 4096, y.size), dtype=np.int64)
        k = (n * p // q)[:, None] + j                                                    # every k with |n p/q - k| < Z/c lies in here
        t = ((n * p)[:, None] - k * q) / q                                               # exact numerator, one rounding
        xk = np.where((k >= 0) & (k < n_in), x[np.clip(k, 0, max(n_in - 1, 0))] if n_in else 0.0, 0.0)
        y[n] = (xk * h(t, p, q)).sum(axis=1)
    return y
