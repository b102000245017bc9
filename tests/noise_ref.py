"""Float64 reference of the noise and reverberation augmentation (Kaldi reverberate_data_dir / WeNet add_reverb, add_noise; the reference
project has nothing of the kind, so this file IS the definition the kernels of csrc/augment.hip are held to).

Reverberation: a response h of L taps whose peak (the direct path) sits at tap p turns x of n samples into
    y[m] = sum_{k < L} h[k] x[m + p - k],   m < n,   x = 0 outside [0, n)
- the length stays and the direct path stays where it was (Kaldi --shift-output).  Beside y the functions return
    A[m] = sum_k |h[k]| |x[m + p - k]|,
the scale of the rounding error of ANY fp32 evaluation of the sum: every product and every partial sum is at most A[m] in magnitude
and each of the L products and L - 1 additions rounds once (a fused multiply-add rounds less), so whatever the order
    |y_fp32[m] - y[m]| <= (L + 1) 2^-24 A[m]      (first order; the tests' bound).

Noise: the clip c of nlen samples, read from offset o and wrapped, v[m] = c[(o + m) mod nlen], is added with the gain
    g = scale sqrt(sum x^2 / sum v^2),   scale = 10^(-snr_dB / 20),
so that 10 log10(sum x^2 / sum (g v)^2) = snr_dB; a silent utterance or a silent stretch of noise leaves x as it is (g = 0).

A bank entry is made from a recorded response by rir_prepare: the samples [s0, s0 + max_taps), s0 = max(0, argmax |h| - 64), scaled to
unit energy after the truncation (WeNet's add_reverb normalises the same way)."""
import numpy as np


def reverb(x, h, p):
    """-> (y, A), float64, len(x) samples each."""
    x, h = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(h, dtype=np.float64).reshape(-1)
    n, L = x.size, h.size
    assert L >= 1 and 0 <= p < L
    if n == 0:
        return np.zeros(0), np.zeros(0)
    # full[m] = sum_k h[k] x[m - k], m < n + L - 1;  y[m] = full[m + p]
    return np.convolve(x, h)[p:p + n], np.convolve(np.abs(x), np.abs(h))[p:p + n]


def noise_segment(clip, o, n):
    clip = np.asarray(clip, dtype=np.float64).reshape(-1)
    return clip[(int(o) + np.arange(n, dtype=np.int64)) % clip.size]


def mix(x, clip, o, scale):
    """-> (out, gain, v), float64.  scale: 10^(-snr_dB / 20) (pass the float32 the kernel is given to compare gains)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size == 0 or np.asarray(clip).size == 0:
        return x.copy(), 0.0, np.zeros(x.size)
    v = noise_segment(clip, o, x.size)
    ex, ev = float(np.sum(x * x)), float(np.sum(v * v))
    if ex == 0.0 or ev == 0.0:
        return x.copy(), 0.0, v
    g = float(scale) * np.sqrt(ex / ev)
    return x + g * v, g, v


def snr_db(x, noise):
    return 10.0 * np.log10(np.sum(np.square(x, dtype=np.float64)) / np.sum(np.square(noise, dtype=np.float64)))


def rir_prepare(h, max_taps=8192, pre=64):
    """-> (taps float64 before the one rounding to float32, peak index inside them)."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    peak = int(np.argmax(np.abs(h)))
    s0 = max(0, peak - pre)
    h = h[s0:s0 + max_taps]
    return h / np.sqrt(np.sum(h * h)), peak - s0
