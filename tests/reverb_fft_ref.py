"""Reference side of the FFT reverberation path (csrc/reverb_fft.hip).  The definition stays tests/noise_ref.py's reverb(); this file
adds what an FFT evaluation of it needs to be judged:

(i)  block_scale: the float64 scale of the rounding error.  The path is a uniformly partitioned overlap-save convolution with
     N = 4096 points and Bk = N / 2 new samples per block: window j of the utterance is w_j = x[(j - 1) Bk, (j + 1) Bk) (zero outside
     [0, len)), partition q of the response is h_q = h[q Bk, (q + 1) Bk), and output block i, full[i Bk, (i + 1) Bk) with
     out[m - p] = full[m], is the last Bk samples of IFFT(sum_{q < P, q <= i} FFT(h_q) FFT(w_{i - q})).  A transform of n points in
     floating point with unit roundoff u returns its input's spectrum with an error of O(u log n) ||input||_2 in the 2-norm, spread
     over all bins; a product of two spectra therefore carries O(u log n) ||h_q||_2 ||w_{i - q}||_2 sqrt(n) in the 2-norm, and the
     inverse (1 / n, unitary up to sqrt(n)) brings each SAMPLE of the block an error of the order u log n ||h_q||_2 ||w_{i - q}||_2 -
     whatever that sample's own magnitude is.  So the error of a sample of block i scales with
         S_i = sum_{q < P, q <= i} ||h_q||_2 ||w_{i - q}||_2,
     not with the direct sum's A[n] = sum_k |h[k]| |x[n + p - k]|, which bounds a direct evaluation sample by sample.

(ii) reverb_fft_f32: the same partitioned overlap-save in float32 on the CPU through torch.fft on complex64 - another radix, another
     accumulation order, other twiddles.  Its largest error over a set of cases in units of 2^-24 S_i, c_ref (worst_ratio), is the
     yardstick: the kernel is gated at 4 c_ref on the same cases.  The factor 4 covers the differences just named; a wrong block,
     partition, twiddle or shift is off by orders of magnitude."""
import numpy as np
import torch

N = 4096
BK = N // 2
U = 2.0 ** -24
GATE_FACTOR = 4.0


def _windows(x, nwin):
    """(nwin, N): window j = x[(j - 1) BK, (j + 1) BK), zero outside the signal; same dtype as x."""
    buf = np.zeros((nwin + 1) * BK, dtype=x.dtype)
    buf[BK:BK + x.size] = x[:nwin * BK]
    return np.stack([buf[j * BK:j * BK + N] for j in range(nwin)])


def _partitions(h):
    """(P, BK): partition q = h[q BK, (q + 1) BK), the last one zero-padded; same dtype as h."""
    P = -(-h.size // BK)
    buf = np.zeros(P * BK, dtype=h.dtype)
    buf[:h.size] = h
    return buf.reshape(P, BK)


def _blocks(n, L, p):
    """Output blocks first .. last that hold full[p, p + n), and the number of signal windows that are not all zero."""
    return p // BK, (p + n - 1) // BK, -(-n // BK) + 1


def block_scale(x, h, p):
    """-> S (n,) float64: S_i of the block each output sample out[m - p] = full[m] lies in (i = m // BK)."""
    x, h = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(h, dtype=np.float64).reshape(-1)
    n, L = x.size, h.size
    assert L >= 1 and 0 <= p < L
    if n == 0:
        return np.zeros(0)
    first, last, nwin = _blocks(n, L, p)
    wn = np.sqrt(np.sum(_windows(x, nwin) ** 2, axis=1))
    hn = np.sqrt(np.sum(_partitions(h) ** 2, axis=1))
    S = np.zeros(last + 1)
    for i in range(first, last + 1):
        S[i] = sum(hn[q] * wn[i - q] for q in range(min(hn.size - 1, i) + 1) if i - q < nwin)
    return S[(np.arange(n) + p) // BK]


def reverb_fft_f32(x, h, p):
    """-> y (n,) float32: the partitioned overlap-save evaluation in float32 (torch.fft on complex64, products summed over q ascending)."""
    x, h = np.asarray(x, dtype=np.float32).reshape(-1), np.asarray(h, dtype=np.float32).reshape(-1)
    n, L = x.size, h.size
    assert L >= 1 and 0 <= p < L
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    first, last, nwin = _blocks(n, L, p)
    X = torch.fft.fft(torch.from_numpy(_windows(x, nwin)).to(torch.complex64), dim=1)
    hp = _partitions(h)
    H = torch.fft.fft(torch.from_numpy(np.concatenate([hp, np.zeros_like(hp)], axis=1)).to(torch.complex64), dim=1)
    assert X.dtype == torch.complex64 and H.dtype == torch.complex64
    full = np.zeros((last + 1) * BK, dtype=np.float32)
    for i in range(first, last + 1):
        acc = torch.zeros(N, dtype=torch.complex64)
        for q in range(min(H.shape[0] - 1, i) + 1):
            if i - q < nwin:
                acc = acc + H[q] * X[i - q]
        full[i * BK:(i + 1) * BK] = torch.fft.ifft(acc).real[BK:].numpy()
    return full[p:p + n]


def worst_ratio(got, ref, S):
    """max |got - ref| / (2^-24 S) over the samples (0 for an empty row); S = 0 (silence) demands an exact zero."""
    if ref.size == 0:
        return 0.0
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(S > 0, err / (U * S), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())
