"""The Kaldi fbank front end's reference side, numpy only (no GPU): the definition in float64, an a-priori fp32 error bound, and a
float32 restatement of the kernel's arithmetic (csrc/fbank.hip) that shows the bound holds for fp32 as such.

Definition (Kaldi's documented fbank - compute-fbank-feats, torchaudio.compliance.kaldi.fbank, kaldi-native-fbank - with the settings
WeNet uses and dither = 0).  Samples in [-1, 1] are multiplied by WAV_SCALE = 32768.  snip_edges = true: T = 0 for len < 400, else
1 + (len - 400) // 160; frame t is samples 160 t .. 160 t + 399; trailing samples that fill no frame are dropped.  Per frame: subtract
the frame's mean; y[n] = x[n] - 0.97 x[n - 1] for n >= 1, y[0] = x[0] - 0.97 x[0]; Povey window (0.5 - 0.5 cos(2 pi n / 399))^0.85;
zero-pad to 512; |X_k|^2 for k = 0 .. 255 (no Nyquist bin).  Mel banks: mel(f) = 1127 ln(1 + f / 700), n_mels + 2 points equally
spaced in mel from mel(20) to mel(8000); bin k with m = mel(k 16000 / 512) has weight (m - left) / (centre - left) for
left < m <= centre, (right - m) / (right - centre) for centre < m < right, else 0.  Output log(max(energy, FLT_EPSILON)), no energy
column.

Bound (from fp32 arithmetic, not from the kernel; u = 2^-24).  Amplitude error of the prepared frame, tap by tap, with s = the scaled
samples, A = mean |s| of the frame, d = s - mean, y, xw = y w the exact values:
  mean:    every tap passes through at most 12 additions (6 in its lane, 6 butterfly levels) -> 12 u sum |s| / 400, one rounding of
           the scale product (u A) and one of the division (u |mean| <= u A), second-order terms rounded up: EM = 15 u A;
  d:       u |s| (scale product) + EM + u |d|                                                 = ed[n];
  y:       ed[n] + 0.97 ed[n - 1] + 2 u 0.97 |d[n - 1]| (0.97 as fp32; the product's rounding) + u |y[n]|      = ey[n];
  xw:      w[n] ey[n] + 2 u |xw[n]| (the window as fp32; the product's rounding).
Their sum over the 400 taps is E_prep.  The DFT adds DELTA sum |xw| with DELTA = 6e-5: 200 steps of the twiddle recurrence at a few
ulp each (about 3.6e-5) and 400 fp32 accumulations (2.4e-5), the figures of tests/logmel_emul.py - the recurrence is the same.  With
E_t = E_prep + DELTA sum |xw| the power error of bin k is at most 2 |X_k| E_t + E_t^2, the mel error that summed over the filterbank.
Relative terms of a cell of filter j with nnz_j non-zero weights: (2 nnz_j + 4) u (re^2 + im^2 in two roundings, the weight as fp32, at
most two roundings per non-zero product inside the matrix pipe; adding an exact zero costs nothing), and logf: the hardware's log2 to 1
ulp times ln 2 plus one rounding is at most LOG_ULPS = 2.5 ulp of a float32 of the size of the result (at least of size 1), which after
exp is a relative error of expm1(that).  max(., FLT_EPSILON) is 1-Lipschitz, so the floor adds nothing.

Floor cells: a frame whose samples are all zero, or a filter without a non-zero weight.  Nothing but FLT_EPSILON is under the log there
whatever the rounding, and the answer logf(FLT_EPSILON) is compared exactly (tests/test_logmel_gpu.is_floor's way).  A constant frame is
NOT a floor cell: whether the mean's rounding leaves exact zeros depends on the values; it is held to the bound (EM carries it)."""
import numpy as np

from tests import logmel_emul

SR, FLEN, HOP, NFFT, NBIN = 16000, 400, 160, 512, 256
WAV_SCALE, PREEMPH, LOW_FREQ, HIGH_FREQ = 32768.0, 0.97, 20.0, 8000.0
FLT_EPSILON = 2.0 ** -23
LOG_FLOOR32 = np.log(np.float32(FLT_EPSILON))      # the float32 nearest to log(FLT_EPSILON) = -15.942385
U = 2.0 ** -24
DELTA, MEAN_ULPS, LOG_ULPS = 6e-5, 15.0, 2.5

signals, N_SIG = logmel_emul.signals, logmel_emul.N_SIG


def num_frames(length):
    length = int(length)
    return 0 if length < FLEN else 1 + (length - FLEN) // HOP


def povey_window():
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FLEN) / (FLEN - 1))) ** 0.85


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


_fb = {}


def mel_filterbank(n_mels):
    """(256, n_mels) float64."""
    if n_mels not in _fb:
        lo, hi = float(mel(LOW_FREQ)), float(mel(HIGH_FREQ))
        delta = (hi - lo) / (n_mels + 1)
        m = mel(np.arange(NBIN) * SR / NFFT)[:, None]
        left = lo + np.arange(n_mels)[None, :] * delta
        centre, right = left + delta, left + 2.0 * delta
        up, down = (m - left) / (centre - left), (right - m) / (right - centre)
        _fb[n_mels] = np.where((m > left) & (m <= centre), up, np.where((m > centre) & (m < right), down, 0.0))
    return _fb[n_mels]


def scaled_frames(wav):
    """wav (len) -> (T, 400) float64 frames of WAV_SCALE * wav (T may be 0)."""
    wav = np.asarray(wav, dtype=np.float64) * WAV_SCALE
    idx = np.arange(num_frames(len(wav)))[:, None] * HOP + np.arange(FLEN)[None, :]
    return wav[idx] if idx.size else np.zeros((0, FLEN))


def _prepare(wav):
    """-> s, d, y, xw (T, 400) float64."""
    s = scaled_frames(wav)
    d = s - s.mean(axis=1, keepdims=True)
    y = d - PREEMPH * np.concatenate([d[:, :1], d[:, :-1]], axis=1)
    return s, d, y, y * povey_window()[None, :]


def mel_power64(wav, n_mels):
    """(T, n_mels) float64 mel energies, without the floor."""
    xw = _prepare(wav)[3]
    X = np.fft.rfft(xw, n=NFFT, axis=1)[:, :NBIN]
    return (np.abs(X) ** 2) @ mel_filterbank(n_mels)


def fbank64(wav, n_mels):
    """(T, n_mels) float64: the definition."""
    return np.log(np.maximum(mel_power64(wav, n_mels), FLT_EPSILON))


def bound(wav, n_mels):
    """(T, n_mels): how far exp(fp32 fbank) may lie from max(mel_power64, FLT_EPSILON) (the module's docstring)."""
    s, d, y, xw = _prepare(wav)
    w = povey_window()[None, :]
    prev = lambda a: np.concatenate([a[:, :1], a[:, :-1]], axis=1)
    em = MEAN_ULPS * U * np.abs(s).mean(axis=1, keepdims=True)
    ed = U * np.abs(s) + em + U * np.abs(d)
    ey = ed + PREEMPH * prev(ed) + 2.0 * U * PREEMPH * np.abs(prev(d)) + U * np.abs(y)
    E = (w * ey + 2.0 * U * np.abs(xw)).sum(axis=1, keepdims=True) + DELTA * np.abs(xw).sum(axis=1, keepdims=True)
    X = np.abs(np.fft.rfft(xw, n=NFFT, axis=1)[:, :NBIN])
    fb = mel_filterbank(n_mels)
    value = np.maximum((X ** 2) @ fb, FLT_EPSILON)
    rel = (2.0 * (fb != 0.0).sum(axis=0)[None, :] + 4.0) * U
    size = np.maximum(np.abs(np.log(value)), 1.0)
    ulp = 2.0 ** (np.floor(np.log2(size)) - 23)
    return (2.0 * X * E + E * E) @ fb + value * (rel + np.expm1(LOG_ULPS * ulp))


def floor_cells(wav, n_mels):
    """(T, n_mels) bool: the frame's samples are all zero, or the filter has no non-zero weight."""
    zero_frame = ~scaled_frames(wav).any(axis=1)
    return zero_frame[:, None] | ~mel_filterbank(n_mels).any(axis=0)[None, :]


def error_ratio(fbank32, wav, n_mels):
    """max over frames and bins of |exp(got) - max(mel64, FLT_EPSILON)| / bound for a float32 fbank (T', n_mels) holding the first
    T' <= T frames of wav, and where it is; the floor cells are left out (they are compared exactly).  NaN if got holds one."""
    got = np.exp(np.asarray(fbank32, dtype=np.float64))
    n = got.shape[0]
    assert 1 <= n <= num_frames(len(wav)) and got.shape[1] == n_mels
    ratio = np.abs(got - np.maximum(mel_power64(wav, n_mels)[:n], FLT_EPSILON)) / bound(wav, n_mels)[:n]
    ratio = np.where(floor_cells(wav, n_mels)[:n], 0.0, ratio)
    if np.isnan(ratio).any():
        return float("nan"), (-1, -1)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[at]), tuple(int(v) for v in at)


_fma32 = logmel_emul._fma32


def emulate32(wav, n_mels):
    """The kernel's arithmetic in float32 numpy -> (T, n_mels) float32.  Scaled samples; the mean as lane l's sum of taps l, l + 64, ..
    in that order, then a xor butterfly over the 64 lanes (32, 16, .. 1), divided by 400; d - 0.97f dp with a rounded product; the
    window rounded to fp32; start twiddles cos / sin(2 pi j / 512) rounded to fp32; for even and for odd taps a rotation by 2 theta per
    step, 200 steps, no restart; one fp32 accumulator per frame and DFT column summed in tap order; fp32 power, fp32 filterbank
    product in bin order, floor, fp32 log."""
    wav32 = np.asarray(wav, dtype=np.float32)
    T = num_frames(len(wav32))
    idx = np.arange(T)[:, None] * HOP + np.arange(FLEN)[None, :]
    x = wav32[idx] * np.float32(WAV_SCALE)                                   # (T, 400) float32
    lanes = np.concatenate([x, np.zeros((T, 448 - FLEN), dtype=np.float32)], axis=1).reshape(T, 7, 64)
    s = lanes[:, 0]
    for j in range(1, 7):
        s = s + lanes[:, j]
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ m]
    mean = (s[:, :1] / np.float32(FLEN)).astype(np.float32)
    d = x - mean
    dp = np.concatenate([d[:, :1], d[:, :-1]], axis=1)
    xw = (d - np.float32(PREEMPH) * dp) * povey_window().astype(np.float32)[None, :]
    assert xw.dtype == np.float32
    fb32 = mel_filterbank(n_mels).astype(np.float32)
    j = np.arange(NFFT)
    tw_c = np.cos(2.0 * np.pi * j / NFFT).astype(np.float32)
    tw_s = np.sin(2.0 * np.pi * j / NFFT).astype(np.float32)
    bins = np.arange(NBIN)
    rc, rs = tw_c[(2 * bins) % NFFT], tw_s[(2 * bins) % NFFT]
    tc = [tw_c[(kh * bins) % NFFT] for kh in (0, 1)]
    ts = [tw_s[(kh * bins) % NFFT] for kh in (0, 1)]
    re = np.zeros((T, NBIN), dtype=np.float32)
    im = np.zeros((T, NBIN), dtype=np.float32)
    for kk in range(FLEN // 2):
        for kh in (0, 1):
            a = xw[:, 2 * kk + kh][:, None]
            re = _fma32(a, tc[kh][None, :], re)
            im = _fma32(a, -ts[kh][None, :], im)
            nc = _fma32(tc[kh], rc, -(ts[kh] * rs))
            ts[kh] = _fma32(ts[kh], rc, tc[kh] * rs)
            tc[kh] = nc
    power = _fma32(re, re, im * im)
    o = np.zeros((T, n_mels), dtype=np.float32)
    for k in range(NBIN):
        o = _fma32(power[:, k][:, None], fb32[k][None, :], o)
    return np.log(np.maximum(o, np.float32(FLT_EPSILON)))
