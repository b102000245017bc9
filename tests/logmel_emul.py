"""The log-mel front end's reference side, numpy only (no GPU): the framing rule for every length, the float64 mel energies, an
a-priori fp32 error bound, and a float32 restatement of the kernel's arithmetic that shows the bound holds for fp32 as such.

Framing: frame t, tap n reads sample i = 160 t - 200 + n; i < 0 -> -i; i >= len -> 2 (len - 1) - i; then clamped to [0, len - 1].
For len > 200 that is np.pad(mode="reflect") framing, which oracle/logmel_ref.log_mel uses.  For len <= 200 the padding is longer
than the signal allows (reflect padding in torch refuses it, np.pad goes on reflecting back and forth) and this rule - one
reflection at each end, then the clamp - is the project's own definition.  T = 1 + len // 160 frames.

Bound (from fp32 arithmetic, not from the kernel): with xw the windowed frame and L1_t = sum_n |xw[t, n]|, the DFT amplitude error is
at most E_t = DELTA L1_t, DELTA = 6e-5 (200 steps of the twiddle recurrence at a few ulp each, about 3.6e-5, plus 400 fp32
accumulations at 2^-24, about 2.4e-5); the power error of bin k at most 2 |X_k| E_t + E_t^2; the mel error at most that summed over
the filterbank plus REL = 1e-6 of the value under the log (fp32 mel product and logf).  The value under the log is mel + 1e-20: the
floor belongs to the definition (logmel_ref.LOG_FLOOR), so a silent cell is held to 1e-20 and not to 0."""
import numpy as np

from oracle import logmel_ref as LM

N_FFT, HOP, NBIN = LM.N_FFT, LM.HOP, LM.N_FFT // 2 + 1
DELTA, REL = 6e-5, 1e-6
FLOOR32 = np.float32(LM.LOG_FLOOR)
LOG_FLOOR32 = np.log(FLOOR32)                  # the float32 nearest to log(1e-20); a device's logf may miss it by an ulp or two


def frame_index(length):
    """(T, 400) sample index of every tap of every frame of an utterance of `length` >= 1 samples."""
    length = int(length)
    assert length >= 1
    i = np.arange(LM.num_frames(length))[:, None] * HOP - N_FFT // 2 + np.arange(N_FFT)[None, :]
    i = np.where(i < 0, -i, i)
    i = np.where(i >= length, 2 * (length - 1) - i, i)
    return np.clip(i, 0, length - 1)


def frames(wav):
    """wav (len >= 1) -> (T, 400) float64 frames, not yet windowed."""
    wav = np.asarray(wav, dtype=np.float64)
    return wav[frame_index(len(wav))]


def _spectrum(wav):
    xw = frames(wav) * LM.hann_periodic()[None, :]
    return xw, np.fft.rfft(xw, n=N_FFT, axis=1)


def mel_power64(wav, n_mels):
    """(T, n_mels) float64 mel energies, without the log floor."""
    _, X = _spectrum(wav)
    return (np.abs(X) ** 2) @ LM.mel_filterbank(n_mels)


def _bound_parts(wav, n_mels):
    xw, X = _spectrum(wav)
    E = DELTA * np.abs(xw).sum(axis=1, keepdims=True)
    fb = LM.mel_filterbank(n_mels)
    return (2.0 * np.abs(X) * E + E * E) @ fb, (np.abs(X) ** 2) @ fb + LM.LOG_FLOOR


def bound(wav, n_mels):
    """(T, n_mels): how far exp(fp32 log-mel) may lie from mel_power64 + 1e-20."""
    arith, value = _bound_parts(wav, n_mels)
    return arith + REL * value


def floor_cells(wav, n_mels):
    """(T, n_mels) bool: cells whose frame is all zero or whose filterbank column is all zero.  Nothing but the floor is under the log
    there, so the one right answer is logf(1e-20f) (LOG_FLOOR32 where logf is correctly rounded) and the tests ask for it exactly.  (The bound has nothing to say about them: fp32
    cannot hold log(1e-20) more closely than 1.3e-6 of 1e-20 after exp, which is past REL whatever the kernel does.)"""
    return _bound_parts(wav, n_mels)[0] == 0.0


def error_ratio(logmel32, wav, n_mels):
    """max over frames and bins of |exp(got) - (mel64 + floor)| / bound for a float32 log-mel (T', n_mels) holding the first
    T' <= T frames of wav, and where it is; the floor cells are left out (they are compared exactly).  NaN if got holds one."""
    got = np.exp(np.asarray(logmel32, dtype=np.float64))
    n = got.shape[0]
    assert 1 <= n <= LM.num_frames(len(wav)) and got.shape[1] == n_mels
    ratio = np.abs(got - (mel_power64(wav, n_mels)[:n] + LM.LOG_FLOOR)) / bound(wav, n_mels)[:n]
    ratio = np.where(floor_cells(wav, n_mels)[:n], 0.0, ratio)
    if np.isnan(ratio).any():
        return float("nan"), (-1, -1)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[at]), tuple(int(v) for v in at)


def _fma32(a, b, c):
    """fl32(a b + c) for float32 arrays: the product of two float32 is exact in float64, the sum is rounded once there and once to
    float32 (a double rounding differs from a true FMA in rare last bits only)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate32(wav, n_mels):
    """The kernel's arithmetic in float32 numpy -> (T, n_mels) float32 log-mel.  fp32 windowed frames; start twiddles
    cos / sin(2 pi j / 400) rounded to fp32; for even and for odd taps a rotation by 2 theta per step, 200 steps, no restart; one
    fp32 accumulator per frame and DFT column summed in tap order; fp32 power, fp32 filterbank product in bin order, fp32 log."""
    wav32 = np.asarray(wav, dtype=np.float32)
    win32 = LM.hann_periodic().astype(np.float32)
    fb32 = LM.mel_filterbank(n_mels).astype(np.float32)
    xw = wav32[frame_index(len(wav32))] * win32[None, :]                     # (T, 400) float32
    j = np.arange(N_FFT)
    tw_c = np.cos(2.0 * np.pi * j / N_FFT).astype(np.float32)
    tw_s = np.sin(2.0 * np.pi * j / N_FFT).astype(np.float32)
    bins = np.arange(NBIN)
    rc, rs = tw_c[(2 * bins) % N_FFT], tw_s[(2 * bins) % N_FFT]
    tc = [tw_c[(kh * bins) % N_FFT] for kh in (0, 1)]                        # tap k = kh, then k += 2 per step
    ts = [tw_s[(kh * bins) % N_FFT] for kh in (0, 1)]
    T = xw.shape[0]
    re = np.zeros((T, NBIN), dtype=np.float32)
    im = np.zeros((T, NBIN), dtype=np.float32)
    for kk in range(N_FFT // 2):
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
    return np.log(o + FLOOR32)


# ---- the signals the accuracy tests use: 8000 samples each, float32, seeded ------------------------------------------------------
SR, N_SIG = LM.SR, 8000


def signals():
    """name -> float32 waveform (8000,)."""
    rng = np.random.RandomState(7)
    t = np.arange(N_SIG) / SR
    tone = 0.5 * np.sin(2.0 * np.pi * 1234.5 * t)
    impulse = np.zeros(N_SIG)
    impulse[4321] = 1.0
    noise = rng.randn(N_SIG)
    sig = {
        "noise 0.1": 0.1 * rng.randn(N_SIG),
        "tone 1234.5 Hz": tone,
        "tone + noise at -60 dB": tone + 0.5e-3 * rng.randn(N_SIG),
        "chirp 100-7100 Hz": 0.5 * np.sin(2.0 * np.pi * (100.0 * t + 0.5 * (7100.0 - 100.0) / (N_SIG / SR) * t * t)),
        "constant 0.25": np.full(N_SIG, 0.25),
        "impulse": impulse,
        "tone 7990 Hz": 0.5 * np.sin(2.0 * np.pi * 7990.0 * t),
        "noise 1e-4": 1e-4 * noise,
        "noise 30": 30.0 * noise,
    }
    return {k: v.astype(np.float32) for k, v in sig.items()}
