"""Host side of the noise and reverberation augmentation (Kaldi reverberate_data_dir / WeNet add_reverb, add_noise; the reference has
no waveform-side augmentation: parity unpinned by the reference).  A room impulse response h of L taps with its peak at p turns an
utterance x into y[n] = sum_k h[k] x[n + p - k], n < len(x): the length stays and the direct path stays aligned (Kaldi
--shift-output).  A noise clip v, started at a drawn offset and wrapped to the utterance's length, is added with the gain that
makes 10 log10(sum x^2 / sum (g v)^2) the drawn signal-to-noise ratio.  The kernels (csrc/augment.hip) work from the device-resident
banks built here; tests/noise_ref.py restates both definitions in float64."""
import random

import numpy as np
import torch

SAMPLE_RATE = 16000
MAX_TAPS = 8192      # ASR_REVERB_MAX_TAPS: the direct kernel's limit, and the default cap
FFT_MAX_TAPS = 65536      # ASR_REVERB_FFT_MAX_TAPS: the FFT path's limit
# "auto" takes the FFT path for a bank whose longest response has at least this many taps: the smallest measured length from which
# asr_reverb_fft_fwd beats asr_reverb_fwd - 42 us against 110 us at 1024 taps, 43 against 30 at 256 (profiles/reverb_fft_bench.json)
AUTO_FFT_FROM_TAPS = 1024
METHODS = ("direct", "fft")
PRE_PEAK = 64        # samples kept in front of a response's peak


def _read(src, what, resample=False, device="cuda"):
    """A path -> (float32 samples, name) through load_wav, refusing another rate - or, with resample=True, converting it to 16 kHz on
    `device` (data_handler.resample, one asr_resample_fwd launch per file, when the bank is built: before any truncation or scaling);
    an array -> itself, in its own precision."""
    if isinstance(src, str):
        from .loader import load_wav
        w, sr = load_wav(src)
        if sr != SAMPLE_RATE:
            if not resample:
                raise ValueError(f"{src}: sample rate {sr}, the {what} bank needs {SAMPLE_RATE}")
            from . import resample as resample_mod
            resample_mod.plan(sr)      # an unsupported rate raises here, naming it
            if w.size:
                out, _, n_out = resample_mod.resample_batch(torch.from_numpy(w)[None].to(device), [w.size], [sr])
                w = out[0, :n_out[0]].cpu().numpy()
        return w, src
    if torch.is_tensor(src):
        src = src.detach().cpu().numpy()
    return np.asarray(src).reshape(-1), None


def rir_entry(h, max_taps=MAX_TAPS, name="response", tap_limit=MAX_TAPS):
    """One response -> (taps float32, peak index inside them): the samples [s0, s0 + max_taps) with s0 = max(0, argmax |h| - 64),
    scaled to unit energy (sum h^2 = 1, as WeNet's add_reverb) in float64 AFTER the truncation and rounded once.
    tap_limit: as rir_table's."""
    if not 1 <= int(max_taps) <= int(tap_limit) <= FFT_MAX_TAPS:
        raise ValueError(f"{name}: max_taps={max_taps} outside 1 .. {int(tap_limit)} (at most {FFT_MAX_TAPS})")
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    if h.size == 0 or not np.any(h):
        raise ValueError(f"{name}: the impulse response is empty or all zeros")
    peak = int(np.argmax(np.abs(h)))
    s0 = max(0, peak - PRE_PEAK)
    h = h[s0:s0 + int(max_taps)]
    return (h / np.sqrt(np.sum(h * h))).astype(np.float32), peak - s0


def rir_table(responses, max_taps=MAX_TAPS, names=None, tap_limit=MAX_TAPS):
    """The table maths of RirBank on the host: -> (table (R, Lcap) float32 zero-padded, lens (R) int32, peaks (R) int32).
    tap_limit: the largest max_taps admitted - the direct kernel's 8192 unless the caller names the FFT path's FFT_MAX_TAPS."""
    if not 1 <= int(tap_limit) <= FFT_MAX_TAPS:
        raise ValueError(f"tap_limit={tap_limit}: no reverberation kernel takes more than {FFT_MAX_TAPS} taps")
    if not 1 <= int(max_taps) <= int(tap_limit):
        raise ValueError(f"max_taps={max_taps}: the reverberation kernel takes 1 .. {int(tap_limit)} taps")
    entries = [rir_entry(h, max_taps, names[i] if names and names[i] else f"response {i}", tap_limit) for i, h in enumerate(responses)]
    if not entries:
        raise ValueError("no impulse responses")
    table = np.zeros((len(entries), max(e[0].size for e in entries)), dtype=np.float32)
    for i, (h, _) in enumerate(entries):
        table[i, :h.size] = h
    return table, np.asarray([e[0].size for e in entries], dtype=np.int32), np.asarray([e[1] for e in entries], dtype=np.int32)


class RirBank:
    """Room impulse responses resident on `device`: table (R, Lcap) f32, lens, peaks (R) int32 (rir_table).
    method: the kernel the loader convolves with - "direct" (asr_reverb_fwd, at most 8192 taps) or "fft" (asr_reverb_fft_fwd, at most
    65536); "auto" reads the responses with the FFT path's limit and settles on "fft" when the longest one kept has at least
    AUTO_FFT_FROM_TAPS taps, on "direct" otherwise.  self.method is always one of METHODS.
    resample: True = files at another rate are converted to 16 kHz on the device (_read) before the truncation and the energy scaling."""

    def __init__(self, paths_or_arrays, device="cuda", max_taps=MAX_TAPS, method="direct", resample=False):
        if method not in METHODS + ("auto",):
            raise ValueError(f"method={method!r}: one of 'direct', 'fft', 'auto'")
        read = [_read(s, "impulse-response", resample, device) for s in paths_or_arrays]
        table, lens, peaks = rir_table([w for w, _ in read], max_taps, [n for _, n in read], MAX_TAPS if method == "direct" else FFT_MAX_TAPS)
        if method == "auto":
            method = "fft" if int(lens.max()) >= AUTO_FFT_FROM_TAPS else "direct"
        self.method = method
        self.n, self.max_taps = int(lens.size), int(max_taps)
        self.table, self.lens, self.peaks = (torch.from_numpy(a).to(device) for a in (table, lens, peaks))

    def __len__(self):
        return self.n


def noise_table(clips, names=None, max_seconds=600):
    """The clips laid end to end: -> (flat float32, off (N + 1) int32).  Clips are added until max_seconds of noise are held."""
    flat, off = [], [0]
    for i, w in enumerate(clips):
        name = names[i] if names and names[i] else f"clip {i}"
        w = np.asarray(w, dtype=np.float32).reshape(-1)
        if w.size == 0 or not np.any(w):
            raise ValueError(f"{name}: the noise clip is empty or all zeros")
        if off[-1] >= max_seconds * SAMPLE_RATE:
            break
        flat.append(w)
        off.append(off[-1] + w.size)
    if not flat:
        raise ValueError("no noise clips")
    if off[-1] >= 2 ** 31:
        raise ValueError("the noise bank holds 2^31 samples or more: lower max_seconds")
    return np.concatenate(flat), np.asarray(off, dtype=np.int32)


class NoiseBank:
    """Noise clips resident on `device`: one flat f32 buffer `noise`, clip j at [off[j], off[j + 1]) (`noise_off`, N + 1 int32);
    `lens`: the clip lengths on the host (the offsets are drawn there).  resample: True = files at another rate are converted (_read)."""

    def __init__(self, paths_or_arrays, device="cuda", max_seconds=600, resample=False):
        clips, names, total = [], [], 0
        for s in paths_or_arrays:
            if total >= max_seconds * SAMPLE_RATE:      # full: the remaining files are not even read
                break
            w, name = _read(s, "noise", resample, device)
            clips.append(w)
            names.append(name)
            total += w.size
        flat, off = noise_table(clips, names, max_seconds)
        self.lens = [int(b - a) for a, b in zip(off[:-1], off[1:])]
        self.n = len(self.lens)
        self.noise, self.noise_off = torch.from_numpy(flat).to(device), torch.from_numpy(off).to(device)

    def __len__(self):
        return self.n


def snr_scale_bits(snr_db):
    """10^(-snr_dB / 20) as the int32 that carries its float32 bits (the kernel's `scale`)."""
    return int(np.asarray(10.0 ** (-float(snr_db) / 20.0), dtype=np.float32).view(np.int32))


def draw_augment(seed, epoch, n, noise_prob=0.5, n_noise=0, noise_lens=(), snr_db=(5, 20), rir_prob=0.5, n_rir=0):
    """Per utterance 0 .. n-1 of the data set -> (noise index or -1, offset in [0, nlen), SNR in dB uniform in [lo, hi], response index
    or -1), four lists.  A pure function of (seed, epoch, utterance index), like speed.draw_factors: one generator of its own, seeded
    from a string that names this augmentation and consumed in index order, six numbers per utterance whatever they decide - so the
    speed draws and the loader's rng (batch order, SpecAugment masks) are untouched and every data-parallel rank draws the same."""
    rng = random.Random(f"noise_reverb/{int(seed)}/{int(epoch)}")
    lo, hi = (float(snr_db[0]), float(snr_db[1])) if isinstance(snr_db, (tuple, list)) else (float(snr_db), float(snr_db))
    nidx, noff, snr, ridx = [], [], [], []
    for _ in range(n):
        a, j, f, s, c, r = rng.random(), rng.randrange(max(n_noise, 1)), rng.random(), rng.uniform(lo, hi), rng.random(), rng.randrange(max(n_rir, 1))
        on = n_noise > 0 and a < noise_prob
        nidx.append(j if on else -1)
        noff.append(min(int(f * noise_lens[j]), noise_lens[j] - 1) if on else 0)
        snr.append(s)
        ridx.append(r if n_rir > 0 and c < rir_prob else -1)
    return nidx, noff, snr, ridx
