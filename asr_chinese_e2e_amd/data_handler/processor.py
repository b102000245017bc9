"""Log-mel front end on the GPU (Predictor/data_handler/processor.py:18-100 of the reference ran
torchaudio on the CPU): waveform batch -> log-mel -> scalar mean/std normalisation -> LFR.
norm="global" normalises every mel bin by corpus statistics instead (cmvn.py): the variant that can stream."""
import math
import os

import numpy as np
import random

import torch

from .. import kernels as K
from . import specaug
from .cmvn import load_cmvn_meta

SR, N_FFT, HOP = 16000, 400, 160
FRONTENDS = ("reference", "kaldi")
KALDI_NFFT, KALDI_WAV_SCALE, KALDI_PREEMPH, KALDI_LOW_FREQ = 512, 32768.0, 0.97, 20.0      # Kaldi's fbank defaults as WeNet uses them


def mel_filterbank(n_mels, f_min=40.0, f_max=SR / 2 - 200.0):
    """HTK-mel triangular filters over FFT-bin frequencies; f_max = sr/2 - 200 Hz is the build's
    reading of the reference's `f_max=-200` (processor.py:24) - see DESIGN.md."""
    hz2mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    freqs = np.arange(N_FFT // 2 + 1, dtype=np.float64) * SR / N_FFT
    m_pts = np.linspace(hz2mel(f_min), hz2mel(f_max), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]
    fb = np.maximum(0.0, np.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]))
    return torch.from_numpy(fb.astype(np.float32))


def povey_window():
    """Kaldi's default window, (0.5 - 0.5 cos(2 pi n / 399))^0.85, float64 rounded once."""
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / (N_FFT - 1))) ** 0.85
    return torch.from_numpy(w.astype(np.float32))


def kaldi_mel_filterbank(n_mels, low_freq=KALDI_LOW_FREQ, high_freq=SR / 2):
    """(256, n_mels) Kaldi mel banks over the bins 0 .. 255 of the 512-point transform: triangles in the mel domain,
    mel(f) = 1127 ln(1 + f / 700), n_mels + 2 points equally spaced from mel(low_freq) to mel(high_freq); float64 rounded once."""
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    lo, hi = mel(low_freq), mel(high_freq)
    delta = (hi - lo) / (n_mels + 1)
    m = mel(np.arange(KALDI_NFFT // 2, dtype=np.float64) * SR / KALDI_NFFT)[:, None]
    left = lo + np.arange(n_mels, dtype=np.float64)[None, :] * delta
    centre, right = left + delta, left + 2.0 * delta
    fb = np.where((m > left) & (m <= centre), (m - left) / (centre - left), np.where((m > centre) & (m < right), (right - m) / (right - centre), 0.0))
    return torch.from_numpy(fb.astype(np.float32))


def equivalent_length(frames):
    """The length in samples that the normalisation kernels (which count frames as 1 + len // 160, 0 for len = 0) take for `frames`
    frames: 160 (frames - 1) + 1, and 0 for no frame.  How the Kaldi front end, whose count is another function of the length, hands
    its frame counts to asr_utt_norm_augment_lfr_fwd, asr_global_norm_augment_lfr_fwd and asr_cmvn_accumulate.  An int, or a tensor of
    frame counts (then computed where the tensor lives)."""
    if torch.is_tensor(frames):
        return ((frames - 1) * HOP + 1).clamp(min=0)
    return HOP * (frames - 1) + 1 if frames >= 1 else 0


def build_LFR_features(inputs, m, n):
    """Host-side LFR with the reference's rule (processor.py:74-100), index form."""
    inputs = np.asarray(inputs)
    T = inputs.shape[0]
    T_out = int(np.ceil(T / n))
    idx = np.minimum(np.arange(T_out)[:, None] * n + np.arange(m)[None, :], T - 1)
    return inputs[idx].reshape(T_out, m * inputs.shape[1])


def sample_spec_augment(n_mels, n_frames, rng=random, F=30, T=40):
    """The mask ranges AudioParser.augment would draw (processor.py:52-58 -> augments.time_mask then
    augments.freq_mask, one mask each, F=30, T=40), with the SAME sequence of randrange calls, so a
    seeded `random` gives the reference's masks.  Returns [t0, t1, f0, f1] (empty ranges = no mask).
    Where the reference would raise (randrange on an empty range: fewer frames than the drawn width)
    no mask is applied."""
    t0 = t1 = f0 = f1 = 0
    t = rng.randrange(0, T)                      # augments.py:29
    if n_frames - t > 0:
        tz = rng.randrange(0, n_frames - t)      # :30
        if t > 0:                                # :33 early return when the width is 0
            t0, t1 = tz, rng.randrange(tz, tz + t)   # :36 (mask_end may equal t_zero: empty)
    f = rng.randrange(0, F)                      # :9
    if n_mels - f > 0:
        fz = rng.randrange(0, n_mels - f)        # :10
        if f > 0:
            f0, f1 = fz, rng.randrange(fz, fz + f)   # :15
    return [t0, t1, f0, f1]


class AudioParser:
    """Batched device front end: parse_batch(wav (B,S) f32 cuda, wav_len (B) int) ->
    (features (B, T_lfr, lfr_m*n_mels), feature_len (B) int32)."""

    def __init__(self, sample_rate=SR, n_mels=80, window_size=N_FFT, hop=HOP, lfr_m=4, lfr_n=3, device="cuda", norm="utterance", cmvn=None,
                 frontend="reference"):
        """norm: "utterance" (the reference's scalar mean / std of each utterance) or "global" (per-bin corpus statistics): then
        cmvn = (mean, istd), one value per mel bin, or the path of a statistics file (tools/compute_cmvn.py, WeNet's JSON, Kaldi's text).
        frontend: "reference" (the reference's log-mel: centred reflect-padded frames, Hann, 400-point DFT, HTK banks) or "kaldi"
        (Kaldi fbank as WeNet configures it: snip_edges frames, DC removal, pre-emphasis, Povey window, 512-point DFT, Kaldi banks)."""
        assert sample_rate == SR and window_size == N_FFT and hop == HOP, "kernel is specialised to 16 kHz / 400 / 160"
        if norm not in ("utterance", "global"):
            raise ValueError(f"norm must be 'utterance' or 'global', got {norm!r}")
        if frontend not in FRONTENDS:
            raise ValueError(f"frontend must be one of {FRONTENDS}, got {frontend!r}")
        self.n_mels, self.lfr_m, self.lfr_n, self.norm, self.frontend = n_mels, lfr_m, lfr_n, norm, frontend
        self.mean = self.istd = None
        if norm == "global":
            if cmvn is None or (isinstance(cmvn, str) and not cmvn):
                raise ValueError("norm='global' needs cmvn=(mean, istd) or the path of a statistics file (tools/compute_cmvn.py)")
            if isinstance(cmvn, (str, os.PathLike)):
                mean, istd, _, file_frontend = load_cmvn_meta(cmvn)
                if file_frontend != frontend:
                    raise ValueError(f"{os.fspath(cmvn)}: statistics of the {file_frontend!r} front end, the parser's is {frontend!r}")
            else:
                mean, istd = cmvn
            mean, istd = (np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.float64) for v in (mean, istd))
            if mean.shape != (n_mels,) or istd.shape != (n_mels,):
                raise ValueError(f"cmvn statistics are for {mean.shape} / {istd.shape} mel bins, the parser has {n_mels}")
            self.mean, self.istd = (torch.from_numpy(v.astype(np.float32)).to(device) for v in (mean, istd))
        elif cmvn is not None:
            raise ValueError("cmvn statistics given, but norm is 'utterance': pass norm='global' to use them")
        self.wav_scale, self.preemph = (KALDI_WAV_SCALE, KALDI_PREEMPH) if frontend == "kaldi" else (1.0, 0.0)
        if frontend == "kaldi":
            self.window, self.melfb = povey_window().to(device), kaldi_mel_filterbank(n_mels).to(device)
        else:
            self.window = torch.hann_window(N_FFT, periodic=True, dtype=torch.float32).to(device)
            self.melfb = mel_filterbank(n_mels).to(device)

    # ---- the frame arithmetic of the two front ends: the one place it is written
    def num_frames(self, length):
        """Frames of an utterance of `length` samples."""
        length = int(length)
        if self.frontend == "kaldi":
            return 1 + (length - N_FFT) // HOP if length >= N_FFT else 0
        return 1 + length // HOP if length > 0 else 0

    def max_frames(self, S):
        """Rows of the feature buffer of a batch whose rows hold S samples (at least 1: the kernels take no empty buffer)."""
        return max(self.num_frames(S), 1) if self.frontend == "kaldi" else 1 + int(S) // HOP

    def frames_ready(self, received, closed=False):
        """Streaming: frames that can be computed after `received` samples; closed: `received` is the whole utterance.  A Kaldi frame
        touches its own 400 samples only, so the close changes nothing."""
        if self.frontend == "kaldi":
            return self.num_frames(received)
        from . import stream_frontend as SF
        return SF.frames_ready(received, closed)

    def oldest_sample(self, t):
        """Streaming: the first sample frame t (and so any later frame) touches."""
        return HOP * t if self.frontend == "kaldi" else max(0, HOP * t - N_FFT // 2)

    def frame_centre_sample(self, t):
        """The sample at the centre of frame t's window."""
        return HOP * t + N_FFT // 2 if self.frontend == "kaldi" else HOP * t

    def frame_counts(self, wav_len, S, Tmax):
        """Frames per utterance, a host list (wav_len is read back), of a batch whose rows hold S samples, cut at Tmax."""
        return [min(self.num_frames(min(int(l), S)), Tmax) for l in wav_len.tolist()]

    def norm_lengths(self, wav_len, S, Tmax):
        """The int32 lengths that make the normalisation kernels count this front end's frames (rows of S samples, cut at Tmax): the
        lengths themselves, for "kaldi" the equivalent lengths - computed where wav_len lives, nothing is read back."""
        wl = wav_len.to(torch.int32)
        if self.frontend != "kaldi":
            return wl
        frames = (torch.div(wl.clamp(0, S) - N_FFT, HOP, rounding_mode="floor") + 1).clamp(0, Tmax)
        return equivalent_length(frames).to(torch.int32)

    def features(self, wav, wav_len, Tmax, feat=None):
        """wav (B, S) f32, wav_len (B) int32 -> (B, Tmax, n_mels) f32 frames of this parser's front end."""
        if self.frontend == "kaldi":
            return K.fbank(wav, wav_len, self.window, self.melfb, Tmax, self.wav_scale, self.preemph, feat=feat)
        return K.logmel(wav, wav_len, self.window, self.melfb, Tmax, feat=feat)

    def spec_ranges(self, policy, draws, lengths, S=None):
        """The (B, policy.width) int32 row block (numpy) of a batch for parse_batch(spec_ranges=...): specaug.resolve for every utterance,
        its frame count taken from the HOST lengths in samples by num_frames, capped at max_frames(S) as the kernels cap it (S: the width
        of the waveform rows, the longest length when None).  draws: the batch's rows of specaug.draw's table.  Nothing touches the device."""
        policy.check_mels(self.n_mels)
        lengths = [int(l) for l in lengths]
        S = max(lengths + [1]) if S is None else int(S)
        Tmax = self.max_frames(S)
        return specaug.resolve_batch(policy, draws, [min(self.num_frames(min(l, S)), Tmax) for l in lengths], self.n_mels)

    def parse_batch(self, wav, wav_len, dtype=torch.float32, augment=False, rng=random, spec_ranges=None, spec_policy=None):
        """augment=True: SpecAugment as AudioParser.parse(path, augment=True) of the reference, masks
        drawn on the host from `rng` (the `random` module by default, as the reference), applied on the
        device between normalisation and frame stacking.
        spec_ranges, spec_policy: a specaug.SpecAugmentPolicy and the batch's resolved rows (spec_ranges(); (B, >= policy.width) int32, on the
        device or a host array that is then copied) - several masks with zero fill, time warp and substitution in place of the reference's
        variant (tests/specaug_ref.py).  Both or neither, and never with augment=True."""
        if (spec_ranges is None) != (spec_policy is None):
            raise ValueError("parse_batch: spec_ranges and spec_policy come together (AudioParser.spec_ranges builds the rows)")
        if spec_policy is not None and augment:
            raise ValueError("parse_batch: spec_policy replaces the reference's SpecAugment - not both it and augment=True")
        B, S = wav.shape
        if spec_policy is not None:      # refused before any launch
            spec_policy.check_mels(self.n_mels)
            if not torch.is_tensor(spec_ranges):
                spec_ranges = torch.from_numpy(np.ascontiguousarray(spec_ranges, dtype=np.int32))
            if spec_ranges.dim() != 2 or spec_ranges.shape[0] != B or spec_ranges.shape[1] < spec_policy.width or spec_ranges.dtype != torch.int32:
                raise ValueError(f"parse_batch: spec_ranges must be (B = {B}, >= {spec_policy.width}) int32, got {tuple(spec_ranges.shape)} {spec_ranges.dtype}")
            spec_ranges = spec_ranges.to(wav.device)
        Tmax = self.max_frames(S)
        wl = wav_len.to(torch.int32)
        feat = self.features(wav.contiguous(), wl, Tmax)
        Tl = (Tmax + self.lfr_n - 1) // self.lfr_n
        if spec_policy is not None:
            counts = (spec_policy.n_t, spec_policy.n_f, spec_policy.n_s)
            wl = self.norm_lengths(wl, S, Tmax)
            if self.norm == "global":
                return K.global_norm_specaug_lfr(feat, wl, spec_ranges, counts, self.mean, self.istd, self.lfr_m, self.lfr_n, Tl, dtype)
            return K.utt_norm_specaug_lfr(feat, wl, spec_ranges, counts, self.lfr_m, self.lfr_n, Tl, dtype)
        masks = None
        if augment:
            frames = self.frame_counts(wav_len, S, Tmax)
            masks = torch.tensor([sample_spec_augment(self.n_mels, fr, rng) for fr in frames], dtype=torch.int32).to(wav.device)
        wl = self.norm_lengths(wl, S, Tmax)
        if self.norm == "global":
            return K.global_norm_lfr(feat, wl, self.mean, self.istd, self.lfr_m, self.lfr_n, Tl, dtype, masks=masks)
        return K.utt_norm_lfr(feat, wl, self.lfr_m, self.lfr_n, Tl, dtype, masks=masks)
