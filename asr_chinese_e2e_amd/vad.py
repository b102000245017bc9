"""Energy voice-activity detection over waveforms: Kaldi's compute-vad-energy on the GPU (csrc/vad.hip), and the host segmenter that
turns its frame mask into stretches of samples a search can take (the definition, in float64 and plain loops: tests/vad_ref.py).

Frames are the Kaldi front end's snip_edges frames at 16 kHz (frame t = samples 160 t .. 160 t + 399).  E[t] = the raw log-energy of
the frame; thr = energy_threshold + energy_mean_scale * mean_t E[t]; frame t is speech iff, of the frames of [t - frames_context,
t + frames_context] that exist, at least proportion_threshold lie above thr.

The segmenter (segments_from_mask) runs on the host over the downloaded mask - 360 KB for an hour of audio - as vectorised numpy
run-length code: a device segmenter would save nothing measurable and would be a second definition to keep exact."""
import math

import numpy as np

FLEN, HOP, SR = 400, 160, 16000


def num_frames(length):
    length = int(length)
    return 0 if length < FLEN else 1 + (length - FLEN) // HOP


def _option(name, v, integer=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"{name} must be a finite number that is not negative, got {v!r}")
    if integer and int(v) != v:
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v) if integer else float(v)


def segment_frames(min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1, max_segment_s=20.0):
    """The segmenter's options in frames (round(100 s)) -> (min_silence, min_speech, pad, max_frames); refuses what it cannot take."""
    min_silence, min_speech, pad, max_frames = (int(round(100 * _option(n, v))) for n, v in
                                                (("min_silence_s", min_silence_s), ("min_speech_s", min_speech_s), ("pad_s", pad_s),
                                                 ("max_segment_s", max_segment_s)))
    if 2 * pad > min_silence:
        raise ValueError(f"pad_s = {pad_s} ({pad} frames) on both sides needs min_silence_s >= {2 * pad / 100.0} (got {min_silence_s}, {min_silence} "
                         "frames): padded segments would overlap")
    if max_frames < 1:
        raise ValueError(f"max_segment_s = {max_segment_s} is less than one frame")
    return min_silence, min_speech, pad, max_frames


def _runs(flags):
    """Maximal runs of true values of a bool vector -> (first, last) int64 arrays."""
    x = np.concatenate(([0], np.asarray(flags, dtype=np.int8), [0]))
    d = np.diff(x)
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1


def segments_from_mask(mask_row, T, length, min_silence, min_speech, pad, max_frames):
    """[(start_sample, end_sample)] of a recording of `length` samples from its speech mask (the first T entries of mask_row; options in
    frames).  Maximal runs of speech; runs fewer than min_silence non-speech frames apart are merged; merged runs shorter than
    min_speech are dropped; the rest are widened by pad on both sides inside [0, T - 1]; a run longer than max_frames is cut, again and
    again, at the centre of the longest pause (non-speech frames of the mask, the first on ties) lying wholly in the second half of its
    first max_frames frames, or behind those when there is none.  Frames [f0, f1] are the samples [160 f0, min(160 f1 + 400, length))."""
    T, min_silence, min_speech, pad, max_frames = int(T), int(min_silence), int(min_speech), int(pad), int(max_frames)
    if 2 * pad > min_silence or min(min_silence, min_speech, pad) < 0 or max_frames < 1:
        raise ValueError(f"segments_from_mask: needs 2 * pad <= min_silence, options that are not negative and max_frames >= 1 (got min_silence "
                         f"{min_silence}, min_speech {min_speech}, pad {pad}, max_frames {max_frames})")
    if T <= 0:
        return []
    mask = np.asarray(mask_row).reshape(-1)[:T] != 0
    if mask.shape[0] != T:
        raise ValueError(f"segments_from_mask: the mask holds {mask.shape[0]} frames, T = {T}")
    a, b = _runs(mask)
    if a.size == 0:
        return []
    new = np.concatenate(([True], a[1:] - b[:-1] - 1 >= min_silence))      # a run starts a merged run unless the pause before it is short
    a, b = a[new], b[np.concatenate((new[1:], [True]))]
    keep = b - a + 1 >= min_speech
    a, b = np.maximum(a[keep] - pad, 0), np.minimum(b[keep] + pad, T - 1)
    out = []
    pa = pb = None                                             # the pauses, found once if a run needs a cut
    for start, end in zip(a.tolist(), b.tolist()):
        while end - start + 1 > max_frames:
            if pa is None:
                pa, pb = _runs(~mask)
            lo, hi = start + max_frames // 2, start + max_frames - 1
            # pauses that touch the window, clipped to it: the runs of non-speech frames lying wholly inside
            i0, i1 = np.searchsorted(pb, lo, side="left"), np.searchsorted(pa, hi, side="right")
            c = hi
            if i1 > i0:
                ca, cb = np.maximum(pa[i0:i1], lo), np.minimum(pb[i0:i1], hi)
                k = int(np.argmax(cb - ca))                    # the first of the longest
                c = int(ca[k] + cb[k]) // 2
            out.append((start, c))
            start = c + 1
        out.append((start, end))
    length = int(length)
    return [(HOP * f0, min(HOP * f1 + FLEN, length)) for f0, f1 in out]


class EnergyVad:
    """Kaldi's energy VAD with its option names and defaults.  frames() runs the kernels; segments() adds the host segmenter."""

    def __init__(self, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6):
        from ._lib import VAD_CTX_MAX
        for name, v in (("energy_threshold", energy_threshold), ("energy_mean_scale", energy_mean_scale), ("proportion_threshold", proportion_threshold)):
            _option(name, v)
        self.frames_context = _option("frames_context", frames_context, integer=True)
        if self.frames_context > VAD_CTX_MAX:
            raise ValueError(f"frames_context must be at most {VAD_CTX_MAX}, got {frames_context!r}")
        if not 0.0 < proportion_threshold <= 1.0:
            raise ValueError(f"proportion_threshold must lie in (0, 1], got {proportion_threshold!r}")
        self.energy_threshold, self.energy_mean_scale = float(energy_threshold), float(energy_mean_scale)
        self.proportion_threshold = float(proportion_threshold)
        self._params = None

    def params(self, device):
        """{energy_threshold, energy_mean_scale, proportion_threshold} as 3 float64 on the device (uploaded once)."""
        import torch
        if self._params is None or self._params.device != torch.device(device):
            self._params = torch.tensor([self.energy_threshold, self.energy_mean_scale, self.proportion_threshold], dtype=torch.float64).to(device)
        return self._params

    def frames(self, wav, wav_len):
        """wav (B, S) f32 on the device at 16 kHz, wav_len (B) int32 on the device -> (E (B, Tmax) f32, speech (B, Tmax) uint8,
        thr (B) f64), device tensors, Tmax = max(frames of S samples, 1): three launches (the decision takes two), no synchronisation."""
        from . import kernels as K
        Tmax = max(num_frames(wav.shape[1]), 1)
        E = K.vad_energy(wav, wav_len, Tmax)
        speech, thr = K.vad_decide(E, wav_len, self.params(wav.device), self.frames_context)
        return E, speech, thr

    def segments(self, wav, wav_len, min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1, max_segment_s=20.0):
        """Per recording [(start_sample, end_sample)]: frames(), one device-to-host copy of the uint8 mask, segments_from_mask.
        wav_len: (B) int32 on the device, or host integers."""
        import torch
        opts = segment_frames(min_silence_s, min_speech_s, pad_s, max_segment_s)
        if torch.is_tensor(wav_len):
            lens, dlen = [int(v) for v in wav_len.tolist()], wav_len.to(device=wav.device, dtype=torch.int32)
        else:
            lens = [int(v) for v in wav_len]
            dlen = torch.tensor(lens, dtype=torch.int32).to(wav.device)
        _, speech, _ = self.frames(wav, dlen)
        mask = speech.cpu().numpy()
        S = wav.shape[1]
        return [segments_from_mask(mask[b], num_frames(min(max(l, 0), S)), min(max(l, 0), S), *opts) for b, l in enumerate(lens)]
