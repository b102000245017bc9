"""The energy VAD's reference side, numpy only (no GPU): the definition in float64 with plain loops, an a-priori fp32 error bound for the
frame energy, and a float32 restatement of the kernel's arithmetic (csrc/vad.hip) that shows the bound holds for fp32 as such.

Definition (Kaldi's compute-vad-energy, restated: nothing of Kaldi is compared against - parity unpinned by Kaldi's binaries).
Frames are the fbank front end's snip_edges frames at 16 kHz: T = 0 for len < 400, else 1 + (len - 400) // 160; frame t is samples
160 t .. 160 t + 399; samples are multiplied by 32768.  Raw log-energy (raw_energy = true, dither 0): m = mean(s),
E[t] = log(max(sum_i (s_i - m)^2, FLT_EPSILON)).  Decision with Kaldi's option names and defaults (energy_threshold 5.0,
energy_mean_scale 0.5, frames_context 0, proportion_threshold 0.6): thr = energy_threshold + energy_mean_scale * (sum_t E[t]) / T;
frame t is speech iff num >= den * proportion_threshold, den = the frames t2 of [t - ctx, t + ctx] that lie in [0, T), num = those of
them with E[t2] > thr.

Segments, integers only, in this order: (1) maximal runs of speech frames; (2) neighbouring runs separated by fewer than min_silence
non-speech frames are merged; (3) merged runs shorter than min_speech frames are dropped; (4) every run is widened by pad frames on both
sides, clipped to [0, T - 1] (2 pad <= min_silence, so padded runs never overlap); (5) a run longer than max_frames is split, again
and again on the remainder: among the cut frames c in [start + max_frames // 2, start + max_frames - 1] the longest run of non-speech
frames (the mask of the decision, before merging) lying wholly inside that window is taken, the first on ties, and c is its centre
(a + b) // 2; without a non-speech frame in the window c = start + max_frames - 1; the piece is [start, c], the next starts at c + 1.
A segment of frames [f0, f1] is the samples [160 f0, min(160 f1 + 400, len)).

Bound (from fp32 arithmetic, not from the kernel; u = 2^-24), stated for Q = sum (s_i - m)^2, the value under the log - a constant
frame cancels to nearly nothing and its log means nothing, so the log is compared only where Q is well above the bound (log_bound).
The scaled samples are exact (a power of two).  With A = mean |s| of the frame and d = s - m the exact values:
  mean:  every tap passes through at most 12 additions (6 in its lane, 6 levels of the lane tree): gamma_12 sum |s| / 400, and the
         division's rounding u |mean| <= u A; second-order terms rounded up: EM = 14 u A;
  d:     the subtraction's rounding on top: ed[i] = EM (1 + u) + u |d[i]|;
  Q:     sum (2 |d[i]| ed[i] + ed[i]^2) for the error of the terms, and every term passes through at most 13 roundings (its own
         product or fused multiply-add, at most 6 more in its lane, 6 levels of the tree): gamma_13 sum (|d[i]| + ed[i])^2;
  logf:  the hardware's log2 to 1 ulp times ln 2 plus one rounding is at most LOG_ULPS = 2.5 ulp of a float32 of the size of the
         result (at least of size 1), which after exp is a relative error of expm1(that) of max(Q, FLT_EPSILON) (tests/fbank_ref.py's
         figure for the same logf).
max(., FLT_EPSILON) is 1-Lipschitz, so the floor adds nothing.  An all-zero frame has mean 0, d = 0 and Q = 0 whatever the rounding:
the answer logf(FLT_EPSILON) is compared exactly."""
import numpy as np

from tests import logmel_emul

SR, FLEN, HOP = 16000, 400, 160
WAV_SCALE = 32768.0
FLT_EPSILON = 2.0 ** -23
LOG_FLOOR32 = np.log(np.array([FLT_EPSILON], dtype=np.float32))[0]      # the float32 nearest to log(FLT_EPSILON)
U = 2.0 ** -24
MEAN_ULPS, SUM_ROUNDINGS, LOG_ULPS = 14.0, 13, 2.5
DEFAULTS = dict(energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0, proportion_threshold=0.6)
SEG_DEFAULTS = dict(min_silence_s=0.3, min_speech_s=0.1, pad_s=0.1, max_segment_s=20.0)


def num_frames(length):
    length = int(length)
    return 0 if length < FLEN else 1 + (length - FLEN) // HOP


def to_frames(seconds):
    return int(round(100 * seconds))


# ------------------------------------------------------------------------------------ the definition, plain loops
def sumsq64(wav):
    """(T,) float64: sum_i (s_i - mean)^2 of every frame, without the floor."""
    wav = [float(v) * WAV_SCALE for v in np.asarray(wav, dtype=np.float64)]
    out = np.zeros(num_frames(len(wav)))
    for t in range(len(out)):
        s = wav[HOP * t: HOP * t + FLEN]
        m = sum(s) / FLEN
        out[t] = sum((v - m) * (v - m) for v in s)
    return out


def energy64(wav):
    """(T,) float64 raw log-energies: the definition."""
    return np.log(np.maximum(sumsq64(wav), FLT_EPSILON))


def threshold(E, energy_threshold=5.0, energy_mean_scale=0.5):
    """thr in float64 from the T log-energies E (a plain left-to-right sum); T = 0 has no mean term."""
    E = [float(v) for v in E]
    if not E:
        return float(energy_threshold)
    tot = 0.0
    for v in E:
        tot += v
    return energy_threshold + energy_mean_scale * tot / len(E)


def decide(E, thr, frames_context=0, proportion_threshold=0.6):
    """(T,) uint8 speech mask from the log-energies E (compared as float64) and the threshold."""
    T = len(E)
    out = np.zeros(T, dtype=np.uint8)
    for t in range(T):
        num = den = 0
        for t2 in range(t - frames_context, t + frames_context + 1):
            if 0 <= t2 < T:
                den += 1
                if float(E[t2]) > thr:
                    num += 1
        out[t] = 1 if num >= den * proportion_threshold else 0
    return out


def segments(mask, T, length, min_silence, min_speech, pad, max_frames):
    """[(start_sample, end_sample)] of one recording of `length` samples from its speech mask (at least T entries): the module's
    docstring, step by step."""
    assert 2 * pad <= min_silence and max_frames >= 1 and min_silence >= 0 and min_speech >= 0 and pad >= 0
    mask = [int(bool(v)) for v in mask[:T]]
    runs, t = [], 0
    while t < T:                                              # 1. maximal runs
        if mask[t]:
            a = t
            while t + 1 < T and mask[t + 1]:
                t += 1
            runs.append([a, t])
        t += 1
    merged = []
    for r in runs:                                            # 2. merge over short pauses
        if merged and r[0] - merged[-1][1] - 1 < min_silence:
            merged[-1][1] = r[1]
        else:
            merged.append(list(r))
    merged = [r for r in merged if r[1] - r[0] + 1 >= min_speech]                # 3. drop short runs
    merged = [[max(r[0] - pad, 0), min(r[1] + pad, T - 1)] for r in merged]      # 4. pad
    out = []
    for start, end in merged:                                 # 5. split
        while end - start + 1 > max_frames:
            lo, hi = start + max_frames // 2, start + max_frames - 1
            best, c, t = 0, hi, lo
            while t <= hi:
                if not mask[t]:
                    a = t
                    while t + 1 <= hi and not mask[t + 1]:
                        t += 1
                    if t - a + 1 > best:
                        best, c = t - a + 1, (a + t) // 2
                t += 1
            out.append((start, c))
            start = c + 1
        out.append((start, end))
    return [(HOP * f0, min(HOP * f1 + FLEN, int(length))) for f0, f1 in out]


# ------------------------------------------------------------------------------------ the bound
def _frames(wav):
    wav = np.asarray(wav, dtype=np.float64) * WAV_SCALE
    idx = np.arange(num_frames(len(wav)))[:, None] * HOP + np.arange(FLEN)[None, :]
    return wav[idx] if idx.size else np.zeros((0, FLEN))


def frame_bounds(wav):
    """(T,) float64: how far exp(fp32 log-energy) may lie from max(sumsq64, FLT_EPSILON) (the module's docstring)."""
    s = _frames(wav)
    d = np.abs(s - s.mean(axis=1, keepdims=True))
    em = MEAN_ULPS * U * np.abs(s).mean(axis=1, keepdims=True)
    ed = em * (1.0 + U) + U * d
    gamma = SUM_ROUNDINGS * U / (1.0 - SUM_ROUNDINGS * U)
    value = np.maximum((d * d).sum(axis=1), FLT_EPSILON)
    size = np.maximum(np.abs(np.log(value)), 1.0)
    ulp = 2.0 ** (np.floor(np.log2(size)) - 23)
    return (2.0 * d * ed + ed * ed).sum(axis=1) + gamma * ((d + ed) ** 2).sum(axis=1) + value * np.expm1(LOG_ULPS * ulp)


def zero_frames(wav):
    """(T,) bool: the frame's samples are all zero (its log-energy is logf(FLT_EPSILON) exactly)."""
    return ~_frames(wav).any(axis=1)


def error_ratio(E32, wav):
    """max over frames of |exp(got) - max(sumsq64, FLT_EPSILON)| / bound for float32 log-energies E32 (T,) of wav, and where it is; the
    all-zero frames are left out (they are compared exactly).  NaN if got holds one."""
    got = np.exp(np.asarray(E32, dtype=np.float64))
    assert got.shape == (num_frames(len(wav)),)
    if got.size == 0:
        return 0.0, -1
    ratio = np.abs(got - np.maximum(sumsq64(wav), FLT_EPSILON)) / frame_bounds(wav)
    ratio = np.where(zero_frames(wav), 0.0, ratio)
    if np.isnan(ratio).any():
        return float("nan"), -1
    at = int(np.argmax(ratio))
    return float(ratio[at]), at


def log_bound(wav, margin=16.0):
    """(T,) float64: the bound on |E32 - energy64| that the linear bound implies where sumsq64 >= margin * bound, inf elsewhere (a frame
    that cancels to nearly nothing: its log means nothing)."""
    q, b = sumsq64(wav), frame_bounds(wav)
    ok = q >= margin * b
    return np.where(ok, -np.log1p(-np.where(ok, b / np.where(ok, q, 1.0), 0.0)), np.inf)


# ------------------------------------------------------------------------------------ the kernel's arithmetic in float32
_fma32 = logmel_emul._fma32


def emulate32(wav):
    """csrc/vad.hip in float32 numpy -> (T,) float32.  Scaled samples; lane l holds taps l, l + 64, .. l + 384 (below 400) and sums them
    in that order; the 64 lane sums are added as a pairwise tree over the lane index (partners at distance 1, 2, 4, 8, 16, 32); the mean
    is that divided by 400; d = x - mean; per lane q = d0 d0, then q = fma(d_j, d_j, q) in tap order over its taps; the same tree;
    fp32 log of max(., FLT_EPSILON)."""
    wav32 = np.asarray(wav, dtype=np.float32)
    T = num_frames(len(wav32))
    if T == 0:
        return np.zeros(0, dtype=np.float32)
    idx = np.arange(T)[:, None] * HOP + np.arange(FLEN)[None, :]
    x = wav32[idx] * np.float32(WAV_SCALE)
    lanes = np.concatenate([x, np.zeros((T, 448 - FLEN), dtype=np.float32)], axis=1).reshape(T, 7, 64)
    valid = (np.arange(448) < FLEN).reshape(7, 64)

    def tree(v):
        for m in (1, 2, 4, 8, 16, 32):
            v = v + v[:, np.arange(64) ^ m]
        return v[:, 63]

    s = lanes[:, 0]
    for j in range(1, 7):
        s = s + lanes[:, j]
    mean = (tree(s) / np.float32(FLEN)).astype(np.float32)
    d = np.where(valid[None], lanes - mean[:, None, None], np.float32(0.0)).astype(np.float32)
    q = d[:, 0] * d[:, 0]
    for j in range(1, 7):
        q = _fma32(d[:, j], d[:, j], q)
    assert q.dtype == np.float32
    return np.log(np.maximum(tree(q), np.float32(FLT_EPSILON))).astype(np.float32)
