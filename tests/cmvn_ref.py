"""Global CMVN, restated in float64 numpy: the definition the kernels are held to (the reference project has no global CMVN).

Statistics run over every valid log-mel frame of a data set (t < Tb, Tb = 1 + len // 160, nothing for len == 0): per mel bin
mean = sum x / N, var = sum x^2 / N - mean^2 (population variance, WeNet's convention), istd = 1 / sqrt(max(var, 1e-20)).
They are applied as (x - mean[m]) * istd[m] in fp32 - one subtraction, then one multiplication, each correctly rounded - then
SpecAugment (time mask filled with the mean of the utterance's normalised feature, then mel mask filled with the mean of the
time-masked feature) and LFR stacking with src = min(r n + j, Tb - 1), Tl = ceil(Tb / n)."""
import numpy as np

HOP = 160


def total_frames(length):
    return 1 + int(length) // HOP if int(length) > 0 else 0


def accumulate(feat, lens, acc=None):
    """feat (B, Tmax, M), lens (B) samples -> (sum (M), sumsq (M), count), added to acc if given."""
    feat = np.asarray(feat, dtype=np.float64)
    M = feat.shape[2]
    s, q, cnt = (np.zeros(M), np.zeros(M), 0) if acc is None else acc
    s, q = s.copy(), q.copy()
    for b, l in enumerate(lens):
        Tb = min(total_frames(l), feat.shape[1])
        x = feat[b, :Tb]
        s += x.sum(axis=0)
        q += (x * x).sum(axis=0)
        cnt += Tb
    return s, q, cnt


def finalize(s, q, cnt):
    mean = s / cnt
    var = q / cnt - mean * mean
    return mean, 1.0 / np.sqrt(np.maximum(var, 1e-20)), cnt


def normalise(x, mean, istd):
    """fp32: one subtraction, one multiplication (numpy rounds each correctly)."""
    return (np.asarray(x, dtype=np.float32) - np.asarray(mean, dtype=np.float32)) * np.asarray(istd, dtype=np.float32)


def apply(feat, lens, mean, istd, m, n, Tlfr_max, masks=None):
    """-> (out (B, Tlfr_max, m M) float32 with zero padding rows, out_len (B), fills (B, 2) float64 = (time fill, mel fill))."""
    feat = np.asarray(feat, dtype=np.float32)
    B, Tmax, M = feat.shape
    out = np.zeros((B, Tlfr_max, m * M), dtype=np.float32)
    out_len = np.zeros(B, dtype=np.int64)
    fills = np.zeros((B, 2))
    for b, l in enumerate(lens):
        Tb = min(total_frames(l), Tmax)
        if Tb == 0:
            continue
        x = normalise(feat[b, :Tb], mean, istd)
        if masks is not None:
            t0, t1, f0, f1 = (int(v) for v in masks[b])
            t0 = min(max(t0, 0), Tb)
            t1 = min(max(t1, t0), Tb)
            f0 = min(max(f0, 0), M)
            f1 = min(max(f1, f0), M)
            fills[b, 0] = x.astype(np.float64).mean()
            x[t0:t1] = np.float32(fills[b, 0])
            fills[b, 1] = x.astype(np.float64).mean()
            x[:, f0:f1] = np.float32(fills[b, 1])
        Tl = min(-(-Tb // n), Tlfr_max)
        idx = np.minimum(np.arange(Tl)[:, None] * n + np.arange(m)[None, :], Tb - 1)
        out[b, :Tl] = x[idx].reshape(Tl, m * M)
        out_len[b] = Tl
    return out, out_len, fills
