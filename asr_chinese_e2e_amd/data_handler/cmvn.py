"""Global CMVN: one mean and one inverse standard deviation per mel bin, computed once over a corpus and fixed before training
(WeNet's global_cmvn, Kaldi's compute-cmvn-stats over a whole set).  The reference normalises every utterance by its own scalar
mean / std, which needs the whole utterance; these statistics need nothing of the utterance, so the features are causal and the
front end can stream (stream_frontend.py).

The sums are taken on the GPU over the log-mel frames the training front end itself produces (kernels.cmvn_accumulate: float64
accumulators that persist across batches); the three lines of arithmetic that turn them into statistics are here."""
import os

import numpy as np

VAR_FLOOR = 1e-20


def finalize_stats(sum_x, sum_xx, count):
    """Per-bin sums over `count` frames -> (mean, istd, count), float64: population variance sum_xx / N - mean^2 (WeNet's convention),
    floored at 1e-20."""
    count = int(round(float(count)))
    if count <= 0:
        raise ValueError("CMVN statistics over zero frames")
    mean = np.asarray(sum_x, dtype=np.float64) / count
    var = np.asarray(sum_xx, dtype=np.float64) / count - mean * mean
    return mean, 1.0 / np.sqrt(np.maximum(var, VAR_FLOOR)), count


def save_cmvn(path, mean, istd, count):
    """`.npz` with mean, istd (float64, one per mel bin), count (frames) and n_mels."""
    mean, istd = np.asarray(mean, dtype=np.float64), np.asarray(istd, dtype=np.float64)
    if mean.ndim != 1 or mean.shape != istd.shape:
        raise ValueError(f"mean and istd must be vectors of one length, got {mean.shape} and {istd.shape}")
    with open(path, "wb") as f:      # a file object: numpy would append .npz to a bare name
        np.savez(f, mean=mean, istd=istd, count=np.int64(count), n_mels=np.int64(mean.size))


def load_cmvn(path):
    """-> (mean, istd, count) as save_cmvn wrote them."""
    with np.load(os.fspath(path), allow_pickle=False) as z:
        mean, istd, count, n_mels = z["mean"], z["istd"], int(z["count"]), int(z["n_mels"])
    if mean.shape != (n_mels,) or istd.shape != (n_mels,):
        raise ValueError(f"{path}: n_mels = {n_mels} but mean / istd have shapes {mean.shape} / {istd.shape}")
    return mean, istd, count


class CmvnAccumulator:
    """update(wav (B, S) f32 cuda, wav_len (B)) over every batch of a corpus, then finalize() -> (mean, istd, count)."""

    def __init__(self, parser):
        import torch
        self.parser = parser
        self.acc = torch.zeros(2 * parser.n_mels + 1, dtype=torch.float64, device=parser.window.device)

    def update(self, wav, wav_len):
        import torch
        from .. import kernels as K
        wl = wav_len.to(device=wav.device, dtype=torch.int32)
        feat = K.logmel(wav.contiguous(), wl, self.parser.window, self.parser.melfb, 1 + wav.shape[1] // 160)
        K.cmvn_accumulate(feat, wl, self.acc)

    def finalize(self):
        a, n = self.acc.cpu().numpy(), self.parser.n_mels
        return finalize_stats(a[:n], a[n:2 * n], a[2 * n])
