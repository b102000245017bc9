"""Global CMVN: one mean and one inverse standard deviation per mel bin, computed once over a corpus and fixed before training
(WeNet's global_cmvn, Kaldi's compute-cmvn-stats over a whole set).  The reference normalises every utterance by its own scalar
mean / std, which needs the whole utterance; these statistics need nothing of the utterance, so the features are causal and the
front end can stream (stream_frontend.py).

The sums are taken on the GPU over the log-mel frames the training front end itself produces (kernels.cmvn_accumulate: float64
accumulators that persist across batches); the three lines of arithmetic that turn them into statistics are here."""
import json
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


def save_cmvn(path, mean, istd, count, frontend="reference"):
    """`.npz` with mean, istd (float64, one per mel bin), count (frames) and n_mels, and for any front end but "reference" a `frontend`
    key naming the one whose features they describe (a file without the key is "reference": the files written before the key existed)."""
    mean, istd = np.asarray(mean, dtype=np.float64), np.asarray(istd, dtype=np.float64)
    if mean.ndim != 1 or mean.shape != istd.shape:
        raise ValueError(f"mean and istd must be vectors of one length, got {mean.shape} and {istd.shape}")
    with open(path, "wb") as f:      # a file object: numpy would append .npz to a bare name
        extra = {} if frontend == "reference" else {"frontend": np.array(str(frontend))}
        np.savez(f, mean=mean, istd=istd, count=np.int64(count), n_mels=np.int64(mean.size), **extra)


def save_wenet_cmvn(path, sum_x, sum_xx, count):
    """WeNet's global_cmvn JSON: the raw sums ({"mean_stat", "var_stat", "frame_num"}), which finalize_stats turns into statistics."""
    with open(path, "w") as f:
        json.dump({"mean_stat": [float(v) for v in sum_x], "var_stat": [float(v) for v in sum_xx], "frame_num": int(round(float(count)))}, f)


def _from_sums(path, sum_x, sum_xx, count):
    sum_x, sum_xx = np.asarray(sum_x, dtype=np.float64), np.asarray(sum_xx, dtype=np.float64)
    if sum_x.ndim != 1 or sum_x.shape != sum_xx.shape or sum_x.size == 0:
        raise ValueError(f"{path}: sums and sums of squares have shapes {sum_x.shape} / {sum_xx.shape}")
    return finalize_stats(sum_x, sum_xx, count) + ("kaldi",)


def load_cmvn_meta(path):
    """-> (mean, istd, count, frontend).  Three formats, told apart by content: the `.npz` save_cmvn wrote (without a `frontend` key:
    "reference"); WeNet's JSON {"mean_stat", "var_stat", "frame_num"}; Kaldi's text matrix `[ sums count \n sums-of-squares 0 ]` of
    compute-cmvn-stats.  The last two hold raw sums, go through finalize_stats and describe Kaldi fbank features."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        head = f.read(2)
    if head == b"PK":      # an .npz is a zip archive
        with np.load(path, allow_pickle=False) as z:
            mean, istd, count, n_mels = z["mean"], z["istd"], int(z["count"]), int(z["n_mels"])
            frontend = str(z["frontend"]) if "frontend" in z.files else "reference"
        if mean.shape != (n_mels,) or istd.shape != (n_mels,):
            raise ValueError(f"{path}: n_mels = {n_mels} but mean / istd have shapes {mean.shape} / {istd.shape}")
        return mean, istd, count, frontend
    neither = f"{path}: neither an .npz of save_cmvn, WeNet's CMVN JSON nor Kaldi's text CMVN matrix"
    try:
        with open(path, "r", encoding="utf-8") as f:
            text = f.read()
    except UnicodeDecodeError:
        raise ValueError(neither) from None
    if text.lstrip().startswith("{"):
        try:
            d = json.loads(text)
            stats = d["mean_stat"], d["var_stat"], d["frame_num"]
        except (ValueError, KeyError, TypeError) as e:
            raise ValueError(f"{path}: not WeNet's CMVN JSON (mean_stat, var_stat, frame_num): {e!r}") from None
        return _from_sums(path, *stats)
    if text.count("[") > 1 or text.count("]") > 1:
        raise ValueError(f"{path}: more than one matrix: give one entry of the archive (copy-matrix --binary=false of a single key)")
    if "[" in text and "]" in text:
        rows = [r.split() for r in text[text.index("[") + 1:text.rindex("]")].strip().splitlines() if r.strip()]
        if len(rows) != 2 or len(rows[0]) != len(rows[1]) or len(rows[0]) < 2:
            raise ValueError(f"{path}: a Kaldi CMVN matrix has two rows of n_mels + 1 numbers, got {[len(r) for r in rows]}")
        m = np.array(rows, dtype=np.float64)
        return _from_sums(path, m[0, :-1], m[1, :-1], m[0, -1])
    raise ValueError(neither)


def load_cmvn(path):
    """-> (mean, istd, count) of a statistics file (load_cmvn_meta also tells the front end)."""
    return load_cmvn_meta(path)[:3]


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
        S, Tmax = wav.shape[1], self.parser.max_frames(wav.shape[1])
        feat = self.parser.features(wav.contiguous(), wl, Tmax)
        K.cmvn_accumulate(feat, self.parser.norm_lengths(wl, S, Tmax), self.acc)

    def sums(self):
        """-> (sum x, sum x^2, frames) as accumulated so far (what WeNet's JSON and Kaldi's matrix hold)."""
        a, n = self.acc.cpu().numpy(), self.parser.n_mels
        return a[:n], a[n:2 * n], a[2 * n]

    def finalize(self):
        return finalize_stats(*self.sums())
