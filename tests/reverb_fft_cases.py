"""The ragged batch the FFT reverberation path is tested on, with its float64 reference, its error scale and the float32 yardstick, built
once per process (tests/test_reverb_fft_cpu.py checks the yardstick, tests/test_reverb_fft_gpu.py holds the kernel to it).

Response lengths 1, 2, Bk - 1, Bk, Bk + 1, 2 Bk + 1 and 65536 (one, two, three and 32 partitions, a last partition of one tap), each with
its peak at 0, L // 2 and L - 1, against utterance lengths 0, 1, Bk - 1, Bk, Bk + 1 and 2 Bk + 3; four out-of-range indices and a 5-sample
row.  Inputs as in tests/test_noise_reverb_gpu.py: x ~ U(-1, 1), h decaying Gaussian noise of unit energy, NaN in the table beyond each
response's length."""
import functools

import numpy as np

from tests import noise_ref as NR
from tests import reverb_fft_ref as FR

BK = FR.BK
LENGTHS = (1, 2, BK - 1, BK, BK + 1, 2 * BK + 1, 65536)
UTTERANCES = (0, 1, BK - 1, BK, BK + 1, 2 * BK + 3)


def response(rng, L):
    h = rng.randn(L) * np.exp(-np.arange(L) / max(L / 4.0, 1.0))
    return (h / np.sqrt(np.sum(h * h))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases(lengths=LENGTHS, width=None):
    """-> dict: resp [(L, p)], table (R, width) f32 with NaN beyond each L, rows, idx, ref [(y, S) float64 or None per row], c_ref (the
    float32 restatement's largest |error| / (2^-24 S_i) over the rows) and c_ref_by_len {L: ...}."""
    rng = np.random.RandomState(0)
    resp = [(L, p) for L in lengths for p in sorted({0, L // 2, L - 1})]
    R = len(resp)
    table = np.full((R, width or max(lengths)), np.nan, dtype=np.float32)
    for r, (L, p) in enumerate(resp):
        table[r, :L] = response(rng, L)
    rows, idx = [], []
    for r in range(R):
        for n in UTTERANCES:
            rows.append(rng.uniform(-1.0, 1.0, size=n).astype(np.float32))
            idx.append(r)
    for bad in (-1, R, -7, R + 100):
        rows.append(rng.uniform(-1.0, 1.0, size=2 * BK + 3).astype(np.float32))
        idx.append(bad)
    rows.append(rng.uniform(-1.0, 1.0, size=5).astype(np.float32))
    idx.append(-1)
    ref, by_len = [], {}
    for x, r in zip(rows, idx):
        if not 0 <= r < R:
            ref.append(None)
            continue
        L, p = resp[r]
        h = table[r, :L]
        y, S = NR.reverb(x, h, p)[0], FR.block_scale(x, h, p)
        ref.append((y, S))
        by_len[L] = max(by_len.get(L, 0.0), FR.worst_ratio(FR.reverb_fft_f32(x, h, p), y, S))
    return dict(resp=resp, table=table, rows=rows, idx=idx, ref=ref, c_ref=max(by_len.values()), c_ref_by_len=by_len)
