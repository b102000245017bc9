"""The host half of the waveform loader (no GPU, no pinned memory): the one int32 buffer of a batch field by field (loader.MetaLayout,
loader.pack_meta), the launch decisions that follow from it, and the WAV reader load_wav and WaveDataset.wave_into share.  Every expected
value is formed here from resample.plan(fs).n_out, speed.perturbed_len and noise.snr_scale_bits, at offsets counted here."""
import wave as wave_module

import numpy as np
import pytest

from asr_chinese_e2e_amd.data_handler import loader as L
from asr_chinese_e2e_amd.data_handler import noise, resample, speed

PQ = [(9, 10), (1, 1), (11, 10)]
TABLE = resample.RateTable([16000, 48000, 8000, 44100])      # device=None: numpy only; rate indices 8000 -> 0, 44100 -> 1, 48000 -> 2
FILL = -77                                                   # every word of the buffer must be written


def run(sizes, tgt, fs=None, rates=None, aug=None):
    B = len(sizes)
    lay = L.MetaLayout(B, max(1, max(len(t) for t in tgt)), factor=fs is not None, rate=rates is not None, aug=aug is not None)
    meta = np.full(lay.size, FILL, dtype=np.int32)
    return lay, meta, L.pack_meta(lay, meta, sizes, tgt, fs=fs, pq=PQ, rates=rates, rate_table=TABLE, aug=aug)


def expected_words(sizes, tgt, fs, rates, aug):
    """The buffer as a flat list, in the order of the fields: n_samples, tgt_len, tgt, [factor], [rate_idx, win], [rir_idx, noise_par]."""
    lmax = max(1, max(len(t) for t in tgt))
    words = list(sizes) + [len(t) for t in tgt]
    for t in tgt:
        words += list(t) + [0] * (lmax - len(t))
    if fs is not None:
        words += list(fs)
    if rates is not None:
        words += [{16000: -1, 8000: 0, 44100: 1, 48000: 2}[r] for r in rates]
        for n, r in zip(sizes, rates):
            words += [0, n, n, 0, resample.plan(r).n_out(n)]
    if aug is not None:
        nidx, noff, snr, ridx = aug
        words += list(ridx)
        for r in range(len(sizes)):
            words += [nidx[r], noff[r], noise.snr_scale_bits(snr[r]), 0]
    return words


SIZES, TGT = [4800, 14401, 2401], [[], [7], [3, 4, 5]]
FS, RATES = [0, 1, 2], [16000, 48000, 8000]
AUG = ([1, -1, 0], [17, 0, 250], [5.0, 12.5, 20.0], [-1, 0, 1])      # noise index, offset, SNR, response index


def test_all_stages_on():
    lay, meta, m = run(SIZES, TGT, FS, RATES, AUG)
    B, lmax = 3, 3
    assert lay.size == meta.size == 2 * B + B * lmax + B + 6 * B + 5 * B
    assert meta.tolist() == expected_words(SIZES, TGT, FS, RATES, AUG)
    # each field where the list above puts it
    off = {"n_samples": 0, "tgt_len": B, "tgt": 2 * B, "factor": 2 * B + B * lmax, "rate_idx": 3 * B + B * lmax, "win": 4 * B + B * lmax,
           "rir_idx": 9 * B + B * lmax, "noise_par": 10 * B + B * lmax}
    shape = {"n_samples": (B,), "tgt_len": (B,), "tgt": (B, lmax), "factor": (B,), "rate_idx": (B,), "win": (B, 5), "rir_idx": (B,), "noise_par": (B, 4)}
    for name, o in off.items():
        v = lay.field(meta, name)
        assert v.shape == shape[name] and np.shares_memory(v, meta)
        assert v.reshape(-1).tolist() == meta[o:o + v.size].tolist(), name
    assert lay.field(meta, "tgt")[0].tolist() == [0, 0, 0]      # the row of the empty label is all padding
    len16 = [4800, 4801, 4802]
    assert len16 == [resample.plan(r).n_out(n) for n, r in zip(SIZES, RATES)]
    len_out = [speed.perturbed_len(n, *PQ[f]) for n, f in zip(len16, FS)]
    assert list(m.len16) == len16 and list(m.len_out) == len_out and len_out[1] == len16[1]
    assert (m.smax16, m.smax_out, m.any_rir, m.any_noise) == (max(len16), max(len_out), True, True)


def test_lmax_is_at_least_one():
    lay, meta, m = run([10, 20], [[], []])
    assert lay.lmax == 1 and lay.size == 2 * 2 + 2 and meta.tolist() == [10, 20, 0, 0, 0, 0]


@pytest.mark.parametrize("off", ["factor", "rate", "aug", "all"])
def test_a_feature_that_is_off_has_no_words(off):
    fs, rates, aug = (None if off in ("factor", "all") else FS), (None if off in ("rate", "all") else RATES), (None if off in ("aug", "all") else AUG)
    lay, meta, m = run(SIZES, TGT, fs, rates, aug)
    B, lmax = 3, 3
    full = 2 * B + B * lmax + B + 6 * B + 5 * B
    assert lay.size == full - {"factor": B, "rate": 6 * B, "aug": 5 * B, "all": 12 * B}[off]
    if off == "all":
        assert lay.size == 2 * B + B * lmax
    assert meta.tolist() == expected_words(SIZES, TGT, fs, rates, aug)
    for name, group in (("factor", "factor"), ("rate_idx", "rate"), ("win", "rate"), ("rir_idx", "aug"), ("noise_par", "aug")):
        assert (name in lay) == (off not in (group, "all"))
    len16 = [4800, 4801, 4802] if rates is not None else SIZES
    assert list(m.len16) == len16 and m.smax16 == (max(len16) if rates is not None else 0)
    len_out = [speed.perturbed_len(n, *PQ[f]) for n, f in zip(len16, FS)] if fs is not None else len16
    assert list(m.len_out) == len_out and m.smax_out == (max(len_out) if fs is not None else 0)
    assert (m.any_rir, m.any_noise) == ((True, True) if aug is not None else (False, False))


def test_stages_a_batch_does_not_need_are_skipped():
    # all 16 kHz in a mixed-rate table: nothing to convert, yet the fields are written (the kernel is not launched, the layout does not move)
    rates = [16000] * 3
    lay, meta, m = run(SIZES, TGT, FS, rates, AUG)
    assert m.smax16 == 0 and list(m.len16) == SIZES
    assert lay.field(meta, "rate_idx").tolist() == [-1] * 3
    assert lay.field(meta, "win").tolist() == [[0, n, n, 0, n] for n in SIZES]
    assert m.smax_out == max(speed.perturbed_len(n, *PQ[f]) for n, f in zip(SIZES, FS))      # the speed lengths: on the unconverted ones
    # every factor with p == q
    lay, meta, m = run(SIZES, TGT, [1, 1, 1], RATES, AUG)
    assert m.smax_out == 0 and list(m.len_out) == list(m.len16) == [4800, 4801, 4802] and lay.field(meta, "factor").tolist() == [1, 1, 1]
    # every drawn index -1
    none = ([-1] * 3, [0] * 3, [5.0, 6.0, 7.0], [-1] * 3)
    lay, meta, m = run(SIZES, TGT, FS, RATES, none)
    assert (m.any_rir, m.any_noise) == (False, False)
    assert meta.tolist() == expected_words(SIZES, TGT, FS, RATES, none)
    only_noise = ([-1, 0, -1], [0, 3, 0], [5.0, 6.0, 7.0], [-1] * 3)
    assert run(SIZES, TGT, FS, RATES, only_noise)[2][4:] == (False, True)


def test_one_zero_length_utterance():
    aug = ([0], [0], [10.0], [0])
    m = run([0], [[1]], [0], [48000], aug)[2]
    assert (m.smax16, m.smax_out, list(m.len16), list(m.len_out)) == (1, 1, [0], [0])      # max(1, ...): a row is never 0 wide
    m = run([0], [[1]], [1], [16000], aug)[2]
    assert (m.smax16, m.smax_out) == (0, 0)                                                # ... but only where the stage runs
    m = run([0], [[1]], [2], [16000], aug)[2]
    assert (m.smax16, m.smax_out) == (0, 1)
    m = run([0], [[1]], [1], [8000], aug)[2]
    assert (m.smax16, m.smax_out) == (1, 0)
    assert run([0], [[1]])[2] == ([0], [0], 0, 0, False, False)


def test_load_wav_and_wave_into_share_one_reader(tmp_path):
    rng = np.random.RandomState(3)
    pcm = (rng.randn(1501, 2) * 9000).astype("<i2")

    def write(name, data, ch, cut=0):
        path = str(tmp_path / name)
        with wave_module.open(path, "wb") as f:
            f.setnchannels(ch); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes(data.tobytes())
        if cut:      # the header keeps its frame count, the data chunk loses `cut` bytes
            raw = open(path, "rb").read()
            open(path, "wb").write(raw[:-cut])
        return path

    cases = [(write("mono.wav", pcm[:, 0], 1), pcm[:, 0].astype(np.float32) / np.float32(32768.0)),
             (write("stereo.wav", pcm, 2), (pcm.astype(np.float32) / np.float32(32768.0)).mean(axis=1)),
             (write("short.wav", pcm[:, 0], 1, cut=1000), pcm[:1001, 0].astype(np.float32) / np.float32(32768.0))]
    ds = L.WaveDataset([(p, [1]) for p, _ in cases])
    for i, (path, want) in enumerate(cases):
        got, sr = L.load_wav(path)
        assert sr == 16000 and got.dtype == np.float32 and np.array_equal(got, want)
        row = np.full(ds.num_samples(i) + 5, 7.0, dtype=np.float32)      # num_samples: what the header says (1501)
        n = ds.wave_into(i, row)
        assert n == want.size and np.array_equal(row[:n], got) and not row[n:].any()
        assert np.array_equal(ds.wave(i), got)
    small = np.full(700, 7.0, dtype=np.float32)                          # never more than the row
    assert ds.wave_into(1, small) == 700 and np.array_equal(small, cases[1][1][:700])
    path = str(tmp_path / "wide.wav")
    with wave_module.open(path, "wb") as f:
        f.setnchannels(1); f.setsampwidth(1); f.setframerate(16000)
        f.writeframes(b"\x01" * 64)
    with pytest.raises(ValueError, match="16-bit"):
        L.load_wav(path)
    with pytest.raises(ValueError, match="16-bit"):
        L.WaveDataset([(path, [1])]).wave_into(0, small)
