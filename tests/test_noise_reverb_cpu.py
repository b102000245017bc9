"""Noise and reverberation augmentation, host side (no GPU): the per-epoch draws, the bank tables, the float64 reference
(tests/noise_ref.py) against known answers, the header, and the argument validation of the new entry points."""
import os
import random
import re

import numpy as np
import pytest

from tests import noise_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _draw(seed=3, epoch=0, n=300, **kw):
    from asr_chinese_e2e_amd.data_handler import noise
    args = dict(noise_prob=0.5, n_noise=3, noise_lens=[1, 7, 16000], snr_db=(5, 20), rir_prob=0.5, n_rir=4)
    args.update(kw)
    return noise.draw_augment(seed, epoch, n, **args)


def test_draws_are_a_pure_function_of_seed_epoch_and_index():
    a, b = _draw(), _draw()
    assert a == b
    nidx, noff, snr, ridx = a
    assert set(nidx) == {-1, 0, 1, 2} and set(ridx) == {-1, 0, 1, 2, 3}
    assert all(0 <= o < [1, 7, 16000][j] for j, o in zip(nidx, noff) if j >= 0) and max(noff) > 7
    assert all(5.0 <= s <= 20.0 for s in snr) and max(snr) - min(snr) > 10
    assert _draw(epoch=1) != a and _draw(seed=4) != a                       # epochs and seeds differ
    assert all(x[:120] == y for x, y in zip(a, _draw(n=120)))                # index order: utterance i does not depend on the data set's size
    assert 0.35 < sum(j >= 0 for j in nidx) / 300 < 0.65 and 0.35 < sum(r >= 0 for r in ridx) / 300 < 0.65


def test_probability_zero_and_one():
    nidx, _, _, ridx = _draw(noise_prob=0.0, rir_prob=0.0)
    assert set(nidx) == {-1} and set(ridx) == {-1}
    nidx, _, _, ridx = _draw(noise_prob=1.0, rir_prob=1.0)
    assert -1 not in nidx and -1 not in ridx
    nidx, noff, _, ridx = _draw(noise_prob=1.0, rir_prob=1.0, n_noise=0, noise_lens=(), n_rir=0)      # no banks: nothing to draw from
    assert set(nidx) == {-1} and set(ridx) == {-1} and set(noff) == {0}


def test_draws_leave_the_speed_draws_and_the_batch_plan_alone():
    from asr_chinese_e2e_amd.data_handler import BatchPlan, speed
    lengths = [4800 + 331 * ((7 * i) % 23) for i in range(50)]
    mk = lambda: BatchPlan(lengths, 4, bucket_size=16, shuffle=True, seed=3, speed_pq=((9, 10), (1, 1), (11, 10)))
    off, on = mk(), mk()
    state = random.getstate()
    for epoch in range(3):
        want = off.next_epoch()
        _draw(seed=3, epoch=on.epoch, n=len(lengths))
        got = on.next_epoch()
        _draw(seed=3, epoch=epoch, n=len(lengths))
        assert got == want and got[2] == speed.draw_factors(3, epoch, len(lengths), 3)
    assert on.rng.random() == off.rng.random()
    assert random.getstate() == state                                       # nor the global generator


def test_rir_table_peak_window_and_energy():
    from asr_chinese_e2e_amd.data_handler import noise
    rng = np.random.RandomState(0)
    h0 = rng.randn(300) * np.exp(-np.arange(300) / 40.0)
    h0[100] = 9.0                                                           # peak at 100: the window starts at 36
    h1 = rng.randn(20000) * 0.01
    h1[10] = -5.0                                                           # peak in front of sample 64: s0 = 0; truncated to max_taps
    h2 = np.array([0.0, 0.0, 2.0])
    table, lens, peaks = noise.rir_table([h0, h1, h2], max_taps=8192)
    assert table.dtype == np.float32 and table.shape == (3, 8192) and lens.tolist() == [264, 8192, 3] and peaks.tolist() == [64, 10, 2]
    for i, h in enumerate((h0, h1, h2)):
        want, p = NR.rir_prepare(h, 8192)
        assert p == peaks[i] and np.array_equal(table[i, :lens[i]], want.astype(np.float32)) and not table[i, lens[i]:].any()
        assert abs(float(np.sum(table[i].astype(np.float64) ** 2)) - 1.0) < 1e-5       # unit energy AFTER the truncation, rounded once
        assert int(np.argmax(np.abs(table[i]))) == peaks[i]
    assert np.array_equal(table[0, :264], (h0[36:] / np.sqrt(np.sum(h0[36:] ** 2))).astype(np.float32))
    t2, l2, p2 = noise.rir_table([h1], max_taps=100)
    assert t2.shape == (1, 100) and l2.tolist() == [100] and p2.tolist() == [10] and abs(float(np.sum(t2.astype(np.float64) ** 2)) - 1.0) < 1e-6
    bank = noise.RirBank([h0, h2], device="cpu")                            # the bank is the table on a device
    assert len(bank) == 2 and np.array_equal(bank.table.numpy(), table[[0, 2], :264]) and bank.lens.tolist() == [264, 3] and bank.peaks.tolist() == [64, 2]


def test_banks_refuse_empty_and_silent_input(tmp_path):
    import wave
    from asr_chinese_e2e_amd.data_handler import noise
    for bad in ([], [np.zeros(0)], [np.ones(4), np.zeros(9)]):
        with pytest.raises(ValueError):
            noise.RirBank(bad, device="cpu")
        with pytest.raises(ValueError):
            noise.NoiseBank(bad, device="cpu")
    with pytest.raises(ValueError, match="clip 1"):
        noise.NoiseBank([np.ones(4), np.zeros(9)], device="cpu")
    with pytest.raises(ValueError):
        noise.rir_table([np.ones(3)], max_taps=8193)

    def write(name, pcm, rate):
        path = str(tmp_path / name)
        with wave.open(path, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes(np.asarray(pcm, dtype="<i2").tobytes())
        return path
    good, slow, silent = write("a.wav", [100, -200, 300], 16000), write("b8k.wav", [1, 2, 3], 8000), write("silent.wav", [0, 0, 0, 0], 16000)
    for cls in (noise.NoiseBank, noise.RirBank):
        with pytest.raises(ValueError, match="b8k.wav"):
            cls([good, slow], device="cpu")
        with pytest.raises(ValueError, match="silent.wav"):
            cls([good, silent], device="cpu")
    bank = noise.NoiseBank([good, np.arange(1, 6)], device="cpu")
    assert bank.lens == [3, 5] and bank.noise_off.tolist() == [0, 3, 8] and bank.noise.dtype.is_floating_point
    assert np.array_equal(bank.noise.numpy(), np.concatenate([np.array([100, -200, 300], dtype=np.float32) / 32768.0, np.arange(1, 6, dtype=np.float32)]))
    # max_seconds: clips are added until that much noise is held
    sec = np.ones(16000, dtype=np.float32)
    assert noise.NoiseBank([sec, sec, sec, sec], device="cpu", max_seconds=2).lens == [16000, 16000]


def test_reference_reverb_known_answers():
    rng = np.random.RandomState(1)
    x = rng.randn(50)
    y, A = NR.reverb(x, [1.0], 0)                                            # a one-tap response is the identity
    assert np.array_equal(y, x) and np.array_equal(A, np.abs(x))
    h = rng.randn(7)
    for p in (0, 3, 6):
        y, A = NR.reverb(x, h, p)
        brute = np.array([sum(h[k] * x[n + p - k] for k in range(7) if 0 <= n + p - k < 50) for n in range(50)])
        bruteA = np.array([sum(abs(h[k] * x[n + p - k]) for k in range(7) if 0 <= n + p - k < 50) for n in range(50)])
        assert y.shape == (50,) and np.allclose(y, brute, rtol=0, atol=1e-13) and np.allclose(A, bruteA, rtol=0, atol=1e-13)
    d = np.zeros(9)
    d[4] = 2.0                                                              # a delayed, scaled delta at the peak: the direct path stays aligned
    assert np.array_equal(NR.reverb(x, d, 4)[0], 2.0 * x)
    y, _ = NR.reverb(x[:3], rng.randn(40), 20)                              # a response longer than the utterance
    assert y.shape == (3,)
    assert NR.reverb(np.zeros(0), h, 0)[0].size == 0


def test_reference_mix_attains_the_requested_snr():
    rng = np.random.RandomState(2)
    x = rng.randn(1000) * 0.1
    for clip, o in ((rng.randn(7), 6), (rng.randn(5000), 4999), (np.array([0.3]), 0)):
        for snr in (5.0, 12.5, 20.0, -3.0):
            out, g, v = NR.mix(x, clip, o, 10.0 ** (-snr / 20.0))
            assert abs(NR.snr_db(x, out - x) - snr) < 1e-12 and abs(NR.snr_db(x, g * v) - snr) < 1e-12
            assert np.array_equal(v, np.array([clip[(o + n) % len(clip)] for n in range(1000)]))
    for xs, clip in ((np.zeros(10), rng.randn(4)), (x[:10], np.zeros(4)), (np.zeros(0), rng.randn(4))):       # nothing to scale by: a copy, gain 0
        out, g, _ = NR.mix(xs, clip, 0, 0.1)
        assert g == 0.0 and np.array_equal(out, xs)


def test_header_declares_the_new_entry_points():
    from asr_chinese_e2e_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    for name in ("asr_reverb_fwd", "asr_noise_mix_fwd", "asr_noise_mix_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", text) and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    const = lambda n: int(re.search(r"#define\s+" + n + r"\s+(\d+)", text).group(1))
    assert const("ASR_REVERB_TILE") == _lib.REVERB_TILE == kernels.REVERB_TILE
    assert const("ASR_REVERB_CHUNK") == _lib.REVERB_CHUNK == kernels.REVERB_CHUNK
    assert const("ASR_REVERB_MAX_TAPS") == _lib.REVERB_MAX_TAPS == kernels.REVERB_MAX_TAPS == 8192
    assert const("ASR_NOISE_MIX_TILE") == _lib.NOISE_MIX_TILE == kernels.NOISE_MIX_TILE
    assert _lib.lib.asr_abi_version() == 10


def test_noise_reverb_error_reporting_without_gpu():
    """Argument validation happens on the host before any launch: callable without a GPU."""
    from asr_chinese_e2e_amd import _lib
    f = _lib.lib.asr_reverb_fwd
    assert f(None, None, None, None, None, None, None, 1, 8, 1, 8, None) == -1 and "null pointer" in _lib.last_error()
    ok = (16, 16, 16, 16, 16, 16, 32)      # non-null, never dereferenced: every call below is refused before a launch
    assert f(*ok, 0, 8, 1, 8, None) == -1 and "B=0" in _lib.last_error()
    assert f(*ok, 1, 0, 1, 8, None) == -1 and "Smax=0" in _lib.last_error()
    assert f(*ok, 1, 8, 0, 8, None) == -1 and "R=0" in _lib.last_error()
    assert f(*ok, 1, 8, 1, 0, None) == -1 and "Lcap=0" in _lib.last_error()
    assert f(*ok, 1, 8, 1, 8193, None) == -1 and "Lcap=8193" in _lib.last_error()
    assert f(16, 16, 16, 16, 16, 16, 16, 1, 8, 1, 8, None) == -1 and "alias" in _lib.last_error()
    assert _lib.fast.asr_reverb_fwd(*ok, 1, 8, 1, 8193, None) == -1 and "Lcap=8193" in _lib.last_error()
    g, wsb = _lib.lib.asr_noise_mix_fwd, _lib.lib.asr_noise_mix_workspace_bytes
    T = _lib.NOISE_MIX_TILE
    assert wsb(32, 80000) == 32 * -(-80000 // T) * 16 == _lib.fast.asr_noise_mix_workspace_bytes(32, 80000)
    assert wsb(1, T) == 16 and wsb(1, T + 1) == 32 and wsb(0, 8) == 0
    assert g(None, None, None, None, None, None, None, None, 0, 1, 8, 1, None) == -1 and "null pointer" in _lib.last_error()
    okm = (16, 16, 16, 16, 16, 16, None, 64)      # gain_out may be NULL
    assert g(*okm, 16, 0, 8, 1, None) == -1 and "B=0" in _lib.last_error()
    assert g(*okm, 16, 1, 0, 1, None) == -1 and "Smax=0" in _lib.last_error()
    assert g(*okm, 16, 1, 8, 0, None) == -1 and "N=0" in _lib.last_error()
    assert g(*okm, 15, 1, 8, 1, None) == -3 and "workspace 15 < 16" in _lib.last_error()
    assert g(16, 16, 16, 16, 16, 16, None, 12, 16, 1, 8, 1, None) == -1 and "aligned" in _lib.last_error()
    assert _lib.fast.asr_noise_mix_fwd(*okm, 15, 1, 8, 1, None) == -3 and "workspace" in _lib.last_error()


def test_train_flags_reach_the_train_part_only(tmp_path):
    import train
    lst = tmp_path / "noise.lst"
    lst.write_text("a.wav\n\n b.wav \n")
    flags = train.parse_flags([f"--noise_list={lst}", "--snr_db=5,20", "--noise_prob=0.7", "--rir_prob=1"])
    assert train.path_list(flags["noise_list"]) == ["a.wav", "b.wav"] and train.path_list(train.TrainConfig.rir_list) is None
    assert train.snr_range(flags["snr_db"]) == (5.0, 20.0) == train.snr_range(train.TrainConfig.snr_db) and train.snr_range(10) == (10.0, 10.0)
    assert float(flags["noise_prob"]) == 0.7 and float(flags["rir_prob"]) == 1.0
    with pytest.raises(ValueError):
        train.snr_range("20,5")
    src = open(os.path.join(ROOT, "train.py")).read()
    assert src.count("noise=path_list(config.noise_list)") == 1 and src.count("rir=path_list(config.rir_list)") == 1
    test_dev = [l for l in src.splitlines() if re.search(r'part="(test|dev)"', l)]
    assert test_dev and not any("noise" in l or "rir" in l for l in test_dev)
    import inspect
    from asr_chinese_e2e_amd.data_handler import loader
    body = inspect.getsource(loader.build_dataloader)
    assert 'if part == "train" else {}' in body
