"""Sample-rate conversion, host side (no GPU): the plans, the tables against the float64 definition (tests/resample_ref.py), the definition
against scipy's polyphase filter and against pure tones, the data set's rate handling, the bucket lengths and the streaming plan."""
import math
import wave as wave_module

import numpy as np
import pytest

from tests import resample_ref as RR

# source rate -> (p, q, ntaps); the first seven are the table of the issue that introduced the resampler, the last three follow from the
# same formulas (12000: c = ROLLOFF, W = 68; 24000: c = ROLLOFF 2/3, Z / c = 101.3; 88200: c = ROLLOFF 80/441, Z / c = 372.3)
PLANS = {8000: (1, 2, 137), 11025: (441, 640, 137), 22050: (441, 320, 189), 32000: (2, 1, 273), 44100: (441, 160, 375), 48000: (3, 1, 407),
         96000: (6, 1, 813), 12000: (3, 4, 137), 24000: (3, 2, 205), 88200: (441, 80, 747)}
TONE_RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000)


def test_plans_of_the_ten_rates():
    from asr_chinese_e2e_amd.data_handler import resample as R
    assert set(R.RATES) == set(PLANS)
    for fs, (p, q, ntaps) in PLANS.items():
        pl = R.plan(fs)
        assert (pl.p, pl.q, pl.ntaps, pl.W) == (p, q, ntaps, (ntaps - 1) // 2), fs
        assert RR.plan(fs) == (p, q, pl.W)
        for n in (0, 1, 2, 159, 160, 161, 44100, 80001):
            assert pl.n_out(n) == RR.n_out(n, p, q) == math.ceil(n * q / p) == -(-n * q // p)
    table_kb = {fs: round(R.kernel_table(R.plan(fs)).nbytes / 1024) for fs in (8000, 11025, 22050, 32000, 44100, 48000, 96000)}
    assert table_kb == {8000: 1, 11025: 342, 22050: 236, 32000: 1, 44100: 234, 48000: 2, 96000: 3}
    pl = R.plan(16000)
    assert (pl.p, pl.q, pl.W, pl.n_out(777)) == (1, 1, 0, 777)


@pytest.mark.parametrize("fs", [44056, 7999, 0, -8000, 16000.5, 192000])
def test_unsupported_rates_raise_when_the_plan_is_built(fs):
    from asr_chinese_e2e_amd.data_handler import resample as R
    with pytest.raises(ValueError, match=str(fs).lstrip("-")):
        R.plan(fs)
    with pytest.raises(ValueError):
        R.RateTable([16000, fs])
    if fs in (44056, 7999):
        with pytest.raises(ValueError):
            RR.plan(fs)


def test_more_than_sixteen_plans_raise():
    from asr_chinese_e2e_amd.data_handler import resample as R
    with pytest.raises(ValueError, match="at most 16"):
        R.RateTable([16000 + 1000 * i for i in range(1, 18)])      # 17000 .. 33000: q = 16 each


@pytest.mark.parametrize("fs", [8000, 11025, 22050, 44100, 48000, 96000])
def test_host_table_is_the_reference_table_rounded_once_and_the_kernel_layout_permutes_it(fs):
    from asr_chinese_e2e_amd.data_handler import resample as R
    pl = R.plan(fs)
    H = RR.table(fs).astype(np.float32)
    assert H.shape == (pl.q, pl.ntaps)
    assert np.array_equal(R.phase_table(pl).astype(np.float32), H)
    T = R.kernel_table(pl)
    assert T.shape == (pl.ntaps, pl.q) and T.dtype == np.float32
    n = np.arange(3 * pl.q + 5)
    assert np.array_equal(T[:, n % pl.q], H[(n * pl.p) % pl.q].T)      # T[j][n mod q] = H[(n p) mod q][j]
    assert np.array_equal(np.sort(T.reshape(-1)), np.sort(H.reshape(-1)))
    tab = R.RateTable([16000, fs, 16000])
    assert tab.index(16000) == -1 and tab.index(fs) == 0 and tab.pq.tolist() == [[pl.p, pl.q]] and tab.tap_off.tolist() == [0, T.size]
    assert np.array_equal(tab.taps, T.reshape(-1))


def test_rate_table_of_a_mixed_set():
    from asr_chinese_e2e_amd.data_handler import resample as R
    tab = R.RateTable([48000, 16000, 8000, 48000, 44100])
    assert [pl.fs for pl in tab.plans] == [8000, 44100, 48000] and tab.pq.tolist() == [[1, 2], [441, 160], [3, 1]]
    assert tab.tap_off.tolist() == [0, 274, 274 + 375 * 160, 274 + 375 * 160 + 407] and tab.taps.size == tab.tap_off[-1]
    win, ridx = tab.windows([100, 0, 7, 48001], [48000, 16000, 8000, 44100])
    assert ridx.tolist() == [2, -1, 0, 1]
    assert win.tolist() == [[0, 100, 100, 0, 34], [0, 0, 0, 0, 0], [0, 7, 7, 0, 14], [0, 48001, 48001, 0, 17416]]
    with pytest.raises(ValueError, match="22050"):
        tab.index(22050)
    empty = R.RateTable([16000])
    assert empty.pq.tolist() == [[1, 1]] and empty.tap_off.tolist() == [0, 0] and empty.taps.size == 1


@pytest.mark.parametrize("fs", TONE_RATES)
def test_reference_agrees_with_scipy_upfirdn(fs):
    from scipy.signal import upfirdn
    p, q, W = RR.plan(fs)
    x = np.random.RandomState(fs).uniform(-1, 1, size=700 if q > 100 else 3000)
    y = RR.resample(x, fs)
    hh = RR.h((np.arange(2 * W * q + 1) - W * q) / q, p, q)              # h(m / q), centred
    full = upfirdn(hh, x, up=q)
    lo = -(-W * q // p)                                                    # interior: outputs whose taps all fall inside x
    hi = ((x.size - 1 - W) * q) // p
    n = np.arange(lo, hi)
    assert n.size > 50
    err = float(np.abs(y[n] - full[n * p + W * q]).max())
    print(f"{fs}: max |ref - upfirdn| = {err:.3g} over {n.size} outputs")
    assert err <= 1e-12


@pytest.mark.parametrize("fs", TONE_RATES)
def test_tones_pass_below_the_knee_and_vanish_above_8_khz(fs):
    """Quarter-second tones, the interior = all but 600 outputs at each end: pass-band error <= 1e-6 at 1, 3.4 and 7 kHz (7 kHz only where
    the source can hold it), stop-band amplitude <= 1e-6 at 8.5 and 10 kHz (where the source can hold them).  Measured: 5e-8."""
    k, n = np.arange(fs // 4), np.arange(4000)
    for f in (1000.0, 3400.0, 7000.0, 8500.0, 10000.0):
        if f >= fs / 2:
            continue
        y = RR.resample(np.sin(2 * np.pi * f * k / fs + 0.3), fs)
        assert y.size == 4000
        want = np.sin(2 * np.pi * f * n / 16000.0 + 0.3) if f < 8000 else np.zeros(4000)
        err = float(np.abs(y - want)[600:-600].max())
        print(f"{fs} Hz source, {f:.0f} Hz tone: {'error' if f < 8000 else 'amplitude'} {err:.3g}")
        assert err <= 1e-6, (fs, f, err)


def _write_wav(path, x, fs):
    with wave_module.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(fs)
        f.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_dataset_rates_and_bucket_lengths(tmp_path):
    from asr_chinese_e2e_amd.data_handler import WaveDataset
    from asr_chinese_e2e_amd.data_handler.loader import BatchPlan, source_rates
    rng = np.random.RandomState(0)
    sizes = {48000: 4801, 16000: 1600, 44100: 4410}
    items = []
    for fs, n in sizes.items():
        _write_wav(tmp_path / f"{fs}.wav", rng.uniform(-0.5, 0.5, n), fs)
        items.append((str(tmp_path / f"{fs}.wav"), [5]))
    items.append((rng.randn(800).astype(np.float32), [6], 8000))      # an array carries its rate
    items.append((rng.randn(99).astype(np.float32), [7]))
    off = WaveDataset(items)
    row = np.zeros(5000, dtype=np.float32)
    for call in (lambda: off.wave(0), lambda: off.wave_into(0, row), lambda: off.rate(2), lambda: off.rate(3)):
        with pytest.raises(ValueError, match="sample rate"):
            call()
    assert off.wave(1).size == 1600 and off.rate(1) == 16000 and off.rate(4) == 16000
    ds = WaveDataset(items, resample=True)
    assert [ds.rate(i) for i in range(5)] == [48000, 16000, 44100, 8000, 16000]
    assert [ds.num_samples(i) for i in range(5)] == [4801, 1600, 4410, 800, 99]      # source samples
    assert ds.wave(0).size == 4801 and ds.wave_into(2, row) == 4410 and not row[4410:].any()
    lengths = [ds.num_samples(i) for i in range(5)]
    rates, lengths16 = source_rates(ds, lengths)
    assert rates == [48000, 16000, 44100, 8000, 16000] and lengths16 == [1601, 1600, 1600, 1600, 99]
    plan = BatchPlan(lengths16, 2, shuffle=False)
    assert plan.next_epoch()[1] == [[4, 1], [2, 3], [0]]              # sorted by the RESAMPLED length (then by index)
    assert source_rates(WaveDataset(items[1:2] + items[4:], resample=True), [1600, 99]) == (None, [1600, 99])
    _write_wav(tmp_path / "odd.wav", rng.uniform(-0.5, 0.5, 100), 44056)
    with pytest.raises(ValueError, match="44056"):
        WaveDataset([(str(tmp_path / "odd.wav"), [5])], resample=True).rate(0)


@pytest.mark.parametrize("fs", [8000, 44100, 48000, 11025])
def test_stream_plan_emits_n_out_and_never_needs_a_dropped_sample(fs):
    from asr_chinese_e2e_amd.data_handler import resample as R
    pl = R.plan(fs)
    tail = 2 * pl.W + pl.p
    blocks = [0, 1, pl.W, pl.p, tail + 1, 7, 0, 3 * tail + 11, 1, 1, 0]
    cuts = {"final with the last samples": blocks, "final with an empty block": blocks + [0], "one block": [sum(blocks)], "nothing at all": [0]}
    for name, bl in cuts.items():
        sp = R.StreamPlan(2, fs)
        assert sp.tail == tail
        total, emitted = 0, 0
        for i, n in enumerate(bl):
            last = i == len(bl) - 1
            held_from = total - tail                                    # the row of this call holds [held_from, total + n)
            win = sp.step([n, 0], [last, False])
            in_base, n_avail, n_total, out_start, n_emit = (int(v) for v in win[0])
            total += n
            assert (in_base, n_avail, n_total, out_start) == (held_from, tail + n, total, emitted), name
            if n_emit:
                first, lastn = out_start, out_start + n_emit - 1
                assert (first * pl.p) // pl.q - pl.W >= held_from, name                          # oldest sample needed is still held
                assert last or (lastn * pl.p) // pl.q + pl.W < total, name                       # newest sample needed has arrived
            if not last:                                                                         # nothing that could go is held back
                assert ((out_start + n_emit) * pl.p) // pl.q + pl.W >= total, name
            emitted += n_emit
            assert win[1].tolist() == [-tail, tail, 0, 0, 0]                                     # the idle utterance emits nothing
        assert emitted == pl.n_out(total) == sp.emitted[0], name
        assert sp.closed == [True, False]
        with pytest.raises(ValueError, match="closed"):
            sp.step([1, 0], [False, False])
        assert sp.step([0, 0], [True, False])[0, 4] == 0                                         # closing again, with nothing


def test_resample_entry_point_validates_its_arguments():
    from asr_chinese_e2e_amd import _lib
    assert "asr_resample_fwd" in _lib.SIGNATURES and _lib.ABI_VERSION == 10 == _lib.lib.asr_abi_version()
    ok = (16, 16, 16, 16, 16, 16, 32, 16)
    assert _lib.lib.asr_resample_fwd(16, 16, 0, 16, 16, 16, 32, 16, 1, 8, 8, 1, 1, None) == -1 and "null" in _lib.last_error()
    assert _lib.fast.asr_resample_fwd(*ok, 0, 8, 8, 1, 1, None) == -1 and "B=0" in _lib.last_error()
    assert _lib.fast.asr_resample_fwd(*ok, 1, 8, 0, 1, 1, None) == -1 and "Smax_out=0" in _lib.last_error()
    assert _lib.fast.asr_resample_fwd(*ok, 1, 8, 8, 17, 1, None) == -1 and "R=17" in _lib.last_error()
    assert _lib.fast.asr_resample_fwd(*ok, 1, 8, 8, 1, 0, None) == -1 and "taps_len=0" in _lib.last_error()
