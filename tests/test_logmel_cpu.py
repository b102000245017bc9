"""The log-mel reference side without a GPU (tests/logmel_emul.py): the framing rule against np.pad, its frame count and index range
at short lengths, and the a-priori fp32 bound against a float32 restatement of the kernel's arithmetic."""
import numpy as np
import pytest

from oracle import logmel_ref as LM
from tests import logmel_emul as E


@pytest.mark.parametrize("length", [201, 202, 359, 360, 400, 4001, 8000])
def test_framing_rule_is_reflect_padding(length):
    wav = np.random.RandomState(length).randn(length)
    x = np.pad(wav, (200, 200), mode="reflect")
    T = LM.num_frames(length)
    ref = x[np.arange(T)[:, None] * 160 + np.arange(400)[None, :]]
    got = E.frames(wav)
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    # and so the float64 mel energies are the oracle's
    for n_mels in (40, 80):
        assert np.array_equal(np.log(E.mel_power64(wav, n_mels) + LM.LOG_FLOOR), LM.log_mel(wav, n_mels))


@pytest.mark.parametrize("length", [1, 2, 150, 200, 201])
def test_framing_rule_at_short_lengths(length):
    idx = E.frame_index(length)
    assert idx.shape == (1 + length // 160, 400)
    assert idx.min() >= 0 and idx.max() <= length - 1
    # the taps that need no rule read their own sample
    t, n = np.meshgrid(np.arange(idx.shape[0]), np.arange(400), indexing="ij")
    raw = 160 * t - 200 + n
    inside = (raw >= 0) & (raw < length)
    assert np.array_equal(idx[inside], raw[inside])
    # one reflection where one suffices, the clamp only past it
    left = (raw < 0) & (-raw < length)
    assert np.array_equal(idx[left], -raw[left])
    right = (raw >= length) & (2 * (length - 1) - raw >= 0)
    assert np.array_equal(idx[right], (2 * (length - 1) - raw)[right])
    # past a second reflection the rule clamps (np.pad would go on reflecting back and forth: no library rule is followed there)
    twice = (raw >= length) & (2 * (length - 1) - raw < 0)
    assert np.all(idx[twice] == 0) and twice.any() == (length < 100)


@pytest.mark.parametrize("n_mels", [40, 80])
def test_emulation_stays_within_the_bound(n_mels):
    """fp32 arithmetic as such keeps the bound on every signal of the GPU accuracy test, with room to spare (the GPU test allows the
    kernel four times the emulation's ratio, so the ratio here must stay below a quarter)."""
    for name, wav in E.signals().items():
        y = E.emulate32(wav, n_mels)
        ratio, at = E.error_ratio(y, wav, n_mels)
        floor = E.floor_cells(wav, n_mels)
        print(f"n_mels {n_mels:3d}  {name:24s} emulation err/bound {ratio:.3e} at {at}  floor cells {int(floor.sum())}")
        assert y.dtype == np.float32 and y.shape == (51, n_mels)
        assert ratio <= 0.25, (name, ratio)
        assert np.all(y[floor] == E.LOG_FLOOR32), name
    assert E.floor_cells(E.signals()["impulse"], n_mels).any() and not E.floor_cells(E.signals()["noise 0.1"], n_mels).any()


def test_bound_scales_with_the_signal():
    """The bound is a relative one: k times the signal, k^2 times the bound (away from the floor), so neither loud nor faint
    audio escapes it."""
    wav = E.signals()["noise 0.1"].astype(np.float64)
    assert np.allclose(E.bound(8.0 * wav, 80), 64.0 * E.bound(wav, 80), rtol=1e-9, atol=0)
    assert np.all(E.bound(np.zeros(3000), 80) == E.REL * LM.LOG_FLOOR) and E.floor_cells(np.zeros(3000), 80).all()
