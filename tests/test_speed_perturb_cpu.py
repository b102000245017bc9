"""Speed perturbation, host side (no GPU): the length formula, factor parsing, the phase tables, the float64 reference
(tests/speed_ref.py) against a known answer, the per-epoch draws and batch lists, and the entry point's argument validation."""
import os
import random
import re

import numpy as np
import pytest

from tests import speed_ref as SR
from tests.helpers import ROOT


def test_perturbed_len_is_the_count_of_output_positions_inside_the_utterance():
    from asr_chinese_e2e_amd.data_handler import speed
    for p in range(1, 13):
        for q in range(1, 13):
            for n_in in range(51):
                brute = sum(1 for n in range(n_in * q + 2) if n * p < n_in * q)
                assert speed.perturbed_len(n_in, p, q) == brute == SR.n_out(n_in, p, q), (n_in, p, q)


def test_factor_parsing():
    from asr_chinese_e2e_amd.data_handler import speed
    assert speed.parse_factor(0.9) == (9, 10) == SR.factor(0.9)
    assert speed.parse_factor(1.1) == (11, 10) == SR.factor(1.1)
    assert speed.parse_factor(1) == (1, 1) and speed.parse_factor(1.0) == (1, 1)
    assert speed.parse_factor("0.95") == (19, 20)
    for bad in (0.123, 3.7, 0, -0.9, "fast", 21):
        with pytest.raises(ValueError):
            speed.parse_factor(bad)
    with pytest.raises(ValueError):
        speed.build_tables(())


def test_phase_tables():
    from asr_chinese_e2e_amd.data_handler import speed
    for s, (lo, hi) in ((0.9, (1.00004, 1.00088)), (1.1, (1.00032, 1.00062))):
        p, q = speed.parse_factor(s)
        H = speed.phase_table(p, q)
        assert speed.half_width(p, q) == 7 == SR.half_width(p, q) and H.shape == (q, 15)
        assert np.array_equal(H, SR.table(p, q)) or np.allclose(H, SR.table(p, q), rtol=0, atol=1e-15)
        dc = H.sum(axis=1)
        assert np.all(np.abs(dc - 1.0) < 1e-3), dc
        assert abs(dc.min() - lo) < 1e-5 and abs(dc.max() - hi) < 1e-5, (dc.min(), dc.max())      # the figures of the definition
        for r in range(1, q):      # h is even: phase r read backwards is phase q - r one sample on
            assert np.allclose(H[r][1:], H[q - r][::-1][:-1], rtol=0, atol=1e-15), r
        assert np.allclose(H[0], H[0][::-1], rtol=0, atol=1e-15)
    pq, taps = speed.build_tables((0.9, 1.0, 1.1, "0.95"))
    assert pq.dtype == np.int32 and pq.tolist() == [[9, 10], [1, 1], [11, 10], [19, 20]]
    assert taps.dtype == np.float32 and taps.shape == (4, 20, 15)
    assert np.array_equal(taps[0, :10], speed.phase_table(9, 10).astype(np.float32)) and not taps[0, 10:].any() and not taps[1].any()
    # a wider filter in the same set: the narrower ones are centred in the common width
    pq2, taps2 = speed.build_tables((0.9, 2))
    W2 = speed.half_width(2, 1)
    assert W2 == 13 and taps2.shape == (2, 10, 27)
    assert np.array_equal(taps2[0, :, W2 - 7:W2 + 8], taps[0, :10]) and not taps2[0, :, :W2 - 7].any() and not taps2[0, :, W2 + 8:].any()


def test_reference_resamples_a_sine_to_the_scaled_frequency():
    n = np.arange(8000)
    x = np.sin(2 * np.pi * 440.0 * n / 16000.0)
    for s, measured in ((0.9, 4.4e-4), (1.1, 2.7e-4)):
        p, q = SR.factor(s)
        y = SR.perturb(x, p, q)
        assert y.size == SR.n_out(8000, p, q)
        want = np.sin(2 * np.pi * 440.0 * (p / q) * np.arange(y.size) / 16000.0)
        err = np.abs(y - want)[50:-50].max()
        print(f"speed {p}/{q}: max |y - sine| = {err:.3g}")
        assert err < 1e-3 and abs(err - measured) < 0.1e-4
    assert np.array_equal(SR.perturb(x, 1, 1), x)
    assert SR.perturb(np.zeros(0), 9, 10).size == 0


def test_reference_direct_sum_equals_its_polyphase_form():
    rng = np.random.RandomState(0)
    x = rng.randn(97)
    for p, q in ((9, 10), (11, 10), (19, 20), (2, 1), (1, 2)):
        H, W = SR.table(p, q), SR.half_width(p, q)
        xp = np.concatenate([np.zeros(W), x, np.zeros(W + 2 * p)])
        y = SR.perturb(x, p, q)
        poly = np.array([xp[(n * p) // q:(n * p) // q + 2 * W + 1] @ H[(n * p) % q] for n in range(y.size)])
        assert np.allclose(y, poly, rtol=0, atol=1e-13)


def _plan(seed=3, rank=0, world=1, speed_pq=((9, 10), (1, 1), (11, 10)), n=50, batch=4, **kw):
    from asr_chinese_e2e_amd.data_handler import BatchPlan
    lengths = [4800 + 331 * ((7 * i) % 23) for i in range(n)]
    return BatchPlan(lengths, batch, bucket_size=16, shuffle=True, seed=seed, rank=rank, world=world, speed_pq=speed_pq, **kw), lengths


def test_draws_are_a_pure_function_of_seed_epoch_and_index():
    from asr_chinese_e2e_amd.data_handler import speed
    a, b = speed.draw_factors(3, 0, 200, 3), speed.draw_factors(3, 0, 200, 3)
    assert a == b and set(a) == {0, 1, 2}
    assert speed.draw_factors(3, 1, 200, 3) != a and speed.draw_factors(4, 0, 200, 3) != a
    assert speed.draw_factors(3, 0, 120, 3) == a[:120]      # index order: the draw of utterance i does not depend on the data set's size
    p1, lengths = _plan()
    p2, _ = _plan()
    e0, e0b = p1.next_epoch(), p2.next_epoch()
    assert e0 == e0b and e0[2] == speed.draw_factors(3, 0, len(lengths), 3)
    e1 = p1.next_epoch()
    assert e1[2] == speed.draw_factors(3, 1, len(lengths), 3) != e0[2]
    for mine, full, fidx in (e0, e1):
        assert mine == full and sorted(i for b in full for i in b) == list(range(len(lengths)))      # every index once per epoch
    # buckets are formed on the perturbed lengths: within a batch they differ by less than the whole data set's spread
    pl = [speed.perturbed_len(n, *p1.speed_pq[f]) for n, f in zip(lengths, e0[2])]
    spread = max(max(pl[i] for i in b) - min(pl[i] for i in b) for b in e0[1])
    order = sorted(pl)
    assert spread <= max(order[min(s + 15, len(order) - 1)] - order[s] for s in range(0, len(order), 16))


def test_every_rank_builds_the_same_batch_list():
    r0, lengths = _plan(rank=0, world=2)
    r1, _ = _plan(rank=1, world=2)
    for _ in range(2):
        m0, full0, f0 = r0.next_epoch()
        m1, full1, f1 = r1.next_epoch()
        assert full0 == full1 and f0 == f1
        assert m0 == full0[: len(full0) // 2 * 2][0::2] and m1 == full0[: len(full0) // 2 * 2][1::2] and len(m0) == len(m1)
        assert all(len(b) == 4 for b in full0)


def test_without_speed_perturbation_the_rng_sequence_is_todays():
    from asr_chinese_e2e_amd.data_handler import bucket_batches
    plan, lengths = _plan(seed=5, speed_pq=None)
    rng = random.Random(5)
    for _ in range(3):
        mine, full, fidx = plan.next_epoch()
        assert fidx is None and mine == full == bucket_batches(lengths, 4, 16, True, False, rng)
    assert plan.rng.random() == rng.random()
    # and with it on, the draw leaves that generator alone: as many calls as without
    on, _ = _plan(seed=5)
    rng = random.Random(5)
    for _ in range(3):
        on.next_epoch()
        bucket_batches(lengths, 4, 16, True, False, rng)
    assert on.rng.random() == rng.random()


def test_entry_point_validates_on_the_host():
    from asr_chinese_e2e_amd import _lib
    f = _lib.lib.asr_speed_perturb_fwd
    assert f(None, None, None, None, None, None, None, 1, 8, 8, 1, 1, 1, None) == -1 and "null pointer" in _lib.last_error()
    ok = (16, 16, 16, 16, 16, 16, 16)      # non-null, never dereferenced: every call below is refused before a launch
    assert f(*ok, 0, 8, 8, 1, 10, 15, None) == -1 and "B=0" in _lib.last_error()
    assert f(*ok, 1, 0, 8, 1, 10, 15, None) == -1 and "Smax=0" in _lib.last_error()
    assert f(*ok, 1, 8, 0, 1, 10, 15, None) == -1 and "Smax_out=0" in _lib.last_error()
    assert f(*ok, 1, 8, 8, 1, 10, 14, None) == -1 and "ntaps=14" in _lib.last_error()
    assert f(*ok, 1, 8, 8, 0, 10, 15, None) == -1 and "F=0" in _lib.last_error()
    assert f(*ok, 1, 8, 8, 1, 21, 15, None) == -1 and "qmax=21" in _lib.last_error()
    assert _lib.fast.asr_speed_perturb_fwd(*ok, 0, 8, 8, 1, 10, 15, None) == -1 and "B=0" in _lib.last_error()


def test_tile_constant_matches_the_header():
    from asr_chinese_e2e_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert int(re.search(r"#define\s+ASR_SPEED_TILE\s+(\d+)", text).group(1)) == _lib.SPEED_TILE == kernels.SPEED_TILE
    assert _lib.lib.asr_abi_version() == 10


def test_train_flag_reaches_the_train_part_only():
    import train
    flags = train.parse_flags(["--speed_perturb=0.9,1.0,1.1"])
    assert train.speed_factors(flags["speed_perturb"]) == (0.9, 1.0, 1.1)
    assert train.speed_factors(train.TrainConfig.speed_perturb) is None and train.speed_factors("") is None
    assert train.speed_factors(0.9) == (0.9,) and train.speed_factors("0.9, 1") == ("0.9", "1")
    src = open(os.path.join(ROOT, "train.py")).read()
    assert src.count("speed_perturb=speed_factors(config.speed_perturb)") == 1
    assert re.search(r'part="train".*speed_perturb=', src) and not re.search(r'part="(test|dev)".*speed_perturb=', src)
