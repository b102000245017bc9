"""Global CMVN and the streaming front end, host side (no GPU): the float64 definition (tests/cmvn_ref.py) against direct numpy, the
statistics file, the parser's arguments, the availability rules against brute force, argument validation of the entry points
through ctypes and through the trampolines, and the command-line flags."""
import os

import numpy as np
import pytest

from tests import cmvn_ref as CR
from tests.helpers import ROOT


def test_reference_statistics_against_direct_numpy():
    rng = np.random.RandomState(0)
    feat = rng.randn(3, 9, 5) * 2.0 - 7.0
    lens = [0, 150, 1290]                                # 0, 1 and 9 frames
    assert [CR.total_frames(l) for l in (0, 1, 159, 160, 12345)] == [0, 1, 1, 2, 78]
    s, q, cnt = CR.accumulate(feat, lens)
    valid = np.concatenate([feat[1, :1], feat[2, :9]])
    assert cnt == 10
    mean, istd, _ = CR.finalize(s, q, cnt)
    assert np.allclose(mean, valid.mean(axis=0), rtol=1e-13, atol=0) and np.allclose(istd, 1.0 / valid.std(axis=0), rtol=1e-11, atol=0)
    # two batches into the same accumulators = one batch of both
    s2, q2, cnt2 = CR.accumulate(feat[2:], lens[2:], CR.accumulate(feat[:2], lens[:2]))
    assert cnt2 == cnt and np.allclose(s2, s, rtol=1e-14) and np.allclose(q2, q, rtol=1e-14)
    # a constant bin: the variance floor keeps istd finite
    c = np.full((1, 4, 2), 3.0)
    assert np.all(np.isfinite(CR.finalize(*CR.accumulate(c, [640]))[1]))
    # the package's three lines agree with the reference's
    from asr_chinese_e2e_amd.data_handler import cmvn
    m2, i2, n2 = cmvn.finalize_stats(s, q, float(cnt))
    assert n2 == cnt and np.array_equal(m2, mean) and np.array_equal(i2, istd)
    with pytest.raises(ValueError):
        cmvn.finalize_stats(s, q, 0)


def test_reference_apply_stacks_and_masks():
    rng = np.random.RandomState(1)
    feat = rng.randn(2, 7, 3).astype(np.float32)
    mean, istd = rng.randn(3), 1.0 + rng.rand(3)
    out, out_len, _ = CR.apply(feat, [1000, 0], mean, istd, 4, 3, 3)      # 7 frames -> 3 rows, the last one repeats frame 6
    x = (feat[0] - mean.astype(np.float32)) * istd.astype(np.float32)
    assert out_len.tolist() == [3, 0] and not out[1].any()
    assert np.array_equal(out[0, 0], x[0:4].reshape(-1)) and np.array_equal(out[0, 2], x[[6, 6, 6, 6]].reshape(-1))
    out, _, fills = CR.apply(feat, [1000, 0], mean, istd, 1, 1, 7, masks=[[2, 4, 1, 2], [0, 0, 0, 0]])
    assert abs(fills[0, 0] - x.astype(np.float64).mean()) < 1e-12
    y = x.copy()
    y[2:4] = np.float32(fills[0, 0])
    assert abs(fills[0, 1] - y.astype(np.float64).mean()) < 1e-12
    assert np.all(out[0, :, 1] == np.float32(fills[0, 1])) and np.all(out[0, 2:4, [0, 2]] == np.float32(fills[0, 0]))
    assert np.array_equal(out[0, [0, 1, 4, 5, 6]][:, [0, 2]], x[[0, 1, 4, 5, 6]][:, [0, 2]])


def test_statistics_file_round_trip(tmp_path):
    from asr_chinese_e2e_amd.data_handler import load_cmvn, save_cmvn
    rng = np.random.RandomState(2)
    mean, istd = rng.randn(40), 1.0 + rng.rand(40)
    path = str(tmp_path / "cmvn.npz")
    save_cmvn(path, mean, istd, 123456789012)
    assert os.path.isfile(path)
    m2, i2, n2 = load_cmvn(path)
    assert np.array_equal(m2, mean) and np.array_equal(i2, istd) and n2 == 123456789012 and m2.dtype == np.float64
    with np.load(path) as z:
        assert sorted(z.files) == ["count", "istd", "mean", "n_mels"] and int(z["n_mels"]) == 40
    with pytest.raises(ValueError):
        save_cmvn(path, mean, istd[:3], 1)


def test_parser_normalisation_arguments(tmp_path):
    from asr_chinese_e2e_amd.data_handler import AudioParser, save_cmvn
    from asr_chinese_e2e_amd.data_handler.loader import parser_norm
    p = AudioParser(device="cpu")
    assert p.norm == "utterance" and p.mean is None and p.istd is None
    with pytest.raises(ValueError, match="cmvn"):
        AudioParser(device="cpu", norm="global")
    with pytest.raises(ValueError):
        AudioParser(device="cpu", norm="global", cmvn="")
    with pytest.raises(ValueError):
        AudioParser(device="cpu", norm="per_bin")
    with pytest.raises(ValueError):
        AudioParser(device="cpu", cmvn=(np.zeros(80), np.ones(80)))      # statistics without norm="global": refused, not ignored
    with pytest.raises(ValueError):
        AudioParser(device="cpu", n_mels=80, norm="global", cmvn=(np.zeros(40), np.ones(40)))
    mean, istd = np.linspace(-9, -3, 40), np.linspace(0.3, 0.6, 40)
    p = AudioParser(device="cpu", n_mels=40, norm="global", cmvn=(mean, istd))
    assert p.norm == "global" and np.array_equal(p.mean.numpy(), mean.astype(np.float32)) and np.array_equal(p.istd.numpy(), istd.astype(np.float32))
    path = str(tmp_path / "s.npz")
    save_cmvn(path, mean, istd, 10)
    q = AudioParser(device="cpu", n_mels=40, **parser_norm(path))
    assert q.norm == "global" and np.array_equal(q.mean.numpy(), p.mean.numpy()) and np.array_equal(q.istd.numpy(), p.istd.numpy())
    assert parser_norm(None) == {} and parser_norm("") == {}


# ------------------------------------------------------------------------------------ availability rules
def _brute_frames(received, length=None):
    """Frames whose every (start-reflected) window index has arrived; with the length known, the offline count."""
    if length is not None:
        return 1 + length // 160 if length > 0 else 0
    t = 0
    while True:
        idx = np.abs(160 * t - 200 + np.arange(400))
        if not np.all(idx < received):
            return t
        t += 1


def _brute_rows(frames, m, n, closed):
    if closed:
        return -(-frames // n)
    r = 0
    while r * n + m - 1 < frames:
        r += 1
    return r


def test_availability_rules_against_brute_force():
    from asr_chinese_e2e_amd.data_handler import stream_frontend as SF
    assert SF.samples_needed(0) == 201 and SF.samples_needed(1) == 360 and SF.samples_needed(2) == 520 and SF.samples_needed(32) == 5320
    prev = 0
    for received in range(0, 2001):
        got = SF.frames_ready(received)
        assert got == _brute_frames(received), received
        assert got >= prev                                   # frames never go away
        prev = got
        for t in range(got):                                 # what is emitted needs no more than what arrived, the next one does
            assert SF.samples_needed(t) <= received
        assert SF.samples_needed(got) > received
        # history: no emitted-later frame touches a sample before oldest_sample(next frame)
        lo = np.abs(160 * got - 200 + np.arange(400)).min() if got >= 2 else 0
        assert SF.oldest_sample(got) == lo
        assert received - SF.oldest_sample(got) < 400        # what a sample ring must keep
    for length in (0, 1, 150, 200, 201, 359, 360, 12345):
        total = SF.frames_ready(length, closed=True)
        assert total == _brute_frames(length, length) == SF.total_frames(length) == CR.total_frames(length)
        for received in range(0, length + 1, 1 if length < 400 else 97):
            assert SF.frames_ready(received) == _brute_frames(received) <= total      # nothing emitted early is lost at the close
        for m, n in ((4, 3), (1, 1)):
            rows_total = SF.rows_ready(total, m, n, closed=True)
            assert rows_total == _brute_rows(total, m, n, True) == -(-total // n)
            for frames in range(total + 1):
                got = SF.rows_ready(frames, m, n)
                assert got == _brute_rows(frames, m, n, False) <= rows_total
    for frames in range(0, 200):
        for m, n in ((4, 3), (1, 1), (7, 6)):
            assert SF.rows_ready(frames, m, n) == _brute_rows(frames, m, n, False)
            assert SF.rows_ready(frames, m, n, closed=True) == _brute_rows(frames, m, n, True)


# ------------------------------------------------------------------------------------ entry points
def test_entry_points_validate_on_the_host():
    from asr_chinese_e2e_amd import _lib
    ok = 16      # non-null, never dereferenced: every call below is refused before a launch
    for lib in (_lib.lib, _lib.fast):
        f = lib.asr_cmvn_accumulate
        assert f(None, None, None, 1, 8, 40, None) == -1 and "null pointer" in _lib.last_error()
        assert f(ok, ok, ok, 0, 8, 40, None) == -1 and "B=0" in _lib.last_error()
        assert f(ok, ok, ok, 1, 0, 40, None) == -1 and "Tmax=0" in _lib.last_error()
        assert f(ok, ok, ok, 1, 8, 257, None) == -1 and "n_mels=257" in _lib.last_error()
        f = lib.asr_global_norm_augment_lfr_fwd
        assert f(None, None, None, None, None, None, None, 1, 8, 40, 4, 3, 3, 0, None) == -1 and "null pointer" in _lib.last_error()
        assert f(ok, ok, None, None, ok, ok, ok, 1, 8, 40, 4, 3, 3, 0, None) == -1 and "null pointer" in _lib.last_error()      # mean
        assert f(ok, ok, None, ok, ok, ok, ok, 1, 8, 40, 0, 3, 3, 0, None) == -1 and "m=0" in _lib.last_error()
        assert f(ok, ok, None, ok, ok, ok, ok, 1, 8, 40, 4, 3, 0, 0, None) == -1 and "Tlfr_max=0" in _lib.last_error()
        assert f(ok, ok, None, ok, ok, ok, ok, 1, 8, 40, 4, 3, 3, 7, None) == -2 and "dtype 7" in _lib.last_error()
        f = lib.asr_stream_append
        assert f(None, None, None, 1, 8, 0, 8, 1024, None) == -1 and "null pointer" in _lib.last_error()
        assert f(ok, ok, ok, 1, 8, 0, 8, 1000, None) == -1 and "scap=1000" in _lib.last_error()
        assert f(ok, ok, ok, 1, 8, 4, 8, 1024, None) == -1 and "pcm_off=4" in _lib.last_error()        # 4 + 8 > S
        assert f(ok, ok, ok, 1, 4096, 0, 2048, 1024, None) == -1 and "max_new=2048" in _lib.last_error()
        f = lib.asr_stream_logmel
        assert f(None, None, None, None, None, 1, 8, 1024, 64, 40, None) == -1 and "null pointer" in _lib.last_error()
        assert f(ok, ok, ok, ok, ok, 1, 8, 512, 64, 40, None) == -1 and "scap=512" in _lib.last_error()
        assert f(ok, ok, ok, ok, ok, 1, 8, 1024, 48, 40, None) == -1 and "fcap=48" in _lib.last_error()
        assert f(ok, ok, ok, ok, ok, 1, 65, 1024, 64, 40, None) == -1 and "max_new=65" in _lib.last_error()
        f = lib.asr_stream_norm_lfr
        assert f(None, None, None, None, None, 1, 4, 64, 40, 4, 3, 0, None) == -1 and "null pointer" in _lib.last_error()
        assert f(ok, ok, ok, ok, ok, 1, 0, 64, 40, 4, 3, 0, None) == -1 and "C=0" in _lib.last_error()
        assert f(ok, ok, ok, ok, ok, 1, 4, 63, 40, 4, 3, 0, None) == -1 and "fcap=63" in _lib.last_error()
        assert f(ok, ok, ok, ok, ok, 1, 4, 64, 40, 4, 3, 5, None) == -2 and "dtype 5" in _lib.last_error()
    assert _lib.lib.asr_abi_version() == 10


def test_open_marker_matches_the_header():
    import re
    from asr_chinese_e2e_amd import _lib, kernels
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert int(re.search(r"#define\s+ASR_STREAM_OPEN\s+(0x[0-9a-f]+)", text).group(1), 16) == _lib.STREAM_OPEN == kernels.STREAM_OPEN


# ------------------------------------------------------------------------------------ flags
def test_cmvn_flags(monkeypatch):
    import train
    import transcribe
    flags = train.parse_flags(["--cmvn=exp/cmvn.npz", "--batch_size=4"])
    assert flags["cmvn"] == "exp/cmvn.npz"
    config = train.TrainConfig()
    assert config.cmvn == ""                                 # off by default
    config.fn_build(flags)
    assert config.cmvn == "exp/cmvn.npz"
    assert "cmvn" in transcribe.CLI_KEYS and "stream_block_samples" in transcribe.CLI_KEYS
    assert transcribe.cmvn_path(train.parse_flags(["--cmvn=exp/cmvn.npz"])) == "exp/cmvn.npz"
    assert transcribe.cmvn_path(train.parse_flags(["--cmvn="])) is None and transcribe.cmvn_path({}) is None


def test_train_passes_cmvn_to_the_loader_of_every_part(monkeypatch):
    import torch
    import train

    class Built(Exception):
        pass

    for flag, want in (("--cmvn=exp/cmvn.npz", "exp/cmvn.npz"), ("--cmvn=", None), (None, None)):
        calls = []

        def fake_loader(**kw):
            calls.append(kw)
            if len(calls) == 3:
                raise Built
            return []

        monkeypatch.setattr(train, "build_dataloader", fake_loader)
        monkeypatch.setattr(train.Vocab, "load", staticmethod(lambda path: train.Vocab.synthetic(10)))
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(torch.cuda, "set_device", lambda i: None)
        monkeypatch.delenv("WORLD_SIZE", raising=False)
        with pytest.raises(Built):
            train.train(**train.parse_flags(["--model_name=TransformerOffical"] + ([flag] if flag else [])))
        assert [c["part"] for c in calls] == ["train", "test", "dev"]
        assert [c["cmvn"] for c in calls] == [want] * 3


def test_frontend_plans_growth_and_refuses_without_side_effects():
    """The host plan of push_audio (no launch): an utterance that runs ahead of a stalled one, beside one that is closed and drained,
    makes the frame rings grow; past max_frames the call is refused before anything changes."""
    from asr_chinese_e2e_amd.data_handler import AudioParser, StreamingFrontEnd
    parser = AudioParser(device="cpu", n_mels=40, norm="global", cmvn=(np.zeros(40), np.ones(40)))
    fe = StreamingFrontEnd(parser, 3, 4, sample_cap=1024, max_frames=200)
    assert fe.fcap == 64 and fe.piece == 512

    def commit(ns, fin):
        acts, (fe.received, fe.closed, fe.next_frame, fe.next_row) = fe.plan(ns, fin)
        for a in acts:
            if a[0] == "grow":
                fe.fcap = a[1]
        return acts

    acts = commit([4000, 6500, 6500], [True, False, False])
    assert [a[0] for a in acts].count("append") == 13 and [a[2] for a in acts if a[0] == "chunk"] == [[4, 4, 4], [4, 4, 4], [1, 4, 4]]
    assert fe.next_row == [9, 12, 12] and fe.next_frame == [26, 40, 40]          # utterance 0: next row's first frame 27 > its 26 frames
    grows = []
    for _ in range(23):
        grows += [a for a in commit([0, 0, 1000], [False] * 3) if a[0] == "grow"]
    assert [g[1] for g in grows] == [128, 256] and all(g[2][0] == (26, 26) for g in grows)      # nothing live for the drained one
    assert all(hi - lo <= cap for g in grows for lo, hi in g[2] for cap in [g[1]])
    before = (list(fe.received), list(fe.closed), list(fe.next_frame), list(fe.next_row))
    with pytest.raises(ValueError, match="lock-step"):
        fe.plan([0, 0, 10000], [False] * 3)
    assert before == (fe.received, fe.closed, fe.next_frame, fe.next_row)
    # the rest arrives: every remaining row of the two long utterances leaves
    acts = commit([0, 5845, 500], [True, True, True])
    assert sum(sum(a[2]) for a in acts if a[0] == "chunk") == (9 - 9) + (26 - 12) + (63 - 12)


def test_frontend_refuses_per_utterance_normalisation():
    from asr_chinese_e2e_amd.data_handler import AudioParser, StreamingFrontEnd
    with pytest.raises(ValueError, match="global"):
        StreamingFrontEnd(AudioParser(device="cpu"), 1, 4)
