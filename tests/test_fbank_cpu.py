"""The Kaldi fbank front end without a GPU: the float64 definition (tests/fbank_ref.py) and its a-priori bound, the frame arithmetic
AudioParser(frontend="kaldi") owns, the streaming plan on the counters alone, and the CMVN file formats those features come with."""
import json

import numpy as np
import pytest
import torch

from tests import fbank_ref as R

LENS = [0, 1, 399, 400, 559, 560, 5359, 5360, 5519, 5520, 10640]
FRAMES = [0, 0, 0, 1, 1, 2, 31, 32, 32, 33, 65]


def kaldi_parser(n_mels=40, m=4, n=3, **kw):
    from asr_chinese_e2e_amd.data_handler import AudioParser
    return AudioParser(device="cpu", n_mels=n_mels, lfr_m=m, lfr_n=n, frontend="kaldi", **kw)


# ------------------------------------------------------------------------------------ the definition
def test_frame_counts():
    assert [R.num_frames(l) for l in LENS] == FRAMES
    p = kaldi_parser()
    assert [p.num_frames(l) for l in LENS] == FRAMES
    assert [R.scaled_frames(np.zeros(l)).shape[0] for l in LENS] == FRAMES


def test_povey_window():
    w = R.povey_window()
    assert w.shape == (400,) and w[0] == 0.0 and abs(w[-1]) < 1e-12
    assert np.allclose(w, w[::-1], rtol=0, atol=1e-12)
    assert w.max() < 1.0 and set(np.flatnonzero(w >= w.max() - 1e-15)) == {199, 200}
    from asr_chinese_e2e_amd.data_handler import processor as P
    assert np.array_equal(P.povey_window().numpy(), w.astype(np.float32))


@pytest.mark.parametrize("n_mels", [23, 40, 80, 128, 160])
def test_mel_banks(n_mels):
    fb = R.mel_filterbank(n_mels)
    assert fb.shape == (256, n_mels) and fb.min() >= 0.0 and fb.max() <= 1.0
    assert not fb[0].any()                                                    # bin 0 (0 Hz) lies below low_freq = 20 Hz
    m = R.mel(np.arange(256) * 16000 / 512)
    lo, hi = float(R.mel(20.0)), float(R.mel(8000.0))
    delta = (hi - lo) / (n_mels + 1)
    inside = (m >= lo + delta) & (m <= lo + n_mels * delta)                   # between the first and the last centre
    assert inside.sum() > 200 and np.allclose(fb[inside].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    empty = int((~fb.any(axis=0)).sum())
    assert empty == {23: 0, 40: 0, 80: 0, 128: 1, 160: 3}[n_mels]
    if n_mels == 80:
        assert (fb != 0).sum(axis=0).min() == 1                               # the narrowest filter holds a single FFT bin
    from asr_chinese_e2e_amd.data_handler import processor as P
    assert np.array_equal(P.kaldi_mel_filterbank(n_mels).numpy(), fb.astype(np.float32))


def test_silence_tone_and_scale():
    assert np.all(R.fbank64(np.zeros(1000), 80) == np.log(R.FLT_EPSILON)) and abs(np.log(R.FLT_EPSILON) + 15.942385) < 1e-6
    assert R.fbank64(np.zeros(399), 80).shape == (0, 80)
    sig = R.signals()
    tone = R.fbank64(sig["tone 1234.5 Hz"], 80)
    fb = R.mel_filterbank(80)
    k = 1234.5 * 512 / 16000
    holds = np.flatnonzero((fb[int(np.floor(k))] > 0) | (fb[int(np.ceil(k))] > 0))
    assert set(np.argmax(tone, axis=1)) <= set(holds)
    x = sig["noise 0.1"].astype(np.float64)
    a, b = R.fbank64(x, 128), R.fbank64(2.0 * x, 128)
    live = ~R.floor_cells(x, 128)
    assert live.any() and not live.all()
    assert np.allclose(b[live] - a[live], np.log(4.0), rtol=0, atol=1e-9) and np.all(b[~live] == np.log(R.FLT_EPSILON))


# ------------------------------------------------------------------------------------ the bound
@pytest.mark.parametrize("n_mels", [40, 80])
def test_emulation_within_bound(n_mels):
    for name, wav in R.signals().items():
        got = R.emulate32(wav, n_mels)
        assert got.dtype == np.float32 and got.shape == (48, n_mels)
        ratio, at = R.error_ratio(got, wav, n_mels)
        floor = R.floor_cells(wav, n_mels)
        print(f"n_mels {n_mels:3d}  {name:24s} err/bound {ratio:.3e} at {at}  floor cells {int(floor.sum())}")
        assert ratio <= 1.0, (name, ratio, at)
        assert np.all(got[floor] == R.LOG_FLOOR32), name
        if name == "constant 0.25":
            assert not floor.any()                                           # held to the bound, not to the floor
        if name == "impulse":
            assert floor.any() and not floor.all()


# ------------------------------------------------------------------------------------ the parser's frame arithmetic
def test_equivalent_length():
    from asr_chinese_e2e_amd.data_handler.processor import equivalent_length
    for T in range(71):
        e = equivalent_length(T)
        assert (1 + e // 160 if e > 0 else 0) == T and e >= 0
    p = kaldi_parser()
    lens = torch.tensor(LENS + [20000, -5])
    wl, frames = p.norm_lengths(lens, 10640, 65), p.frame_counts(lens, 10640, 65)
    assert frames == FRAMES + [65, 0] and wl.dtype == torch.int32
    assert p.norm_lengths(lens, 10640, 20).tolist() == [160 * (min(f, 20) - 1) + 1 if f else 0 for f in frames]
    assert equivalent_length(torch.tensor([0, 1, 2, 65])).tolist() == [0, 1, 161, 10241]
    assert [1 + e // 160 if e > 0 else 0 for e in wl.tolist()] == frames
    assert p.max_frames(10640) == 65 and p.max_frames(399) == 1 and p.max_frames(400) == 1


def _brute_ready(received):
    """Frames all of whose samples 160 t .. 160 t + 399 lie below `received`."""
    t = 0
    while 160 * t + 399 < received:
        t += 1
    return t


def test_kaldi_availability_rules():
    p = kaldi_parser()
    for received in range(2001):
        want = _brute_ready(received)
        assert p.frames_ready(received) == p.frames_ready(received, closed=True) == want == R.num_frames(received)
    for t in range(40):
        assert p.oldest_sample(t) == 160 * t and p.frame_centre_sample(t) == 160 * t + 200
        assert p.frames_ready(p.oldest_sample(t) + 399) == t and p.frames_ready(p.oldest_sample(t) + 400) == t + 1


def test_reference_rules_are_unchanged():
    from asr_chinese_e2e_amd.data_handler import AudioParser
    from asr_chinese_e2e_amd.data_handler import stream_frontend as SF
    p = AudioParser(device="cpu", n_mels=40)
    assert p.frontend == "reference" and tuple(p.melfb.shape) == (201, 40)
    for received in range(0, 2001, 7):
        for closed in (False, True):
            assert p.frames_ready(received, closed) == SF.frames_ready(received, closed)
        assert p.num_frames(received) == SF.total_frames(received)
    assert [p.oldest_sample(t) for t in range(5)] == [SF.oldest_sample(t) for t in range(5)]
    assert p.frame_centre_sample(3) == 480 and p.max_frames(1000) == 7


# ------------------------------------------------------------------------------------ StreamingFrontEnd.plan on the counters
def _run_plan(fe, length, block):
    """Feed `length` samples in blocks (final on the last) through plan() alone, committing the counters as push_audio does."""
    frames = rows = 0
    chunks = []
    pos = 0
    while True:
        n = min(block, length - pos)
        pos += n
        acts, after = fe.plan([n], [pos == length])
        for a in acts:
            if a[0] == "logmel":
                assert a[1][0][0] == frames
                frames += a[1][0][1]
                assert 160 * (frames - 1) + 400 <= pos                        # no frame touches a sample that has not arrived
            elif a[0] == "chunk":
                assert a[1][0][0] == rows
                rows += a[2][0]
                chunks.append(a[2][0])
        fe.received, fe.closed, fe.next_frame, fe.next_row = after
        if pos == length:
            return frames, rows, chunks


@pytest.mark.parametrize("block", [1, 160, 401, 7680])
def test_streaming_plan_counts(block):
    from asr_chinese_e2e_amd.data_handler import StreamingFrontEnd
    p = kaldi_parser(norm="global", cmvn=(np.zeros(40), np.ones(40)))
    for length in (400, 5519, 8000):
        fe = StreamingFrontEnd(p, 1, 4, sample_cap=1024)
        frames, rows, chunks = _run_plan(fe, length, block)
        T = R.num_frames(length)
        assert frames == T and rows == -(-T // 3), (length, block)
        assert all(c == 4 for c in chunks[:-1]) and 0 < chunks[-1] <= 4


def test_streaming_plan_of_an_utterance_without_a_frame():
    from asr_chinese_e2e_amd.data_handler import StreamingFrontEnd
    p = kaldi_parser(norm="global", cmvn=(np.zeros(40), np.ones(40)))
    for block in (399, 100):
        fe = StreamingFrontEnd(p, 1, 4, sample_cap=1024)
        frames, rows, chunks = _run_plan(fe, 399, block)
        assert (frames, rows, chunks) == (0, 0, [0])                          # one empty final chunk
        assert fe.plan([0], [True])[0] == []                                  # and nothing after it
    fe = StreamingFrontEnd(p, 2, 4, sample_cap=1024)                          # beside a longer utterance its rows are simply none
    acts, _ = fe.plan([300, 2000], [True, True])
    assert [a[2] for a in acts if a[0] == "chunk"] == [[0, 4]]


# ------------------------------------------------------------------------------------ CMVN formats
def _sums(n_mels, seed=3):
    rng = np.random.RandomState(seed)
    count = 1234
    x = rng.randn(count, n_mels) * 2.0 + 5.0
    return x.sum(axis=0), (x * x).sum(axis=0), count


def test_cmvn_formats_round_trip(tmp_path):
    from asr_chinese_e2e_amd.data_handler import cmvn as C
    sx, sxx, count = _sums(40)
    mean, istd, _ = C.finalize_stats(sx, sxx, count)
    npz, js, ark = (str(tmp_path / f) for f in ("a.npz", "b.json", "c.ark.txt"))
    C.save_cmvn(npz, mean, istd, count, frontend="kaldi")
    C.save_wenet_cmvn(js, sx, sxx, count)
    assert sorted(json.load(open(js))) == ["frame_num", "mean_stat", "var_stat"]
    with open(ark, "w") as f:
        f.write(" [\n  " + " ".join(repr(float(v)) for v in sx) + f" {count}\n  " + " ".join(repr(float(v)) for v in sxx) + " 0 ]\n")
    for path in (npz, js, ark):
        m, i, c = C.load_cmvn(path)
        assert c == count and np.array_equal(m, mean) and np.array_equal(i, istd), path
        assert C.load_cmvn_meta(path)[3] == "kaldi"
    # the key's default, and a file from before it
    C.save_cmvn(npz, mean, istd, count)
    assert C.load_cmvn_meta(npz)[3] == "reference"
    with open(npz, "wb") as f:
        np.savez(f, mean=mean, istd=istd, count=np.int64(count), n_mels=np.int64(40))
    assert C.load_cmvn_meta(npz)[3] == "reference" and len(C.load_cmvn(npz)) == 3
    # what is none of the three, or a broken one of them, is a ValueError that names the file
    bad = str(tmp_path / "bad")
    for content, what in ((b"neither\n", "neither"), (b"\xff\xfe\x00binary\x80", "neither"), (b'{"mean_stat": [1.0]}', "WeNet"), (b'{"mean_stat": ', "WeNet"),
                          (b"a [ 1 2 3\n 4 5 0 ]\nb [ 1 2 3\n 4 5 0 ]\n", "more than one"), (b"[ 1 2 3 ]", "two rows")):
        with open(bad, "wb") as f:
            f.write(content)
        with pytest.raises(ValueError, match=what) as e:
            C.load_cmvn(bad)
        assert bad in str(e.value)


def test_cmvn_front_end_mismatch_and_width(tmp_path):
    from asr_chinese_e2e_amd.data_handler import AudioParser
    from asr_chinese_e2e_amd.data_handler import cmvn as C
    sx, sxx, count = _sums(40)
    mean, istd, _ = C.finalize_stats(sx, sxx, count)
    ref_file, kaldi_file, js = (str(tmp_path / f) for f in ("ref.npz", "kaldi.npz", "wenet.json"))
    C.save_cmvn(ref_file, mean, istd, count)
    C.save_cmvn(kaldi_file, mean, istd, count, frontend="kaldi")
    C.save_wenet_cmvn(js, sx, sxx, count)
    for path in (kaldi_file, js):
        p = kaldi_parser(norm="global", cmvn=path)
        assert np.array_equal(p.mean.numpy(), mean.astype(np.float32)) and np.array_equal(p.istd.numpy(), istd.astype(np.float32))
        with pytest.raises(ValueError, match="'kaldi'.*'reference'"):
            AudioParser(device="cpu", n_mels=40, norm="global", cmvn=path)
    with pytest.raises(ValueError, match="'reference'.*'kaldi'"):
        kaldi_parser(norm="global", cmvn=ref_file)
    assert AudioParser(device="cpu", n_mels=40, norm="global", cmvn=ref_file).frontend == "reference"
    with pytest.raises(ValueError, match="mel bins"):
        kaldi_parser(n_mels=80, norm="global", cmvn=kaldi_file)
    with pytest.raises(ValueError, match="mel bins"):
        kaldi_parser(n_mels=80, norm="global", cmvn=js)


# ------------------------------------------------------------------------------------ arguments
def test_parser_and_wrapper_arguments():
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.data_handler import AudioParser
    with pytest.raises(ValueError, match="frontend"):
        AudioParser(device="cpu", frontend="bogus")
    p = kaldi_parser(n_mels=23)
    assert tuple(p.melfb.shape) == (256, 23) and p.window.numel() == 400 and (p.wav_scale, p.preemph) == (32768.0, 0.97)
    wav, wl = torch.zeros(2, 800), torch.tensor([800, 800], dtype=torch.int32)
    with pytest.raises(AssertionError):
        K.fbank(wav, wl, p.window, torch.zeros(201, 23), 3, 32768.0, 0.97)      # the reference's banks
    with pytest.raises(AssertionError):
        K.fbank(wav, wl, torch.zeros(512), p.melfb, 3, 32768.0, 0.97)
    with pytest.raises(AssertionError):
        K.stream_fbank(torch.zeros(2, 1024), torch.zeros(2, 3, dtype=torch.int32), p.window, p.melfb, torch.zeros(2, 64, 23), 4, 32768.0, 0.97)
    with pytest.raises(ValueError, match="CUDA"):
        K.fbank(wav, wl, p.window, p.melfb, 3, 32768.0, 0.97)                   # no CPU fall-back


def test_entry_points_refuse_bad_arguments():
    from asr_chinese_e2e_amd import _lib
    L = _lib.lib
    assert L.asr_fbank_fwd(None, None, None, None, None, 1, 400, 1, 80, 32768.0, 0.97, None) == -1 and "null" in _lib.last_error()
    for B, S, T, n in ((0, 400, 1, 80), (65536, 400, 1, 80), (1, 0, 1, 80), (1, 400, 0, 80), (1, 400, 1, 0)):
        assert L.asr_fbank_fwd(8, 8, 8, 8, 8, B, S, T, n, 32768.0, 0.97, None) == -1 and "bad shape" in _lib.last_error()
    assert L.asr_stream_fbank(None, 8, 8, 8, 8, 1, 4, 1024, 64, 80, 32768.0, 0.97, None) == -1
    for B, mx, scap, fcap, n in ((0, 4, 1024, 64, 80), (1, 0, 1024, 64, 80), (1, 4, 1000, 64, 80), (1, 4, 512, 64, 80), (1, 4, 1024, 48, 80),
                                 (1, 65, 1024, 64, 80), (1, 4, 1024, 64, 0)):
        assert L.asr_stream_fbank(8, 8, 8, 8, 8, B, mx, scap, fcap, n, 32768.0, 0.97, None) == -1 and "bad shape" in _lib.last_error()
