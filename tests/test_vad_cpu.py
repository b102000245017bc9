"""The energy VAD's host side (no GPU): the production segmenter against the definition's loops (tests/vad_ref.py), the fp32 error bound
against a float32 restatement of the kernel, the decision rule, every refusal, transcribe_long's stitching with a stub model and stub
kernels, transcribe.py's flags, and the inputs the GPU tests count on."""
import math
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import vad_cases as C
from tests import vad_ref as R
from tests.helpers import ROOT


# ------------------------------------------------------------------------------------ the segmenter
def seg(mask, T=None, length=None, min_silence=30, min_speech=10, pad=10, max_frames=2000):
    from asr_chinese_e2e_amd.vad import segments_from_mask
    mask = np.asarray(mask, dtype=np.uint8)
    T = len(mask) if T is None else T
    length = (160 * (T - 1) + 400 + 37 if T else 399) if length is None else length
    got = segments_from_mask(mask, T, length, min_silence, min_speech, pad, max_frames)
    want = R.segments(mask, T, length, min_silence, min_speech, pad, max_frames)
    assert got == want, (got, want)
    assert all(isinstance(v, int) for s in got for v in s)
    return got


def frames(*runs, T):
    m = np.zeros(T, dtype=np.uint8)
    for a, b in runs:
        m[a:b + 1] = 1
    return m


def test_segmenter_hand_made_masks():
    assert seg(np.zeros(500)) == []                                            # all silence
    assert seg(np.ones(500)) == [(0, 160 * 499 + 400)]                         # all speech
    assert seg(np.ones(500), length=160 * 499 + 400 - 0) == [(0, 80240)]
    # runs touching frame 0 and frame T - 1: the padding is clipped
    assert seg(frames((0, 49), (450, 499), T=500)) == [(0, 160 * 59 + 400), (160 * 440, 160 * 499 + 400)]
    # the last segment ends with the recording, not behind it
    assert seg(frames((450, 499), T=500), length=160 * 499 + 400 + 5) == [(160 * 440, 160 * 499 + 400)]
    # a pause of min_silence - 1 frames is bridged, one of min_silence frames cuts
    assert seg(frames((100, 149), (179, 220), T=500)) == [(160 * 90, 160 * 230 + 400)]
    assert seg(frames((100, 149), (180, 220), T=500)) == [(160 * 90, 160 * 159 + 400), (160 * 170, 160 * 230 + 400)]
    # a run of min_speech - 1 frames is dropped, one of min_speech frames is kept
    assert seg(frames((100, 108), T=500)) == []
    assert seg(frames((100, 109), T=500)) == [(160 * 90, 160 * 119 + 400)]
    # two short runs that merge are long enough together
    assert seg(frames((100, 103), (110, 113), T=500)) == [(160 * 90, 160 * 123 + 400)]
    assert seg([], T=0) == [] and seg([1], T=1, min_speech=1) == [(0, 400)] and seg([1], T=1) == [] and seg([0], T=1) == []


def test_segmenter_splits():
    # a pause inside the cut window [start + 100, start + 199]: cut at its centre
    m = frames((10, 129), (140, 300), T=400)                  # run [0, 310] after padding; the pause 130 .. 139 lies in [100, 199]
    assert seg(m, max_frames=200) == [(0, 160 * 134 + 400), (160 * 135, 160 * 310 + 400)]
    # two pauses of one length: the first; a longer one later wins
    m = frames((10, 119), (125, 149), (155, 300), T=400)
    assert seg(m, max_frames=200)[0] == (0, 160 * 122 + 400)
    m = frames((10, 119), (125, 149), (157, 300), T=400)
    assert seg(m, max_frames=200)[0] == (0, 160 * 153 + 400)
    # a pause that reaches out of the window counts with the part inside it only
    m = frames((10, 94), (106, 170), (174, 300), T=400)       # pause 95 .. 105: frames 100 .. 105 inside (6), pause 171 .. 173 (3)
    assert seg(m, max_frames=200)[0] == (0, 160 * 102 + 400)
    # no pause in the window: the hard cut behind max_frames frames
    assert seg(frames((10, 300), T=400), max_frames=200) == [(0, 160 * 199 + 400), (160 * 200, 160 * 310 + 400)]
    # three times max_frames and more: cut again and again on the remainder
    got = seg(frames((0, 649), T=650), max_frames=200)
    assert got == [(0, 160 * 199 + 400), (160 * 200, 160 * 399 + 400), (160 * 400, 160 * 599 + 400), (160 * 600, 160 * 649 + 400)]
    assert seg(np.ones(5), max_frames=1, min_speech=1, min_silence=0, pad=0) == [(160 * t, 160 * t + 400) for t in range(5)]


def test_segmenter_random_masks():
    rng = random.Random(11)
    nrng = np.random.RandomState(11)
    total = 0
    for _ in range(200):
        T = rng.choice([1, 2, 7, 50, 300, 1000])
        # run-structured masks: alternate stretches of random lengths, so that pauses and runs of every length near the options occur
        m, v = [], rng.random() < 0.5
        while len(m) < T:
            m += [int(v)] * rng.choice([1, 2, 3, 5, 8, 13, 30, 31, 60, 200])
            v = not v
        m = np.asarray(m[:T], dtype=np.uint8)
        if rng.random() < 0.2:
            m = (nrng.rand(T) < 0.5).astype(np.uint8)
        pad = rng.choice([0, 1, 5, 10])
        min_silence = 2 * pad + rng.choice([0, 1, 3, 10])
        total += len(seg(m, min_silence=min_silence, min_speech=rng.choice([0, 1, 3, 10]), pad=pad, max_frames=rng.choice([1, 2, 9, 50, 120, 5000]),
                         length=160 * (T - 1) + 400 + rng.choice([0, 1, 159])))
    assert total > 100


def test_segmenter_refuses_and_options_become_frames():
    from asr_chinese_e2e_amd.vad import segment_frames, segments_from_mask
    assert segment_frames() == (30, 10, 10, 2000) == tuple(R.to_frames(v) for v in R.SEG_DEFAULTS.values())
    assert segment_frames(0.25, 0.0, 0.125, 0.015) == (25, 0, 12, 2)          # round(100 s), half to even as Python rounds
    with pytest.raises(ValueError, match="overlap"):
        segment_frames(min_silence_s=0.1, pad_s=0.1)
    for bad in (float("nan"), float("inf"), -0.1, "0.3", None, True):
        for name in ("min_silence_s", "min_speech_s", "pad_s", "max_segment_s"):
            with pytest.raises(ValueError, match=name):
                segment_frames(**{name: bad})
    with pytest.raises(ValueError, match="one frame"):
        segment_frames(max_segment_s=0.004)
    with pytest.raises(ValueError):
        segments_from_mask(np.ones(5), 5, 1200, 10, 1, 6, 100)
    with pytest.raises(ValueError):
        segments_from_mask(np.ones(3), 5, 1200, 10, 1, 5, 100)                 # fewer mask entries than frames


# ------------------------------------------------------------------------------------ the energy bound
def energy_signals():
    rng = np.random.RandomState(5)
    n = 400 + 160 * 47
    t = np.arange(n)
    sig = {f"noise_{a:g}": (a * rng.randn(n)).astype(np.float32) for a in (1e-4, 1e-2, 0.5)}
    sig["tone_440"] = (0.3 * np.sin(2 * np.pi * 440 * t / 16000)).astype(np.float32)
    sig["tone_on_dc"] = (0.6 + 1e-3 * np.sin(2 * np.pi * 1000 * t / 16000)).astype(np.float32)
    sig["constant"] = np.full(n, 0.37, dtype=np.float32)
    sig["impulse"] = np.zeros(n, dtype=np.float32)
    sig["impulse"][1000] = 0.9
    sig["zeros"] = np.zeros(n, dtype=np.float32)
    return sig


def test_float32_restatement_stays_inside_the_bound():
    worst = 0.0
    for name, x in energy_signals().items():
        e32 = R.emulate32(x)
        assert e32.dtype == np.float32 and e32.shape == (48,) and not np.isnan(e32).any()
        ratio, at = R.error_ratio(e32, x)
        zero = R.zero_frames(x)
        assert np.all(e32[zero].view(np.uint32) == np.array([R.LOG_FLOOR32]).view(np.uint32)[0]), name      # exactly logf(FLT_EPSILON)
        lb = R.log_bound(x)
        err = np.abs(e32.astype(np.float64) - R.energy64(x))
        assert np.all(err[~zero] <= lb[~zero]), name
        print(f"{name:12s} err/bound {ratio:.3e} at frame {at}; frames held in the log domain {int(np.isfinite(lb).sum())} of 48")
        assert ratio <= 1.0, (name, ratio, at)
        worst = max(worst, ratio)
    print(f"largest err / bound {worst:.3e}")
    assert int(R.zero_frames(energy_signals()["impulse"]).sum()) == 45 and R.zero_frames(energy_signals()["zeros"]).all()
    assert not np.isfinite(R.log_bound(energy_signals()["constant"])).any()      # a constant frame cancels: held in the linear domain only
    assert np.isfinite(R.log_bound(energy_signals()["noise_0.01"])).all()


def test_frame_count_and_definition():
    assert [R.num_frames(n) for n in (0, 399, 400, 559, 560, 10320, 10480, 10640, 41360)] == [0, 0, 1, 1, 2, 63, 64, 65, 257]
    from asr_chinese_e2e_amd import vad
    assert all(vad.num_frames(n) == R.num_frames(n) for n in (0, 1, 399, 400, 559, 560, 41360))
    x = np.arange(560, dtype=np.float64) / 32768.0             # a ramp: sum (i - mean)^2 = n (n^2 - 1) / 12
    assert np.allclose(R.sumsq64(x), [400 * (400 ** 2 - 1) / 12.0] * 2, rtol=1e-12)
    assert R.energy64(np.zeros(400))[0] == pytest.approx(math.log(2.0 ** -23), rel=1e-15)


# ------------------------------------------------------------------------------------ the decision rule
@pytest.mark.parametrize("ctx", [0, 2, 5])
def test_decision_rule(ctx):
    rng = np.random.RandomState(ctx)
    for T in (0, 1, 2, 3, 8, 11, 12, 100):
        E = rng.uniform(5.0, 25.0, T).astype(np.float32)
        thr = R.threshold(E)
        if T:
            assert thr == pytest.approx(5.0 + 0.5 * float(np.mean(E.astype(np.float64))), rel=1e-14)
        else:
            assert thr == 5.0
        for prop in (0.6, 1.0, 0.2):
            got = R.decide(E, thr, ctx, prop)
            above = np.concatenate(([0], np.cumsum(E.astype(np.float64) > thr)))
            lo, hi = np.maximum(np.arange(T) - ctx, 0), np.minimum(np.arange(T) + ctx, T - 1)      # windows clipped at both ends
            want = (above[hi + 1] - above[lo] >= (hi - lo + 1) * prop).astype(np.uint8) if T else np.zeros(0, dtype=np.uint8)
            assert np.array_equal(got, want), (T, prop)
    # by hand, five frames, the outer two above the threshold: with ctx 2 the votes are 1/3, 1/4, 2/5, 1/4, 1/3
    E = np.array([10.0, 0.0, 0.0, 0.0, 10.0])
    assert R.decide(E, 5.0, 0, 0.6).tolist() == [1, 0, 0, 0, 1]
    assert R.decide(E, 5.0, 2, 0.6).tolist() == [0, 0, 0, 0, 0] and R.decide(E, 5.0, 2, 0.3).tolist() == [1, 0, 1, 0, 1]


def test_gpu_test_inputs_are_clear_of_the_threshold():
    """What tests/test_vad_gpu.py counts on, vetted on the float32 restatement of the kernel: no frame of the decision case within 1e-6
    of its threshold, both classes present; the end-to-end recording gives five segments, one of them from a split."""
    wav, lens = C.decide_case()
    for b, n in enumerate(lens):
        E = R.emulate32(wav[b, :n])
        assert len(E) == [257, 3, 8, 0][b]
        for kw in C.DECIDE_OPTIONS if len(E) else ():
            thr = R.threshold(E, kw.get("energy_threshold", 5.0), kw.get("energy_mean_scale", 0.5))
            assert np.abs(E.astype(np.float64) - thr).min() >= 1e3 * C.MARGIN
            assert 0 < int(R.decide(E, thr).sum()) < len(E), b             # both classes
    x = C.long_case()
    E = R.emulate32(x)
    thr = R.threshold(E)
    assert np.abs(E.astype(np.float64) - thr).min() >= 1e3 * C.MARGIN
    mask = R.decide(E, thr)
    from asr_chinese_e2e_amd.vad import segment_frames
    opts = segment_frames(**C.LONG_OPTS)
    segs = R.segments(mask, len(E), len(x), *opts)
    unsplit = R.segments(mask, len(E), len(x), *opts[:3], 10 ** 6)
    assert len(segs) == C.LONG_SEGMENTS == len(unsplit) + 1 and all(400 <= b - a <= 160 * 299 + 400 for a, b in segs)
    assert segs[0][1] - 240 == segs[1][0] and segs[0][0] == unsplit[0][0] and segs[1][1] == unsplit[0][1]      # the cut: consecutive frames


# ------------------------------------------------------------------------------------ refusals
def test_energy_vad_refuses():
    from asr_chinese_e2e_amd.vad import EnergyVad
    v = EnergyVad()
    assert (v.energy_threshold, v.energy_mean_scale, v.frames_context, v.proportion_threshold) == tuple(R.DEFAULTS.values())
    EnergyVad(proportion_threshold=1.0, frames_context=1024)
    for kw in (dict(proportion_threshold=0.0), dict(proportion_threshold=1.01), dict(proportion_threshold=float("nan")), dict(energy_threshold=-1.0),
               dict(energy_threshold=float("inf")), dict(energy_mean_scale=-0.5), dict(energy_mean_scale=float("nan")), dict(frames_context=-1),
               dict(frames_context=1.5), dict(frames_context=1025), dict(frames_context=float("inf")), dict(energy_threshold="5")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            EnergyVad(**kw)


def test_entry_points_validate_before_any_launch():
    from asr_chinese_e2e_amd import _lib
    lib, ok = _lib.lib, 64
    assert lib.asr_vad_energy(None, None, None, 1, 400, 1, None) == -1 and "null pointer" in _lib.last_error()
    assert lib.asr_vad_energy(ok, ok, ok, 0, 400, 1, None) == -1 and "B=0" in _lib.last_error()
    assert lib.asr_vad_energy(ok, ok, ok, 1, 400, 0, None) == -1 and "Tmax=0" in _lib.last_error()
    assert lib.asr_vad_energy(ok, ok, ok, 65536, 400, 1, None) == -1
    assert lib.asr_vad_decide(ok, ok, ok, ok, ok, None, 1, 1, 0, None) == -1 and "null pointer" in _lib.last_error()
    assert lib.asr_vad_decide(ok, ok, ok, ok, ok, ok, 1, 1, -1, None) == -1 and "ctx=-1" in _lib.last_error()
    assert lib.asr_vad_decide(ok, ok, ok, ok, ok, ok, 1, 1, 1025, None) == -1 and "ctx=1025" in _lib.last_error()
    assert lib.asr_vad_decide(ok, ok, ok, ok, ok, 68, 1, 1, 0, None) == -1 and "alignment" in _lib.last_error()
    assert lib.asr_vad_decide(ok, ok, ok, ok, ok, ok, 1, 0, 0, None) == -1 and "Tmax=0" in _lib.last_error()
    assert lib.asr_segment_gather(ok, 400, ok, ok, None, ok, 1, 400, None) == -1 and "null pointer" in _lib.last_error()
    assert lib.asr_segment_gather(ok, 0, ok, ok, ok, ok, 1, 400, None) == -1 and "S=0" in _lib.last_error()
    assert lib.asr_segment_gather(ok, 400, ok, ok, ok, ok, 0, 400, None) == -1 and "N=0" in _lib.last_error()
    assert lib.asr_segment_gather(ok, 400, ok, ok, ok, ok, 1, 0, None) == -1 and "Smax=0" in _lib.last_error()
    assert lib.asr_vad_decide_workspace_bytes(3, 1024) == 3 * 8 and lib.asr_vad_decide_workspace_bytes(3, 1025) == 3 * 2 * 8
    assert _lib.fast.asr_vad_decide_workspace_bytes(2, 360000) == lib.asr_vad_decide_workspace_bytes(2, 360000) == 2 * 352 * 8
    assert lib.asr_vad_decide_workspace_bytes(0, 5) == 0
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert int(re.search(r"#define\s+ASR_VAD_CTX_MAX\s+(\d+)", text).group(1)) == _lib.VAD_CTX_MAX
    assert _lib.lib.asr_abi_version() == 10


# ------------------------------------------------------------------------------------ transcribe_long with a stub model and stub kernels
class StubParser:
    lfr_n = 3

    def __init__(self):
        self.window = torch.zeros(1)
        self.batches = []

    def num_frames(self, n):
        return 1 + n // 160 if n > 0 else 0

    def parse_batch(self, wav, wav_len):
        self.batches.append((wav.clone(), wav_len.tolist()))
        return wav, wav_len


class StubModel:
    """transcribe: utterance u of a batch of samples whose first is v gives the text "<v>;", ids [v], two tokens at 0.5 .. 1.0 s and at
    None (a token without times)."""
    table = 1000

    def __init__(self):
        self.calls = []

    def _ensure_engine(self, device):
        class Eng:
            pe = torch.zeros(self.table, 4)
        return Eng()

    def transcribe(self, pack, **kw):
        self.calls.append((pack.wave.shape, pack.wave_len.tolist(), kw))
        out = []
        for row in pack.wave:
            v = int(row[0])
            out.append({"text": f"<{v}>;", "ids": [v], "score": -float(v), "extra": "kept",
                        "tokens": [{"id": v, "start_frame": 5, "end_frame": 9, "start_s": 0.5, "end_s": 1.0}, {"id": 0, "start_frame": None, "end_frame": None, "start_s": None, "end_s": None}]})
        return out


class StubVad:
    def __init__(self, segs):
        self.segs, self.calls = segs, []

    def segments(self, wav, wav_len, *opts):
        self.calls.append((tuple(wav.shape), list(wav_len), opts))
        return self.segs


@pytest.fixture
def stub_gather(monkeypatch):
    from asr_chinese_e2e_amd import longform
    launches = []

    def gather(wav, rec, start, n, Smax):
        launches.append((list(rec), list(start), list(n), Smax))
        out = torch.zeros(len(rec), Smax)
        for i, (r, s, l) in enumerate(zip(rec, start, n)):
            out[i, :l] = wav[r, s:s + l]
        return out
    monkeypatch.setattr(longform.K, "segment_gather", gather)
    return launches


def test_transcribe_long_stitches(stub_gather):
    from asr_chinese_e2e_amd.longform import transcribe_long
    wav = torch.arange(2 * 64000, dtype=torch.float32).reshape(2, 64000) % 64000      # a sample's value is its index
    segs = [[(1600, 9600), (16000, 16400), (32000, 48000)], []]
    model, parser, vad = StubModel(), StubParser(), StubVad(segs)
    res = transcribe_long(model, parser, wav, [64000, 32000], vad=vad, batch_size=2, beam_size=3, joint="one_pass", timestamps=True)
    assert vad.calls == [((2, 64000), [64000, 32000], (0.3, 0.1, 0.1, 20.0))]
    # batches in time order, the last one partial; one gather, one parse_batch, one transcribe per batch; keywords pass through
    assert stub_gather == [([0, 0], [1600, 16000], [8000, 400], 8000), ([0], [32000], [16000], 16000)]
    assert [c[:2] for c in model.calls] == [((2, 8000), [8000, 400]), ((1, 16000), [16000])]
    assert all(c[2] == dict(beam_size=3, joint="one_pass", timestamps=True) for c in model.calls)
    assert bool((parser.batches[0][0][1, 400:] == 0).all()) and parser.batches[0][0][1, :400].tolist() == list(range(16000, 16400))
    a, b = res
    assert b == {"text": "", "ids": [], "duration_s": 2.0, "segments": []}          # no speech
    assert a["text"] == "<1600>;<16000>;<32000>;" and a["ids"] == [1600, 16000, 32000] and a["duration_s"] == 4.0
    assert [(s["start_s"], s["end_s"], s["start_sample"]) for s in a["segments"]] == [(0.1, 0.6, 1600), (1.0, 1.025, 16000), (2.0, 3.0, 32000)]
    for s, (s0, _) in zip(a["segments"], segs[0]):
        assert s["score"] == -float(s0) and s["extra"] == "kept" and s["text"] == f"<{s0}>;"
        t0, t1 = s["tokens"]
        assert (t0["start_s"], t0["end_s"]) == (0.5 + s0 / 16000.0, 1.0 + s0 / 16000.0)          # moved by the segment's start
        assert (t0["start_frame"], t0["end_frame"]) == (5, 9)                                     # relative to the segment
        assert t1["start_s"] is None and t1["end_s"] is None
    # tokens None (timestamps off) stay None; context_ids follow the recording
    model.transcribe = lambda pack, **kw: [{"text": "x", "ids": [1], "score": 0.0, "tokens": None, "kw": kw} for _ in pack.wave]
    res = transcribe_long(model, parser, wav, torch.tensor([64000, 64000]), vad=StubVad([[(0, 400)], [(160, 800), (1600, 2400), (3200, 4000)]]), batch_size=2,
                          context_ids=[4, -1])
    assert [s["tokens"] for r in res for s in r["segments"]] == [None] * 4 and res[1]["text"] == "xxx"
    assert res[0]["segments"][0]["kw"] == {"context_ids": [4]} and [s["kw"]["context_ids"] for s in res[1]["segments"]] == [[-1, -1], [-1, -1], [-1]]


def test_transcribe_long_refuses_before_any_launch(stub_gather):
    from asr_chinese_e2e_amd.longform import check_max_segment, encoder_rows, transcribe_long
    from asr_chinese_e2e_amd.vad import EnergyVad
    wav = torch.zeros(1, 16000)

    class NoVad:
        def segments(self, *a):
            raise AssertionError("the VAD ran before the refusal")
    model, parser = StubModel(), StubParser()
    call = lambda **kw: transcribe_long(model, parser, wav, [16000], vad=NoVad(), **kw)      # noqa: E731
    # the stub parser counts 1 + n // 160 frames: a segment of f VAD frames is f + 2 of them, ceil((f + 2) / 3) encoder frames
    assert encoder_rows(parser, 2998) == 1000 and encoder_rows(parser, 2999) == 1001
    with pytest.raises(ValueError, match=r"largest admissible max_segment_s is 29\.98"):
        call(max_segment_s=30.0)
    with pytest.raises(ValueError, match=r"largest admissible max_segment_s is 29\.98"):
        call(max_segment_s=29.99)
    check_max_segment(parser, 1000, 2998, 29.98)
    with pytest.raises(ValueError, match="overlap"):
        call(pad_s=0.2)
    for name in ("min_silence_s", "min_speech_s", "pad_s", "max_segment_s"):
        for bad in (float("nan"), float("inf"), -1.0):
            with pytest.raises(ValueError, match=name):
                call(**{name: bad})
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="batch_size"):
            call(batch_size=bad)
    with pytest.raises(ValueError, match="wav_len"):
        transcribe_long(model, parser, wav, [16001], vad=NoVad())
    with pytest.raises(ValueError, match="context_ids"):
        call(context_ids=[0, 1])
    with pytest.raises(ValueError, match="proportion_threshold"):
        EnergyVad(proportion_threshold=1.5)
    assert stub_gather == [] and model.calls == [] and parser.batches == []


# ------------------------------------------------------------------------------------ transcribe.py
def test_transcribe_py_long_flags():
    import train
    import transcribe
    flags = lambda *a: train.parse_flags(list(a))      # noqa: E731
    for k in ("long", "vad_energy_threshold", "vad_energy_mean_scale", "vad_frames_context", "vad_proportion_threshold", "min_silence_s", "min_speech_s",
              "pad_s", "max_segment_s"):
        assert k in transcribe.CLI_KEYS
    assert transcribe.long_options({}) is None and transcribe.long_options(flags("--long=0")) is None      # without --long: what it does today
    vad, seg = transcribe.long_options(flags("--long=1"))
    assert (vad.energy_threshold, vad.energy_mean_scale, vad.frames_context, vad.proportion_threshold) == (5.0, 0.5, 0, 0.6) and seg == {}
    vad, seg = transcribe.long_options(flags("--long=1", "--vad_energy_threshold=6.5", "--vad_energy_mean_scale=0.4", "--vad_frames_context=2",
                                             "--vad_proportion_threshold=0.5", "--min_silence_s=0.5", "--min_speech_s=0.2", "--pad_s=0.25", "--max_segment_s=15"))
    assert (vad.energy_threshold, vad.energy_mean_scale, vad.frames_context, vad.proportion_threshold) == (6.5, 0.4, 2, 0.5)
    assert seg == dict(min_silence_s=0.5, min_speech_s=0.2, pad_s=0.25, max_segment_s=15)
    with pytest.raises(SystemExit, match="--stream"):
        transcribe.long_options(flags("--long=1", "--stream=1"))
    with pytest.raises(SystemExit, match="--sessions"):
        transcribe.long_options(flags("--long=1", "--sessions=4"))
    with pytest.raises(SystemExit, match="applies to --long=1"):
        transcribe.long_options(flags("--pad_s=0.2"))
    with pytest.raises(SystemExit, match="applies to --long=1"):
        transcribe.long_options(flags("--vad_frames_context=2", "--long=0"))
    with pytest.raises(SystemExit, match="overlap"):
        transcribe.long_options(flags("--long=1", "--pad_s=0.2"))
    with pytest.raises(SystemExit, match="proportion_threshold"):
        transcribe.long_options(flags("--long=1", "--vad_proportion_threshold=0"))
    with pytest.raises(SystemExit, match="max_segment_s"):
        transcribe.long_options(flags("--long=1", "--max_segment_s=-3"))
    # the refusal comes before a model is loaded or a GPU asked for
    with pytest.raises(SystemExit, match="--long=1 cannot be combined with --stream"):
        transcribe.transcribe(**flags("--long=1", "--stream=1", "--model_name=TransformerOffical"))


def test_segment_lines():
    import transcribe
    res = {"text": "ab", "ids": [5, 6], "duration_s": 3.0,
           "segments": [{"start_s": 0.5, "end_s": 1.5, "start_sample": 8000, "text": "a", "ids": [5], "score": -1.0, "confidence": 0.5,
                         "tokens": [{"id": 5, "start_s": 0.5, "end_s": 0.75}, {"id": 0, "start_s": None, "end_s": None}]},
                        {"start_s": 2.0, "end_s": 3.0, "start_sample": 32000, "text": "b", "ids": [6], "score": float("-inf"),
                         "tokens": [{"id": 6, "start_s": 2.5, "end_s": 2.875}]}]}
    lines = transcribe.segment_lines("f.wav", 24000, 8000, res, 0.25, 16000)
    assert [l.get("segment") for l in lines] == [0, 1, None]
    assert lines[0]["tokens"][0] == {"id": 5, "start_s": 0.75, "end_s": 1.0} and lines[0]["tokens"][1]["start_s"] is None
    assert lines[1]["tokens"][0]["end_s"] == 3.0 and lines[1]["score"] is None and lines[0]["confidence"] == 0.5      # never past the end; -inf is no JSON
    assert lines[2] == {"file": "f.wav", "duration_s": 3.0, "text": "ab", "ids": [5, 6], "segments": 2, "source_rate": 8000}
    assert lines[0]["file"] == "f.wav" and lines[0]["start_s"] == 0.5 and lines[0]["text"] == "a"


def test_transcribe_py_long_files(monkeypatch, capsys):
    """--long=1's loop with a stub model: a file at another rate is refused without --resample=1 and passed on with it, an empty file
    still reaches the model, the model's ValueError ends the run, and the lines come out in order."""
    import json
    import transcribe
    files = {"a.wav": (np.zeros(32000, dtype=np.float32), 16000), "b.wav": (np.zeros(8000, dtype=np.float32), 8000), "e.wav": (np.zeros(0, dtype=np.float32), 16000)}
    monkeypatch.setattr(transcribe, "load_wav", lambda path: files[path])
    calls = []

    class Model:
        def transcribe_long(self, parser, wav, wav_len, **kw):
            calls.append((tuple(wav.shape), wav_len, kw))
            if kw.get("max_segment_s") == 999:
                raise ValueError("past the table")
            dur = wav_len[0] / float(kw["source_rate"] or 16000)
            return [{"text": "x", "ids": [7], "duration_s": dur, "segments": [{"start_s": 0.0, "end_s": dur, "start_sample": 0, "text": "x", "ids": [7], "score": -1.0, "tokens": None}] if wav_len[0] else []}]
    run = lambda names, seg, resample: transcribe.transcribe_long_files(Model(), "parser", names, "vad", seg, 4, resample, 0.0, 16000, beam_size=3)      # noqa: E731
    with pytest.raises(SystemExit, match="sample rate 8000"):
        run(["b.wav"], {}, False)
    assert calls == []
    run(["a.wav", "b.wav", "e.wav"], {"pad_s": 0.05}, True)
    assert [(c[0], c[1], c[2]["source_rate"]) for c in calls] == [((1, 32000), [32000], None), ((1, 8000), [8000], 8000), ((1, 1), [0], None)]
    assert all(c[2]["vad"] == "vad" and c[2]["batch_size"] == 4 and c[2]["pad_s"] == 0.05 and c[2]["beam_size"] == 3 for c in calls)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert [(l["file"], l.get("segment"), l.get("segments")) for l in lines] == [("a.wav", 0, None), ("a.wav", None, 1), ("b.wav", 0, None), ("b.wav", None, 1), ("e.wav", None, 0)]
    assert lines[1]["duration_s"] == 2.0 and lines[3] == {"file": "b.wav", "duration_s": 1.0, "text": "x", "ids": [7], "segments": 1, "source_rate": 8000}
    with pytest.raises(SystemExit, match="past the table"):
        run(["a.wav"], {"max_segment_s": 999}, False)
