"""Long-recording alignment without a GPU: the definition (tests/align_long_ref.py) against brute force and against the existing
alignment semantics, the stitching of tokens and lines on hand-made spans, every refusal with stand-in models, align.py's flags and
collector output on a stubbed model, and the agreement of header, binding and library on the two new symbols."""
import json
import math
import os
import re
import wave

import numpy as np
import pytest
import torch

from tests import align_long_ref as A
from tests.helpers import ROOT

NEG = -math.inf
LABEL_SETS = [[], [1], [1, 2], [2, 2], [1, 1, 1], [3, 1, 3], [1, 2, 1], [1, 1, 2], [2, 1, 1]]


# ------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("seed", range(3))
def test_definition_matches_brute_force(seed):
    """Every (T, L) with T <= 7, L <= 3, repeated labels included: the score is the best alignment's to the bit (the same additions in
    the same order), the path is one of the best, and infeasible exactly when the frames are too few."""
    rng = np.random.RandomState(seed)
    for T in range(0, 8):
        for labels in LABEL_SETS:
            rows = rng.normal(0, 2.0, (T, 4)).astype(np.float32)
            lse = A.lse_of(rows) if T else np.zeros(0, np.float32)
            r = A.align(rows, lse, labels)
            best, paths = A.brute(rows, lse, labels)
            if not paths:
                assert r["score"] == NEG and (r["spans"] == -1).all() and (r["path"] == -1).all() and np.isneginf(r["tok"]).all()
                assert T < len(labels) + A.repeats(labels)
                continue
            assert T >= len(labels) + A.repeats(labels) and r["score"] == best
            if T:
                assert A.states_of(r["path"], r["spans"], T) in paths
            lp = A.emissions(rows, lse)
            for i, c in enumerate(labels):      # spans are the token's run; tok the f32 sum from 0.f in ascending t, the extremes
                a, b = r["spans"][i]
                assert (r["path"][a:b + 1] == i).all() and (a == 0 or r["path"][a - 1] != i) and (b == T - 1 or r["path"][b + 1] != i)
                sm = np.float32(0.0)
                for t in range(a, b + 1):
                    sm = np.float32(sm + lp[t, c])
                assert r["tok"][i, 0] == sm and r["tok"][i, 1] == lp[a:b + 1, c].max() and r["tok"][i, 2] == lp[a:b + 1, c].min()


def test_tie_rule_and_margin():
    """All-equal rows: every cell ties.  Read backwards from the end (the blank, on the tie), "s before s-1 before s-2" keeps a state as
    long as it is reachable, so the last blank takes every spare frame and the tokens sit as early as they can, one frame each, with the
    one blank the repeat needs.  The margin of a tied lattice is 0, of a peaky one far from it."""
    r = A.align(np.zeros((9, 5), np.float32), A.lse_of(np.zeros((9, 5))), [1, 2, 2], want_margin=True)
    assert r["margin"] == 0.0 and r["path"].tolist() == [0, 1, -1, 2, -1, -1, -1, -1, -1]
    rows, lse, lab = A.peaky_case(60, 20, 12, 3.0, 0)
    assert A.align(rows, lse, lab, want_margin=True)["margin"] > 1e-3


def test_definition_against_the_existing_alignment_semantics():
    """Where they overlap: fed the same float64 emissions, test_ctc_align_cpu's viterbi_ref (the restatement asr_ctc_align is pinned to)
    takes the same path and reaches the same score to the bit; and no single path beats the sum over all of them (oracle/decode_ref)."""
    from oracle.decode_ref import ctc_label_logprob_bruteforce
    from tests.test_ctc_align_cpu import viterbi_ref
    rng = np.random.RandomState(11)
    for T, labels in ((5, [1, 2]), (5, [2, 2]), (4, [3]), (6, [1, 3, 1]), (40, [1, 2, 2, 3, 1, 1, 2]), (3, [1, 1])):
        rows = rng.normal(0, 2.0, (T, 4)).astype(np.float32)
        lse = A.lse_of(rows)
        lp = A.emissions(rows, lse).astype(np.float64)
        r = A.align(rows, lse, labels)
        score, states = viterbi_ref(lp, labels)
        if states is None:
            assert r["score"] == NEG
            continue
        assert r["score"] == score and A.states_of(r["path"], r["spans"], T) == states
        if T <= 6:
            assert r["score"] <= ctc_label_logprob_bruteforce(lp, labels) + 1e-12


# ------------------------------------------------------------------------------------ stitching
class Vocabulary:
    PAD, UNK, BOS, EOS = "$", "%", "^", "&"
    _id2token = ["$", "%", "^", "&", "a", "b", "c", "d"]
    _token2id = {t: i for i, t in enumerate(_id2token)}
    _tokenize_fn = staticmethod(list)

    def convert_str(self, s, use_bos=True, use_eos=True):
        assert not use_bos and not use_eos
        return [self._token2id.get(c, 1) for c in s]


def test_text_ids():
    from asr_chinese_e2e_amd.align_long import text_ids
    v = Vocabulary()
    (lines, ids, line_of), (l2, ids2, of2), (l3, ids3, of3) = text_ids(v, 8, 0, ["a b\tc", ["ab", "", " x d "], [[4, 5], [], [1]]], 3)
    assert lines == [{"text": "abc", "ids": [4, 5, 6], "unk": 0}] and ids == [4, 5, 6] and line_of == [0, 0, 0]
    assert [l["text"] for l in l2] == ["ab", "", "xd"] and l2[2]["unk"] == 1 and ids2 == [4, 5, 1, 7] and of2 == [0, 0, 2, 2]
    assert [l["text"] for l in l3] == ["ab", "", "%"] and l3[2]["unk"] == 1 and ids3 == [4, 5, 1] and of3 == [0, 0, 2]
    with pytest.raises(ValueError, match="2 transcripts for 1"):
        text_ids(v, 8, 0, ["a", "b"], 1)
    with pytest.raises(ValueError, match=r"label 0: labels are ids in \[0, 8\) other than the blank"):
        text_ids(v, 8, 0, [[[4, 0]]], 1)
    with pytest.raises(ValueError, match="label 8"):
        text_ids(v, 8, 0, [[[8]]], 1)
    with pytest.raises(ValueError, match="label -1"):
        text_ids(v, 8, 0, [[[-1]]], 1)
    with pytest.raises(ValueError, match="8193 tokens, the limit is 8192"):
        text_ids(v, 8, 0, ["a" * 8193], 1)
    assert len(text_ids(v, 8, 0, ["a" * 8192], 1)[0][1]) == 8192


def test_stitching_on_hand_made_spans():
    """Two segments of 10 and 6 frames at 1.0 s and 5.0 s, frames of 30 ms; four tokens in three lines, the second token's run crossing
    the segment boundary (frames 8 .. 11), the middle line empty."""
    from asr_chinese_e2e_amd.align_long import stitch_alignment
    lines = [{"text": "ab", "ids": [4, 5], "unk": 0}, {"text": "", "ids": [], "unk": 0}, {"text": "cd", "ids": [6, 7], "unk": 0}]
    ids, line_of = [4, 5, 6, 7], [0, 0, 2, 2]
    segs, seg_rows = [(16000, 20800), (80000, 82880)], [10, 6]
    spans = [[2, 3], [8, 11], [12, 12], [14, 15]]
    tok = [[-0.5, -0.125, -0.375], [-2.0, -0.25, -1.0], [-0.25, -0.25, -0.25], [-1.0, -0.5, -0.5]]
    r = stitch_alignment(lines, ids, line_of, segs, seg_rows, -7.5, spans, tok, 0.03, Vocabulary._id2token, "post_mean", 6.0)
    assert r["score"] == -7.5 and r["duration_s"] == 6.0 and r["frames"] == 16 and r["segments"] == [(1.0, 1.3), (5.0, 5.18)]
    t = r["tokens"]
    assert [(x["id"], x["token"], x["line"], x["segment"], x["start_frame"], x["end_frame"]) for x in t] == \
        [(4, "a", 0, 0, 2, 3), (5, "b", 0, 0, 8, 11), (6, "c", 2, 1, 12, 12), (7, "d", 2, 1, 14, 15)]
    assert t[0]["start_s"] == 1.0 + 2 * 0.03 and t[0]["end_s"] == 1.0 + 4 * 0.03
    # the run that crosses: its start from the first segment's clock, its end from the second's (frame 11 is that segment's frame 1)
    assert t[1]["start_s"] == 1.0 + 8 * 0.03 and t[1]["end_s"] == 5.0 + 2 * 0.03
    assert t[2]["start_s"] == 5.0 + 2 * 0.03 and t[3]["end_s"] == 5.0 + 6 * 0.03
    assert t[1]["logp"] == -2.0 and t[1]["measures"] == {"post_max": math.exp(-0.25), "post_min": math.exp(-1.0), "post_mean": math.exp(-2.0 / 4)}
    assert t[1]["confidence"] == t[1]["measures"]["post_mean"]
    a, e, c = r["lines"]
    assert (a["start_s"], a["end_s"], a["logp"], a["frames"]) == (t[0]["start_s"], t[1]["end_s"], -2.5, 6)
    assert a["confidence"] == math.exp(-2.5 / 6) and a["min_confidence"] == min(math.exp(-0.25), math.exp(-0.5))
    assert e == {"text": "", "ids": [], "start_s": None, "end_s": None, "logp": None, "frames": None, "confidence": None, "min_confidence": None, "unk": 0}
    assert (c["logp"], c["frames"], c["start_s"], c["end_s"]) == (-1.25, 3, t[2]["start_s"], t[3]["end_s"])
    for l in (a, c):      # a line's times enclose its tokens'
        mine = [x for x in t if r["lines"][x["line"]] is l]
        assert l["start_s"] <= min(x["start_s"] for x in mine) and l["end_s"] >= max(x["end_s"] for x in mine)
    assert stitch_alignment(lines, ids, line_of, segs, seg_rows, -7.5, spans, tok, 0.03, Vocabulary._id2token, "post_max", 6.0)["tokens"][3]["confidence"] == math.exp(-0.5)
    # an infeasible recording: every token and every line carries None, the text and the segments stay
    bad = stitch_alignment(lines, ids, line_of, segs, seg_rows, NEG, [[-1, -1]] * 4, [[NEG] * 3] * 4, 0.03, Vocabulary._id2token, "post_mean", 6.0)
    assert bad["score"] == NEG and bad["segments"] == r["segments"] and bad["frames"] == 16
    for x in bad["tokens"]:
        assert x["id"] in ids and all(x[k] is None for k in ("start_s", "end_s", "segment", "start_frame", "end_frame", "logp", "measures", "confidence"))
    for l in bad["lines"]:
        assert all(l[k] is None for k in ("start_s", "end_s", "logp", "frames", "confidence", "min_confidence"))
    assert [l["text"] for l in bad["lines"]] == ["ab", "", "cd"]


# ------------------------------------------------------------------------------------ refusals, with stand-in models
class StubParser:
    lfr_n = 3

    def __init__(self):
        self.window = torch.zeros(1)

    def num_frames(self, n):
        return 1 + n // 160 if n > 0 else 0

    def parse_batch(self, wav, wav_len):
        raise AssertionError("the front end ran before the refusal")


class StubModel:
    use_ctc, V, vocab = True, 8, Vocabulary()

    def _ensure_engine(self, device):
        class Eng:
            pe = torch.zeros(1000, 4)
        return Eng()

    def _ctc_logits(self, pack):
        raise AssertionError("the encoder ran before the refusal")

    def frame_seconds(self):
        return 0.03


class NoVad:
    def segments(self, *a):
        raise AssertionError("the VAD ran before the refusal")


def test_align_long_refuses_before_any_launch(monkeypatch):
    from asr_chinese_e2e_amd import align_long as AL
    monkeypatch.setattr(AL.K, "segment_gather", lambda *a: (_ for _ in ()).throw(AssertionError("a kernel ran before the refusal")))
    wav, parser = torch.zeros(1, 16000), StubParser()
    call = lambda model=None, texts=("ab",), **kw: AL.align_long(model or StubModel(), parser, wav, [16000], list(texts), vad=NoVad(), **kw)      # noqa: E731
    headless = StubModel()
    headless.use_ctc = False
    with pytest.raises(ValueError, match="CTC head"):
        call(headless)
    with pytest.raises(ValueError, match="other than the blank"):
        call(texts=[[[4, 0]]])
    with pytest.raises(ValueError, match=r"in \[0, 8\)"):
        call(texts=[[[9]]])
    with pytest.raises(ValueError, match="8200 tokens, the limit is 8192"):
        call(texts=["ab" * 4100])
    with pytest.raises(ValueError, match="2 transcripts for 1 recordings"):
        call(texts=["a", "b"])
    for name in ("ent_mean", "ent_min"):
        with pytest.raises(ValueError, match="entropy measures"):
            call(confidence=name)
    with pytest.raises(ValueError, match="confidence must be"):
        call(confidence="loud")
    # what transcribe_long refuses about its options
    with pytest.raises(ValueError, match=r"largest admissible max_segment_s is 29\.98"):
        call(max_segment_s=30.0)
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
        AL.align_long(StubModel(), parser, wav, [16001], ["ab"], vad=NoVad())
    with pytest.raises(ValueError, match=r"wav must be \(B, S\)"):
        AL.align_long(StubModel(), parser, wav[0], [16000], ["ab"], vad=NoVad())


def test_align_long_refuses_past_max_bytes_after_the_vad(monkeypatch):
    """The rows and the workspace are known once the VAD has run: 2 segments of 3.0 s = 301 frames of the stub parser = 101 encoder frames
    each, V = 8 f32 rows (6464 bytes) and 202 frames x 64 bytes of back-pointers + 64 (12992): refused at max_bytes 19455, and the
    encoder is reached (the stub's assertion) at 19456."""
    from asr_chinese_e2e_amd import align_long as AL

    class Vad:
        def segments(self, wav, lens, *opts):
            return [[(0, 48000), (64000, 112000)]]
    wav, parser = torch.zeros(1, 120000), StubParser()
    assert AL.segment_rows(parser, 48000) == 101 and AL.K.ctc_align_long_workspace_bytes(1, 202, 2) == 202 * 64 + 64
    with pytest.raises(ValueError, match=r"202 frames of logits \(6464 bytes\) plus 12992 bytes of back-pointers for 2 tokens exceed max_bytes = 19455"):
        AL.align_long(StubModel(), parser, wav, [120000], ["ab"], vad=Vad(), max_bytes=19455)
    monkeypatch.setattr(AL.K, "segment_gather", lambda *a: (_ for _ in ()).throw(AssertionError("reached the gather")))
    with pytest.raises(AssertionError, match="reached the gather"):
        AL.align_long(StubModel(), parser, wav, [120000], ["ab"], vad=Vad(), max_bytes=19456)


def test_wrapper_checks_offsets_and_labels_on_the_host():
    """kernels.ctc_align_long refuses what the kernel would have to trust before it touches a device pointer (CPU tensors never get that far)."""
    from asr_chinese_e2e_amd import kernels as K
    rows, lse = torch.zeros(10, 8), torch.zeros(10)
    for kw, msg in ((dict(row_off=[0, 9]), "offsets must ascend"), (dict(row_off=[1, 10]), "offsets must ascend"), (dict(lab_off=[0, 2]), "offsets must ascend"),
                    (dict(row_off=[0, 11, 10], lab_off=[0, 1, 3]), "offsets must ascend"), (dict(lab_off=[0, 1, 3]), "R \\+ 1 each"),
                    (dict(labels=[1, 2, 8]), "label 2 = 8"), (dict(labels=[1, 0, 3]), "label 1 = 0"), (dict(labels=[1, -2, 3]), "label 1 = -2"),
                    (dict(blank=8), "blank = 8"), (dict(lse=torch.zeros(9)), "lse holds 9 values for 10 rows"),
                    (dict(rows=torch.zeros(10, 16)[:, ::2]), "unit column stride")):
        args = dict(rows=rows, lse=lse, row_off=[0, 10], labels=[1, 2, 3], lab_off=[0, 3], blank=0)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            K.ctc_align_long(**args)
    with pytest.raises(ValueError, match="recording 0 has 8193 labels, the limit is 8192"):
        K.ctc_align_long(rows, lse, [0, 10], [1] * 8193, [0, 8193])
    with pytest.raises(ValueError, match="no CPU fallback"):
        K.ctc_align_long(rows, lse, [0, 10], [1, 2, 3], [0, 3])


# ------------------------------------------------------------------------------------ the library
def test_header_binding_and_library_agree():
    from asr_chinese_e2e_amd import _lib
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    for name in ("asr_ctc_align_long", "asr_ctc_align_long_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
        assert re.search(r"\b" + name + r"\(", text)
    decl = re.search(r"int asr_ctc_align_long\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["asr_ctc_align_long"][1]) == 17
    assert int(re.search(r"#define\s+ASR_ALIGN_LONG_MAX_LABELS\s+(\d+)", text).group(1)) == _lib.ALIGN_LONG_MAX_LABELS == 8192
    assert _lib.lib.asr_abi_version() == 10 == _lib.ABI_VERSION
    make = open(os.path.join(ROOT, "asr_chinese_e2e_amd", "csrc", "Makefile")).read()
    assert "align_long.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1)
    wb = _lib.lib.asr_ctc_align_long_workspace_bytes
    assert wb(1, 100, 65) == 100 * 128 + 64 and wb(3, 9000, 8192) == 9000 * 8192 + 64 and wb(1, 0, 0) == 64 and wb(2, 7, 0) == 7 * 64 + 64
    assert wb(0, 5, 5) == 0 and wb(1, -1, 5) == 0
    assert _lib.fast.asr_ctc_align_long_workspace_bytes(2, 60000, 8192) == wb(2, 60000, 8192) == 60000 * 8192 + 64


def test_entry_point_validates_before_any_launch():
    from asr_chinese_e2e_amd import _lib
    f, ok = _lib.fast.asr_ctc_align_long, 64
    good = dict(rows=ok, lse=ok, row_off=ok, labels=ok, lab_off=ok, path=ok, spans=ok, tok=ok, score=ok, ws=ok, ws_bytes=4096, R=1, V=12, ld=12, dtype=0, blank=0,
                stream=None)
    call = lambda **kw: f(*{**good, **kw}.values())      # noqa: E731
    for name in ("rows", "lse", "row_off", "labels", "lab_off", "path", "spans", "tok", "score", "ws"):
        assert call(**{name: None}) == -1 and "asr_ctc_align_long: null pointer" in _lib.last_error(), name
    for kw, msg in ((dict(R=0), "R=0"), (dict(V=1), "V=1"), (dict(blank=12), "blank=12"), (dict(blank=-1), "blank=-1"), (dict(ld=11), "ld=11"),
                    (dict(ws_bytes=63), "workspace 63"), (dict(ws=72), "misaligned"), (dict(score=68), "misaligned"), (dict(rows=65, dtype=1), "misaligned")):
        assert call(**kw) == -1 and msg in _lib.last_error(), kw
    assert call(dtype=5) == -2


# ------------------------------------------------------------------------------------ align.py
def test_align_py_flags():
    import align
    import train
    flags = lambda *a: train.parse_flags(list(a))      # noqa: E731
    for k in ("ckpt", "wav", "text", "cmvn", "frontend", "resample", "min_confidence", "out_prefix", "part", "vad_energy_threshold", "vad_frames_context",
              "min_silence_s", "min_speech_s", "pad_s", "max_segment_s"):
        assert k in align.CLI_KEYS
    vad, seg, mc, conf, part = align.align_options(flags("--wav=a.wav", "--text=a.txt"))
    assert (vad.energy_threshold, vad.energy_mean_scale, vad.frames_context, vad.proportion_threshold) == (5.0, 0.5, 0, 0.6)
    assert seg == {} and mc == 0.0 and conf == "post_mean" and part == "train"
    vad, seg, mc, conf, part = align.align_options(flags("--wav=a.wav", "--text=a.txt", "--vad_energy_threshold=6.5", "--vad_frames_context=2", "--min_silence_s=0.5",
                                                         "--pad_s=0.25", "--max_segment_s=15", "--min_confidence=0.25", "--confidence=post_max", "--part=dev"))
    assert (vad.energy_threshold, vad.frames_context) == (6.5, 2) and seg == dict(min_silence_s=0.5, pad_s=0.25, max_segment_s=15)
    assert (mc, conf, part) == (0.25, "post_max", "dev")
    for args, msg in ((("--text=a.txt",), "--wav"), (("--wav=a.wav",), "--text"), (("--wav=a.wav", "--text=a.txt", "--pad_s=0.2"), "overlap"),
                      (("--wav=a.wav", "--text=a.txt", "--vad_proportion_threshold=0"), "proportion_threshold"),
                      (("--wav=a.wav", "--text=a.txt", "--min_confidence=1.5"), "min_confidence"), (("--wav=a.wav", "--text=a.txt", "--confidence=ent_mean"), "--confidence"),
                      (("--wav=a.wav", "--text=a.txt", "--part=eval"), "--part")):
        with pytest.raises(SystemExit, match=msg):
            align.align_options(flags(*args))
    # the refusal comes before a model is loaded or a GPU asked for
    with pytest.raises(SystemExit, match="--wav"):
        align.align(**flags("--text=a.txt", "--model_name=TransformerOffical"))


def test_align_py_lines_and_collector(monkeypatch, capsys, tmp_path):
    """align.py's loop on a stubbed model: three transcript lines at 8 kHz (--resample=1), one below --min_confidence, one empty; the
    kept line's wav holds the file's own samples at the reported range, and build_dataloader's reader accepts the collector file."""
    import align
    pcm = (np.arange(40000) % 20000 - 10000).astype("<i2")      # 5 s at 8 kHz
    monkeypatch.setattr(align, "read_pcm", lambda path: (pcm, 1, 8000))
    txt = tmp_path / "rec.txt"
    txt.write_text("ab\n\n  cd \nba\n", encoding="utf-8")
    assert align.read_lines(str(txt)) == ["ab", "cd", "ba"]
    calls = []

    def tok(i, line, s, e, lp):
        return {"id": i, "token": "x", "line": line, "start_s": s, "end_s": e, "segment": 0, "start_frame": 0, "end_frame": 0, "logp": lp,
                "measures": {"post_max": 1.0, "post_min": 1.0, "post_mean": 1.0}, "confidence": 1.0}

    class Model:
        def align_long(self, parser, wav, wav_len, texts, **kw):
            calls.append((tuple(wav.shape), wav_len, texts, kw))
            if kw.get("max_segment_s") == 999:
                raise ValueError("past the table")
            line = lambda text, ids, s, e, c: {"text": text, "ids": ids, "start_s": s, "end_s": e, "logp": None if s is None else -1.0,      # noqa: E731
                                               "frames": None if s is None else 4, "confidence": c, "min_confidence": c, "unk": 0}
            return [{"score": -3.0, "duration_s": 5.0, "frames": 100, "segments": [(0.5, 5.0)],
                     "tokens": [tok(4, 0, 0.5, 0.75, -0.5), tok(5, 0, 1.0, 1.5, -0.5), tok(6, 1, 2.0, 2.5, -2.0), tok(7, 1, 2.5, 3.0, -2.0), tok(5, 2, 4.0, 4.5, -0.1), tok(4, 2, 4.5, 5.01, -0.1)],
                     "lines": [line("ab", [4, 5], 0.5, 1.5, 0.8), line("cd", [6, 7], 2.0, 3.0, 0.2), line("ba", [5, 4], 4.0, 5.01, 0.9)]}]
    pfx = str(tmp_path / "out" / "rec")
    run = lambda resample, seg=None, mc=0.5: align.align_file(Model(), "parser", "rec.wav", ["ab", "cd", "ba"], "vad", seg or {}, 4, resample, 16000, "post_mean", mc, pfx, "train")      # noqa: E731
    with pytest.raises(SystemExit, match="sample rate 8000"):
        run(False)
    assert calls == []
    run(True, {"pad_s": 0.05})
    assert calls[0][0] == (1, 40000) and calls[0][1] == [40000] and calls[0][2] == [["ab", "cd", "ba"]]
    assert calls[0][3] == dict(vad="vad", batch_size=4, source_rate=8000, confidence="post_mean", pad_s=0.05)
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert [(l["file"], l.get("line"), l.get("kept")) for l in out] == [("rec.wav", 0, True), ("rec.wav", 1, False), ("rec.wav", 2, True), ("rec.wav", None, 2)]
    assert (out[0]["start_sample"], out[0]["end_sample"]) == (4000, 12000) and (out[2]["start_sample"], out[2]["end_sample"]) == (32000, 40000)
    assert out[2]["end_s"] == 5.0 and out[2]["tokens"][1]["end_s"] == 5.0 and len(out[0]["tokens"]) == 2      # never past the recording's end
    assert out[3] == {"file": "rec.wav", "duration_s": 5.0, "score": -3.0, "frames": 100, "lines": 3, "kept": 2, "segments": [[0.5, 5.0]]}
    man = [json.loads(l) for l in open(pfx + "_train.json", encoding="utf-8")]
    assert man == [{"wave": pfx + "_0.wav", "tgt": "ab"}, {"wave": pfx + "_2.wav", "tgt": "ba"}] and not os.path.exists(pfx + "_1.wav")
    for rec, (a, b) in zip(man, ((4000, 12000), (32000, 40000))):
        with wave.open(rec["wave"], "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 8000, b - a)
            assert np.array_equal(np.frombuffer(w.readframes(b - a), dtype="<i2"), pcm[a:b])
    # the collector file is what build_dataloader reads: its reader's loop over {"wave", "tgt"}, and WaveDataset takes the files
    from asr_chinese_e2e_amd.data_handler.loader import WaveDataset
    ds = WaveDataset([(r["wave"], r["tgt"]) for r in man], Vocabulary(), sample_rate=16000, resample=True)
    assert ds.num_samples(0) == 8000 and ds.rate(0) == 8000
    # an infeasible recording keeps nothing, and -inf is no JSON
    Model.align_long = lambda self, parser, wav, wav_len, texts, **kw: [{"score": NEG, "duration_s": 5.0, "frames": 3, "segments": [], "tokens": [dict(tok(4, 0, None, None, None), confidence=None, measures=None)],
                                                                         "lines": [{"text": "a", "ids": [4], "start_s": None, "end_s": None, "logp": None, "frames": None, "confidence": None, "min_confidence": None, "unk": 0}]}]
    run(True)
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert out[0]["kept"] is False and out[0]["start_sample"] is None and out[1]["score"] is None and out[1]["kept"] == 0
    assert len(open(pfx + "_train.json", encoding="utf-8").readlines()) == 2
    Model.align_long = lambda self, *a, **kw: (_ for _ in ()).throw(ValueError("past the table"))
    with pytest.raises(SystemExit, match="past the table"):
        run(True)
