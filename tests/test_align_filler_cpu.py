"""Filler frames of the long-recording alignment without a GPU: the definition (tests/align_filler_ref.py) against brute force, its tie
rule, its identities with tests/align_long_ref.py and what it means on a toy recording; the stitching of filler runs on hand-made paths;
every refusal before any launch; the agreement of header, binding and library on the new symbol; align.py's flags and printed lines."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import align_filler_ref as F
from tests import align_long_ref as A
from tests.helpers import ROOT
from tests.test_align_long_cpu import LABEL_SETS, NoVad, StubModel, StubParser, Vocabulary

NEG = -math.inf


def same(got, want):
    assert np.float64(got["score"]).view(np.int64) == np.float64(want["score"]).view(np.int64)
    assert np.array_equal(got["path"], want["path"]) and np.array_equal(got["spans"], want["spans"])
    assert np.array_equal(got["tok"].view(np.uint32), want["tok"].view(np.uint32))


# ------------------------------------------------------------------------------------ the definition
def test_definition_matches_brute_force():
    """Every (T, L) with T <= 7, L <= 3 over random flags and a random star (around the emissions, -inf on some frames): the score is the
    best alignment's to the bit, the path is one of the best, -2 stands exactly on the frames in a wide state with star above the blank,
    feasibility is align_long_ref's, and a share of the cases has filler frames."""
    with_filler = cases = 0
    for seed in range(3):
        rng = np.random.RandomState(seed)
        for T in range(0, 8):
            for labels in LABEL_SETS:
                L = len(labels)
                rows = rng.normal(0, 2.0, (T, 4)).astype(np.float32)
                lse = A.lse_of(rows) if T else np.zeros(0, np.float32)
                star = rng.normal(-1.5, 1.5, T).astype(np.float32)
                star[rng.uniform(size=T) < 0.2] = NEG
                gap, tail = (rng.uniform(size=L) < 0.6).astype(np.uint8), int(rng.uniform() < 0.6)
                r = F.align(rows, lse, star, labels, gap, tail)
                best, paths = F.brute(rows, lse, star, labels, gap, tail)
                plain = A.align(rows, lse, labels)
                assert (r["score"] == NEG) == (plain["score"] == NEG)      # a filler frame is still a frame in a state: feasibility stays
                if not paths:
                    assert r["score"] == NEG and (r["spans"] == -1).all() and (r["path"] == -1).all() and np.isneginf(r["tok"]).all()
                    continue
                assert r["score"] == best and r["score"] >= plain["score"]
                if not T:
                    continue
                states = F.states_of(r["path"], T)
                assert states in paths
                cases += 1
                with_filler += bool((r["path"] == -2).any())
                lp, wide = A.emissions(rows, lse), F.wide_states(L, gap, tail)
                for t, s in enumerate(states):
                    assert (r["path"][t] == -2) == bool(s % 2 == 0 and wide[s] and star[t] > lp[t, 0])
                for i, c in enumerate(labels):
                    a, b = r["spans"][i]
                    assert (r["path"][a:b + 1] == i).all() and (a == 0 or r["path"][a - 1] != i) and (b == T - 1 or r["path"][b + 1] != i)
                    sm = np.float32(0.0)
                    for t in range(a, b + 1):
                        sm = np.float32(sm + lp[t, c])
                    assert r["tok"][i, 0] == sm and r["tok"][i, 1] == lp[a:b + 1, c].max() and r["tok"][i, 2] == lp[a:b + 1, c].min()
    assert cases > 100 and with_filler > cases // 4, (cases, with_filler)      # of 3 x 8 x 9 draws, the feasible ones with T > 0


def test_hand_made_tie():
    """star[t] with the bits of eb[t]: the blank wins, so the frame is -1 and the score the plain one; one ulp above, it is -2."""
    rows = np.array([[0.0, 3.0, 0.0], [2.0, 0.0, 0.0], [2.0, 0.0, 0.0]], np.float32)
    lse = A.lse_of(rows)
    eb = A.emissions(rows, lse)[:, 0]
    r = F.align(rows, lse, eb.copy(), [1], [1], 1)
    assert r["path"].tolist() == [0, -1, -1]
    same(r, A.align(rows, lse, [1]))
    up = np.nextafter(eb, np.float32(np.inf))
    r = F.align(rows, lse, up, [1], [1], 1)
    assert r["path"].tolist() == [0, -2, -2] and r["score"] == np.float64(A.emissions(rows, lse)[0, 1]) + np.float64(up[1]) + np.float64(up[2])
    assert F.align(rows, lse, up, [1], [1], 0)["path"].tolist() == [0, -1, -1]      # the tail not wide: plain blanks


def test_identities_with_the_plain_definition():
    """All flags 0 (any star), and star = -inf (any flags): score, path, spans and tok of align_long_ref.align, bit for bit."""
    rng = np.random.RandomState(4)
    for T, L, V in ((0, 0, 5), (9, 0, 5), (3, 4, 5), (40, 12, 6), (200, 70, 12)):
        rows = rng.normal(0, 2.0, (T, V)).astype(np.float32)
        lab = 1 + rng.randint(0, V - 1, L)
        lse = A.lse_of(rows) if T else np.zeros(0, np.float32)
        want = A.align(rows, lse, lab)
        star = rng.normal(0.0, 1.0, T).astype(np.float32)      # often above the blank
        same(F.align(rows, lse, star, lab, np.zeros(L, np.uint8), 0), want)
        same(F.align(rows, lse, np.full(T, NEG, np.float32), lab, np.ones(L, np.uint8), 1), want)


def test_meaning_on_the_toy_recording():
    """[1, 2 | 3, 4] over 1 _ 2 _ 5 5 5 _ 5 _ 3 _ 4 _: at penalties 0 and 2 exactly the four class-5 frames are filler and every token
    keeps its own frame; penalty 20 gives the plain result, whose path has to spend label or blank states on the foreign frames."""
    for penalty in (0.0, 2.0):
        rows, lse, star, lab, gap, tail, peaked = F.toy(penalty)
        r = F.align(rows, lse, star, lab, gap, tail)
        assert np.array_equal(r["path"] == -2, peaked == 5), (penalty, r["path"])
        for i, c in enumerate(lab):
            t = int(np.flatnonzero(peaked == c)[0])
            assert tuple(r["spans"][i]) == (t, t)
        assert r["score"] > A.align(rows, lse, lab)["score"]
    rows, lse, star, lab, gap, tail, peaked = F.toy(20.0)
    r = F.align(rows, lse, star, lab, gap, tail)
    same(r, A.align(rows, lse, lab))
    assert not (r["path"] == -2).any()
    # a script that matches its audio (no foreign frames): the filler changes nothing, score included, at any penalty
    keep = peaked != 5
    for penalty in (0.0, 2.0):
        rows, lse, star, lab, gap, tail, _ = F.toy(penalty)
        same(F.align(rows[keep], lse[keep], star[keep], lab, gap, tail), A.align(rows[keep], lse[keep], lab))


# ------------------------------------------------------------------------------------ stitching
def test_stitching_of_filler_runs():
    """Two segments of 10 and 6 frames at 1.0 s and 5.0 s, frames of 30 ms; tokens 0, 1 in line 0, line 1 empty, tokens 2, 3 in line 2."""
    from asr_chinese_e2e_amd.align_long import stitch_fillers
    line_of, segs, seg_rows = [0, 0, 2, 2], [(16000, 20800), (80000, 82880)], [10, 6]
    #        0   1  2  3   4   5   6   7   8   9 | 10  11  12 13  14  15
    path = [-2, -2, 0, 1, -1, -2, -1, -1, -2, -2, -2, -1,  2, 3, -2, -2]
    n, runs = stitch_fillers(path, line_of, 3, segs, seg_rows, 0.03)
    assert n == 8 and [(r["start_frame"], r["end_frame"], r["frames"], r["segment"], r["before_token"], r["before_line"]) for r in runs] == \
        [(0, 1, 2, 0, 0, 0), (5, 5, 1, 0, 2, 2), (8, 10, 3, 0, 2, 2), (14, 15, 2, 1, 4, 3)]
    assert runs[0]["start_s"] == 1.0 and runs[0]["end_s"] == 1.0 + 2 * 0.03                      # in front of line 0
    assert runs[1]["start_s"] == 1.0 + 5 * 0.03 and runs[1]["end_s"] == 1.0 + 6 * 0.03            # the empty line is skipped: before_line 2
    assert runs[2]["start_s"] == 1.0 + 8 * 0.03 and runs[2]["end_s"] == 5.0 + 1 * 0.03            # across the boundary: each end on its own clock
    assert runs[3]["start_s"] == 5.0 + 4 * 0.03 and runs[3]["end_s"] == 5.0 + 6 * 0.03            # the tail: before_token L, before_line len(lines)
    assert set(runs[0]) == {"start_frame", "end_frame", "frames", "start_s", "end_s", "segment", "before_token", "before_line"}
    assert stitch_fillers([-1, 0, -1, 1, 2, 3, -1] + [-1] * 9, line_of, 3, segs, seg_rows, 0.03) == (0, [])      # no filler
    assert stitch_fillers([-1] * 16, line_of, 3, segs, seg_rows, 0.03, feasible=False) == (0, [])                # infeasible
    assert stitch_fillers([-2] * 16, [], 0, segs, seg_rows, 0.03)[1][0]["before_line"] == 0                      # no token at all: the tail


def test_filler_gaps():
    from asr_chinese_e2e_amd.align_long import filler_gaps
    lines = [{"ids": [4, 5]}, {"ids": []}, {"ids": [6]}, {"ids": [7, 4, 5]}]
    assert filler_gaps(lines, 6, "lines") == [1, 0, 1, 1, 0, 0] and filler_gaps(lines, 6, "tokens") == [1] * 6
    assert filler_gaps([{"ids": []}], 0, "lines") == []


# ------------------------------------------------------------------------------------ refusals
def test_align_long_refuses_filler_options_before_any_launch(monkeypatch):
    from asr_chinese_e2e_amd import align_long as AL
    monkeypatch.setattr(AL.K, "segment_gather", lambda *a: (_ for _ in ()).throw(AssertionError("a kernel ran before the refusal")))
    monkeypatch.setattr(AL.K, "ctc_align_long_filler", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a kernel ran before the refusal")))
    wav, parser = torch.zeros(1, 16000), StubParser()
    call = lambda **kw: AL.align_long(StubModel(), parser, wav, [16000], ["ab"], vad=NoVad(), **kw)      # noqa: E731
    for bad in (True, False, float("nan"), float("inf"), -float("inf"), -0.5, "2"):
        with pytest.raises(ValueError, match="filler must be"):
            call(filler=bad)
    with pytest.raises(ValueError, match="filler_scope must be one of lines, tokens"):
        call(filler=1.0, filler_scope="words")
    with pytest.raises(ValueError, match="filler_scope must be one of"):
        call(filler_scope="words")
    with pytest.raises(ValueError, match="without a filler penalty"):
        call(filler_scope="tokens")
    # what align_long refuses anyway is refused with the filler on too; accepted options reach the VAD (the stub's assertion)
    with pytest.raises(ValueError, match="other than the blank"):
        AL.align_long(StubModel(), parser, wav, [16000], [[[4, 0]]], vad=NoVad(), filler=1.0)
    for kw in (dict(filler=0), dict(filler=2.5, filler_scope="tokens"), dict(filler=None, filler_scope="lines")):
        with pytest.raises(AssertionError, match="the VAD ran"):
            call(**kw)
    # the model's method forwards both
    import inspect
    from asr_chinese_e2e_amd import Models
    sig = inspect.signature(Models.TransformerOffical.align_long).parameters
    assert sig["filler"].default is None and sig["filler_scope"].default == "lines"


def test_wrapper_checks_star_and_flags_on_the_host():
    """kernels.ctc_align_long_filler refuses what ctc_align_long refuses, and a wrong star / gap / gap_tail, before a device pointer is formed."""
    from asr_chinese_e2e_amd import kernels as K
    rows, lse, star = torch.zeros(10, 8), torch.zeros(10), torch.zeros(10)
    nan = star.clone()
    nan[7] = float("nan")
    for kw, msg in ((dict(row_off=[0, 9]), "offsets must ascend"), (dict(lab_off=[0, 1, 3]), "R \\+ 1 each"), (dict(labels=[1, 2, 8]), "label 2 = 8"),
                    (dict(labels=[1, 0, 3]), "label 1 = 0"), (dict(blank=8), "blank = 8"), (dict(lse=torch.zeros(9)), "lse holds 9 values for 10 rows"),
                    (dict(rows=torch.zeros(10, 16)[:, ::2]), "unit column stride"),
                    (dict(star=torch.zeros(9)), "star must be a contiguous f32 tensor of 10 values"), (dict(star=torch.zeros(11)), "star must be"),
                    (dict(star=torch.zeros(10, dtype=torch.float64)), "star must be"), (dict(star=torch.zeros(10, dtype=torch.bfloat16)), "star must be"),
                    (dict(star=[0.0] * 10), "star must be"), (dict(star=nan), "star holds NaN"),
                    (dict(gap=[1, 0]), "gap holds 2 flags for 3 labels"), (dict(gap=[1, 0, 0, 1]), "gap holds 4 flags for 3 labels"),
                    (dict(gap_tail=[]), "gap_tail holds 0 flags for 1 recordings"), (dict(gap_tail=[1, 1]), "gap_tail holds 2 flags for 1 recordings")):
        args = dict(rows=rows, lse=lse, star=star, row_off=[0, 10], labels=[1, 2, 3], lab_off=[0, 3], gap=[1, 0, 0], gap_tail=[1], blank=0)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            K.ctc_align_long_filler(**args)
    with pytest.raises(ValueError, match="ctc_align_long_filler: recording 0 has 8193 labels, the limit is 8192"):
        K.ctc_align_long_filler(rows, lse, star, [0, 10], [1] * 8193, [0, 8193], [0] * 8193, [0])
    with pytest.raises(ValueError, match="no CPU fallback"):
        K.ctc_align_long_filler(rows, lse, star, [0, 10], [1, 2, 3], [0, 3], [1, 0, 0], [1])


# ------------------------------------------------------------------------------------ the library
def test_header_binding_and_library_agree():
    from asr_chinese_e2e_amd import _lib
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    name = "asr_ctc_align_long_filler"
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
    decl = re.search(r"int asr_ctc_align_long_filler\((.*?)\);", text, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == 20
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["rows", "lse", "star", "row_off", "labels", "lab_off", "gap", "gap_tail", "path", "spans", "tok",
                                                                    "score", "ws", "ws_bytes", "R", "V", "ld", "dtype", "blank", "stream"]
    assert _lib.lib.asr_abi_version() == 10 == _lib.ABI_VERSION
    old = re.search(r"int asr_ctc_align_long\((.*?)\);", text, re.S).group(1)
    assert len(old.split(",")) == len(_lib.SIGNATURES["asr_ctc_align_long"][1]) == 17


def test_entry_point_validates_before_any_launch():
    from asr_chinese_e2e_amd import _lib
    f, ok = _lib.fast.asr_ctc_align_long_filler, 64
    good = dict(rows=ok, lse=ok, star=ok, row_off=ok, labels=ok, lab_off=ok, gap=ok, gap_tail=ok, path=ok, spans=ok, tok=ok, score=ok, ws=ok, ws_bytes=4096, R=1,
                V=12, ld=12, dtype=0, blank=0, stream=None)
    call = lambda **kw: f(*{**good, **kw}.values())      # noqa: E731
    for name in ("rows", "lse", "star", "row_off", "labels", "lab_off", "gap", "gap_tail", "path", "spans", "tok", "score", "ws"):
        assert call(**{name: None}) == -1 and "asr_ctc_align_long_filler: null pointer" in _lib.last_error(), name
    for kw, msg in ((dict(R=0), "R=0"), (dict(V=1), "V=1"), (dict(blank=12), "blank=12"), (dict(blank=-1), "blank=-1"), (dict(ld=11), "ld=11"),
                    (dict(ws_bytes=63), "workspace 63"), (dict(ws=72), "misaligned"), (dict(score=68), "misaligned"), (dict(rows=65, dtype=1), "misaligned"),
                    (dict(star=66), "misaligned")):
        assert call(**kw) == -1 and "asr_ctc_align_long_filler" in _lib.last_error() and msg in _lib.last_error(), kw
    assert call(dtype=5) == -2


# ------------------------------------------------------------------------------------ align.py
def test_align_py_filler_flags():
    import align
    import train
    flags = lambda *a: train.parse_flags(["--wav=a.wav", "--text=a.txt"] + list(a))      # noqa: E731
    assert "filler" in align.CLI_KEYS and "filler_scope" in align.CLI_KEYS
    assert len(align.align_options(flags("--filler=2"))) == 5
    assert align.filler_options(flags()) == {}
    assert align.filler_options(flags("--filler=2")) == {"filler": 2.0, "filler_scope": "lines"}
    assert align.filler_options(flags("--filler=0", "--filler_scope=tokens")) == {"filler": 0.0, "filler_scope": "tokens"}
    assert align.filler_options(flags("--filler=1.5", "--filler_scope=lines")) == {"filler": 1.5, "filler_scope": "lines"}
    for args, msg in ((("--filler=-1",), "--filler must"), (("--filler=nan",), "--filler must"), (("--filler=inf",), "--filler must"), (("--filler",), "--filler must"),
                      (("--filler=soft",), "--filler must"), (("--filler=2", "--filler_scope=words"), "--filler_scope must"),
                      (("--filler_scope=tokens",), "--filler_scope=tokens needs --filler")):
        with pytest.raises(SystemExit, match=msg):
            align.filler_options(flags(*args))
    # the refusal comes before a model is loaded or a GPU asked for
    with pytest.raises(SystemExit, match="--filler must"):
        align.align(**train.parse_flags(["--wav=a.wav", "--text=" + os.path.join(ROOT, "README.md"), "--filler=-2", "--model_name=TransformerOffical"]))


def test_align_py_prints_filler_lines(monkeypatch, capsys, tmp_path):
    """align.py's loop on a stubbed model: the keywords reach align_long, the filler runs are printed after the transcript lines and in
    front of the summary, never past the recording's end, and the cuts are the lines' own."""
    import align
    pcm = (np.arange(80000) % 20000 - 10000).astype("<i2")      # 5 s at 16 kHz
    monkeypatch.setattr(align, "read_pcm", lambda path: (pcm, 1, 16000))
    calls = []

    def tok(i, line, s, e):
        return {"id": i, "token": "x", "line": line, "start_s": s, "end_s": e, "segment": 0, "start_frame": 0, "end_frame": 0, "logp": -0.5,
                "measures": {"post_max": 1.0, "post_min": 1.0, "post_mean": 1.0}, "confidence": 1.0}

    def run_of(a, b, frames, line):
        return {"start_frame": 0, "end_frame": frames - 1, "frames": frames, "start_s": a, "end_s": b, "segment": 0, "before_token": line, "before_line": line}

    class Model:
        def align_long(self, parser, wav, wav_len, texts, **kw):
            calls.append(kw)
            line = lambda text, ids, s, e: {"text": text, "ids": ids, "start_s": s, "end_s": e, "logp": -1.0, "frames": 4, "confidence": 0.9,      # noqa: E731
                                            "min_confidence": 0.9, "unk": 0}
            res = {"score": -3.0, "duration_s": 5.0, "frames": 100, "segments": [(0.0, 5.0)], "tokens": [tok(4, 0, 1.0, 1.5), tok(5, 1, 3.0, 3.5)],
                   "lines": [line("a", [4], 1.0, 1.5), line("b", [5], 3.0, 3.5)]}
            if "filler" in kw:
                res.update(filler_frames=30, fillers=[run_of(0.0, 0.9, 10, 0), run_of(1.8, 2.7, 10, 1), run_of(4.2, 5.01, 10, 2)])
            return [res]
    pfx = str(tmp_path / "out" / "rec")
    run = lambda fill: align.align_file(Model(), "parser", "rec.wav", ["a", "b"], "vad", {}, 4, False, 16000, "post_mean", 0.0, pfx, "train", fill)      # noqa: E731
    run({"filler": 2.0, "filler_scope": "lines"})
    assert calls[0]["filler"] == 2.0 and calls[0]["filler_scope"] == "lines"
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert [l.get("line") for l in out[:2]] == [0, 1] and "kept" in out[-1] and out[-1]["lines"] == 2 and len(out) == 6
    assert out[2:5] == [{"filler": True, "start_s": 0.0, "end_s": 0.9, "frames": 10, "before_line": 0},
                        {"filler": True, "start_s": 1.8, "end_s": 2.7, "frames": 10, "before_line": 1},
                        {"filler": True, "start_s": 4.2, "end_s": 5.0, "frames": 10, "before_line": 2}]
    assert (out[0]["start_sample"], out[0]["end_sample"]) == (16000, 24000) and (out[1]["start_sample"], out[1]["end_sample"]) == (48000, 56000)
    assert len(open(pfx + "_train.json", encoding="utf-8").readlines()) == 2
    run(None)      # off: no keyword, no filler line
    assert "filler" not in calls[1] and "filler_scope" not in calls[1]
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert len(out) == 3 and not any("filler" in l for l in out)
