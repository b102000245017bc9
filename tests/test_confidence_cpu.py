"""Token confidence without a GPU: the float64 definitions (tests/confidence_ref.py) against closed forms, the run segmentation against
oracle/decode_ref.py's collapse, the float32 restatement inside the derived bounds, the refusals of the Python surface (raised before any
launch, on host-model stand-ins), and the C ABI of the three new entry points."""
import math
import os
import re
import types

import numpy as np
import pytest

from tests import confidence_ref as CR
from tests.helpers import ROOT

NAMES = ("asr_ctc_frame_stats", "asr_ctc_token_conf", "asr_session_ctc_step_tokens")
NINF = float("-inf")


# ------------------------------------------------------------------------------------------------ the definitions
def test_frame_stats_closed_forms():
    V = 7
    one_hot = np.full((2, V), -1e4)
    one_hot[0, 3], one_hot[1, 0] = 1e4, 1e4
    st = CR.frame_stats(one_hot)
    assert st["path"].tolist() == [3, 0] and st["ent"].tolist() == [1.0, 1.0] and st["best_lp"].tolist() == [0.0, 0.0]
    assert st["blank_lp"][0] == -2e4 and st["blank_lp"][1] == 0.0
    const = CR.frame_stats(np.full((1, V), 2.5))
    assert const["path"][0] == 0 and abs(const["ent"][0]) < 1e-15 and abs(const["best_lp"][0] + math.log(V)) < 1e-15      # the first maximum wins
    # -inf entries: p = 0 adds exactly 0 to H; two live classes of p = (0.8, 0.2)
    row = np.full((1, V), NINF)
    row[0, 2], row[0, 5] = math.log(0.8), math.log(0.2)
    st = CR.frame_stats(row)
    H = -(0.8 * math.log(0.8) + 0.2 * math.log(0.2))
    assert st["path"][0] == 2 and abs(st["ent"][0] - (1 - H / math.log(V))) < 1e-15 and not np.isnan(st["ent"]).any()
    assert st["blank_lp"][0] == NINF and abs(st["best_lp"][0] - math.log(0.8)) < 1e-15 and abs(st["lse"][0]) < 1e-15
    # two classes: ent = 1 - H2(p) / ln 2, 0 at p = 1/2 and 1 at p = 1
    for p in (0.5, 0.9, 0.999, 1.0 - 1e-12):
        st = CR.frame_stats(np.array([[math.log(p), math.log1p(-p)]]))
        H = -(p * math.log(p) + (1 - p) * math.log1p(-p))
        assert abs(st["ent"][0] - (1 - H / math.log(2))) < 1e-14
    assert CR.frame_stats(np.array([[0.0, 0.0]]))["ent"][0] == 0.0
    # an exponential that underflows adds 0, not NaN
    st = CR.frame_stats(np.array([[0.0, -800.0, -1e6]]))
    assert st["ent"][0] == 1.0 and st["lse"][0] == 0.0


def test_token_measures_and_utterance():
    rng = np.random.default_rng(0)
    st = CR.frame_stats(rng.standard_normal((12, 9)) * 3)
    m = CR.token_measures(st["logp"], st["ent"], 4, 3, 8)
    lp = st["logp"][3:9, 4]
    assert m["post_max"] == math.exp(lp.max()) and m["post_min"] == math.exp(lp.min()) and m["post_max"] >= m["post_mean"] >= m["post_min"]
    assert abs(math.log(m["post_mean"]) * 6 - lp.sum()) < 1e-12      # the geometric mean: ctc_align's logp
    assert abs(m["ent_mean"] - st["ent"][3:9].mean()) < 1e-15 and m["ent_min"] == st["ent"][3:9].min()
    one = CR.token_measures(st["logp"], st["ent"], 2, 5, 5)
    assert one["post_max"] == one["post_min"] and abs(one["post_mean"] - one["post_max"]) < 1e-15 and one["ent_mean"] == one["ent_min"]
    assert CR.utterance([0.5, None, 1.0]) == 0.75 and CR.utterance([None]) is None and CR.utterance([]) is None
    from asr_chinese_e2e_amd import confidence as C
    assert C.MEASURES == CR.MEASURES and C.utterance([0.5, None, 1.0]) == 0.75 and C.utterance([]) is None
    assert C.measure(None) is None and C.measure(True) == "post_max" and C.measure("ent_min") == "ent_min"
    with pytest.raises(ValueError, match="confidence must be"):
        C.measure("entropy")
    assert C.measures_dict([float("nan")] * 5) is None and C.measures_dict([1, 2, 3, 4, 5])["ent_min"] == 5.0


def test_greedy_runs_collapse_to_the_oracles_ids():
    from oracle import decode_ref as D
    rng = np.random.default_rng(3)
    for trial in range(120):
        small = trial < 40
        T, V = (int(rng.integers(1, 7)), 3) if small else (int(rng.integers(1, 40)), int(rng.integers(2, 5)))
        path = rng.integers(0, V, T).tolist()
        runs = CR.greedy_runs(path)
        if small:      # decode_ref's collapse, reached through its enumeration: only `path` has probability, so only its collapse scores 0
            logp = np.full((T, V), D.NEG)
            logp[np.arange(T), path] = 0.0
            ids = [r[0] for r in runs]
            assert D.ctc_label_logprob_bruteforce(logp, ids) == 0.0, path
            assert D.ctc_label_logprob_bruteforce(logp, ids + [1]) == D.NEG and (not ids or D.ctc_label_logprob_bruteforce(logp, ids[:-1]) == D.NEG)
        covered = [0] * T
        for y, s, e in runs:
            assert y != 0 and all(path[t] == y for t in range(s, e + 1))
            assert s == 0 or path[s - 1] != y
            assert e == T - 1 or path[e + 1] != y
            for t in range(s, e + 1):
                covered[t] += 1
        assert covered == [int(c != 0) for c in path]      # every non-blank frame lies in exactly one run
    assert CR.greedy_runs([0, 5, 5, 0, 5, 7, 7]) == [(5, 1, 2), (5, 4, 4), (7, 5, 6)]


def test_float32_restatement_stays_inside_the_bounds():
    rng = np.random.default_rng(1)
    worst = 0.0
    for V in (2, 63, 64, 65, 4232, 4233):
        x = (rng.standard_normal((24, V)) * rng.choice([0.1, 1.0, 4.0, 12.0], size=(24, 1))).astype(np.float32)
        x[0], x[1] = -1e4, 0.25
        x[0, V // 2] = 1e4
        x[2] = NINF
        x[2, 0], x[2, V - 1] = 0.5, -0.75
        want, bound, got = CR.frame_stats(x), CR.frame_bounds(x), CR.frame_stats_f32(x)
        assert got["ent"][0] == 1.0 and got["ent"][1] == 0.0 and not np.isnan(got["ent"]).any()
        rows = np.arange(len(x))
        for key, b in (("lse", bound["lse"]), ("best_lp", bound["lp"][rows, want["path"]]), ("blank_lp", bound["lp"][:, 0]), ("ent", bound["ent"])):
            fin = np.isfinite(want[key])
            ratio = np.abs(got[key][fin].astype(np.float64) - want[key][fin]) / b[fin]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (V, key, float(ratio.max()))
    print(f"float32 restatement: largest err / bound {worst:.3f}")


def test_the_fixed_step_input_has_the_runs_the_tests_need():
    x = CR.step_logits()
    assert x.shape == (CR.STEP_SLOTS, CR.STEP_T, CR.STEP_V) and x.dtype == np.float32
    assert np.array_equal(x, CR.step_logits())
    lengths = set()
    for b, n in enumerate(CR.STEP_LENS):
        assert CR.top2_gap(x[b, :n]).min() > 1e-3      # no frame's best class is a near tie (greedy against Viterbi)
        runs = CR.greedy_runs(CR.frame_stats(x[b, :n])["path"])
        lengths |= {e - s + 1 for _, s, e in runs}
        for C in (1, 5, 16, 64, 65):      # a run lies across a cut of every chunking
            assert any(s < k <= e for _, s, e in runs for k in range(C, n, C)), (b, C)
    assert 1 in lengths and 2 in lengths and max(lengths) > 64
    last = CR.frame_stats(x[2])["path"][-1]
    assert last != 0 and CR.frame_stats(x[0])["path"][-1] == 0      # slot 2 ends on an open run, slot 0 does not
    ids0 = [y for y, _, _ in CR.greedy_runs(CR.frame_stats(x[0])["path"])]
    assert ids0[:5] == [5, 7, 7, 3, 4]      # a repeat separated by a blank is a new token; 3 -> 4 closes and opens on one frame


# ------------------------------------------------------------------------------------------------ refusals before any launch
class _Model:
    decoding_chunk_size, decoding_left_chunks, use_ctc, V = 8, -1, True, 30
    vocab = types.SimpleNamespace(_id2token=[str(i) for i in range(30)])

    def frame_seconds(self):
        return 0.03


def test_python_surface_refuses_before_any_launch():
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.sessions import Sessions
    from asr_chinese_e2e_amd.stream import StreamingEncoder
    T = Models.TransformerCTC
    ctc = types.SimpleNamespace(use_ctc=True, use_decoder=False)
    att = types.SimpleNamespace(use_ctc=False, use_decoder=True)
    with pytest.raises(ValueError, match="timestamps"):
        T.transcribe(ctc, None, timestamps=False, confidence="post_max")
    with pytest.raises(ValueError, match="timestamps"):
        T.transcribe(att, None, timestamps=False, confidence=True)
    with pytest.raises(ValueError, match="CTC head"):
        T.transcribe(att, None, confidence="ent_mean")
    with pytest.raises(ValueError, match="confidence must be"):
        T.transcribe(ctc, None, confidence="entropy")
    with pytest.raises(ValueError, match="CTC head"):
        T.ctc_align(att, None, confidence="post_min")
    with pytest.raises(ValueError, match="confidence must be"):
        T.ctc_align(ctc, None, confidence="max")
    for make in (lambda **kw: Sessions(_Model(), 2, **kw), lambda **kw: StreamingEncoder(_Model(), 2, **kw)):
        with pytest.raises(ValueError, match="timed=True needs search='greedy'"):
            make(timed=True, search="prefix_beam")
        with pytest.raises(ValueError, match="confidence must be"):
            make(timed=True, confidence="best")
        with pytest.raises(ValueError, match="timed=True"):
            make().tokens(0) if make().__class__ is Sessions else make().tokens()
        timed = make(timed=True, confidence="ent_min")
        assert timed.log.which == "ent_min" and (timed.tokens(1) if isinstance(timed, Sessions) else timed.tokens()[1]) == []
    ss = Sessions(_Model(), 2, timed=True)
    ss.open(0)
    with pytest.raises(ValueError, match="timestamps"):
        ss.finish(0, timestamps=False, confidence="post_max")
    assert ss.status(0)["state"] == "open"      # the refusal freed nothing
    st = StreamingEncoder(_Model(), 1)
    with pytest.raises(ValueError, match="timestamps"):
        st.finish(timestamps=False, confidence=True)


def test_token_log_follows_the_step_buffer():
    """TokenLog over hand-made buffers of asr_session_ctc_step_tokens' layout: closed runs accumulate, the open run is replaced each
    tick and closed by the host, a reset empties the list."""
    import torch
    from asr_chinese_e2e_amd.confidence import TokenLog
    C, d = 4, 0.03
    log = TokenLog(2, "post_mean", [str(i) for i in range(30)], d)

    def buf(closed, open_):
        ints = torch.zeros(2, 13 + 9 * C, dtype=torch.int32)
        flt = ints.view(torch.float32)
        ints[0, 4 + C] = len(closed)
        for r, (y, s, e, five) in enumerate(closed + [open_]):
            lo = 5 + C + 8 * (r if r < len(closed) else C)
            if y is None:
                ints[0, lo] = -1
                continue
            ints[0, lo], ints[0, lo + 1], ints[0, lo + 2] = y, s, e
            flt[0, lo + 3:lo + 8] = torch.tensor(five)
        return ints
    five = [0.9, 0.5, 0.75, 0.8, 0.6]
    log.ingest(buf([(7, 1, 2, five)], (9, 3, 3, five)), C, [0])
    got = log.tokens(0)
    assert [(t["id"], t["start_frame"], t["end_frame"], t["final"]) for t in got] == [(7, 1, 2, True), (9, 3, 3, False)] and log.tokens(1) == []
    assert got[0]["confidence"] == 0.75 and got[0]["measures"]["post_min"] == 0.5 and got[0]["token"] == "7"
    assert got[0]["start_s"] == 1 * d and got[0]["end_s"] == 3 * d
    log.ingest(buf([], (9, 3, 7, five)), C, [0])
    assert [(t["id"], t["end_frame"], t["final"]) for t in log.tokens(0)] == [(7, 2, True), (9, 7, False)]
    log.ingest(buf([(9, 3, 8, five)], (None, 0, 0, five)), C, [0])
    assert [(t["id"], t["end_frame"], t["final"]) for t in log.tokens(0)] == [(7, 2, True), (9, 8, True)]
    log.ingest(buf([], (4, 12, 12, five)), C, [0])
    log.close(0)
    assert [t["final"] for t in log.tokens(0)] == [True, True, True] and log.tokens(0)[-1]["id"] == 4
    log.reset(0)
    assert log.tokens(0) == []


# ------------------------------------------------------------------------------------------------ the C ABI
def test_library_header_and_binding_agree_on_the_new_symbols():
    from asr_chinese_e2e_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asr_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n) and hasattr(_lib.fast, n), n
        decl = re.search(r"\bint\s+" + n + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{n} is not declared in include/asr_hip.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        kinds = [_lib.P if "*" in p else (_lib.F if p.startswith("float") else _lib.I) for p in params]
        assert kinds == _lib.SIGNATURES[n][1], n      # pointer / int / float, argument by argument
    assert _lib.lib.asr_abi_version() == 10      # additive: the ABI version stays


def _call(fn, base, **over):
    a = dict(base)
    a.update(over)
    return fn(*a.values())


def test_argument_checks_run_before_any_launch():
    """Every refusal is ASR_EINVAL (-1) / ASR_EDTYPE (-2) from the host-side checks with fake, never dereferenced pointers."""
    from asr_chinese_e2e_amd import _lib
    f = _lib.fast
    fs = dict(logits=1024, in_len=256, path=2048, best_lp=4096, blank_lp=8192, lse=16384, ent=32768, B=4, T=8, V=30, ld=30, blank=0, dtype=0, stream=None)
    for name in ("logits", "path", "best_lp", "blank_lp", "lse", "ent"):
        assert _call(f.asr_ctc_frame_stats, fs, **{name: None}) == -1 and "null pointer" in _lib.last_error(), name
    for over in (dict(B=0), dict(T=0), dict(V=1), dict(blank=30), dict(blank=-1), dict(ld=29), dict(path=2050), dict(best_lp=4098), dict(blank_lp=8194),
                 dict(lse=16386), dict(ent=32770), dict(logits=1026), dict(in_len=258)):
        assert _call(f.asr_ctc_frame_stats, fs, **over) == -1, over
    assert _call(f.asr_ctc_frame_stats, fs, dtype=5) == -2

    tc = dict(logits=1024, labels=256, lab_len=512, spans=2048, lse=4096, ent=8192, out=16384, B=3, T=40, V=50, ld=50, Lmax=7, dtype=0, stream=None)
    for name in ("logits", "labels", "lab_len", "spans", "lse", "ent", "out"):
        assert _call(f.asr_ctc_token_conf, tc, **{name: None}) == -1 and "null pointer" in _lib.last_error(), name
    for over in (dict(B=0), dict(T=0), dict(V=1), dict(ld=49), dict(Lmax=0), dict(Lmax=256), dict(labels=258), dict(spans=2050), dict(out=16386), dict(lse=4098)):
        assert _call(f.asr_ctc_token_conf, tc, **over) == -1, over
    assert _call(f.asr_ctc_token_conf, tc, dtype=2) == -2

    st = dict(path=1024, blank_lp=2048, best_lp=4096, ent=8192, n_valid=256, reset=512, state=16384, run=32768, out=65536, slots=4, C=8, blank=0,
              silence_lp=-0.2, stream=None)
    for name in ("path", "blank_lp", "best_lp", "ent", "n_valid", "reset", "state", "run", "out"):
        assert _call(f.asr_session_ctc_step_tokens, st, **{name: None}) == -1 and "null pointer" in _lib.last_error(), name
    for over in (dict(slots=0), dict(C=0), dict(blank=-1), dict(silence_lp=float("nan")), dict(state=16386), dict(run=32770), dict(path=1026), dict(out=65538),
                 dict(best_lp=4098), dict(ent=8194)):
        assert _call(f.asr_session_ctc_step_tokens, st, **over) == -1, over
