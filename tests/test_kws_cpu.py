"""Keyword spotting without a GPU: the definition (tests/kws_ref.py) against a float64 brute force over every alignment, its tie orders
and edges on hand-made rows, the resumable form under any cutting, KeywordList's parsing and refusals, the stitching of spot_long, the
header / binding / library agreement, the launchers' refusals before any launch, and spot.py's argument handling."""
import ctypes
import itertools
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import kws_ref as R
from tests.helpers import ROOT

NEG = R.NEG


def _peaky(seq, V, p=0.99):
    """lp (T, V): class seq[t] has probability p on frame t, the others share the rest."""
    lp = np.full((len(seq), V), math.log((1.0 - p) / (V - 1)), dtype=np.float32)
    for t, c in enumerate(seq):
        lp[t, c] = np.float32(math.log(p))
    return lp


# ------------------------------------------------------------------------------------------------ the definition
def test_float32_definition_equals_the_float64_brute_force():
    """Every T <= 6, every keyword of L <= 3 over V = 3 (ids 1, 2), log-probabilities on a grid of eighths (some -inf): float32 sums are
    exact there, so H must equal the enumeration's maximum exactly, and hs must be a start that reaches it."""
    rng = np.random.default_rng(0)
    kws = [list(k) for L in (1, 2, 3) for k in itertools.product((1, 2), repeat=L)]
    cases = 0
    for T in range(1, 7):
        for draw in range(3):
            lp = -(rng.integers(0, 9, (T, 3)) / 8.0).astype(np.float32)
            if draw == 2:
                lp[rng.random((T, 3)) < 0.15] = NEG
            H, hs = R.scan(lp, kws)
            for k, kw in enumerate(kws):
                want, starts = R.brute_force(lp, kw)
                assert np.array_equal(H[:, k].astype(np.float64), want), (T, kw)
                Hl, hl = R.scan_loops(lp, kw)      # the loops and the array form are one definition
                assert np.array_equal(Hl.view(np.int32), H[:, k].view(np.int32)) and np.array_equal(hl, hs[:, k])
                for t in range(T):
                    if want[t] > -np.inf:
                        assert hs[t, k] in starts[t], (T, kw, t)
                    elif t < len(kw) - 1 + sum(a == b for a, b in zip(kw, kw[1:])):
                        assert hs[t, k] == -1      # too early for any alignment: no start
                cases += 1
    assert cases == 6 * 3 * 14


def test_tie_orders():
    z, lp = np.float32(0.0), np.zeros(4, dtype=np.float32)
    # state 2 of "1 2": stay (start 9) against s-1 (start 3) against s-2 (start 5), all equal -> stay
    D, st = R.frame_step([z, z, z], [5, 3, 9], lp, [1, 2], 7)
    assert st == [7, 3, 9] and D == [z, z, z]      # state 1: stay (3) beats s-1 (5); state 0 is entered afresh
    # stay lower: s-1 and s-2 equal -> s-1
    D, st = R.frame_step([z, z, np.float32(-1.0)], [5, 3, 9], lp, [1, 2], 7)
    assert st[2] == 3
    # s-1 lower than s-2 -> s-2, but not across a doubled character
    D, st = R.frame_step([z, np.float32(-0.5), np.float32(-1.0)], [5, 3, 9], lp, [1, 2], 7)
    assert st[2] == 5 and D[2] == z
    D, st = R.frame_step([z, np.float32(-0.5), np.float32(-1.0)], [5, 3, 9], lp, [1, 1], 7)
    assert st[2] == 3 and D[2] == np.float32(-0.5)
    # nothing to continue: no start
    D, st = R.frame_step([NEG, NEG, NEG], [-1, -1, -1], lp, [1, 2], 0)
    assert st == [0, -1, -1] and D[1] == NEG and D[2] == NEG
    # all-zero rows: every comparison ties on every frame, and the end state keeps the earliest start
    H, hs = R.scan(np.zeros((9, 3), dtype=np.float32), [[1, 2], [1, 2, 1]])
    assert hs[:, 0].tolist() == [-1] + [0] * 8 and hs[:, 1].tolist() == [-1, -1] + [0] * 7
    # the first frame of equal H wins the run
    H = np.array([-1.0, -0.5, -0.5, -0.75, -9.0, -0.5], dtype=np.float32)
    assert R.hits_of(H, np.arange(6), np.float32(-1.0), 99) == [(1, 1, np.float32(-0.5)), (5, 5, np.float32(-0.5))]


def test_doubled_character_needs_its_blank():
    thr, span = R.threshold(2, 0.5), 100
    for seq, found in (([1, 0, 1], True), ([1, 1], False), ([1, 1, 0, 1, 1], True), ([0, 1, 1, 1, 0], False)):
        H, hs = R.scan(_peaky(seq, 3), [[1, 1]])
        assert bool(R.hits_of(H[:, 0], hs[:, 0], thr, span)) == found, seq
    H, hs = R.scan(_peaky([1, 0, 1], 3), [[1, 1]])
    assert R.hits_of(H[:, 0], hs[:, 0], thr, span)[0][:2] == (0, 2)


def test_threshold_and_span_edges():
    assert R.is_candidate(np.float32(-1.5), 3, 5, np.float32(-1.5), 3)                      # H == thr, and a match of exactly span frames
    assert not R.is_candidate(np.float32(-1.5), 2, 5, np.float32(-1.5), 3)                  # one frame more
    assert not R.is_candidate(np.nextafter(np.float32(-1.5), np.float32(-2)), 3, 5, np.float32(-1.5), 3)
    assert not R.is_candidate(np.float32("nan"), 3, 5, np.float32(-1.5), 3) and not R.is_candidate(np.float32(0), -1, 5, np.float32(-1.5), 3)
    # through the scan: "1 _ _ 2" spans 4 frames
    H, hs = R.scan(_peaky([1, 0, 0, 2], 3), [[1, 2]])
    assert R.hits_of(H[:, 0], hs[:, 0], R.threshold(2, 0.5), 4) == [(0, 3, H[3, 0])] and R.hits_of(H[:, 0], hs[:, 0], R.threshold(2, 0.5), 3) == []
    for L, p in ((1, 0.5), (2, 0.5), (7, 0.3), (16, 1e-6), (3, 1.0)):
        t = R.threshold(L, p)
        assert t.dtype == np.float32 and t == np.float32(L * math.log(p)) and t <= 0
    from asr_chinese_e2e_amd import keywords as KW
    assert KW.threshold_lp(7, 0.3) == float(R.threshold(7, 0.3))
    assert [R.max_token_frames(0.5, d) for d in (0.03, 0.04, 0.5, 0.6, 0.01)] == [16, 12, 1, 1, 50]      # floor, never below 1; 0.5 / 0.01 is 50, not 49
    assert R.span_cap(3, 0.5, 0.03) == 48 == KW.KeywordList([[1, 2, 3]]).spans(0.03)[0]


def test_the_peaky_toy():
    seq = [1, 0, 2, 0, 0, 1, 1, 0, 2, 0, 3, 0, 1] + [0] * 40 + [2]
    H, hs = R.scan(_peaky(seq, 4), [[1, 2]])
    thr = R.threshold(2, 0.5)
    hits = R.hits_of(H[:, 0], hs[:, 0], thr, R.span_cap(2, 0.5, 0.03))
    assert [h[:2] for h in hits] == [(0, 2), (6, 8)]      # (6, 8): the start is the LAST frame of the "1 1" run
    lifted = R.hits_of(H[:, 0], hs[:, 0], thr, 10 ** 6)
    assert [h[:2] for h in lifted] == [(0, 2), (6, 8), (12, 53)]      # blanks are almost free: only the cap keeps the long gap out


def test_any_cutting_of_a_stream_gives_the_whole():
    rng = np.random.default_rng(4)
    kws = [[1], [1, 2], [2, 2], [3, 1, 2], [1, 2, 3, 1, 2]]
    thr, span = [R.threshold(len(k), 0.3) for k in kws], [R.span_cap(len(k), 0.2, 0.03) for k in kws]
    for trial in range(20):
        T = int(rng.integers(1, 90))
        seq = [int(rng.choice([0, 0, 1, 2, 3])) for _ in range(T)]
        lp = _peaky(seq, 4, 0.9)
        whole = R.search([lp], kws, thr, span)[0]
        st, got, at = R.Stream(kws, thr, span), [[] for _ in kws], 0
        while at < T:
            n = min(int(rng.choice([0, 0, 1, 5, 16, 64, 65])), T - at)
            for k, h in enumerate(st.push(lp[at:at + n])):
                got[k] += h
            at += n
        for k, h in enumerate(st.push(lp[:0], final=True)):
            got[k] += h
        assert got == whole
    assert sum(len(h) for h in whole) > 0


def test_compact_orders_by_keyword_then_end_and_counts_what_it_drops():
    per = [[(0, 2, np.float32(-0.5)), (5, 9, np.float32(-0.25)), (11, 12, np.float32(-1))], [], [(1, 1, np.float32(-0.125))]]
    n, dropped, rows = R.compact(per, 2, 8)
    assert (n, dropped) == (3, 1) and rows[:3, :3].tolist() == [[0, 0, 2], [0, 5, 9], [2, 1, 1]] and not rows[3:].any()
    assert rows[1, 3] == R.bits(np.float32(-0.25))
    n, dropped, rows = R.compact(per, 2, 2)
    assert (n, dropped) == (2, 2) and rows[:, 0].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ KeywordList
def test_keyword_list_tables_and_refusals(tmp_path):
    from asr_chinese_e2e_amd.keywords import KeywordList
    kl = KeywordList([[5, 6, 7, 8, 9], [1, 2], ([3], 0.25), [4] * 16, [1, 2]], threshold=0.5, vocab_size=30)
    assert kl.K == 5 and kl.ids[2] == (3,) and kl.thresholds == (0.5, 0.5, 0.25, 0.5, 0.5) and kl.ids[1] == kl.ids[4]      # duplicates stay
    assert [np.float32(t) for t in kl.thr] == [R.threshold(len(i), p) for i, p in zip(kl.ids, kl.thresholds)]
    assert kl.order == (1, 2, 4, 0, 3)      # by length bucket (<= 4, <= 8, <= 16), stable inside one
    tok, ln, thr, index = kl._host
    assert index.tolist() == [1, 2, 4, 0, 3] and ln.tolist() == [2, 1, 2, 5, 16] and tok[3, :5].tolist() == [5, 6, 7, 8, 9] and tok[0].tolist() == [1, 2] + [0] * 14
    assert thr.dtype == torch.float32 and thr[1].item() == float(R.threshold(1, 0.25))
    assert kl.hits_per_keyword == 8 and kl.max_hits == 40 and KeywordList([[1]] * 300).max_hits == 1024
    with pytest.raises(AttributeError):
        kl.K = 3
    for bad, msg in (([], "no phrase"), ([[]], "empty"), ([[1, 0]], "blank"), ([[1] * 17], "at most 16"), ([[30]], "outside"), ([[-1]], "outside"),
                     ([([1], 0.0)], r"\(0, 1\]"), ([([1], 1.5)], r"\(0, 1\]"), ([([1], float("nan"))], r"\(0, 1\]"), ([([1], float("inf"))], r"\(0, 1\]"),
                     ([([1], "x")], "not a number")):
        with pytest.raises(ValueError, match=msg):
            KeywordList(bad, vocab_size=30)
    for kw_, msg in ((dict(threshold=0), r"\(0, 1\]"), (dict(max_token_s=0), "max_token_s"), (dict(max_token_s=float("inf")), "max_token_s"),
                     (dict(hits_per_keyword=0), "hits_per_keyword"), (dict(hits_per_keyword=65), "hits_per_keyword"), (dict(hits_per_keyword=2.5), "hits_per_keyword"),
                     (dict(max_hits=0), "max_hits")):
        with pytest.raises(ValueError, match=msg):
            KeywordList([[1]], **kw_)
    with pytest.raises(ValueError, match="outside"):
        KeywordList([[1, 40]]).check_vocab(30)
    # from_file: one phrase per line, an optional tab and threshold, blank lines skipped, duplicates kept
    vocab = {"_": 0, "a": 1, "b": 2, "c": 3}
    path = tmp_path / "kw.txt"
    path.write_text("ab\n\n c a \t0.25\nab\nb\t\n", encoding="utf-8")
    kl = KeywordList.from_file(str(path), vocab, threshold=0.6)
    assert kl.ids == ((1, 2), (3, 1), (1, 2), (2,)) and kl.thresholds == (0.6, 0.25, 0.6, 0.6) and kl.texts == ("ab", "ca", "ab", "b") and kl.vocab_size == 4
    assert kl.hit(1, 3, 7, -0.5, 0.03) == {"keyword": 1, "phrase": "ca", "ids": [3, 1], "start_frame": 3, "end_frame": 7, "start_s": 3 * 0.03, "end_s": 8 * 0.03,
                                           "score": -0.5, "confidence": math.exp(-0.25)}
    for text, msg in (("ax\n", "line 1: character 'x'"), ("a\nb\t2\n", r"line 2: threshold 2.0 outside"), ("a\tq\n", "line 1: threshold 'q'"),
                      ("\t0.5\n", "line 1: a threshold without a phrase"), ("a_\n", "line 1: the phrase holds the CTC blank"), ("a" * 17 + "\n", "line 1: 17 characters"),
                      ("\n \n", "no phrase")):
        path.write_text(text, encoding="utf-8")
        with pytest.raises(ValueError, match=msg):
            KeywordList.from_file(str(path), vocab)


def test_spot_long_stitching():
    from asr_chinese_e2e_amd.keywords import stitch_hits
    h = dict(keyword=0, phrase="ab", ids=[1, 2], start_frame=3, end_frame=5, start_s=0.09, end_s=0.18, score=-0.5, confidence=0.7)
    res = [{"hits": [h], "dropped": 0}, {"hits": [], "dropped": 2}, {"hits": [dict(h, keyword=1), h], "dropped": 1}]
    got = stitch_hits(res, [(1600, 32000), (40000, 48000), (64000, 80000)])
    assert got["dropped"] == 3 and [x["segment"] for x in got["hits"]] == [0, 2, 2] and [x["keyword"] for x in got["hits"]] == [0, 1, 0]
    assert got["hits"][0]["start_s"] == 0.09 + 0.1 and got["hits"][2]["end_s"] == 0.18 + 4.0
    assert all(x["start_frame"] == 3 and x["end_frame"] == 5 for x in got["hits"])      # frames stay relative to the segment
    assert stitch_hits([], []) == {"hits": [], "dropped": 0}      # a recording without speech


class _Model:
    decoding_chunk_size, decoding_left_chunks, use_ctc, use_decoder, V = 8, -1, True, True, 30
    vocab = types.SimpleNamespace(_id2token=[str(i) for i in range(30)])

    def frame_seconds(self):
        return 0.03


def test_model_level_refusals_before_any_launch():
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.keywords import KeywordList
    from asr_chinese_e2e_amd.sessions import Sessions
    from asr_chinese_e2e_amd.stream import StreamingEncoder
    T = Models.TransformerOffical
    kl = KeywordList([[1, 2]])
    headless = types.SimpleNamespace(use_ctc=False, use_decoder=True, V=30)
    with pytest.raises(ValueError, match="CTC head"):
        T.spot_keywords(headless, None, kl)
    with pytest.raises(ValueError, match="CTC head"):
        T.spot_long(headless, None, None, None, kl)
    stub = types.SimpleNamespace(use_ctc=True, use_decoder=True, V=30)
    with pytest.raises(ValueError, match="KeywordList"):
        T.spot_keywords(stub, None, [[1, 2]])
    with pytest.raises(ValueError, match="outside"):
        T.spot_keywords(stub, None, KeywordList([[1, 31]]))
    for make in (Sessions, StreamingEncoder):
        with pytest.raises(ValueError, match="KeywordList"):
            make(_Model(), 2, keywords=[[1, 2]])
        with pytest.raises(ValueError, match="blank_skip"):
            make(_Model(), 2, search="prefix_beam", blank_skip=0.98, keywords=kl)
        with pytest.raises(ValueError, match="outside"):
            make(_Model(), 2, keywords=KeywordList([[1, 31]]))
    ss = Sessions(_Model(), 2, keywords=kl)
    assert ss.kw is kl and ss.kw_rows == 8 and ss.keyword_hits(0) == [] and ss.keywords_dropped(1) == 0
    with pytest.raises(ValueError, match="keyword_hits"):
        Sessions(_Model(), 2).keyword_hits(0)
    import inspect
    for fn in (T.stream, T.sessions):
        assert inspect.signature(fn).parameters["keywords"].default is None


# ------------------------------------------------------------------------------------------------ header, binding, library
ENTRY_POINTS = {"asr_kws_state_bytes": 2, "asr_kws_records_bytes": 3, "asr_kws_search": 14, "asr_kws_chunk": 17, "asr_kws_compact": 10, "asr_kws_state_init": 4,
                "asr_kws_state_reset": 5}


def test_header_binding_and_library_list_the_same_entry_points():
    from asr_chinese_e2e_amd import _lib
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.keywords import KwsTables
    assert _lib.lib.asr_abi_version() == 10 == _lib.ABI_VERSION      # additive: the ABI version stays
    raw = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(asr_kws_[a-z_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS) == sorted(n for n in _lib.SIGNATURES if n.startswith("asr_kws_"))
    for name, n_args in ENTRY_POINTS.items():
        assert hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    for macro, value in (("ASR_KWS_MAX_LEN", _lib.KWS_MAX_LEN), ("ASR_KWS_MAX_KEYWORDS", _lib.KWS_MAX_KEYWORDS), ("ASR_KWS_MAX_CAP", _lib.KWS_MAX_CAP)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", raw).group(1)) == value
    fields = re.search(r"typedef struct asr_kws_list \{(.*?)\} asr_kws_list;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [n for n, _ in KwsTables._fields_]
    assert ctypes.sizeof(KwsTables) == 8 * 8 + 8
    make = open(os.path.join(ROOT, "asr_chinese_e2e_amd", "csrc", "Makefile")).read()
    assert "kws.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1)
    for name in ("kws_search", "kws_chunk", "kws_compact", "kws_unpack", "kws_state", "kws_state_reset"):
        assert hasattr(K, name)
    assert _lib.fast.asr_kws_state_bytes(3, 65) == 3 * 2 * 67 * 64 * 4 and _lib.fast.asr_kws_records_bytes(2, 5, 8) == 2 * 5 * 8 * 3 * 4
    assert _lib.fast.asr_kws_state_bytes(0, 5) == 0 == _lib.fast.asr_kws_records_bytes(2, 0, 8)


class _Tables:
    """A keyword list whose host copies are real memory and whose device pointers are fake (aligned, never read)."""

    def __init__(self, toks, index=None):
        from asr_chinese_e2e_amd.keywords import KwsTables
        K_ = len(toks)
        self.tok = np.zeros((K_, 16), dtype=np.int32)
        for j, t in enumerate(toks):
            self.tok[j, :min(len(t), 16)] = t[:16]
        self.len = np.array([len(t) for t in toks], dtype=np.int32)
        self.index = np.arange(K_, dtype=np.int32) if index is None else np.array(index, dtype=np.int32)
        self.struct = KwsTables(1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, self.tok.ctypes.data, self.len.ctypes.data, self.index.ctypes.data, K_)
        self.addr = ctypes.addressof(self.struct)


A = 1 << 24
SEARCH = dict(logits=A, lse=2 * A, in_len=3 * A, kw=None, cnt=4 * A, rec=5 * A, B=2, T=10, V=30, ld=30, blank=0, cap=8, dtype=0, stream=None)
CHUNK = dict(logits=A, lse=2 * A, n_valid=3 * A, reset=4 * A, final=5 * A, kw=None, state=6 * A, cnt=7 * A, rec=8 * A, slots=2, C=10, V=30, ld=30, blank=0, cap=8,
             dtype=0, stream=None)


@pytest.mark.parametrize("name, ok", [("asr_kws_search", SEARCH), ("asr_kws_chunk", CHUNK)])
def test_launchers_refuse_before_any_launch(name, ok):
    """The pointers are fake and never dereferenced, so no case here may pass the checks."""
    from asr_chinese_e2e_amd import _lib
    good = _Tables([[1, 2], [3], [4] * 16])

    def refused(words, code=-1, **over):
        a = {**ok, "kw": good.addr, **over}
        assert getattr(_lib.fast, name)(*a.values()) == code, over
        err = _lib.last_error()
        assert err.startswith(name + ":") and any(w in err for w in words), (over, err)

    for arg, v in ok.items():
        if isinstance(v, int) and v >= A and arg != "in_len":      # in_len alone is optional
            refused(["null pointer"], **{arg: None})
            refused(["misaligned"], **{arg: v + (1 if arg == "logits" else 2)})
    refused(["null keyword list"], kw=None)
    refused(["misaligned"], logits=A + 2)      # f32 rows on a 2-byte boundary
    for tables, words in ((_Tables([[1, 2], []]), ["length 0"]), (_Tables([[1] * 17]), ["length 17"]), (_Tables([[1, 0]]), ["blank"]), (_Tables([[1, 30]]), ["outside"]),
                          (_Tables([[-1]]), ["outside"]), (_Tables([[1], [2]], index=[0, 0]), ["taken"]), (_Tables([[1], [2]], index=[0, 2]), ["taken"])):
        refused(words, kw=tables.addr)
    empty = _Tables([[1]])
    empty.struct.K = 0
    refused(["K=0"], kw=empty.addr)
    for field in ("tok", "len", "thr", "span", "index", "host_tok", "host_len", "host_index"):
        broken = _Tables([[1, 2]])
        setattr(broken.struct, field, None)
        refused(["null pointer in the keyword list"], kw=broken.addr)
    refused(["blank"], blank=1)      # the list holds id 1
    for over in (dict(V=1), dict(blank=30), dict(blank=-1)):
        refused(["bad shape"], **over)
    for arg in ("B" if "B" in ok else "slots", "T" if "T" in ok else "C", "cap"):
        refused(["bad shape"], **{arg: 0})
    refused(["bad shape"], cap=65)
    refused(["bad shape"], **{"B" if "B" in ok else "slots": 70000})
    refused(["row stride"], ld=29)
    refused(["dtype"], code=-2, dtype=2)


def test_compact_and_state_entries_refuse_before_any_launch():
    from asr_chinese_e2e_amd import _lib
    f = _lib.fast
    ok = dict(cnt=A, rec=2 * A, count=3 * A, dropped=4 * A, hits=5 * A, B=2, K=5, cap=8, max_hits=16, stream=None)
    for over in [{n: None} for n in ("cnt", "rec", "count", "dropped", "hits")] + [dict(B=0), dict(K=0), dict(cap=0), dict(cap=65), dict(max_hits=0), dict(K=65537),
                                                                                   dict(B=70000), dict(hits=5 * A + 2)]:
        assert f.asr_kws_compact(*{**ok, **over}.values()) == -1, over
        assert _lib.last_error().startswith("asr_kws_compact:")
    for bad in ((None, 2, 5), (A + 2, 2, 5), (A, 0, 5), (A, 2, 0), (A, 70000, 5), (A, 2, 65537)):
        assert f.asr_kws_state_init(bad[0], bad[1], bad[2], None) == -1, bad
        assert _lib.last_error().startswith("asr_kws_state_init:")
    for bad in ((None, A, 2, 5), (A, None, 2, 5), (A, A + 1, 2, 5), (A, A, 0, 5), (A, A, 2, 0)):
        assert f.asr_kws_state_reset(*bad, None) == -1, bad
        assert _lib.last_error().startswith("asr_kws_state_reset:")


# ------------------------------------------------------------------------------------------------ spot.py
def test_spot_py_argument_handling():
    import spot
    base = dict(keywords="kw.txt", wavs="a.wav")
    kw, long_form = spot.spot_options(dict(base))
    assert kw == dict(threshold=0.5, max_token_s=0.5, hits_per_keyword=8) and long_form is None
    kw, long_form = spot.spot_options(dict(base, threshold=0.25, hits=3, long=1, min_silence_s=0.5, vad_energy_threshold=6.0))
    assert kw["threshold"] == 0.25 and kw["hits_per_keyword"] == 3 and long_form[1] == {"min_silence_s": 0.5} and long_form[0].energy_threshold == 6.0
    for bad, msg in ((dict(wavs="a.wav"), "--keywords"), (dict(keywords="kw.txt"), "--wavs"), (dict(base, threshold=0), "--threshold"), (dict(base, threshold=1.5), "--threshold"),
                     (dict(base, threshold="x"), "--threshold"), (dict(base, threshold=True), "--threshold"), (dict(base, max_token_s=0), "--max_token_s"),
                     (dict(base, hits=0), "--hits"), (dict(base, hits=2.5), "--hits"), (dict(base, hits=65), "--hits"), (dict(base, min_silence_s=0.5), "--long=1"),
                     (dict(base, long=1, pad_s=1.0), "pad_s"), (dict(base, long=1, vad_frames_context=-1), "frames_context")):
        with pytest.raises(SystemExit, match=msg):
            spot.spot_options(bad)
    h = dict(keyword=0, phrase="ab", ids=[1, 2], start_frame=3, end_frame=5, start_s=0.09, end_s=0.18, score=-0.5, confidence=0.7)
    lines = spot.hit_lines("a.wav", 0.17, {"hits": [h], "dropped": 2})
    assert lines == [dict({"file": "a.wav"}, **dict(h, end_s=0.17)), {"file": "a.wav", "duration_s": 0.17, "hits": 1, "dropped": 2}]      # never past the audio's end
    assert set(spot.CLI_KEYS) >= {"keywords", "wavs", "threshold", "long", "cmvn", "resample", "ckpt"}
