"""Independent sessions without a GPU: the front end's two cadences (the lock-step plan is the parent's for every input, the
independent plan gives every slot the chunks of a B = 1 front end), the endpoint rules against their literal restatement
(tests/session_ref.py), and the argument checks of the new entry points, which refuse before any launch."""
import os
import random
import re

import numpy as np
import pytest

from tests import session_ref as SR
from tests.helpers import ROOT

NAMES = ("asr_add_ln_slots_fwd", "asr_slot_rows_put", "asr_slot_rows_slide", "asr_ctc_frame_best_blank", "asr_session_ctc_step",
         "asr_ctc_prefix_beam_state_reset")


# ------------------------------------------------------------------------------------------------ the front end's plan
def _parser(frontend, m=4, n=3, n_mels=8):
    from asr_chinese_e2e_amd.data_handler import AudioParser
    return AudioParser(device="cpu", n_mels=n_mels, lfr_m=m, lfr_n=n, norm="global", cmvn=(np.zeros(n_mels), np.ones(n_mels)), frontend=frontend)


def _lockstep_plan(fe, ns, fin):
    """StreamingFrontEnd.plan as it stood before the independent mode existed, statement by statement."""
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.data_handler.stream_frontend import _pow2_at_least, rows_ready
    B, C, m, n = fe.B, fe.C, fe.m, fe.n
    received, closed, next_frame, next_row, fcap = list(fe.received), list(fe.closed), list(fe.next_frame), list(fe.next_row), fe.fcap
    acts = []
    for off in range(0, max(max(ns), 1), fe.piece):
        take = [max(0, min(fe.piece, x - off)) for x in ns]
        if max(take) > 0:
            acts.append(("append", off, [[received[b], take[b]] for b in range(B)], max(take)))
        for b in range(B):
            received[b] += take[b]
            if fin[b] and off + take[b] >= ns[b]:
                closed[b] = True
        new = [fe.parser.frames_ready(received[b], closed[b]) - next_frame[b] for b in range(B)]
        if max(new) > 0:
            live = [(min(next_row[b] * n, next_frame[b] + new[b]), next_frame[b] + new[b]) for b in range(B)]
            need = max(hi - lo for lo, hi in live)
            if need > fe.max_frames:
                raise ValueError("stall")
            if need > fcap:
                fcap = _pow2_at_least(need)
                acts.append(("grow", fcap, [(lo, next_frame[b]) for b, (lo, _) in enumerate(live)]))
            acts.append(("logmel", [[next_frame[b], new[b], received[b] if closed[b] else K.STREAM_OPEN] for b in range(B)], max(new)))
            for b in range(B):
                next_frame[b] += new[b]
        while True:
            ready = [rows_ready(next_frame[b], m, n, closed[b]) - next_row[b] for b in range(B)]
            if not any(r > 0 for r in ready) or not all(closed[b] or ready[b] >= C for b in range(B)):
                break
            nv = [min(C, r) for r in ready]
            acts.append(("chunk", [[next_row[b], nv[b], next_frame[b] if closed[b] else K.STREAM_OPEN] for b in range(B)], nv))
            for b in range(B):
                next_row[b] += nv[b]
    if fe.kaldi and all(closed) and not all(fe.closed) and not any(next_row) and not any(a[0] == "chunk" for a in acts):
        acts.append(("chunk", [[0, 0, 0] for _ in range(B)], [0] * B))
    return acts, (received, closed, next_frame, next_row)


@pytest.mark.parametrize("frontend", ["reference", "kaldi"])
def test_lockstep_plan_is_the_parents_on_random_schedules(frontend):
    from asr_chinese_e2e_amd.data_handler.stream_frontend import StreamingFrontEnd
    rng = random.Random(11)
    for trial in range(40):
        B, C = rng.choice([1, 2, 4]), rng.choice([1, 4, 5])
        fe = StreamingFrontEnd(_parser(frontend), B, C, sample_cap=1024)
        assert fe.independent is False
        for _ in range(rng.randint(1, 12)):
            ns = [0 if fe.closed[b] else rng.choice([0, 0, 37, 160, 399, 400, 700, 1500, 2600]) for b in range(B)]
            fin = [not fe.closed[b] and rng.random() < 0.15 for b in range(B)]
            try:
                want = _lockstep_plan(fe, ns, fin)
            except ValueError:
                with pytest.raises(ValueError):
                    fe.plan(ns, fin)
                break
            got = fe.plan(ns, fin)
            assert got == want, (trial, ns, fin)
            fe.received, fe.closed, fe.next_frame, fe.next_row = got[1]
            for a in got[0]:
                if a[0] == "grow":
                    fe.fcap = a[1]


def _chunks(acts, b):
    """Slot b's (r_begin, n_rows) of every chunk that carries rows of it, and whether its end was reported."""
    out, done = [], False
    for a in acts:
        if a[0] == "chunk":
            if a[2][b] > 0:
                out.append((a[1][b][0], a[2][b]))
            if len(a) > 3 and a[3][b]:
                done = True
    return out, done


@pytest.mark.parametrize("frontend", ["reference", "kaldi"])
def test_independent_plan_gives_every_slot_the_chunks_of_a_front_end_of_its_own(frontend):
    """Random block cuts, staggered opens, closes and reopens: every slot's sequence of (r_begin, n_rows) is what a B = 1 front end
    plans for that slot's audio alone; no chunk holds a partial piece of an open session; every closed session's end is reported
    exactly once, with or behind its last row."""
    from asr_chinese_e2e_amd.data_handler.stream_frontend import StreamingFrontEnd
    rng = random.Random(5)
    for trial in range(25):
        S, C = rng.choice([2, 4]), rng.choice([1, 4, 5])
        parser = _parser(frontend)
        fe = StreamingFrontEnd(parser, S, C, sample_cap=1024, independent=True)
        solo = [None] * S                      # the slot's own B = 1 front end while a session is open in it
        start = [rng.randint(0, 4) for _ in range(S)]
        ended = [0] * S
        for tick in range(30):
            ns, fin = [0] * S, [False] * S
            for b in range(S):
                if solo[b] is None and tick >= start[b] and rng.random() < 0.7:      # (re)open
                    solo[b] = StreamingFrontEnd(parser, 1, C, sample_cap=1024)
                    fe.reset(b)
                if solo[b] is not None and not fe.closed[b]:
                    ns[b] = rng.choice([0, 0, 13, 160, 399, 400, 480, 1700, 2600])
                    fin[b] = rng.random() < 0.12
            acts, after = fe.plan(ns, fin)
            assert not any(a[0] == "grow" for a in acts)      # no slot waits for another: nothing piles up
            for b in range(S):
                got, done = _chunks(acts, b)
                if solo[b] is None:
                    assert got == [] and not done
                    continue
                want_acts, want_after = solo[b].plan([ns[b]], [fin[b]])
                want, _ = _chunks(want_acts, 0)
                assert got == want, (trial, tick, b, ns, fin)
                assert [x[b] for x in after] == [x[0] for x in want_after]
                closed_now = after[1][b] and not fe.closed[b]
                assert done == closed_now, (trial, tick, b)
                for a in acts:      # a partial chunk only once the session is closed, and then it is the last one
                    if a[0] == "chunk" and 0 < a[2][b] < C:
                        assert after[1][b] and a[3][b]
                solo[b].received, solo[b].closed, solo[b].next_frame, solo[b].next_row = want_after
                if done:
                    ended[b] += 1
            fe.received, fe.closed, fe.next_frame, fe.next_row = after
            for b in range(S):
                if solo[b] is not None and fe.closed[b]:
                    solo[b], start[b] = None, tick + rng.randint(1, 3)
        assert sum(ended) > 0


# ------------------------------------------------------------------------------------------------ endpoint rules
class _Model:
    decoding_chunk_size, decoding_left_chunks, use_ctc, V = 8, -1, True, 30

    def frame_seconds(self):
        return 0.03


def test_endpoint_rules_match_the_literal_restatement():
    from asr_chinese_e2e_amd import sessions as SS
    cfg = SS.endpoint_config({})
    assert cfg["blank_threshold"] == 0.8 and cfg["rules"] == SR.DEFAULT_RULES
    frame_us = 30000
    for rules in (SR.DEFAULT_RULES, SS.endpoint_config({"silence_after_speech": (True, 300, 0), "max_length": (False, 0, 900)})["rules"]):
        for trailing in (0, 1, 9, 10, 11, 33, 34, 166, 167, 700):
            for frames in (0, 29, 30, 31, 666, 667, 5000):
                if trailing > frames:
                    continue
                for decoded in (False, True):
                    assert SS.endpoint_rule(rules, frame_us, trailing, frames, decoded) == SR.endpoint_rule(trailing, frames, decoded, frame_us, rules)
    # rule 2 needs "decoded": 1 s of silence (34 frames of 30 ms) alone is not an endpoint, after speech it is
    assert SR.endpoint_rule(34, 60, False, frame_us) is None and SR.endpoint_rule(34, 60, True, frame_us) == "silence_after_speech"
    assert SR.endpoint_rule(33, 60, True, frame_us) is None
    assert SR.endpoint_rule(167, 167, False, frame_us) == "silence_start" and SR.endpoint_rule(166, 166, False, frame_us) is None
    assert SR.endpoint_rule(0, 667, True, frame_us) == "max_length" and SR.endpoint_rule(0, 666, True, frame_us) is None
    with pytest.raises(ValueError):
        SS.endpoint_config({"blank_treshold": 0.5})
    with pytest.raises(ValueError):
        SS.endpoint_config({"blank_threshold": 1.0})


def test_counters_restart_when_a_slot_is_reopened():
    """A silence run that spans a reopen: the second session's trailing silence counts its own frames only (session_ref.ctc_step's
    reset), and the host side of Sessions reports no endpoint for a slot that was just reopened."""
    from asr_chinese_e2e_amd import sessions as SS
    lp_sil, lp_speech, thr = np.log(0.95), np.log(0.5), np.log(0.8)
    path = [3, 3, 0, 0, 0, 0, 0, 0]
    blp = [lp_speech, lp_speech] + [lp_sil] * 6
    ids, st = SR.ctc_step(path, blp, 8, True, None, thr)
    assert ids == [3] and st == (0, 6, 8, 1)
    ids, st = SR.ctc_step([0] * 8, [lp_sil] * 8, 8, False, st, thr)
    assert ids == [] and st == (0, 14, 16, 1)
    rules = SS.endpoint_config({"silence_after_speech": (True, 400, 0)})["rules"]      # 14 frames = 420 ms
    assert SR.endpoint_rule(st[1], st[2], st[3], 30000, rules) == "silence_after_speech"
    # reopened: the run of silence goes on, the counters do not
    ids, st2 = SR.ctc_step([0] * 8, [lp_sil] * 8, 8, True, st, thr)
    assert st2 == (0, 8, 8, 0) and SR.endpoint_rule(st2[1], st2[2], st2[3], 30000, rules) is None
    # the carried last class: a repeat across the chunk boundary is not emitted twice, and a reset forgets it
    _, st = SR.ctc_step([0, 5, 5], [lp_speech] * 3, 3, True, None, thr)
    assert SR.ctc_step([5, 5, 7], [lp_speech] * 3, 3, False, st, thr)[0] == [7]
    assert SR.ctc_step([5, 5, 7], [lp_speech] * 3, 3, True, st, thr)[0] == [5, 7]
    # beam sessions: no path, nothing emitted, the counters still run
    assert SR.ctc_step(None, [lp_sil] * 4, 4, False, (0, 2, 10, 0), thr) == ([], (0, 6, 14, 0))
    # the host side: open / drop / reopen
    ss = SS.Sessions(_Model(), 2, endpoint={"silence_after_speech": (True, 400, 0)})
    assert ss.frame_us == 30000
    with pytest.raises(ValueError):
        SS.Sessions(_Model(), 2).endpoints()      # endpointing was not asked for
    ss.open(1)
    ss.trailing[1], ss.frames[1], ss.decoded[1], ss.fresh[1] = 14, 16, True, False
    assert ss.endpoints() == [None, "silence_after_speech"]
    assert ss.status(1) == {"state": "open", "frames": 16, "trailing_silence_frames": 14, "decoded": True}
    with pytest.raises(ValueError):
        ss.open(1)
    ss.drop(1)
    ss.open(1)
    assert ss.endpoints() == [None, None] and ss.status(1)["frames"] == 0 and ss.status(0)["state"] == "free"
    with pytest.raises(ValueError):
        SS.Sessions(_Model(), 2, source_rate=8000)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_library_exports_and_header_declares_the_session_entry_points():
    from asr_chinese_e2e_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asr_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(_lib.lib, n), n
        assert hasattr(_lib.fast, n), n
        assert re.search(r"\b" + n + r"\s*\(", text), f"{n} is not declared in include/asr_hip.h"
    assert _lib.lib.asr_abi_version() == 10      # additive: the ABI version stays


def _call(fn, base, **over):
    a = dict(base)
    a.update(over)
    return fn(*a.values())


def test_argument_checks_run_before_any_launch():
    """Every refusal is ASR_EINVAL (-1) / ASR_EDTYPE (-2) from the host-side checks with fake, never dereferenced pointers."""
    from asr_chinese_e2e_amd import _lib
    f = _lib.fast
    ln = dict(x=1024, gamma=2048, beta=3072, pe=4096, pe_off=5120, lens=6144, y=7168, rstd=9216, slots=4, T=8, d=64, pe_rows=5000, dtype=0, stream=None)
    for name in ("x", "gamma", "beta", "pe", "pe_off", "lens", "y", "rstd"):
        assert _call(f.asr_add_ln_slots_fwd, ln, **{name: None}) == -1 and "null pointer" in _lib.last_error(), name
    for over in (dict(slots=0), dict(T=0), dict(d=0), dict(d=2049), dict(pe_rows=7), dict(pe_off=5122), dict(lens=6146), dict(d=512, x=1028), dict(d=512, pe=4100), dict(y=1024), dict(rstd=9218)):
        assert _call(f.asr_add_ln_slots_fwd, ln, **over) == -1, over
    assert _call(f.asr_add_ln_slots_fwd, ln, dtype=7) == -2

    put = dict(src=1024, dst=8192, start=256, n=512, slots=4, C=8, cap=32, cols=128, ld_src=192, dtype=0, stream=None)
    for name in ("src", "dst", "start", "n"):
        assert _call(f.asr_slot_rows_put, put, **{name: None}) == -1, name
    for over in (dict(slots=0), dict(slots=70000), dict(C=0), dict(C=33), dict(cap=0), dict(cols=0), dict(cols=130, ld_src=192), dict(ld_src=127),
                 dict(ld_src=194), dict(src=1032), dict(dst=8200), dict(start=258), dict(cols=124, dtype=1)):
        assert _call(f.asr_slot_rows_put, put, **over) == -1, over
    assert _call(f.asr_slot_rows_put, put, dtype=3) == -2

    sl = dict(src=1 << 20, dst=2 << 20, frm=256, count=512, slots=4, max_count=16, cap=24, cols=128, dtype=0, stream=None)
    for name in ("src", "dst", "frm", "count"):
        assert _call(f.asr_slot_rows_slide, sl, **{name: None}) == -1, name
    for over in (dict(max_count=0), dict(max_count=25), dict(slots=0), dict(cols=126), dict(dst=(2 << 20) + 8), dict(count=514)):
        assert _call(f.asr_slot_rows_slide, sl, **over) == -1, over
    assert _call(f.asr_slot_rows_slide, sl, dst=(1 << 20) + 4096) == -1 and "overlap" in _lib.last_error()      # never in place
    assert _call(f.asr_slot_rows_slide, sl, dst=1 << 20) == -1
    assert _call(f.asr_slot_rows_slide, sl, dtype=2) == -2

    bb = dict(logits=1024, in_len=256, path=2048, blank_lp=4096, B=4, T=8, V=30, ld=30, blank=0, dtype=0, stream=None)
    for name in ("logits", "path", "blank_lp"):
        assert _call(f.asr_ctc_frame_best_blank, bb, **{name: None}) == -1, name
    for over in (dict(B=0), dict(T=0), dict(V=1), dict(blank=30), dict(blank=-1), dict(ld=29), dict(path=2050), dict(blank_lp=4098), dict(logits=1026), dict(in_len=258)):
        assert _call(f.asr_ctc_frame_best_blank, bb, **over) == -1, over
    assert _call(f.asr_ctc_frame_best_blank, bb, dtype=5) == -2

    st = dict(path=1024, blank_lp=2048, n_valid=256, reset=512, state=4096, out=8192, slots=4, C=8, blank=0, silence_lp=-0.2, stream=None)
    for name in ("blank_lp", "n_valid", "reset", "state", "out"):
        assert _call(f.asr_session_ctc_step, st, **{name: None}) == -1, name
    for over in (dict(slots=0), dict(C=0), dict(blank=-1), dict(silence_lp=float("nan")), dict(state=4098), dict(path=1026), dict(out=8194)):
        assert _call(f.asr_session_ctc_step, st, **over) == -1, over

    rs = dict(state=64, ws=128, flags=256, B=2, beam=4, T_cap=16, stream=None)
    for name in ("state", "ws", "flags"):
        assert _call(f.asr_ctc_prefix_beam_state_reset, rs, **{name: None}) == -1, name
    for over in (dict(B=0), dict(beam=0), dict(beam=17), dict(T_cap=0), dict(state=68), dict(ws=130), dict(flags=258)):
        assert _call(f.asr_ctc_prefix_beam_state_reset, rs, **over) == -1, over
