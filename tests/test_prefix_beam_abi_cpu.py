"""The host side of the CTC prefix beam search, one table for its four modes (plain, ctx, lm, timed): every launcher and every state
init / reset entry point refuses the same bad arguments with the same code before any launch.  The pointers are fake and never
dereferenced (the graph / LM structs are real host memory whose table pointers are fake), so no case here may pass the checks."""
import ctypes

import pytest

P4, P8, OPT, TAB, WS, WSB, INT = "p4", "p8", "optional", "table", "ws", "ws_bytes", "int"
INTS = dict(B=2, T=6, C=4, k=5, beam=4, nbest=4, Lcap=8, T_cap=16, blank=0)
IN = [("vals", P4), ("ids", P4), ("blank_lp", P4)]
OUT = [("out_tok", P4), ("out_len", P4), ("out_score", P4)]
BIAS = [("out_bias", P8), ("out_state", P4)]
TIMES = [("out_vit", P8), ("out_start", P4), ("out_end", P4), ("out_mx", P4), ("out_mn", P4), ("out_sm", P4)]
OFF_DIMS = [(n, INT) for n in ("B", "T", "k", "beam", "nbest", "Lcap", "blank")] + [("stream", None)]
CHUNK_DIMS = [(n, INT) for n in ("B", "C", "k", "beam", "nbest", "Lcap", "T_cap", "blank")] + [("stream", None)]
STATE_DIMS = [(n, INT) for n in ("B", "beam", "T_cap")] + [("stream", None)]
WSPACE = [("ws", WS), ("ws_bytes", WSB)]
CHUNK_IN = IN + [("n_valid", P4), ("state", P8)] + WSPACE

# entry point -> (its arguments in order, the mode's workspace size query, the mode's message for a null graph / LM struct)
# in_len is the one optional pointer: None means "every utterance has T frames" and is accepted, so it is never set to None here
PLAIN_WS, STREAM_WS = "asr_ctc_prefix_beam_workspace_bytes", "asr_ctc_prefix_beam_stream_workspace_bytes"
LM_WS, TIMED_WS = "asr_ctc_prefix_beam_lm_workspace_bytes", "asr_ctc_prefix_beam_timed_workspace_bytes"
LAUNCHERS = {
    "asr_ctc_prefix_beam": (IN + [("in_len", OPT)] + WSPACE + OUT + OFF_DIMS, PLAIN_WS, None),
    "asr_ctc_prefix_beam_ctx": (IN + [("in_len", OPT), ("root", P4), ("ctx", TAB)] + WSPACE + OUT + BIAS + OFF_DIMS, PLAIN_WS, "null context table"),
    "asr_ctc_prefix_beam_lm": (IN + [("in_len", OPT), ("lm", TAB)] + WSPACE + OUT + BIAS + OFF_DIMS, LM_WS, "null LM table"),
    "asr_ctc_prefix_beam_timed": (IN + [("in_len", OPT)] + WSPACE + OUT + TIMES + OFF_DIMS, TIMED_WS, None),
    "asr_ctc_prefix_beam_chunk": (CHUNK_IN + OUT + [("out_stable", P4)] + CHUNK_DIMS, STREAM_WS, None),
    "asr_ctc_prefix_beam_chunk_ctx": (CHUNK_IN + [("ctx", TAB)] + OUT + BIAS + [("out_stable", P4)] + CHUNK_DIMS, STREAM_WS, "null context table"),
    "asr_ctc_prefix_beam_chunk_lm": (CHUNK_IN + [("lm", TAB)] + OUT + BIAS + [("out_stable", P4)] + CHUNK_DIMS, LM_WS, "null LM table"),
    "asr_ctc_prefix_beam_chunk_timed": (CHUNK_IN + OUT + TIMES + [("out_stable", P4), ("out_final", P4)] + CHUNK_DIMS, TIMED_WS, None),
}
STATE = [("state", P8), ("ws", WS)]
STATES = {
    "asr_ctc_prefix_beam_state_init": (STATE + STATE_DIMS, None, None),
    "asr_ctc_prefix_beam_state_reset": (STATE + [("flags", P4)] + STATE_DIMS, None, None),
    "asr_ctc_prefix_beam_ctx_state_init": (STATE + [("root", P4)] + STATE_DIMS, None, None),
    "asr_ctc_prefix_beam_ctx_state_reset": (STATE + [("flags", P4), ("root", P4)] + STATE_DIMS, None, None),
    "asr_ctc_prefix_beam_lm_state_init": (STATE + [("lm", TAB)] + STATE_DIMS, None, "null LM table"),
    "asr_ctc_prefix_beam_lm_state_reset": (STATE + [("flags", P4), ("lm", TAB)] + STATE_DIMS, None, "null LM table"),
    "asr_ctc_prefix_beam_timed_state_init": (STATE + STATE_DIMS, None, None),
    "asr_ctc_prefix_beam_timed_state_reset": (STATE + [("flags", P4)] + STATE_DIMS, None, None),
}


def _tables():
    """A graph and an LM that pass their checks: real structs, fake (aligned, never read) table pointers."""
    from asr_chinese_e2e_amd.context import ContextTables
    from asr_chinese_e2e_amd.lm import LmTables
    return {"ctx": ContextTables(64, 128, 192, 256, 1, 0, 3.0), "lm": LmTables(64, 128, 192, 256, 320, 384, 448, 512, 1, 0, 8, 2, 0, 0.0)}


def _call(name, table, tabs, **over):
    """The entry point with fake, aligned pointers; `over` breaks one argument.  ws_bytes: by default the mode's own size query."""
    from asr_chinese_e2e_amd import _lib
    spec, query, _ = table[name]
    a = {}
    for i, (arg, kind) in enumerate(spec):
        a[arg] = INTS[arg] if kind == INT else ctypes.addressof(tabs[arg]) if kind == TAB else None if kind in (WSB, None) else 4096 * (i + 1)
    a.update(over)
    if "ws_bytes" in a and a["ws_bytes"] is None:
        a["ws_bytes"] = max(getattr(_lib.fast, query)(max(a["B"], 1), max(a.get("T", a.get("T_cap")), 1), max(a["beam"], 1)), 1)
    return getattr(_lib.fast, name)(*a.values())


def _refused(name, table, tabs, words, code=-1, **over):
    from asr_chinese_e2e_amd import _lib
    assert _call(name, table, tabs, **over) == code, (name, over)
    err = _lib.last_error()
    assert err.startswith(name + ":"), (name, over, err)      # every other entry point's name begins with asr_ctc_prefix_beam, hence the colon
    assert any(w in err for w in words), (name, over, err)


@pytest.mark.parametrize("name", list(LAUNCHERS))
def test_launcher_refuses_before_any_launch(name):
    spec, query, tab_msg = LAUNCHERS[name]
    tabs = _tables()
    chunk = "chunk" in name
    for arg, kind in spec:
        if kind in (P4, P8, WS):
            _refused(name, LAUNCHERS, tabs, ["null pointer"], **{arg: None})
        elif kind == TAB:
            _refused(name, LAUNCHERS, tabs, [tab_msg], **{arg: None})
    any_word = [""]
    for over in (dict(beam=17, nbest=1, k=1), dict(k=33, beam=1, nbest=1), dict(beam=5, k=12), dict(nbest=INTS["beam"] + 1)):
        _refused(name, LAUNCHERS, tabs, any_word, **over)
    for arg in ("B", "C" if chunk else "T", "k", "beam", "nbest", "Lcap") + (("T_cap",) if chunk else ()):
        _refused(name, LAUNCHERS, tabs, ["bad shape"], **{arg: 0})
    # T * beam + 1 trie nodes must fit an int32
    # tightening, asr_ctc_prefix_beam / _ctx / _lm: the offline copies had no node-count bound (the timed one had)
    _refused(name, LAUNCHERS, tabs, any_word, **{"T_cap" if chunk else "T": 1 << 29})
    for arg, kind in spec:
        if kind == P8:
            _refused(name, LAUNCHERS, tabs, ["misaligned"], **{arg: 1 << 20 | 4})
    # tightening, asr_ctc_prefix_beam / _ctx / _lm / _timed: the offline copies did not test the alignment of vals / ids / blank_lp
    for arg in ("vals", "ids", "blank_lp"):
        _refused(name, LAUNCHERS, tabs, ["misaligned"], **{arg: 1 << 20 | 2})
    from asr_chinese_e2e_amd import _lib
    size = getattr(_lib.fast, query)(INTS["B"], INTS["T_cap" if chunk else "T"], INTS["beam"])
    assert size > 0
    _refused(name, LAUNCHERS, tabs, ["workspace"], code=-3, ws_bytes=size - 1)


@pytest.mark.parametrize("name", list(STATES))
def test_state_entry_refuses_before_any_launch(name):
    spec, _, tab_msg = STATES[name]
    tabs = _tables()
    for arg, kind in spec:
        if kind in (P4, P8, WS):
            _refused(name, STATES, tabs, ["null pointer"], **{arg: None})
        elif kind == TAB:
            _refused(name, STATES, tabs, [tab_msg], **{arg: None})
    _refused(name, STATES, tabs, ["bad shape"], beam=17)
    for arg in ("B", "beam", "T_cap"):
        _refused(name, STATES, tabs, ["bad shape"], **{arg: 0})
    _refused(name, STATES, tabs, ["bad shape"], T_cap=1 << 29)      # T_cap * beam + 1 trie nodes must fit an int32
    _refused(name, STATES, tabs, ["misaligned"], state=1 << 20 | 4)
