"""The resumable CTC prefix beam search without a GPU: the four entry points are exported and declared, the size functions behave, the
argument checks refuse what the kernel cannot take before any launch, and the definition of the stable prefix (the longest common
prefix of the live beam entries) is monotone on the host restatement of the search."""
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import ROOT

NAMES = ("asr_ctc_prefix_beam_state_bytes", "asr_ctc_prefix_beam_stream_workspace_bytes", "asr_ctc_prefix_beam_state_init",
         "asr_ctc_prefix_beam_chunk")


def test_library_exports_and_header_declares_the_stream_search():
    from asr_chinese_e2e_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asr_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(_lib.lib, n), n
        assert hasattr(_lib.fast, n), n
        assert re.search(r"\b" + n + r"\s*\(", text), f"{n} is not declared in include/asr_hip.h"
    assert _lib.lib.asr_abi_version() == 10      # additive: the ABI version stays


def test_state_and_workspace_sizes():
    from asr_chinese_e2e_amd import _lib
    f = _lib.fast
    for B, beam in ((1, 1), (3, 5), (32, 16)):
        s = f.asr_ctc_prefix_beam_state_bytes(B, beam)
        assert s > 0 and s % 8 == 0
        # the header and per entry node, token, parent, depth (int32) and pb, pnb (fp64): nothing the frame step carries is missing
        assert s >= B * (3 * 4 + beam * (4 * 4 + 2 * 8))
        assert f.asr_ctc_prefix_beam_state_bytes(B + 1, beam) > s and f.asr_ctc_prefix_beam_state_bytes(B, beam + 1) > s
        for T in (1, 37, 5000):
            w = f.asr_ctc_prefix_beam_stream_workspace_bytes(B, T, beam)
            assert w >= B * 2 * (T * beam + 1) * 4      # parent and token of T * beam + 1 nodes per utterance
            assert f.asr_ctc_prefix_beam_stream_workspace_bytes(B + 1, T, beam) > w
            assert f.asr_ctc_prefix_beam_stream_workspace_bytes(B, T + 1, beam) > w
            assert f.asr_ctc_prefix_beam_stream_workspace_bytes(B, T, beam + 1) > w
    for args in ((0, 5), (5, 0), (-1, 5), (5, -1)):
        assert f.asr_ctc_prefix_beam_state_bytes(*args) == 0
    for args in ((0, 10, 5), (3, 0, 5), (3, 10, 0), (-3, 10, 5), (3, -10, 5), (3, 10, -5)):
        assert f.asr_ctc_prefix_beam_stream_workspace_bytes(*args) == 0
    assert f.asr_ctc_prefix_beam_stream_workspace_bytes(32, 5000, 16) == 32 * 2 * (5000 * 16 + 1) * 4      # about 20 MB


def _chunk(f, **over):
    """asr_ctc_prefix_beam_chunk with fake (never dereferenced) aligned pointers; `over` breaks one argument."""
    B, C, k, beam, T_cap = 2, 4, 5, 4, 16
    a = dict(vals=64, ids=128, blank_lp=192, n_valid=256, state=320, ws=384, ws_bytes=None, out_tok=448, out_len=512, out_score=576,
             out_stable=640, B=B, C=C, k=k, beam=beam, nbest=beam, Lcap=8, T_cap=T_cap, blank=0, stream=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(f.asr_ctc_prefix_beam_stream_workspace_bytes(max(a["B"], 1), max(a["T_cap"], 1), max(a["beam"], 1)), 1)
    return f.asr_ctc_prefix_beam_chunk(*a.values())


def test_chunk_argument_checks_run_before_any_launch():
    """Every refusal below comes back as ASR_EINVAL (-1) / ASR_EWORKSPACE (-3) from the host-side checks: no device is touched."""
    from asr_chinese_e2e_amd import _lib
    f = _lib.fast
    for name in ("vals", "ids", "blank_lp", "n_valid", "state", "ws", "out_tok", "out_len", "out_score", "out_stable"):
        assert _chunk(f, **{name: None}) == -1, name
        assert "null pointer" in _lib.last_error()
    assert _chunk(f, beam=8, nbest=8, k=10) == -1 and "beam * (k + 1) <= 64" in _lib.last_error()      # 88 slots
    assert _chunk(f, beam=17, nbest=1, k=1) == -1                                                        # beam <= 16
    assert _chunk(f, nbest=5) == -1                                                                      # nbest <= beam
    assert _chunk(f, C=0) == -1 and "C=0" in _lib.last_error()
    assert _chunk(f, T_cap=0) == -1 and "T_cap=0" in _lib.last_error()
    for name in ("B", "k", "beam", "nbest", "Lcap"):
        assert _chunk(f, **{name: 0}) == -1, name
    assert _chunk(f, state=324) == -1 and "misaligned" in _lib.last_error()      # fp64 scores: 8-byte alignment
    assert _chunk(f, vals=66) == -1 and "misaligned" in _lib.last_error()
    assert _chunk(f, out_stable=642) == -1
    assert _chunk(f, ws=386) == -3
    assert _chunk(f, ws_bytes=f.asr_ctc_prefix_beam_stream_workspace_bytes(2, 16, 4) - 1) == -3 and "workspace" in _lib.last_error()
    # state_init
    assert f.asr_ctc_prefix_beam_state_init(None, 64, 2, 4, 16, None) == -1
    assert f.asr_ctc_prefix_beam_state_init(64, None, 2, 4, 16, None) == -1
    assert f.asr_ctc_prefix_beam_state_init(64, 128, 0, 4, 16, None) == -1
    assert f.asr_ctc_prefix_beam_state_init(64, 128, 2, 17, 16, None) == -1
    assert f.asr_ctc_prefix_beam_state_init(64, 128, 2, 4, 0, None) == -1
    assert f.asr_ctc_prefix_beam_state_init(68, 128, 2, 4, 16, None) == -1


def _common_prefix_len(prefixes):
    n = 0
    for col in zip(*prefixes):
        if any(c != col[0] for c in col):
            break
        n += 1
    return n if prefixes else 0


@pytest.mark.parametrize("peak", [3.0, 0.3])
@pytest.mark.parametrize("beam,k", [(1, 5), (4, 5), (10, 5), (16, 3)])
def test_stable_prefix_is_monotone_on_the_host_restatement(beam, k, peak):
    """The definition, not the kernel: the longest common prefix of the finite-score entries of the search run on frames [0, t) never
    gets shorter as t grows (every entry of the next beam descends from an entry of this one), and the prefix itself is never retracted."""
    from oracle import decode_ref as D
    T, V = 37, 12
    g = torch.Generator().manual_seed(3000 + 37)
    logits = torch.randn(3, T, V, generator=g) * peak
    logp = torch.log_softmax(logits.double(), -1).numpy()
    for b in range(3):
        cand = [list(np.argsort(-logp[b, t], kind="stable")[:k]) for t in range(T)]
        prev = ()
        for t in range(T + 1):
            live = [p for p, s in D.ctc_prefix_beam_search(logp[b, :t], beam, candidates=cand[:t]) if s > -np.inf]
            n = _common_prefix_len(live)
            stable = live[0][:n]
            assert len(stable) >= len(prev) and stable[:len(prev)] == prev, (b, t, prev, stable)
            if beam == 1:
                assert n == len(live[0])
            prev = stable
