"""Blank-frame skipping without a GPU: the definition (tests/blank_skip_ref.py) on hand-made rows, its invariance under any cutting
into chunks, the host loop of decode.ctc_prefix_beam_search(on_device=False, blank_skip=p) against oracle/decode_ref.py's search on
the reference-compacted rows, the doubled character that the run-head rule protects, and the argument checks and exports."""
import math
import os
import random
import re
import types

import numpy as np
import pytest
import torch

from oracle import decode_ref
from tests import blank_skip_ref as R
from tests.helpers import ROOT

P = 0.98
THR = R.threshold(P)
HI, LO = np.float32(math.log(0.99)), np.float32(math.log(0.5))      # a high and a low blank log-posterior under p = 0.98


def _rows(pattern):
    """'h' -> a high frame, 'l' -> a low one, 'e' -> exactly the threshold, 'n' -> NaN."""
    return np.array([{"h": HI, "l": LO, "e": THR, "n": np.float32("nan")}[c] for c in pattern], dtype=np.float32)


def _loops(blank_lp, thr):
    """The definition once more, as plainly as it can be said: two loops over booleans."""
    high = []
    for x in blank_lp:
        high.append(bool(x > thr))
    kept = []
    for t in range(len(high)):
        if t > 0 and high[t] and high[t - 1]:
            continue
        kept.append(t)
    return kept


@pytest.mark.parametrize("pattern, want", [
    ("", []),                                          # T = 0
    ("h", [0]), ("l", [0]),                            # T = 1
    ("llll", [0, 1, 2, 3]),                            # no high frame
    ("hhhhhh", [0]),                                   # all high: exactly frame 0 survives
    ("hlhlhl", [0, 1, 2, 3, 4, 5]),                    # alternating: every run has length 1
    ("hhhlh", [0, 3, 4]),                              # a run that starts at frame 0
    ("lhhhlhhl", [0, 1, 4, 5, 7]),
    ("heh", [0, 1, 2]), ("hee", [0, 1, 2]),            # blank_lp == thr exactly: not high (strict), kept, and it ends the run
    ("hnh", [0, 1, 2]), ("nnn", [0, 1, 2]),            # NaN: not high, kept
])
def test_hand_made_rows(pattern, want):
    lp = _rows(pattern)
    assert R.kept_frames(lp, THR)[0] == want == _loops(lp, THR)


def test_threshold_is_float32_and_p_one_keeps_everything():
    assert THR.dtype == np.float32 and THR == np.float32(np.log(np.float32(0.98))) and THR < 0
    one = R.threshold(1.0)
    assert one == 0.0
    lp = np.array([0.0, -0.0, -1e-30, -1e-8, -0.01, -5.0, 0.0, 0.0], dtype=np.float32)      # log-posteriors are <= 0: none is > 0
    assert R.kept_frames(lp, one)[0] == list(range(len(lp)))
    from asr_chinese_e2e_amd import kernels as K
    assert K.blank_skip_threshold(0.98) == float(THR) and K.blank_skip_threshold(1) == 0.0


def test_random_masks_against_the_loops():
    rng = random.Random(11)
    for _ in range(200):
        T = rng.randrange(0, 150)
        share = rng.random()
        lp = _rows("".join("h" if rng.random() < share else rng.choice("lllen") for _ in range(T)))
        kept, carry = R.kept_frames(lp, THR)
        assert kept == _loops(lp, THR)
        assert carry == (T > 0 and bool(lp[-1] > THR))
        from asr_chinese_e2e_amd.decode import blank_skip_kept
        assert blank_skip_kept(lp.tolist(), T, float(THR)) == kept      # the host loop's statement of the rule
        assert blank_skip_kept(lp.tolist() + [float(HI)] * 3, T, float(THR)) == kept      # frames past the count are not looked at


def test_any_cutting_gives_the_same_kept_set():
    rng = random.Random(5)
    for _ in range(100):
        T = rng.randrange(0, 120)
        lp = _rows("".join(rng.choice("hhhl") for _ in range(T)))
        whole = R.kept_frames(lp, THR)[0]
        cuts, left = [], T
        while left > 0:
            n = rng.choice([0, 0, 1, 1, 2, 5, 16, 64, 65])
            n = min(n, left)
            cuts.append(n)
            left -= n
        cuts += [0]
        assert R.kept_frames_chunked(lp, cuts, THR) == whole
        assert R.kept_frames_chunked(lp, [1] * T, THR) == whole


# ------------------------------------------------------------------------------------------------ the host loop of the product
class _HostModel:
    """What decode.ctc_prefix_beam_search(on_device=False) needs of a model, without a GPU: the CTC head's output is given."""

    def __init__(self, logits, lens=None):
        self.logits = torch.as_tensor(np.asarray(logits)).float()
        self.lens = [self.logits.shape[1]] * self.logits.shape[0] if lens is None else lens
        self.V = self.logits.shape[2]
        self.use_ctc = True
        self.eng = types.SimpleNamespace(use_ctc=True, training=False)

    def _ensure_engine(self, device):
        return self.eng

    def forward(self, input):
        return types.SimpleNamespace(ctc_logits=self.logits)

    def input(self):
        return types.SimpleNamespace(wave=types.SimpleNamespace(device="cpu"), wave_len=torch.tensor(self.lens))


def _host_topk(logits, k, blank=0):
    """asr_ctc_frame_topk on the host: log_softmax, the k best classes per frame (ties: smaller index first), the blank's value."""
    lsm = torch.log_softmax(logits.double(), -1)
    order = np.stack([np.lexsort((np.arange(lsm.shape[1]), -lsm[r].numpy()))[:k] for r in range(lsm.shape[0])])
    ids = torch.from_numpy(order.astype(np.int32))
    return lsm.gather(1, ids.long()).float(), ids, lsm[:, blank].float()


def _host_search(monkeypatch, logits, beam, nbest, k, lens=None, **kw):
    from asr_chinese_e2e_amd import decode
    monkeypatch.setattr(decode.K, "ctc_frame_topk", _host_topk)
    m = _HostModel(logits, lens)
    return decode.ctc_prefix_beam_search(m, m.input(), beam, nbest, k, on_device=False, **kw)


def _peaky_logits(rng, B, T, V, share):
    """Logits whose blank posterior is above 0.98 on about `share` of the frames, in runs, and contested elsewhere."""
    x = rng.normal(0.0, 1.0, (B, T, V)).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            run = int(rng.integers(1, 9))
            if rng.random() < share:
                x[b, t:t + run, 0] += 12.0
            else:
                x[b, t:t + run, int(rng.integers(1, V))] += 3.0
            t += run
    return x


def test_host_loop_with_blank_skip_is_the_oracle_search_on_the_kept_rows(monkeypatch):
    rng = np.random.default_rng(3)
    B, T, V, k, beam = 3, 60, 12, 5, 6
    lens = [60, 41, 7]
    logits = _peaky_logits(rng, B, T, V, 0.6)
    got = _host_search(monkeypatch, logits, beam, beam, k, lens, blank_skip=P)
    plain = _host_search(monkeypatch, logits, beam, beam, k, lens)
    vals, ids, blank_lp = (t.numpy() for t in _host_topk(torch.from_numpy(logits).reshape(B * T, V), k))
    vals, ids, blank_lp = vals.reshape(B, T, k), ids.reshape(B, T, k), blank_lp.reshape(B, T)
    dropped = 0
    for b in range(B):
        kept, _ = R.kept_frames(blank_lp[b, :lens[b]], THR)
        dropped += lens[b] - len(kept)
        # the oracle over the float32 log-probabilities the host loop sees: the kept frames' candidates, the blank's value in column 0
        logp = np.full((len(kept), V), -np.inf)
        for i, t in enumerate(kept):
            logp[i, ids[b, t]] = vals[b, t].astype(np.float64)
            logp[i, 0] = float(blank_lp[b, t])
        want = decode_ref.ctc_prefix_beam_search(logp, beam, 0, candidates=[ids[b, t] for t in kept])
        assert [tuple(h["yseq"]) for h in got[b]] == [p for p, _ in want[:beam]]
        # both sum in fp64 over the same float32 terms, in different orders: at most a few ulp of a score of magnitude < 1e3
        assert all(abs(h["score"] - s) < 1e-9 for h, (_, s) in zip(got[b], want))
        # and the same code on host-compacted logits, bit for bit
        again = _host_search(monkeypatch, logits[b:b + 1, kept], beam, beam, k)[0]
        assert again == got[b]
    assert dropped > 0.3 * sum(lens)
    assert got != plain      # scores sum over the kept frames only
    assert _host_search(monkeypatch, logits, beam, beam, k, lens, blank_skip=1.0) == plain
    assert _host_search(monkeypatch, logits, beam, beam, k, lens, blank_skip=None) == plain


def test_the_doubled_character_survives(monkeypatch):
    A, B_ = 3, 4
    spell = [A, 0, 0, 0, A, B_, 0, 0]
    V = 6
    post = np.full((len(spell), V), 1e-6 / (V - 1))
    for t, c in enumerate(spell):
        post[t, c] = 1.0 - 1e-6
    assert (post.max(axis=1) >= 1.0 - 1e-6).all()
    logits = np.log(post).astype(np.float32)[None]
    plain = _host_search(monkeypatch, logits, 4, 1, 3)[0][0]["yseq"]
    got = _host_search(monkeypatch, logits, 4, 4, 3, blank_skip=P)[0]
    assert got[0]["yseq"] == plain == [A, A, B_]
    blank_lp = _host_topk(torch.from_numpy(logits[0]), 3)[2].numpy()
    assert R.kept_frames(blank_lp, THR)[0] == [0, 1, 4, 5, 6]
    # the variant that drops EVERY high frame loses the blank between the two As, and with it the second A
    every = R.kept_frames_drop_every_high(blank_lp, THR)
    assert every == [0, 4, 5]
    assert _host_search(monkeypatch, logits[:, every], 4, 1, 3)[0][0]["yseq"] == [A, B_]


# ------------------------------------------------------------------------------------------------ argument checks and exports
class _Model:
    decoding_chunk_size, decoding_left_chunks, use_ctc, use_decoder, V = 8, -1, True, True, 30
    vocab = types.SimpleNamespace(_id2token=[str(i) for i in range(30)])

    def frame_seconds(self):
        return 0.03


BAD = (0, 0.0, -0.5, 1.0000001, 2, float("nan"), float("inf"), -float("inf"), "x")


def test_bad_values_and_searches_without_a_prefix_beam_raise_before_any_launch():
    from asr_chinese_e2e_amd import Models, decode
    from asr_chinese_e2e_amd.sessions import Sessions
    from asr_chinese_e2e_amd.stream import StreamingEncoder
    T = Models.TransformerOffical
    stub = types.SimpleNamespace(use_ctc=True, use_decoder=True)      # no engine, no device: anything past the checks would fail otherwise
    for bad in BAD:
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            decode.ctc_prefix_beam_search(stub, None, blank_skip=bad)
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            decode.ctc_rescore_search(stub, None, blank_skip=bad)
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            T.beam_search(stub, None, joint="ctc_rescore", blank_skip=bad)
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            T.ctc_prefix_beam_search(stub, None, blank_skip=bad)
        for make in (Sessions, StreamingEncoder):
            with pytest.raises(ValueError, match=r"\(0, 1\]"):
                make(_Model(), 2, search="prefix_beam", blank_skip=bad)
    for make in (Sessions, StreamingEncoder):
        with pytest.raises(ValueError, match="blank_skip needs search='prefix_beam'"):
            make(_Model(), 2, search="greedy", blank_skip=0.98)
        with pytest.raises(ValueError, match="blank_skip needs search='prefix_beam'"):
            make(_Model(), 2, blank_skip=0.98)
    assert Sessions(_Model(), 2, search="prefix_beam", blank_skip=0.98).skip_thr == float(THR)
    assert StreamingEncoder(_Model(), 2, search="prefix_beam", blank_skip=0.98).core.skip_thr == float(THR)
    assert Sessions(_Model(), 2, search="prefix_beam").skip_thr is None
    for kw in (dict(joint="one_pass", ctc_weight=0.3), dict(joint="rescore", ctc_weight=0.3), dict(joint="rescore", ctc_weight=0.0), dict()):
        with pytest.raises(ValueError, match="blank_skip is not supported"):
            T.beam_search(stub, None, blank_skip=0.98, **kw)
    joint = types.SimpleNamespace(use_ctc=True, use_decoder=True, config=types.SimpleNamespace(ctc_weight=0.3))
    joint.beam_search = lambda *a, **kw: T.beam_search(joint, *a, **kw)
    with pytest.raises(ValueError, match="blank_skip is not supported"):
        T.transcribe(joint, None, blank_skip=0.98)      # the joint model's default search is the attention beam's
    with pytest.raises(ValueError, match="blank_skip is not supported"):
        T.transcribe(joint, None, blank_skip=0.98, joint="one_pass")


def test_header_binding_and_exports():
    from asr_chinese_e2e_amd import _lib
    from asr_chinese_e2e_amd import kernels as K
    assert _lib.lib.asr_abi_version() == 10 == _lib.ABI_VERSION      # additive: the ABI version stays
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asr_hip.h")).read(), flags=re.S)
    for name, n_args in (("asr_ctc_blank_skip_compact", 17), ("asr_frame_index_remap", 7)):
        assert hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
    assert _lib.SIGNATURES["asr_ctc_blank_skip_compact"][1][4] is _lib.F      # thr travels as a float32
    for name in ("blank_skip_threshold", "BlankSkipState", "ctc_blank_skip_compact", "frame_index_remap"):
        assert hasattr(K, name)
    import inspect
    from asr_chinese_e2e_amd import Models, decode
    for fn in (decode.ctc_prefix_beam_search, decode.ctc_rescore_search, Models.TransformerOffical.beam_search, Models.TransformerOffical.transcribe,
               Models.TransformerOffical.ctc_prefix_beam_search, Models.TransformerOffical.stream, Models.TransformerOffical.sessions):
        assert inspect.signature(fn).parameters["blank_skip"].default is None


def test_the_wrappers_refuse_bad_arguments_without_a_gpu():
    """The validation of the two entry points runs on the host before any launch."""
    from asr_chinese_e2e_amd import _lib
    f = _lib.fast
    a = 4096      # aligned, never dereferenced: every call below is refused first
    ok = dict(vals=a, ids=a + 4096, blank_lp=a + 8192, count=a + 12288, thr=-0.02, state=None, reset=None, out_vals=a + 16384, out_ids=a + 20480,
              out_blank_lp=a + 24576, out_len=a + 28672, out_frame=a + 32768, B=2, T=10, k=5, map_cap=10, stream=None)

    def call(**over):
        return f.asr_ctc_blank_skip_compact(*{**ok, **over}.values())
    for name in ("vals", "ids", "blank_lp", "out_vals", "out_ids", "out_blank_lp", "out_len"):
        assert call(**{name: None}) == -1, name
    for over in (dict(B=0), dict(T=0), dict(k=0), dict(k=64), dict(thr=0.5), dict(thr=float("nan")), dict(reset=a), dict(map_cap=9), dict(map_cap=0),
                 dict(out_frame=None), dict(out_vals=a), dict(out_ids=a + 4096), dict(out_blank_lp=a + 8192), dict(vals=a + 2), dict(B=70000)):
        assert call(**over) == -1, over
    assert "asr_ctc_blank_skip_compact" in _lib.last_error()
    for ptrs in ((None, a, a), (a, None, a), (a, a + 4096, None), (a + 1, a + 4096, a), (a, a + 4096, a + 4096)):      # null, misaligned, map as output
        assert f.asr_frame_index_remap(*ptrs, 2, 10, 10, None) == -1, ptrs
    for bad in ((0, 10, 10), (2, 0, 10), (2, 10, 0)):
        assert f.asr_frame_index_remap(a, a + 4096, a, *bad, None) == -1
