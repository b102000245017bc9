"""Blank-frame skipping on the GPU, bit for bit against its definition (tests/blank_skip_ref.py): asr_ctc_blank_skip_compact on hand-made
and random rows, the offline search with blank_skip against the plain entry point on host-compacted inputs in all four modes, the
resumable compaction + search under every cutting against the offline result on the frames so far, and model.stream / model.sessions."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import blank_skip_ref as R  # noqa: E402

DEV = "cuda"
P = 0.98
THR = R.threshold(P)
HI, LO = np.float32(math.log(0.99)), np.float32(math.log(0.5))
V = 30      # the vocabulary of the small streaming models


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------------------ the compaction kernel
def _hand_rows(T, seed):
    """blank_lp (6, T) and in_len: random runs with high runs laid across the block boundaries 63 | 64 and 127 | 128, all high, none
    high, NaN and threshold-equal values among high ones, a ragged random row, and a row of length 0."""
    rng = np.random.default_rng(seed)
    lp = np.where(rng.random((6, T)) < 0.7, HI, LO).astype(np.float32)
    for lo, hi in ((60, 70), (120, 135), (190, 193)):
        lp[0, lo:hi] = HI
    lp[0, 59:60], lp[0, 119:120] = LO, LO
    lp[1], lp[2] = HI, LO
    lp[3] = HI
    lp[3, 2::5], lp[3, 3::7] = np.float32("nan"), THR
    in_len = [T, T, T, T, (2 * T) // 3, 0]
    return lp, in_len


@pytest.mark.parametrize("k", [1, 5, 10])
@pytest.mark.parametrize("T", [0, 1, 63, 64, 65, 129, 257])
def test_compaction_kernel_matches_the_reference(K, T, k):
    lp, in_len = _hand_rows(T, 100 * T + k)
    B = lp.shape[0]
    rng = np.random.default_rng(T + k)
    vals = rng.normal(size=(B, T, k)).astype(np.float32)
    ids = rng.integers(0, V, (B, T, k)).astype(np.int32)
    want = R.compact(vals, ids, lp, in_len, THR)
    for b in range(B):      # rows past the count are NaN / a poison id on the device: they are not read, so nothing of them comes out
        lp[b, in_len[b]:], vals[b, in_len[b]:], ids[b, in_len[b]:] = np.float32("nan"), np.float32("nan"), -7
    dev = (torch.from_numpy(vals).to(DEV).reshape(B * T, k), torch.from_numpy(ids).to(DEV).reshape(B * T, k), torch.from_numpy(lp).to(DEV).reshape(B * T))
    runs = [K.ctc_blank_skip_compact(*dev, _i32(in_len), float(THR), B, T) for _ in range(2)]
    ov, oi, ob, out_len, out_frame = (t.cpu().numpy() for t in runs[0])
    assert out_len.tolist() == want[3].tolist()
    assert np.array_equal(out_frame, want[4])      # zero behind the kept rows
    ov, oi, ob = ov.reshape(B, T, k), oi.reshape(B, T, k), ob.reshape(B, T)
    for b in range(B):
        n = int(out_len[b])
        assert np.array_equal(ov[b, :n].view(np.int32), want[0][b, :n].view(np.int32)) and np.array_equal(oi[b, :n], want[1][b, :n])
        assert np.array_equal(ob[b, :n].view(np.int32), want[2][b, :n].view(np.int32))
    if T >= 63:
        assert out_len[1] == 1 and out_len[2] == T and 0 < out_len[0] < T and out_len[5] == 0
        assert np.isnan(ob[3, :out_len[3]]).any() and (ob[3, :out_len[3]] == THR).any()      # NaN and the threshold itself are kept
    # two runs write the same bytes into the rows they own
    for a, b_ in zip(runs[0][:3], runs[1][:3]):
        a, b_ = (_bits(x).view(B, T, x.shape[1] if x.dim() == 2 else 1) for x in (a, b_))
        assert all(torch.equal(a[b, :int(out_len[b])], b_[b, :int(out_len[b])]) for b in range(B))
    assert torch.equal(runs[0][3], runs[1][3]) and torch.equal(runs[0][4], runs[1][4])
    # p = 1 keeps every row; no count = T rows each
    if T > 0:
        lp1 = torch.from_numpy(np.minimum(np.nan_to_num(lp, nan=-1.0), 0.0)).to(DEV).reshape(B * T)
        a = K.ctc_blank_skip_compact(dev[0], dev[1], lp1, None, 0.0, B, T)
        assert a[3].tolist() == [T] * B and torch.equal(_bits(a[0]), _bits(dev[0])) and torch.equal(a[1], dev[1]) and torch.equal(a[2], lp1)
        assert a[4].tolist() == [list(range(T))] * B


def test_frame_index_remap(K):
    g = torch.Generator().manual_seed(2)
    fmap = torch.sort(torch.randint(0, 1000, (3, 40), generator=g), dim=1)[0].to(torch.int32).to(DEV)
    idx = torch.randint(-2, 45, (3, 4, 9), generator=g).to(torch.int32).to(DEV)      # negative and past-the-map values stay
    want = idx.clone()
    for b in range(3):
        m = (idx[b] >= 0) & (idx[b] < 40)
        want[b][m] = fmap[b][idx[b][m].long()]
    out = K.frame_index_remap(idx, fmap)
    assert torch.equal(out, want) and out.data_ptr() != idx.data_ptr()
    assert K.frame_index_remap(idx, fmap, out=idx) is idx and torch.equal(idx, want)      # in place


# ------------------------------------------------------------------------------------------------------------ peaky candidates
B, T = 3, 130
LENS = [130, 97, 66]


def _peaky(seed, Bn=B, Tn=T):
    """Logits (Bn, Tn, V) built directly: runs of 1 - 8 frames, blank-dominated (p(blank) > 0.99) with probability 0.7, otherwise a token of
    4 .. 12 leads a contested frame; a blank run is laid across frames 60 .. 70 and 120 .. 129, the block boundaries of the compaction."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (Bn, Tn, V)).astype(np.float32)
    x[:, :, 2:4] -= 30.0      # sos / eos are never spelled
    for b in range(Bn):
        t = 0
        while t < Tn:
            run = int(rng.integers(1, 9))
            if rng.random() < 0.7:
                x[b, t:t + run, 0] += 12.0
            else:
                x[b, t:t + run, int(rng.integers(4, 13))] += 2.5
            t += run
        if Tn >= 130:
            x[b, 60:70, 0] = 14.0
            x[b, 120:130, 0] = 14.0
    return torch.from_numpy(x).to(DEV)


_CAND = {}


def _cand(K, k, seed=1):
    """(logits, vals, ids, blank_lp, the reference's compaction of them for LENS as numpy), computed once per k."""
    if (k, seed) not in _CAND:
        logits = _peaky(seed)
        vals, ids, blank_lp = K.ctc_frame_topk(logits.reshape(B * T, V), k, 0)
        host = R.compact(vals.view(B, T, k).cpu().numpy(), ids.view(B, T, k).cpu().numpy(), blank_lp.view(B, T).cpu().numpy(), LENS, THR)
        share = 1.0 - host[3].sum() / sum(LENS)
        assert 0.5 <= share <= 0.8, share      # the share of dropped frames: the tests below cannot pass by skipping nothing
        _CAND[(k, seed)] = (logits, vals, ids, blank_lp, host)
    return _CAND[(k, seed)]


_LM = {}


def _mode_kw(mode):
    if mode == "ctx":
        from asr_chinese_e2e_amd.context import ContextGraph
        if "ctx" not in _LM:
            _LM["ctx"] = ContextGraph([[(5, 6), (7, 8, 9), (10,), (4, 11)]], score=3.0, device=DEV, vocab_size=V)
        return dict(context=_LM["ctx"])
    if mode == "lm":
        from tests.test_lm_gpu import _model_lm
        if "lm" not in _LM:
            _LM["lm"] = _model_lm(V)[0]
        return dict(lm=_LM["lm"])
    return dict(times=True) if mode == "timed" else {}


def _model_kw(mode):
    """The same modes as keywords of the model's entry points."""
    return dict(beam_times=True) if mode == "timed" else _mode_kw(mode)


MODES = ["plain", "ctx", "lm", "timed"]
SHAPES = [(1, 10), (5, 10), (16, 3)]      # (beam, k): beam * (k + 1) <= 64


@pytest.mark.parametrize("beam,k", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_offline_kernels_with_compaction_equal_the_search_on_host_compacted_rows(K, mode, beam, k):
    """Every output of the search - tokens, lengths, scores, and per mode bias and state, or the best alignments' records."""
    _, vals, ids, blank_lp, host = _cand(K, k)
    kw = _mode_kw(mode)
    cv, ci, cb, out_len, fmap = K.ctc_blank_skip_compact(vals, ids, blank_lp, _i32(LENS), float(THR), B, T)
    assert out_len.tolist() == host[3].tolist() and np.array_equal(fmap.cpu().numpy(), host[4])
    got = K.ctc_prefix_beam(cv, ci, cb, out_len, B, T, beam, beam, 0, **kw)
    hv, hi, hb = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in host[:3])
    want = K.ctc_prefix_beam(hv.reshape(B * T, k), hi.reshape(B * T, k), hb.reshape(B * T), _i32(host[3].tolist()), B, T, beam, beam, 0, **kw)
    assert len(got) == len(want) == {"plain": 3, "ctx": 5, "lm": 5, "timed": 9}[mode]
    for g, w in zip(got, want):
        assert torch.equal(_bits(g) if g.dtype != torch.float64 else g.view(torch.int64), _bits(w) if w.dtype != torch.float64 else w.view(torch.int64))
    plain = K.ctc_prefix_beam(vals, ids, blank_lp, _i32(LENS), B, T, beam, beam, 0, **kw)
    assert not torch.equal(plain[2], got[2])      # the scores sum over the kept frames only
    if mode == "timed":      # the records count kept rows; the map takes them to the frames they were
        tok, ln = got[0].cpu().numpy(), got[1].cpu().numpy()
        for i in (4, 5):
            real = K.frame_index_remap(got[i], fmap).cpu().numpy()
            comp = got[i].cpu().numpy()
            for b in range(B):
                for r in range(beam):
                    n = max(int(ln[b, r]), 0)
                    assert real[b, r, :n].tolist() == host[4][b][comp[b, r, :n]].tolist()
        assert int(ln.max()) > 3


def _stream_model():
    from tests.test_stream_beam_gpu import _stream_model as make
    if "model" not in _LM:
        _LM["model"] = make("fp32", "TransformerCTC", 4)
    return _LM["model"]


class _Inject:
    """K.ctc_frame_topk over logits the test built directly (a random-weight model has no blank-dominated frames): the encoder and the CTC
    head run as they do, the candidates come from `rows`, which the test sets to the frames the launch is about."""

    def __init__(self, K):
        self.real, self.rows = K.ctc_frame_topk, None

    def __call__(self, logits, k, blank=0):
        assert self.rows.shape == logits.shape, (self.rows.shape, logits.shape)
        return self.real(self.rows, k, blank)


@pytest.mark.parametrize("beam,k", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_offline_search_with_blank_skip_equals_the_plain_entry_point_on_host_compacted_input(K, monkeypatch, mode, beam, k):
    from asr_chinese_e2e_amd.Utils import Pack
    logits, _, _, _, host = _cand(K, k)
    model = _stream_model()
    kw = _model_kw(mode)
    inj = _Inject(K)
    monkeypatch.setattr(K, "ctc_frame_topk", inj)
    feats = torch.randn(B, T, 16, generator=torch.Generator().manual_seed(3)).to(DEV)
    pack = Pack(wave=feats, wave_len=_i32(LENS))
    inj.rows = logits.reshape(B * T, V)
    got = model.ctc_prefix_beam_search(pack, beam, beam, k, blank_skip=P, **kw)
    plain = model.ctc_prefix_beam_search(pack, beam, beam, k, **kw)
    assert model.ctc_prefix_beam_search(pack, beam, beam, k, blank_skip=1.0, **kw) == plain      # p = 1 keeps every frame
    assert model.ctc_prefix_beam_search(pack, beam, beam, k, blank_skip=None, **kw) == plain
    # the reference's kept rows of the logits, in front; top-k is row by row, so these are the host-compacted candidates
    comp = torch.zeros_like(logits)
    for b in range(B):
        n = int(host[3][b])
        comp[b, :n] = logits[b, torch.from_numpy(host[4][b, :n]).long().to(DEV)]
    inj.rows = comp.reshape(B * T, V)
    want = model.ctc_prefix_beam_search(Pack(wave=feats, wave_len=_i32(host[3].tolist())), beam, beam, k, **kw)
    if mode == "timed":      # start_frame / end_frame = out_frame[...] of the compact indices, the times follow; measures and viterbi_score bit for bit
        d, moved = model.frame_seconds(), 0
        for b in range(B):
            for h in want[b]:
                for t in h["tokens"]:
                    moved += int(host[4][b, t["start_frame"]]) > t["start_frame"]
                    t["start_frame"], t["end_frame"] = int(host[4][b, t["start_frame"]]), int(host[4][b, t["end_frame"]])
                    t["start_s"], t["end_s"] = t["start_frame"] * d, (t["end_frame"] + 1) * d
        assert moved > 0      # frames were dropped in front of some token
    assert got == want
    assert got != plain and all(l and l[0]["yseq"] for l in got)


# ------------------------------------------------------------------------------------------------------------ the resumable form
def _cuts(name):
    if isinstance(name, int):
        return [name] * (-(-T // name))
    return [58, 7, 3, 62]      # frames 60 .. 70 are one high run: the chunk boundary at 65 splits it, so does 68


def _lcp(tok, ln):
    """The length of the longest common prefix of the entries of one utterance (rows with ln < 0 are missing ranks)."""
    rows = [tok[r][:ln[r]] for r in range(len(ln)) if ln[r] >= 0]
    n = 0
    while all(len(r) > n for r in rows) and len({r[n] for r in rows}) == 1:
        n += 1
    return n


@pytest.mark.parametrize("cut", [1, 5, 16, 64, 65, "split_run"])
@pytest.mark.parametrize("mode", MODES)
def test_chunked_compaction_and_search_equal_the_offline_result_on_the_frames_so_far(K, mode, cut):
    beam, k = 5, 5
    _, vals, ids, blank_lp, _ = _cand(K, k)
    kw = _mode_kw(mode)
    vals3, ids3, lp2 = vals.view(B, T, k), ids.view(B, T, k), blank_lp.view(B, T)
    st = K.ctc_prefix_beam_state(B, beam, T, DEV, **kw)
    sk = K.BlankSkipState(B, T, DEV)
    t0, checked = 0, 0
    cuts = _cuts(cut)
    for i, C in enumerate(cuts):
        for empty in ((True, False) if i % 3 == 1 else (False,)):      # an empty chunk in between: it keeps the carry bit and every other word
            nv = [0 if empty else max(0, min(C, l - t0)) for l in LENS]
            cv = torch.zeros(B, C, k, device=DEV)
            ci = torch.zeros(B, C, k, dtype=torch.int32, device=DEV)
            cb = torch.full((B, C), float("nan"), device=DEV)
            n = min(C, T - t0)
            cv[:, :n], ci[:, :n], cb[:, :n] = vals3[:, t0:t0 + n], ids3[:, t0:t0 + n], lp2[:, t0:t0 + n]
            before = sk.state.clone()
            ov, oi, ob, n_dev, fmap = K.ctc_blank_skip_compact(cv.view(B * C, k), ci.view(B * C, k), cb.view(B * C), _i32(nv), float(THR), B, C, sk)
            if empty:
                assert torch.equal(sk.state, before) and n_dev.tolist() == [0] * B
            res = K.ctc_prefix_beam_chunk(st, ov, oi, ob, nv, C, beam, 0, max_len=T, nv_dev=n_dev)
        t0 += C
        if cut == 1 and i % 9 and i != len(cuts) - 1:      # single frames: compare every ninth chunk and the last
            continue
        seen = [min(l, t0) for l in LENS]
        assert sk.state[:, 1].tolist() == seen
        wv, wi, wb, w_len, w_map = K.ctc_blank_skip_compact(vals, ids, blank_lp, _i32(seen), float(THR), B, T)
        assert sk.state[:, 2].tolist() == w_len.tolist() and sk.state[:, 0].tolist() == [int(R.is_high(float(lp2[b, s - 1]), THR)) if s else 0 for b, s in enumerate(seen)]
        assert all(torch.equal(fmap[b, :int(w_len[b])], w_map[b, :int(w_len[b])]) for b in range(B))
        want = K.ctc_prefix_beam(wv, wi, wb, w_len, B, T, beam, beam, 0, **kw)
        names = [f[0] for f in K.prefix_beam_layout(B, beam, T, st.mode)[0]]
        by = dict(zip(names, res))
        off = dict(zip([n_ for n_ in names if n_ not in ("stable", "final")], want))
        for name, w in off.items():
            g = by[name]
            assert torch.equal(g.view(torch.int64) if g.dtype == torch.float64 else _bits(g), w.view(torch.int64) if w.dtype == torch.float64 else _bits(w)), (name, t0)
        tok, ln = want[0].cpu().tolist(), want[1].cpu().tolist()
        assert by["stable"].tolist() == [_lcp(tok[b], ln[b]) for b in range(B)]      # the stable prefix is that of the offline beam
        if mode == "timed":
            for name in ("start", "end"):
                assert torch.equal(K.frame_index_remap(by[name], sk.frame_map), K.frame_index_remap(off[name], w_map))
        checked += 1
    assert checked >= 2 and t0 >= T and st.frames == LENS


def test_a_reset_clears_the_carry_bit_and_the_map(K):
    k, C = 3, 8
    lp = torch.full((2, C), float(HI), device=DEV)
    vals, ids = torch.randn(2 * C, k, device=DEV), torch.ones(2 * C, k, dtype=torch.int32, device=DEV)
    sk = K.BlankSkipState(2, 64, DEV)
    K.ctc_blank_skip_compact(vals, ids, lp.view(-1), _i32([C, C]), float(THR), 2, C, sk)
    assert sk.state.tolist() == [[1, C, 1, 0]] * 2
    out = K.ctc_blank_skip_compact(vals, ids, lp.view(-1), _i32([C, 3]), float(THR), 2, C, sk, _i32([1, 0]))
    # utterance 0 starts over in the middle of the high run: its first frame is frame 0 again and is kept; utterance 1 goes on
    assert out[3].tolist() == [1, 0] and sk.state.tolist() == [[1, C, 1, 0], [1, C + 3, 1, 0]]
    assert sk.frame_map[:, :2].tolist() == [[0, 0], [0, 0]]
    lo = torch.full((2, C), float(LO), device=DEV)
    out = K.ctc_blank_skip_compact(vals, ids, lo.view(-1), _i32([0, 2]), float(THR), 2, C, sk, _i32([1, 0]))      # a reset without a frame
    assert out[3].tolist() == [0, 2] and sk.state.tolist() == [[0, 0, 0, 0], [0, C + 5, 3, 0]] and sk.frame_map[1, :3].tolist() == [0, C + 3, C + 4]


# ------------------------------------------------------------------------------------------------------------ model.stream, model.sessions
def _push_rows(inj, synth, pos, C):
    """The candidates' logits of one tick: slot s gets rows pos[s] .. pos[s] + C of synth[s] (None: a slot without frames), zeros behind."""
    rows = torch.zeros(len(synth), C, V, device=DEV)
    for s, (u, p0) in enumerate(zip(synth, pos)):
        if u is not None:
            n = max(0, min(C, u.shape[0] - p0))
            rows[s, :n] = u[p0:p0 + n]
    inj.rows = rows.view(len(synth) * C, V)


@pytest.mark.parametrize("mode", MODES)
def test_stream_with_blank_skip_equals_the_offline_search_on_the_frames_so_far(K, monkeypatch, mode):
    from asr_chinese_e2e_amd.Utils import Pack
    C, Bm, beam, k = 4, 3, 4, 5
    lens = [38, 27, 12]
    Tm = 40
    model = _stream_model()
    kw = _model_kw(mode)
    synth = _peaky(9, Bm, Tm)
    synth[:, 10:18, 0] = 14.0      # a high run across the chunk boundaries 12 and 16: the carry bit works
    feats = torch.randn(Bm, Tm, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    inj = _Inject(K)
    monkeypatch.setattr(K, "ctc_frame_topk", inj)
    st = model.stream(Bm, search="prefix_beam", beam_size=beam, frame_topk=k, blank_skip=P, **kw)
    said = [[] for _ in range(Bm)]
    dropped = False
    for c0 in range(0, Tm, C):
        nv = [max(0, min(C, l - c0)) for l in lens]
        _push_rows(inj, list(synth), [c0] * Bm, C)
        for b, ids in enumerate(st.push(feats[:, c0:c0 + C].contiguous(), nv)):
            said[b] += ids
        got, part = st.nbest(), st.partial()
        toks = st.tokens() if mode == "timed" else None
        so_far = [min(l, c0 + C) for l in lens]
        enc, _ = st.encoder_output()
        wave = torch.zeros(Bm, enc.shape[1], 1, device=DEV)
        rows = torch.zeros(Bm, enc.shape[1], V, device=DEV)
        rows[:, :min(Tm, enc.shape[1])] = synth[:, :enc.shape[1]]
        inj.rows = rows.view(-1, V)
        with model.given_encoder_output(enc):
            want = model.ctc_prefix_beam_search(Pack(wave=wave, wave_len=_i32(so_far)), beam, beam, k, blank_skip=P, **kw)
            plain = model.ctc_prefix_beam_search(Pack(wave=wave, wave_len=_i32(so_far)), beam, beam, k, **kw)
        assert got == want, c0      # tokens, scores, bias / lm_score, viterbi_score and the timed records in real frames
        dropped = dropped or got != plain
        for b in range(Bm):
            assert part[b]["stable_len"] == len(said[b]) == _lcp([h["yseq"] for h in want[b]], [len(h["yseq"]) for h in want[b]])
            assert all(h["yseq"][:len(said[b])] == said[b] for h in got[b])
            if toks is not None and want[b] and want[b][0]["yseq"]:
                assert [{k_: v for k_, v in t.items() if k_ != "final"} for t in toks[b]] == want[b][0]["tokens"]
                fin = [t["final"] for t in toks[b]]
                assert fin == sorted(fin, reverse=True)
    assert dropped and any(said)
    # the greedy stream refuses it, and a stream without it launches no compaction
    with pytest.raises(ValueError, match="prefix_beam"):
        model.stream(Bm, blank_skip=P)
    called = []
    monkeypatch.setattr(K, "ctc_blank_skip_compact", lambda *a, **k_: called.append(1))
    monkeypatch.setattr(K, "frame_index_remap", lambda *a, **k_: called.append(1))
    st0 = model.stream(Bm, search="prefix_beam", beam_size=beam, frame_topk=k, **kw)
    _push_rows(inj, list(synth), [0] * Bm, C)
    st0.push(feats[:, :C].contiguous(), [C] * Bm)
    inj.rows = synth.reshape(-1, V)
    model.ctc_prefix_beam_search(Pack(wave=feats, wave_len=_i32(lens)), beam, beam, k, **kw)
    assert not called


def test_sessions_with_blank_skip_each_slot_equals_its_own_stream(K, monkeypatch):
    """A staggered schedule with a sat-out tick, and slot 0 closed and reopened in the middle of a high run of its neighbour's clock: each
    slot equals its own B = 1 stream tick by tick, the reopened slot starts with a clear carry bit and map, and the endpoint counters are
    those of the same schedule without blank_skip."""
    C, beam, k = 4, 4, 5
    model = _stream_model()
    synth = _peaky(13, 3, 24)
    synth[0, 13:24, 0] = 14.0      # utterance 0 ends inside a high run ...
    synth[1, 0:6, 0] = 14.0        # ... and utterance 1, which takes its slot, begins with one: a carried bit would drop its frame 0
    synth[2, 6:14, 0] = 14.0
    utts = [synth[0, :22], synth[1, :19], synth[2]]
    feats = [torch.randn(u.shape[0], 16, generator=torch.Generator().manual_seed(20 + i)).to(DEV) for i, u in enumerate(utts)]
    inj = _Inject(K)
    monkeypatch.setattr(K, "ctc_frame_topk", inj)

    def alone(i):
        st = model.stream(1, search="prefix_beam", beam_size=beam, frame_topk=k, blank_skip=P, beam_times=True)
        outs = []
        for c0 in range(0, utts[i].shape[0], C):
            n = min(C, utts[i].shape[0] - c0)
            x = torch.zeros(1, C, 16, device=DEV)
            x[0, :n] = feats[i][c0:c0 + n]
            _push_rows(inj, [utts[i]], [c0], C)
            outs.append((st.push(x, [n])[0], st.nbest()[0], st.tokens()[0]))
        return outs
    want = [alone(i) for i in range(3)]
    frame_ms = model.frame_seconds() * 1000.0
    rule = {"silence_start": (False, int(round(5 * frame_ms)), 0)}      # five silent frames in a row, decoded or not
    # slot 0: utterance 0, then utterance 1; slot 1: utterance 2, one tick later, sitting out tick 3
    plan = [  # per tick: per slot (utterance, chunk index) or None
        [(0, 0), None], [(0, 1), (2, 0)], [(0, 2), (2, 1)], [(0, 3), None], [(0, 4), (2, 2)], [(0, 5), (2, 3)],
        [(1, 0), (2, 4)], [(1, 1), (2, 5)], [(1, 2), None], [(1, 3), None], [(1, 4), None]]
    status = {}
    for skip in (P, None):
        ss = model.sessions(2, search="prefix_beam", beam_size=beam, frame_topk=k, beam_times=True, endpoint=rule, **(dict(blank_skip=skip) if skip else {}))
        ss.open(0)
        log = []
        for tick, row in enumerate(plan):
            if tick == 1:
                ss.open(1)
            if row[0] == (1, 0):      # utterance 0 is over: finish its slot and open it again
                ss.finish(0, joint="ctc_rescore", timestamps=False)
                ss.open(0)
            x = torch.zeros(2, C, 16, device=DEV)
            nv, fin, src, pos = [0, 0], [False, False], [None, None], [0, 0]
            for s, job in enumerate(row):
                if job is not None:
                    u, c = job
                    n = min(C, utts[u].shape[0] - c * C)
                    x[s, :n], nv[s], fin[s], src[s], pos[s] = feats[u][c * C:c * C + n], n, (c + 1) * C >= utts[u].shape[0], utts[u], c * C
            _push_rows(inj, src, pos, C)
            got = ss.push(x, nv, fin)
            for s, job in enumerate(row):
                if job is not None and skip:
                    u, c = job
                    assert (got[s], ss.nbest(s), ss.tokens(s)) == want[u][c], (tick, s)
            if skip and row[0] == (1, 0):      # the reopened slot: its four high frames are frames 0 .. 3 of a new session, frame 0 is kept
                assert ss.skip.state[0].tolist() == [1, C, 1, 0] and int(ss.skip.frame_map[0, 0]) == 0
            log.append((ss.endpoints(), [ss.status(s)["trailing_silence_frames"] for s in range(2)], [ss.status(s)["frames"] for s in range(2)]))
        status[skip] = log
    # endpointing reads every frame: the reported rules, the trailing silence and the frame counts do not change
    assert status[P] == status[None]
    assert any(e == "silence_start" for l in status[P] for e in l[0]) and any(t > 0 for l in status[P] for t in l[1])


# ------------------------------------------------------------------------------------------------------------ command line
def test_transcribe_cli_blank_skip(K, tmp_path, capsys, monkeypatch):
    """transcribe.py --blank_skip offline, with --long=1 and with --stream=1 --stream_search=prefix_beam (--sessions=2 included), in this
    process: 1.0 prints the lines of the run without the flag, a threshold that every frame of the random model passes runs the compaction
    and changes scores, and a bad value or a search without a prefix beam ends the run."""
    import json
    import sys
    from asr_chinese_e2e_amd.data_handler import Vocab
    from asr_chinese_e2e_amd.data_handler.cmvn import save_cmvn
    from tests.helpers import ROOT
    from tests.test_ctc_align_gpu import _write_wav
    sys.path.insert(0, ROOT)
    import transcribe as T_
    from train import TrainConfig, get_model_class, parse_flags
    flags = dict(model_name="TransformerCTC", d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1, dtype="fp32", n_mels=40,
                 decoding_chunk_size=8, decoding_left_chunks=2)
    config = TrainConfig()
    config.fn_build(dict(flags))
    Model, MC = get_model_class(config.model_name)
    config.fn_combine(MC())
    config.fn_build(dict(flags))
    vocab = Vocab.synthetic(40)
    vocab.save(str(tmp_path / "vocab.t"))
    torch.manual_seed(0)
    Model(config, vocab).save(str(tmp_path / "m.model"))
    save_cmvn(str(tmp_path / "cmvn.npz"), np.full(40, -6.0), np.full(40, 0.4), 1000)
    wavs = [tmp_path / "a.wav", tmp_path / "b.wav", tmp_path / "c.wav"]
    for i, (p, s) in enumerate(zip(wavs, [0.9, 0.5, 0.7])):
        _write_wav(p, s, i)
    argv = [f"--{k}={v}" for k, v in flags.items()] + [f"--ckpt={tmp_path / 'm.model'}", f"--vocab_path={tmp_path / 'vocab.t'}",
                                                       "--wavs=" + ",".join(map(str, wavs)), "--beam_size=3", f"--cmvn={tmp_path / 'cmvn.npz'}"]
    streamed = ["--stream=1", "--stream_search=prefix_beam", "--frame_topk=5"]
    launches = []
    real = K.ctc_blank_skip_compact
    monkeypatch.setattr(K, "ctc_blank_skip_compact", lambda *a, **kw: launches.append(1) or real(*a, **kw))
    capsys.readouterr()

    def run(extra):
        del launches[:]
        T_.transcribe(**parse_flags(argv + extra))
        lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        finals = {l["file"]: l for l in lines if "ids" in l and "file" in l and "duration_s" in l}
        assert sorted(finals) == sorted(map(str, wavs)), extra
        return finals, len(launches)
    # under p = 1e-30 every frame of a random model is "high" and only the first of each utterance stays; under p = 1 none is
    for mode in ([], streamed, streamed + ["--sessions=2"], ["--long=1"]):
        plain, n0 = run(mode)
        same, n1 = run(mode + ["--blank_skip=1.0"])
        low, n2 = run(mode + ["--blank_skip=1e-30"])
        searched = mode != ["--long=1"] or any(l.get("segments") for l in plain.values())      # a recording without speech reaches no search
        assert n0 == 0 and (n1 > 0) == searched and (n2 > 0) == searched, mode
        assert same == plain, mode
        if mode != ["--long=1"]:
            assert any(low[f]["score"] != plain[f]["score"] for f in plain), mode
    for bad in ("0", "1.5", "nan", "x"):
        with pytest.raises(SystemExit, match="blank_skip"):
            T_.transcribe(**parse_flags(argv + [f"--blank_skip={bad}"]))
    with pytest.raises(SystemExit, match="prefix_beam"):
        T_.transcribe(**parse_flags(argv + ["--blank_skip=0.98", "--stream=1"]))      # the greedy stream reads every frame
