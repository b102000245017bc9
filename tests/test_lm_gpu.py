"""N-gram LM shallow fusion on the GPU: asr_ctc_prefix_beam_lm against the fp64 definition (tests/lm_ref.py), weight 0 against
asr_ctc_prefix_beam bit for bit, the resumable kernel against the offline one under every cutting, the reset, and the model level
(model.stream, model.sessions, ctc_rescore, the refusals, transcribe.py --lm)."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lm_ref as R  # noqa: E402

DEV = "cuda"
B, T, V = 3, 48, R.V
LENS = [T, 29, 41]      # ragged, the first is full; 29 and 41 end inside a chunk of 16 and of 5
# an insertion bonus on purpose: on the flat lattices a prefix then leaves the beam while a longer one stays, and comes back later - the case
# the LM kernels' child lists exist for (without them the same string is held twice and its ctc_score comes out 0.14 off at k, beam = 5, 10)
WEIGHT, INS = 0.5, 0.3
SEED = 10               # chosen on the CPU: the reference's smallest ranking gap over all cases below is 3.1e-5 (asserted > 1e-9)
SHAPES = [(5, 4), (5, 10), (3, 16)]      # (k, beam)
PEAKS = [3.0, 0.3]


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


_LM, _CAND = {}, {}


def _lm(weight=WEIGHT, ins=INS):
    from asr_chinese_e2e_amd.lm import NgramLM
    if (weight, ins) not in _LM:
        _LM[(weight, ins)] = NgramLM(R.table(), R.ORDER, V, weight=weight, ins=ins, device=DEV)
    return _LM[(weight, ins)]


def _cand(K, k, peak):
    """One random lattice (the generator of tests/test_context_gpu.py) and its per-frame candidates."""
    if (k, peak) not in _CAND:
        g = torch.Generator().manual_seed(SEED)
        logits = torch.randn(B, T, V, generator=g) * peak
        vals, ids, blank_lp = K.ctc_frame_topk(logits.reshape(B * T, V).to(DEV), k, 0)
        _CAND[(k, peak)] = (logits, vals, ids, blank_lp)
    return _CAND[(k, peak)]


def _len(lens=LENS):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------------------ the offline kernel
@pytest.mark.parametrize("peak", PEAKS, ids=["peaky", "flat"])
@pytest.mark.parametrize("k,beam", SHAPES)
def test_offline_kernel_matches_the_fp64_definition(K, k, beam, peak):
    from asr_chinese_e2e_amd.decode import lm_entries
    lm = _lm()
    ref = R.Model(R.table(), R.ORDER, WEIGHT, INS)
    logits, vals, ids, blank_lp = _cand(K, k, peak)
    res = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0, lm=lm)
    tok, ln, sc, bias, state = (x.cpu().tolist() for x in res)
    ptok, pln, _ = (x.cpu().tolist() for x in K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0))
    logp = torch.log_softmax(logits.double(), -1).numpy()
    ids_h = ids.view(B, T, k).cpu().numpy()
    differs = 0
    for b in range(B):
        want, gap = R.ctc_prefix_beam_search(logp[b, :LENS[b]], beam, candidates=[list(ids_h[b, t]) for t in range(LENS[b])], lm=ref)
        print(f"k={k} beam={beam} peak={peak} b={b}: smallest ranking gap of the reference {gap:.3e}")
        assert gap > 1e-9, (b, gap)      # a failure below is the kernel's, not a near tie
        want = [h for h in want if h[2] > -1e300]
        got = lm_entries(lm, tok[b], ln[b], sc[b], bias[b], state[b])
        assert [tuple(h["yseq"]) for h in got] == [h[0] for h in want], (b, got, want)      # in order, over the whole beam
        for h, (_, w_sc, w_ctc, w_lm) in zip(got, want):
            assert abs(h["ctc_score"] - w_ctc) < 1e-5 * max(1.0, abs(w_ctc)), (b, h, w_ctc)
            assert h["lm_score"] == w_lm, (b, h, w_lm)      # exactly: the same fp64 additions
            assert h["score"] == h["ctc_score"] + h["lm_score"]
        for r in range(beam):      # the raw outputs: the bias and the state of each entry are those of its string
            if ln[b][r] >= 0:
                assert (state[b][r], bias[b][r]) == lm.walk(tok[b][r][:ln[b][r]]), (b, r)
        plain = [tuple(ptok[b][r][:pln[b][r]]) for r in range(beam) if pln[b][r] >= 0]
        differs += [tuple(h["yseq"]) for h in got] != plain
    assert differs > 0      # the LM has an effect on this lattice


@pytest.mark.parametrize("peak", PEAKS, ids=["peaky", "flat"])
@pytest.mark.parametrize("k,beam", SHAPES)
def test_weight_zero_has_the_plain_kernels_bits(K, k, beam, peak):
    _, vals, ids, blank_lp = _cand(K, k, peak)
    wt, wl, ws = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0)
    z = _lm(0.0, 0.0)
    tok, ln, sc, bias, state = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0, lm=z)
    assert torch.equal(tok, wt) and torch.equal(ln, wl) and torch.equal(sc, ws)
    assert (bias == 0.0).all() and not torch.signbit(bias).any()      # all +0.0
    assert ((state >= 0) == (ln >= 0)).all() and (state < z.S).all()
    tok, ln, sc, bias, state = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0, lm=_lm())
    assert not torch.equal(tok, wt)      # and with its weight the LM changes the beam


def test_wrappers_refuse_what_they_can_check(K):
    from asr_chinese_e2e_amd._lib import AsrHipError
    from asr_chinese_e2e_amd.context import ContextGraph
    lm = _lm()
    _, vals, ids, blank_lp = _cand(K, 5, 3.0)
    with pytest.raises(AsrHipError):      # 12 * 6 > 64 slots
        K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, 12, 12, 0, lm=lm)
    with pytest.raises(ValueError, match="cannot be combined"):
        K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, 4, 4, 0, lm=lm, context=ContextGraph([[(4, 5)]], vocab_size=V))
    st = K.ctc_prefix_beam_state(B, 4, T, DEV, lm=lm)
    flags = torch.zeros(B, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="context state"):
        K.ctc_prefix_beam_state_reset(st, flags, roots=[0, 0, 0])
    with pytest.raises(ValueError, match="the state was made with"):
        K.ctc_prefix_beam_state_reset(st, flags, lm=_lm(0.0, 0.0))
    with pytest.raises(ValueError, match="the state was made with"):
        K.ctc_prefix_beam_state_reset(K.ctc_prefix_beam_state(B, 4, T, DEV), flags, lm=lm)


# ------------------------------------------------------------------------------------------------------------ the resumable kernel
def _cuttings():
    """tests/test_stream_beam_gpu.py's cuttings for this T: name -> [(C, c0 or None)], None = a chunk that consumes nothing."""
    by5 = [(5, c0) for c0 in range(0, T, 5)]
    gaps = []
    for ch in by5:
        gaps += [ch, (5, None)]
    return {"whole": [(T, 0)], "frames": [(1, t) for t in range(T)], "C16": [(16, c0) for c0 in range(0, T, 16)], "C5": by5,
            "C5_gaps": [(5, None)] + gaps}


def _rows(x, c0, C):
    x = x.view(B, T, *x.shape[1:])
    part = x[:, c0:c0 + C]
    if part.shape[1] < C:
        part = torch.cat([part, torch.zeros(B, C - part.shape[1], *x.shape[2:], dtype=x.dtype, device=x.device)], dim=1)
    return part.reshape(B * C, *x.shape[2:]).contiguous()


def _lcp(rows):
    n = 0
    for col in zip(*rows):
        if any(c != col[0] for c in col):
            break
        n += 1
    return n


@pytest.mark.parametrize("peak", PEAKS, ids=["peaky", "flat"])
@pytest.mark.parametrize("k,beam", SHAPES)
def test_chunk_kernel_equals_offline_kernel_under_every_cutting(K, k, beam, peak):
    lm = _lm()
    _, vals, ids, blank_lp = _cand(K, k, peak)
    ref = {}
    for t in range(1, T + 1):      # the offline kernel on the first t frames, once
        ref[t] = K.ctc_prefix_beam(vals, ids, blank_lp, _len([min(l, t) for l in LENS]), B, T, beam, beam, 0, lm=lm)
    for name, chunks in _cuttings().items():
        st = K.ctc_prefix_beam_state(B, beam, T, DEV, lm=lm)
        assert st.state.numel() * 8 == K.lib.asr_ctc_prefix_beam_lm_state_bytes(B, beam)
        done, last_stable = 0, [0] * B
        for C, c0 in chunks:
            nv = [0] * B if c0 is None else [max(0, min(C, l - c0)) for l in LENS]
            c0 = 0 if c0 is None else c0
            before = (st.state.clone(), st.ws.clone()) if not any(nv) else None
            tok, ln, sc, stable, bias, state = K.ctc_prefix_beam_chunk(st, _rows(vals, c0, C), _rows(ids, c0, C), _rows(blank_lp, c0, C), nv, C, beam, 0,
                                                                       max_len=T)
            if before is not None:      # a chunk that consumes nothing changes no byte of the state (nor of the trie)
                assert torch.equal(st.state, before[0]) and torch.equal(st.ws, before[1]), name
            done = max(done, c0 + max(nv)) if any(nv) else done
            if done == 0:
                assert ln[:, 0].tolist() == [0] * B and sc[:, 0].tolist() == [0.0] * B and stable.tolist() == [0] * B
                assert bias[:, 0].tolist() == [0.0] * B and state[:, 0].tolist() == [lm.start] * B
                continue
            wt, wl, ws_, wb, wst = ref[done]      # equal, not close
            assert torch.equal(ln, wl) and torch.equal(tok, wt), (name, done)
            assert torch.equal(sc, ws_), (name, done, sc, ws_)
            assert torch.equal(bias, wb) and torch.equal(state, wst), (name, done, bias, wb, state, wst)
            tl, ll = wt.cpu().tolist(), wl.cpu().tolist()
            want_stable = [_lcp([tl[b][r][:ll[b][r]] for r in range(beam) if ll[b][r] >= 0]) for b in range(B)]
            got_stable = stable.tolist()
            assert got_stable == want_stable, (name, done, got_stable, want_stable)      # the LCP of the full beam, whatever the ranking
            assert all(g >= p for g, p in zip(got_stable, last_stable)), (name, done, got_stable, last_stable)      # never retracted
            last_stable = got_stable
        assert done == T and st.frames == LENS, name


def test_lm_state_reset_restarts_the_flagged_slot_and_touches_no_other(K):
    C, beam, k, T_cap = 8, 4, 5, 64
    lm = _lm()
    g = torch.Generator().manual_seed(21)
    chunks = [torch.randn(B * C, V, generator=g).to(DEV) * 2 for _ in range(6)]
    st = K.ctc_prefix_beam_state(B, beam, T_cap, DEV, lm=lm)
    fresh0 = st.state.clone()
    for x in chunks[:3]:
        K.ctc_prefix_beam_chunk(st, *K.ctc_frame_topk(x, k, 0), [C, C - 3, C], C, beam)
    state0, ws0 = st.state.clone(), st.ws.clone()
    flags = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    K.ctc_prefix_beam_state_reset(st, flags, [1], lm=lm)
    per = st.state.numel() // B
    nodes, nodes0 = st.ws.view(torch.int32).view(B, -1), ws0.view(torch.int32).view(B, -1)
    for b in (0, 2):
        assert torch.equal(st.state.view(B, per)[b], state0.view(B, per)[b]) and torch.equal(nodes[b], nodes0[b])
    assert torch.equal(st.state.view(B, per)[1], fresh0.view(B, per)[1])      # byte for byte a fresh state: the start state, no bias
    assert not torch.equal(st.state.view(B, per)[1], state0.view(B, per)[1])
    # the start state is in it
    words = st.state.view(torch.int32).view(B, -1)[1]
    plain_words = K.lib.asr_ctc_prefix_beam_state_bytes(1, beam) // 4
    assert words[plain_words + 2 * beam:plain_words + 3 * beam].tolist() == [lm.start] * beam and lm.start != 0
    assert st.frames == [3 * C, 0, 3 * C]
    fresh = K.ctc_prefix_beam_state(B, beam, T_cap, DEV, lm=lm)
    for x in chunks[3:]:
        cand = K.ctc_frame_topk(x, k, 0)
        a = K.ctc_prefix_beam_chunk(st, *cand, [C, C, 0], C, beam, max_len=T_cap)
        f = K.ctc_prefix_beam_chunk(fresh, *cand, [0, C, 0], C, beam, max_len=T_cap)
        assert all(torch.equal(x_[1], y_[1]) for x_, y_ in zip(a, f))
    assert int(a[1][1, 0]) > 0 and float(a[4][1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------ the model level
def _model_lm(Vm, weight=0.5, ins=0.6, seed=5):
    """A random order-3 LM over the tiny models' vocabularies (ids 4 .. Vm - 1, <s> and </s>), with holes as the test LM has."""
    from asr_chinese_e2e_amd.lm import NgramLM
    rng = random.Random(seed)
    table = {(c,): (-0.5 - 2.0 * rng.random(), None if rng.random() < 0.3 else -rng.random()) for c in range(2, Vm - 1)}
    for a in range(2, Vm):
        for b in range(3, Vm):
            if a != 3 and rng.random() < 0.25:
                table[(a, b)] = (-0.1 - 2.0 * rng.random(), None if rng.random() < 0.3 else -rng.random())
    for _ in range(6 * Vm):
        g = (4 + int(rng.random() * (Vm - 4)), 4 + int(rng.random() * (Vm - 4)), 3 + int(rng.random() * (Vm - 3)))
        table[g] = (-0.05 - 1.5 * rng.random(), None)
    return NgramLM(table, 3, Vm, weight=weight, ins=ins, device=DEV), R.Model(table, 3, weight, ins)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stream_with_lm_matches_the_offline_search_on_the_streamed_frames(K, monkeypatch, dtype):
    from asr_chinese_e2e_amd.decode import lm_entries
    from tests.test_stream_beam_gpu import _stream_model
    C, Bm, beam, topk, Tm = 4, 3, 4, 5, 20
    lens = [19, 14, 6]
    model = _stream_model(dtype, "TransformerOffical", C)
    lm, ref = _model_lm(model.V)
    torch.manual_seed(7)
    feats = torch.randn(Bm, Tm, 16, device=DEV).to(torch.float32 if dtype == "fp32" else torch.bfloat16)
    fed = []
    real = K.ctc_frame_topk

    def recording(logits, k, blank=0):
        out = real(logits, k, blank)
        fed.append(tuple(t.clone() for t in out))
        return out
    monkeypatch.setattr(K, "ctc_frame_topk", recording)
    st = model.stream(Bm, search="prefix_beam", beam_size=beam, frame_topk=topk, lm=lm)
    end0 = ref.lm_score(())
    assert st.nbest() == [[{"yseq": [], "score": 0.0 + end0, "ctc_score": 0.0, "lm_score": end0}]] * Bm
    said = [[] for _ in range(Bm)]
    for c0 in range(0, Tm, C):
        nv = [max(0, min(C, l - c0)) for l in lens]
        for b, ids in enumerate(st.push(feats[:, c0:c0 + C].contiguous(), nv)):
            said[b] += ids
        part, nb = st.partial(), st.nbest()
        for b in range(Bm):      # what push handed out is the stable part of every revisable hypothesis, whatever the order by score
            assert part[b]["stable_len"] == len(said[b]) and all(h["yseq"][:len(said[b])] == said[b] for h in nb[b]), (c0, b)
            assert part[b]["ids"] == nb[b][0]["yseq"] and part[b]["score"] == nb[b][0]["score"] and part[b]["lm_score"] == nb[b][0]["lm_score"]
            assert [h["score"] for h in nb[b]] == sorted((h["score"] for h in nb[b]), reverse=True)
            assert all(h["lm_score"] == ref.lm_score(h["yseq"]) for h in nb[b])      # the definition, exactly
    monkeypatch.setattr(K, "ctc_frame_topk", real)
    vals, ids, blank_lp = (torch.cat([f[i].view(Bm, C, -1) for f in fed], dim=1) for i in range(3))
    cand = (vals.reshape(Bm * Tm, topk).contiguous(), ids.reshape(Bm * Tm, topk).contiguous(), blank_lp.reshape(Bm * Tm).contiguous())
    res = K.ctc_prefix_beam(*cand, _len(lens), Bm, Tm, beam, beam, 0, lm=lm)
    tok, ln, sc, bias, state = (x.cpu().tolist() for x in res)
    want = [lm_entries(lm, tok[b], ln[b], sc[b], bias[b], state[b]) for b in range(Bm)]
    assert st.nbest() == want
    ptok, pln, _ = (x.cpu().tolist() for x in K.ctc_prefix_beam(*cand, _len(lens), Bm, Tm, beam, beam, 0))
    assert any([h["yseq"] for h in want[b]] != [ptok[b][r][:pln[b][r]] for r in range(beam) if pln[b][r] >= 0] for b in range(Bm))      # the LM bites
    # the model's own offline search under the same chunk mask sees the same frames: the same lists
    from asr_chinese_e2e_amd.Utils import Pack
    enc, enc_len = st.encoder_output()
    with model.given_encoder_output(enc):
        off = model.ctc_prefix_beam_search(Pack(wave=feats, wave_len=enc_len), beam, beam, topk, lm=lm)
        host = model.ctc_prefix_beam_search(Pack(wave=feats, wave_len=enc_len), beam, beam, topk, on_device=False, lm=lm)
    assert off == want
    for b in range(Bm):      # the host loop applies the same definition through NgramLM.walk
        assert [h["yseq"] for h in host[b]] == [h["yseq"] for h in want[b]] and [h["lm_score"] for h in host[b]] == [h["lm_score"] for h in want[b]]
        assert all(abs(h["ctc_score"] - w["ctc_score"]) < 1e-5 * max(1.0, abs(w["ctc_score"])) for h, w in zip(host[b], want[b]))
    fin = st.finish(joint="ctc_rescore")
    for b in range(Bm):
        assert fin[b]["ids"][:len(said[b])] == said[b] and fin[b]["ids"] in [h["yseq"] for h in want[b]]
        assert fin[b]["lm_score"] == next(h["lm_score"] for h in want[b] if h["yseq"] == fin[b]["ids"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_session_reopened_mid_run_equals_a_fresh_stream(dtype):
    from tests.test_sessions_gpu import _chunk_of, _feats, _model
    C = 8
    model = _model(dtype, -1, C=C)
    lm, _ = _model_lm(model.V)
    first, second, other = _feats([20, 27, 13], dtype, seed=5)

    def alone(u, with_lm=True):
        st = model.stream(1, search="prefix_beam", beam_size=4, frame_topk=6, **(dict(lm=lm) if with_lm else {}))
        outs = []
        for c0 in range(0, u.shape[0], C):
            x, nv = _chunk_of([u], [c0], C)
            outs.append((st.push(x, nv)[0], st.nbest()[0]))
        return outs
    ss = model.sessions(2, search="prefix_beam", beam_size=4, frame_topk=6, lm=lm)
    with pytest.raises(ValueError, match="needs model.sessions"):
        ss.open(0, context=0)
    ss.open(0)
    ss.open(1)
    for n, utt in enumerate((first, second)):      # slot 0: one session, then reopened while its neighbour is in the middle of its own
        want = alone(utt)
        for i, c0 in enumerate(range(0, utt.shape[0], C)):
            x, nv = _chunk_of([utt, other if n == 0 else None], [c0, c0], C)
            fin = [c0 + C >= utt.shape[0], nv[1] > 0 and c0 + C >= other.shape[0]]
            got = ss.push(x, nv, fin)
            assert got[0] == want[i][0] and ss.nbest(0) == want[i][1], (n, i)
        assert all(set(h) == {"yseq", "score", "ctc_score", "lm_score"} for h in ss.nbest(0))
        res = ss.finish(0, joint="ctc_rescore")
        assert "lm_score" in res
        if n == 0:
            ss.open(0)
    assert [h["yseq"] for h in want[-1][1]] != [h["yseq"] for h in alone(second, with_lm=False)[-1][1]]      # the LM matters for this utterance


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ctc_rescore_with_lm_combines_the_lm_score_with_the_ctc_score(dtype):
    from tests.test_stream_beam_gpu import _rescore_model
    from tests.test_model_gpu import to_pack
    lam = 0.4
    _, _, batch, model = _rescore_model(dtype, lam)
    pack = to_pack(batch)
    lm, ref = _model_lm(model.V)
    from asr_chinese_e2e_amd import decode
    got = model.beam_search(pack, beam_size=4, nbest=4, ctc_weight=lam, joint="ctc_rescore", lm=lm)
    first = model.ctc_prefix_beam_search(pack, 4, 4, lm=lm)
    # the call without an LM for the same hypotheses: the same list without "lm_score", scored by the same decoder pass
    eng = model._ensure_engine(DEV)
    was, eng.training = eng.training, False
    with torch.no_grad():
        enc = model.forward(pack).encoder_out
    eng.training = was
    plain = decode.attention_rescore(model, enc, pack.wave_len, [[{"yseq": h["yseq"], "score": h["ctc_score"]} for h in l] for l in first], lam)
    for b, l in enumerate(got):
        assert set(l[0]) == {"yseq", "score", "att_score", "ctc_score", "lm_score"}
        assert [h["score"] for h in l] == sorted((h["score"] for h in l), reverse=True)
        assert sorted(tuple(h["yseq"]) for h in l) == sorted(tuple(h["yseq"]) for h in first[b])
        by = {tuple(h["yseq"]): h for h in first[b]}
        un = {tuple(h["yseq"]): h for h in plain[b]}
        for h in l:
            y = tuple(h["yseq"])
            assert h["att_score"] > -math.inf
            assert h["score"] == lam * (h["ctc_score"] + h["lm_score"]) + (1.0 - lam) * h["att_score"]
            assert h["ctc_score"] == by[y]["ctc_score"] and h["lm_score"] == by[y]["lm_score"] == ref.lm_score(y)      # ctc_score stays pure
            assert h["att_score"] == un[y]["att_score"] and "lm_score" not in un[y]      # the decoder's score does not depend on the LM
            assert un[y]["score"] == lam * h["ctc_score"] + (1.0 - lam) * h["att_score"]
    assert any(h["lm_score"] != 0.0 for l in got for h in l)
    res = model.transcribe(pack, beam_size=4, joint="ctc_rescore", lm=lm)
    assert all("lm_score" in r for r in res) and [r["ids"] for r in res] == [l[0]["yseq"] for l in model.beam_search(pack, 4, 1, ctc_weight=model.config.ctc_weight, joint="ctc_rescore", lm=lm)]
    assert all("lm_score" not in r for r in model.transcribe(pack, beam_size=4, joint="ctc_rescore"))


def test_searches_without_a_prefix_beam_refuse_an_lm():
    from tests.test_stream_beam_gpu import _rescore_model, _stream_model
    from tests.test_model_gpu import to_pack
    from asr_chinese_e2e_amd.context import ContextGraph
    from asr_chinese_e2e_amd.lm import NgramLM
    _, _, batch, model = _rescore_model("fp32")
    pack = to_pack(batch)
    lm, _ = _model_lm(model.V)
    cg = ContextGraph([[(5, 6)]], device=DEV, vocab_size=model.V)
    streaming = _stream_model("fp32", "TransformerOffical")
    slm, _ = _model_lm(streaming.V)
    with pytest.raises(ValueError, match="prefix_beam"):
        streaming.stream(2, search="greedy", lm=slm)
    with pytest.raises(ValueError, match="prefix_beam"):
        streaming.stream(2, lm=slm)
    with pytest.raises(ValueError, match="prefix_beam"):
        streaming.sessions(2, search="greedy", lm=slm)
    with pytest.raises(ValueError, match="cannot be combined"):
        streaming.stream(2, search="prefix_beam", lm=slm, context=ContextGraph([[(5, 6)]], vocab_size=streaming.V))
    with pytest.raises(ValueError, match="cannot be combined"):
        streaming.sessions(2, search="prefix_beam", lm=slm, context=ContextGraph([[(5, 6)]], vocab_size=streaming.V))
    for kw in (dict(joint="one_pass", ctc_weight=0.3), dict(joint="rescore", ctc_weight=0.3), dict(joint="rescore", ctc_weight=0.0)):
        with pytest.raises(ValueError, match="ctc_rescore"):
            model.beam_search(pack, beam_size=3, lm=lm, **kw)
    with pytest.raises(ValueError, match="ctc_rescore"):
        model.transcribe(pack, beam_size=3, lm=lm)      # the joint model's default search is the attention beam's
    with pytest.raises(ValueError, match="cannot be combined"):
        model.ctc_prefix_beam_search(pack, 3, 1, lm=lm, context=cg)
    with pytest.raises(ValueError, match="cannot be combined"):
        model.beam_search(pack, beam_size=3, joint="ctc_rescore", lm=lm, context=cg)
    with pytest.raises(ValueError, match="the model has"):
        model.ctc_prefix_beam_search(pack, 3, 1, lm=NgramLM({(4,): (-1.0, None)}, 1, model.V + 1))      # another vocabulary
    with pytest.raises(TypeError):
        model.ctc_prefix_beam_search(pack, 3, 1, lm={(4,): (-1.0, None)})


def test_transcribe_cli_lm(tmp_path, capsys):
    """transcribe.py --lm offline and with --stream=1 (--sessions=2 included), in this process (transcribe.transcribe is the script's
    body): the final lines carry "lm_score", and a malformed file, --context beside it or a search without a prefix beam ends the run."""
    import json
    import sys
    import numpy as np
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
    tok = vocab._id2token
    uni = ["-1.0\t<s>\t-0.4", "-1.3\t</s>"] + [f"{-1.0 - 0.01 * i:.2f}\t{tok[i]}\t-0.2" for i in range(4, 40)] + ["-2.0\tq"]
    bi = [f"{-0.3 - 0.01 * i:.2f}\t{tok[i]} {tok[i + 1]}" for i in range(4, 39)] + [f"-0.5\t<s> {tok[4]}"]
    arpa = tmp_path / "lm.arpa"
    arpa.write_text("\\data\\\nngram 1=%d\nngram 2=%d\n\n\\1-grams:\n%s\n\n\\2-grams:\n%s\n\n\\end\\\n" % (len(uni), len(bi), "\n".join(uni), "\n".join(bi)),
                    encoding="utf-8")
    argv = [f"--{k}={v}" for k, v in flags.items()] + [f"--ckpt={tmp_path / 'm.model'}", f"--vocab_path={tmp_path / 'vocab.t'}",
                                                       "--wavs=" + ",".join(map(str, wavs)), "--beam_size=3", f"--cmvn={tmp_path / 'cmvn.npz'}"]
    lmf = [f"--lm={arpa}", "--lm_weight=0.4", "--lm_ins=0.5"]
    streamed = ["--stream=1", "--stream_search=prefix_beam", "--frame_topk=5"]
    capsys.readouterr()
    finals = {}
    for name, extra in (("plain", []), ("offline", lmf), ("stream", lmf + streamed), ("sessions", lmf + streamed + ["--sessions=2"])):
        T_.transcribe(**parse_flags(argv + extra))
        lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        finals[name] = {l["file"]: l for l in lines if "ids" in l and "file" in l and "duration_s" in l}
        assert sorted(finals[name]) == sorted(map(str, wavs)), name
    assert all("lm_score" not in l for l in finals["plain"].values())
    from asr_chinese_e2e_amd.lm import NgramLM
    lm = NgramLM.from_arpa(str(arpa), vocab, weight=0.4, ins=0.5)
    assert lm.dropped == 1
    for name in ("offline", "stream", "sessions"):
        for l in finals[name].values():
            assert isinstance(l["lm_score"], float) and l["lm_score"] == lm.score(l["ids"]), (name, l)
        assert any(l["ids"] for l in finals[name].values()), name
    with pytest.raises(SystemExit, match="prefix_beam"):
        T_.transcribe(**parse_flags(argv + lmf + ["--stream=1"]))      # the greedy stream has no beam to fuse the LM into
    hot = tmp_path / "hot.txt"
    hot.write_text(tok[4] + "\n", encoding="utf-8")
    with pytest.raises(SystemExit, match="cannot be combined"):
        T_.transcribe(**parse_flags(argv + lmf + [f"--context={hot}"]))
    bad = tmp_path / "bad.arpa"
    bad.write_text(arpa.read_text(encoding="utf-8").replace("\\end\\\n", ""), encoding="utf-8")
    with pytest.raises(SystemExit, match="end"):
        T_.transcribe(**parse_flags(argv + [f"--lm={bad}"]))
