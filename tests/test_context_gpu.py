"""Hotword biasing on the GPU: asr_ctc_prefix_beam_ctx against the fp64 definition (tests/context_ref.py), the unbiased cases against
asr_ctc_prefix_beam bit for bit, the resumable kernel against the offline one under every cutting, the reset, and the model level
(model.stream, model.sessions, ctc_rescore, the refusals, transcribe.py --context)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import context_ref as CR  # noqa: E402

DEV = "cuda"
B, T, V = 3, 48, CR.V
LENS = [T, 29, 41]      # ragged, the first is full; 29 and 41 end inside a chunk of 16 and of 5
GRAPH_OF = [0, 1, -1]   # utterance 0: graph 0, utterance 1: graph 1, utterance 2: not biased
SEED = 4                # chosen on the CPU: the reference's smallest ranking gap over all cases below is 1.7e-5 (asserted > 1e-9)
SHAPES = [(5, 4), (5, 10), (3, 16)]      # (k, beam)
PEAKS = [3.0, 0.3]


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


_CG, _CAND = {}, {}


def _cg(w=3.0):
    from asr_chinese_e2e_amd.context import ContextGraph
    if w not in _CG:
        _CG[w] = ContextGraph(CR.GRAPHS, score=w, device=DEV, vocab_size=V)
    return _CG[w]


def _roots(cg):
    return cg.roots(GRAPH_OF, B)


def _cand(K, k, peak):
    """One random lattice (the generator of test_ctc_prefix_beam_kernel_matches_host_restatement) and its per-frame candidates."""
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
    from asr_chinese_e2e_amd.decode import context_entries
    cg = _cg()
    logits, vals, ids, blank_lp = _cand(K, k, peak)
    res = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0, context=cg, roots=_roots(cg))
    tok, ln, sc, bias, state = (x.cpu().tolist() for x in res)
    logp = torch.log_softmax(logits.double(), -1).numpy()
    ids_h = ids.view(B, T, k).cpu().numpy()
    active = 0
    for b in range(B):
        trie = CR.Trie(CR.GRAPHS[GRAPH_OF[b]], 3.0) if GRAPH_OF[b] >= 0 else None
        want, gap = CR.ctc_prefix_beam_search(logp[b, :LENS[b]], beam, candidates=[list(ids_h[b, t]) for t in range(LENS[b])], trie=trie)
        print(f"k={k} beam={beam} peak={peak} b={b}: smallest ranking gap of the reference {gap:.3e}")
        assert gap > 1e-9, (b, gap)      # a failure below is the kernel's, not a near tie
        want = [h for h in want if h[2] > -1e300]
        got = context_entries(cg, tok[b], ln[b], sc[b], bias[b], state[b])
        assert [tuple(h["yseq"]) for h in got] == [h[0] for h in want], (b, got, want)
        for h, (_, w_sc, w_ctc, w_bias) in zip(got, want):
            assert abs(h["ctc_score"] - w_ctc) < 1e-5 * max(1.0, abs(w_ctc)), (b, h, w_ctc)
            assert h["bias"] == w_bias, (b, h, w_bias)      # exactly: the same fp64 additions
            assert h["score"] == h["ctc_score"] + h["bias"]
            active += h["bias"] != 0.0
        if GRAPH_OF[b] < 0:
            assert all(h["bias"] == 0.0 for h in got) and all(s == -1 for s in state[b])
    assert active > 0      # the graphs bite on this lattice


@pytest.mark.parametrize("peak", PEAKS, ids=["peaky", "flat"])
@pytest.mark.parametrize("k,beam", SHAPES)
def test_unbiased_utterance_and_w_zero_have_the_plain_kernels_bits(K, k, beam, peak):
    _, vals, ids, blank_lp = _cand(K, k, peak)
    wt, wl, ws = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0)
    cg = _cg()
    tok, ln, sc, bias, state = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0, context=cg, roots=_roots(cg))
    assert torch.equal(tok[2], wt[2]) and torch.equal(ln[2], wl[2]) and torch.equal(sc[2], ws[2])
    assert (bias[2] == 0.0).all() and (state[2] == -1).all()
    assert not (torch.equal(tok[0], wt[0]) and torch.equal(tok[1], wt[1]))      # the biased ones differ from the plain search here
    z = _cg(0.0)
    tok, ln, sc, bias, state = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0, context=z, roots=_roots(z))
    assert torch.equal(tok, wt) and torch.equal(ln, wl) and torch.equal(sc, ws)
    assert (bias == 0.0).all() and not torch.signbit(bias).any()
    # every root -1: the plain search for all
    tok, ln, sc, bias, state = K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, beam, beam, 0, context=cg, roots=[-1] * B)
    assert torch.equal(tok, wt) and torch.equal(ln, wl) and torch.equal(sc, ws) and (state == -1).all()


def test_wrappers_refuse_what_they_can_check(K):
    from asr_chinese_e2e_amd._lib import AsrHipError
    cg = _cg()
    _, vals, ids, blank_lp = _cand(K, 5, 3.0)
    with pytest.raises(ValueError, match="roots"):
        K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, 4, 4, 0, context=cg, roots=[0, cg.S, -1])
    with pytest.raises(ValueError, match="roots"):
        K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, 4, 4, 0, context=cg, roots=[0, 0])
    with pytest.raises(AsrHipError):      # 12 * 6 > 64 slots
        K.ctc_prefix_beam(vals, ids, blank_lp, _len(), B, T, 12, 12, 0, context=cg, roots=_roots(cg))
    st = K.ctc_prefix_beam_state(B, 4, T, DEV)
    with pytest.raises(ValueError, match="context state"):
        K.ctc_prefix_beam_state_reset(st, torch.zeros(B, dtype=torch.int32, device=DEV), roots=[0, 0, 0])


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
    cg = _cg()
    roots = _roots(cg)
    _, vals, ids, blank_lp = _cand(K, k, peak)
    ref = {}
    for t in range(1, T + 1):      # the offline kernel on the first t frames, once
        ref[t] = K.ctc_prefix_beam(vals, ids, blank_lp, _len([min(l, t) for l in LENS]), B, T, beam, beam, 0, context=cg, roots=roots)
    for name, chunks in _cuttings().items():
        st = K.ctc_prefix_beam_state(B, beam, T, DEV, context=cg, roots=roots)
        assert st.state.numel() * 8 == K.lib.asr_ctc_prefix_beam_ctx_state_bytes(B, beam)
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
                assert bias[:, 0].tolist() == [0.0] * B and state[:, 0].tolist() == roots
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


def test_context_state_reset_takes_the_new_root_and_touches_only_the_flagged_slot(K):
    C, beam, k, T_cap = 8, 4, 5, 64
    cg = _cg()
    r0, r1 = cg.root_of_graph
    g = torch.Generator().manual_seed(21)
    chunks = [torch.randn(B * C, V, generator=g).to(DEV) * 2 for _ in range(6)]
    st = K.ctc_prefix_beam_state(B, beam, T_cap, DEV, context=cg, roots=[r0, r1, -1])
    for x in chunks[:3]:
        K.ctc_prefix_beam_chunk(st, *K.ctc_frame_topk(x, k, 0), [C, C - 3, C], C, beam)
    state0, ws0 = st.state.clone(), st.ws.clone()
    flags = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    K.ctc_prefix_beam_state_reset(st, flags, [1], roots=[r1, r0, r0])      # only slot 1's new root counts: graph 0 instead of graph 1
    per = st.state.numel() // B
    nodes, nodes0 = st.ws.view(torch.int32).view(B, -1), ws0.view(torch.int32).view(B, -1)
    for b in (0, 2):
        assert torch.equal(st.state.view(B, per)[b], state0.view(B, per)[b]) and torch.equal(nodes[b], nodes0[b])
    fresh = K.ctc_prefix_beam_state(B, beam, T_cap, DEV, context=cg, roots=[r0, r0, -1])
    assert torch.equal(st.state.view(B, per)[1], fresh.state.view(B, per)[1])      # byte for byte a fresh state with that root
    other = K.ctc_prefix_beam_state(B, beam, T_cap, DEV, context=cg, roots=[r0, r1, -1])
    assert not torch.equal(st.state.view(B, per)[1], other.state.view(B, per)[1])      # and the root is part of it
    assert st.frames == [3 * C, 0, 3 * C] and st.roots == [r0, r0, -1]
    for x in chunks[3:]:
        cand = K.ctc_frame_topk(x, k, 0)
        a = K.ctc_prefix_beam_chunk(st, *cand, [C, C, 0], C, beam, max_len=T_cap)
        f = K.ctc_prefix_beam_chunk(fresh, *cand, [0, C, 0], C, beam, max_len=T_cap)
        assert all(torch.equal(x_[1], y_[1]) for x_, y_ in zip(a, f))
    assert int(a[1][1, 0]) > 0 and float(a[4][1].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------ the model level
MODEL_GRAPHS = [[(t,) for t in range(4, 17, 2)] + [(5, 7), (9, 11, 13)], [(t,) for t in range(17, 30, 2)] + [(18, 20)]]      # over V = 30


def _model_cg(w=3.0):
    from asr_chinese_e2e_amd.context import ContextGraph
    return ContextGraph(MODEL_GRAPHS, score=w, device=DEV, vocab_size=30)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stream_with_context_matches_the_offline_search_on_the_streamed_frames(K, monkeypatch, dtype):
    from asr_chinese_e2e_amd.decode import context_entries
    from tests.test_stream_beam_gpu import _stream_model
    C, Bm, beam, topk, Tm = 4, 3, 4, 5, 20
    lens = [19, 14, 6]
    graphs = [0, 1, -1]
    cg = _model_cg()
    model = _stream_model(dtype, "TransformerOffical", C)
    torch.manual_seed(7)
    feats = torch.randn(Bm, Tm, 16, device=DEV).to(torch.float32 if dtype == "fp32" else torch.bfloat16)
    fed = []
    real = K.ctc_frame_topk

    def recording(logits, k, blank=0):
        out = real(logits, k, blank)
        fed.append(tuple(t.clone() for t in out))
        return out
    monkeypatch.setattr(K, "ctc_frame_topk", recording)
    st = model.stream(Bm, search="prefix_beam", beam_size=beam, frame_topk=topk, context=cg, context_ids=graphs)
    assert st.nbest() == [[{"yseq": [], "score": 0.0, "ctc_score": 0.0, "bias": 0.0}]] * Bm
    said = [[] for _ in range(Bm)]
    for c0 in range(0, Tm, C):
        nv = [max(0, min(C, l - c0)) for l in lens]
        for b, ids in enumerate(st.push(feats[:, c0:c0 + C].contiguous(), nv)):
            said[b] += ids
        part, nb = st.partial(), st.nbest()
        for b in range(Bm):      # what push handed out is the stable part of every revisable hypothesis, whatever the order by score
            assert part[b]["stable_len"] == len(said[b]) and all(h["yseq"][:len(said[b])] == said[b] for h in nb[b]), (c0, b)
            assert part[b]["ids"] == nb[b][0]["yseq"] and part[b]["score"] == nb[b][0]["score"] and part[b]["bias"] == nb[b][0]["bias"]
            assert [h["score"] for h in nb[b]] == sorted((h["score"] for h in nb[b]), reverse=True)
    monkeypatch.setattr(K, "ctc_frame_topk", real)
    vals, ids, blank_lp = (torch.cat([f[i].view(Bm, C, -1) for f in fed], dim=1) for i in range(3))
    res = K.ctc_prefix_beam(vals.reshape(Bm * Tm, topk).contiguous(), ids.reshape(Bm * Tm, topk).contiguous(), blank_lp.reshape(Bm * Tm).contiguous(),
                            _len(lens), Bm, Tm, beam, beam, 0, context=cg, roots=cg.roots(graphs, Bm))
    tok, ln, sc, bias, state = (x.cpu().tolist() for x in res)
    want = [context_entries(cg, tok[b], ln[b], sc[b], bias[b], state[b]) for b in range(Bm)]
    assert st.nbest() == want
    assert any(h["bias"] != 0.0 for b in (0, 1) for h in want[b]) and all(h["bias"] == 0.0 for h in want[2])
    # the model's own offline search under the same chunk mask sees the same frames: the same lists
    from asr_chinese_e2e_amd.Utils import Pack
    enc, enc_len = st.encoder_output()
    with model.given_encoder_output(enc):
        off = model.ctc_prefix_beam_search(Pack(wave=feats, wave_len=enc_len), beam, beam, topk, context=cg, context_ids=graphs)
        host = model.ctc_prefix_beam_search(Pack(wave=feats, wave_len=enc_len), beam, beam, topk, on_device=False, context=cg, context_ids=graphs)
    assert off == want
    for b in range(Bm):      # the host loop applies the same definition through ContextGraph.walk
        assert [h["yseq"] for h in host[b]] == [h["yseq"] for h in want[b]] and [h["bias"] for h in host[b]] == [h["bias"] for h in want[b]]
        assert all(abs(h["ctc_score"] - w["ctc_score"]) < 1e-5 * max(1.0, abs(w["ctc_score"])) for h, w in zip(host[b], want[b]))
    fin = st.finish(joint="ctc_rescore")
    for b in range(Bm):
        assert fin[b]["ids"][:len(said[b])] == said[b] and fin[b]["ids"] in [h["yseq"] for h in want[b]]
        assert fin[b]["bias"] == next(h["bias"] for h in want[b] if h["yseq"] == fin[b]["ids"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_session_reopened_with_another_graph_equals_a_fresh_stream_with_it(dtype):
    from tests.test_sessions_gpu import _chunk_of, _feats, _model
    C = 8
    model = _model(dtype, -1, C=C)
    cg = _model_cg()
    first, second, other = _feats([20, 27, 13], dtype, seed=5)

    def alone(u, graph):
        st = model.stream(1, search="prefix_beam", beam_size=4, frame_topk=6, context=cg, context_ids=[graph])
        outs = []
        for c0 in range(0, u.shape[0], C):
            x, nv = _chunk_of([u], [c0], C)
            outs.append((st.push(x, nv)[0], st.nbest()[0]))
        return outs
    ss = model.sessions(2, search="prefix_beam", beam_size=4, frame_topk=6, context=cg)
    with pytest.raises(ValueError, match="graph 2 of 2"):
        ss.open(0, context=2)
    ss.open(0)                  # graph 0 by default
    ss.open(1, context=-1)      # the neighbour is not biased
    for (utt, graph) in ((first, 0), (second, 1)):      # slot 0: a session with graph 0, then reopened with graph 1
        want = alone(utt, graph)
        for i, c0 in enumerate(range(0, utt.shape[0], C)):
            x, nv = _chunk_of([utt, other if graph == 0 else None], [c0, c0], C)
            fin = [c0 + C >= utt.shape[0], nv[1] > 0 and c0 + C >= other.shape[0]]
            got = ss.push(x, nv, fin)
            assert got[0] == want[i][0] and ss.nbest(0) == want[i][1], (graph, i)
            if graph == 0 and nv[1] > 0:
                assert all(h["bias"] == 0.0 for h in ss.nbest(1))
        assert any(h["bias"] != 0.0 for h in ss.nbest(0))
        res = ss.finish(0, joint="ctc_rescore")
        assert "bias" in res
        if graph == 0:
            ss.open(0, context=1)
    assert want[-1][1] != alone(second, 0)[-1][1]      # the graph matters for this utterance


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ctc_rescore_with_context_combines_the_bias_with_the_ctc_score(dtype):
    from tests.test_stream_beam_gpu import _rescore_model
    from tests.test_model_gpu import to_pack
    lam = 0.4
    _, _, batch, model = _rescore_model(dtype, lam)
    pack = to_pack(batch)
    from asr_chinese_e2e_amd.context import ContextGraph
    cg = ContextGraph([[(t,) for t in range(4, 14)] + [(5, 6)]], device=DEV, vocab_size=24)
    from asr_chinese_e2e_amd import decode
    got = model.beam_search(pack, beam_size=4, nbest=4, ctc_weight=lam, joint="ctc_rescore", context=cg)
    first = model.ctc_prefix_beam_search(pack, 4, 4, context=cg)
    # the unbiased call for the same hypotheses: the same list without "bias", scored by the same decoder pass
    eng = model._ensure_engine(DEV)
    was, eng.training = eng.training, False
    with torch.no_grad():
        enc = model.forward(pack).encoder_out
    eng.training = was
    plain = decode.attention_rescore(model, enc, pack.wave_len, [[{"yseq": h["yseq"], "score": h["ctc_score"]} for h in l] for l in first], lam)
    for b, l in enumerate(got):
        assert set(l[0]) == {"yseq", "score", "att_score", "ctc_score", "bias"}
        assert [h["score"] for h in l] == sorted((h["score"] for h in l), reverse=True)
        assert sorted(tuple(h["yseq"]) for h in l) == sorted(tuple(h["yseq"]) for h in first[b])
        by = {tuple(h["yseq"]): h for h in first[b]}
        un = {tuple(h["yseq"]): h for h in plain[b]}
        for h in l:
            y = tuple(h["yseq"])
            assert h["att_score"] > -math.inf
            assert h["score"] == lam * (h["ctc_score"] + h["bias"]) + (1.0 - lam) * h["att_score"]
            assert h["ctc_score"] == by[y]["ctc_score"] and h["bias"] == by[y]["bias"]      # ctc_score stays pure
            assert h["att_score"] == un[y]["att_score"] and "bias" not in un[y]      # the decoder's score does not depend on the biasing
            assert un[y]["score"] == lam * h["ctc_score"] + (1.0 - lam) * h["att_score"]
    assert any(h["bias"] != 0.0 for l in got for h in l)
    res = model.transcribe(pack, beam_size=4, joint="ctc_rescore", context=cg)
    assert all("bias" in r for r in res) and [r["ids"] for r in res] == [l[0]["yseq"] for l in model.beam_search(pack, 4, 1, ctc_weight=model.config.ctc_weight, joint="ctc_rescore", context=cg)]
    assert all("bias" not in r for r in model.transcribe(pack, beam_size=4, joint="ctc_rescore"))


def test_searches_without_a_prefix_beam_refuse_a_context():
    from tests.test_stream_beam_gpu import _rescore_model
    from tests.test_model_gpu import to_pack
    from asr_chinese_e2e_amd.context import ContextGraph
    _, _, batch, model = _rescore_model("fp32")
    pack = to_pack(batch)
    cg = ContextGraph([[(5, 6)]], device=DEV, vocab_size=24)
    from tests.test_stream_beam_gpu import _stream_model
    streaming = _stream_model("fp32", "TransformerOffical")
    with pytest.raises(ValueError, match="prefix_beam"):
        streaming.stream(2, search="greedy", context=cg)
    with pytest.raises(ValueError, match="prefix_beam"):
        streaming.stream(2, context=cg)
    with pytest.raises(ValueError, match="prefix_beam"):
        streaming.sessions(2, search="greedy", context=cg)
    with pytest.raises(ValueError, match="needs model.sessions"):
        streaming.sessions(2, search="prefix_beam").open(0, context=0)
    for kw in (dict(joint="one_pass", ctc_weight=0.3), dict(joint="rescore", ctc_weight=0.3), dict(joint="rescore", ctc_weight=0.0)):
        with pytest.raises(ValueError, match="ctc_rescore"):
            model.beam_search(pack, beam_size=3, context=cg, **kw)
    with pytest.raises(ValueError, match="ctc_rescore"):
        model.transcribe(pack, beam_size=3, context=cg)      # the joint model's default search is the attention beam's
    with pytest.raises(ValueError, match="outside"):
        model.ctc_prefix_beam_search(pack, 3, 1, context=ContextGraph([[(30,)]]))      # a token the model does not have
    with pytest.raises(ValueError, match="needs a context"):
        model.ctc_prefix_beam_search(pack, 3, 1, context_ids=[0, 0, 0])
    with pytest.raises(TypeError):
        model.ctc_prefix_beam_search(pack, 3, 1, context=[[(5, 6)]])


def test_transcribe_cli_context(tmp_path, capsys):
    """transcribe.py --context offline and with --stream=1 --sessions=2 (in this process: transcribe.transcribe is the script's body):
    the final lines carry "bias", and an unknown character or a search without a prefix beam ends the run."""
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
    hot = tmp_path / "hot.txt"
    hot.write_text("\n".join(vocab._id2token[i] for i in range(4, 40, 2)) + "\n\n" + vocab._id2token[5] + vocab._id2token[7] + "\n", encoding="utf-8")
    argv = [f"--{k}={v}" for k, v in flags.items()] + [f"--ckpt={tmp_path / 'm.model'}", f"--vocab_path={tmp_path / 'vocab.t'}",
                                                       "--wavs=" + ",".join(map(str, wavs)), "--beam_size=3", f"--cmvn={tmp_path / 'cmvn.npz'}"]
    ctx = [f"--context={hot}", "--context_score=2.5"]
    capsys.readouterr()
    finals = {}
    for name, extra in (("plain", []), ("offline", ctx), ("sessions", ctx + ["--stream=1", "--stream_search=prefix_beam", "--frame_topk=5", "--sessions=2"])):
        T_.transcribe(**parse_flags(argv + extra))
        lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        finals[name] = {l["file"]: l for l in lines if "ids" in l}
        assert sorted(finals[name]) == sorted(map(str, wavs)), name
    assert all("bias" not in l for l in finals["plain"].values())
    for name in ("offline", "sessions"):
        assert all(isinstance(l["bias"], float) and l["bias"] >= 0.0 and l["bias"] % 2.5 == 0.0 for l in finals[name].values()), name
        assert any(l["bias"] > 0.0 for l in finals[name].values()), name
    with pytest.raises(SystemExit, match="prefix_beam"):
        T_.transcribe(**parse_flags(argv + ctx + ["--stream=1"]))      # the greedy stream has no beam to bias
    bad = tmp_path / "bad.txt"
    bad.write_text(vocab._id2token[4] + "\nq\n", encoding="utf-8")
    with pytest.raises(SystemExit, match="line 2"):
        T_.transcribe(**parse_flags(argv + [f"--context={bad}"]))
