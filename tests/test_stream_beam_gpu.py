"""The resumable CTC prefix beam search (asr_ctc_prefix_beam_chunk), model.stream(search="prefix_beam") on top of it, and the second
pass (decode.attention_rescore, joint="ctc_rescore").

The chunk kernel's oracle is exact: the offline kernel asr_ctc_prefix_beam on the frames consumed so far - tokens, lengths and scores
must be equal (==) under every cutting of the frames, because both run one frame-step body.  The offline kernel in turn is pinned to the
fp64 host restatement (oracle/decode_ref.py) by tests/test_kernels_gpu.py; the final lists are checked against it here as well."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import decode_ref as D  # noqa: E402
from oracle import ref_model as R  # noqa: E402
from tests.test_model_gpu import build, oracle_case, to_pack  # noqa: E402

DEV = "cuda"
SOS, EOS = 2, 3
B, T, V = 3, 37, 12
LENS = [T, 23, 30]      # ragged: the first is full; 23 ends inside a chunk of 16 and of 5, 30 inside one of 16


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


# ------------------------------------------------------------------------------------------------------------ the kernel
_LATTICE = {}


def _lattice(K, beam, k, peak):
    """The candidates of one random lattice (the generator of test_ctc_prefix_beam_kernel_matches_host_restatement) and, computed once,
    the offline kernel's full beam after t = 0 .. T frames: ref[t] = (tokens, lengths, scores) with every utterance cut at min(len, t)."""
    key = (beam, k, peak)
    if key not in _LATTICE:
        g = torch.Generator().manual_seed(B * 1000 + T)
        logits = torch.randn(B, T, V, generator=g) * peak
        vals, ids, blank_lp = K.ctc_frame_topk(logits.reshape(B * T, V).to(DEV), k, 0)
        ref = {}
        for t in range(1, T + 1):
            cut = torch.tensor([min(l, t) for l in LENS], dtype=torch.int32, device=DEV)
            ref[t] = K.ctc_prefix_beam(vals, ids, blank_lp, cut, B, T, beam, beam, 0)
        _LATTICE[key] = (logits, vals.view(B, T, k), ids.view(B, T, k), blank_lp.view(B, T), ref)
    return _LATTICE[key]


def _cuttings():
    """name -> list of (C, c0 or None): the chunk covers frames [c0, c0 + C) of every utterance (lock-step), None = a chunk that
    consumes nothing."""
    by16 = [(16, c0) for c0 in range(0, T, 16)]
    by5 = [(5, c0) for c0 in range(0, T, 5)]
    gaps = []
    for ch in by5:
        gaps += [ch, (5, None)]
    return {"whole": [(T, 0)], "frames": [(1, t) for t in range(T)], "C16": by16, "C5": by5, "C5_gaps": [(5, None)] + gaps}


def _rows(x, c0, C):
    """Rows [c0, c0 + C) of every utterance as the chunk's (B * C, ...) block (zero rows past T: the kernel never reads them)."""
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


def _stable_of(tok, ln):
    """The longest common prefix of the entries with len >= 0 of a full beam (nbest = beam), per utterance."""
    tok, ln = tok.cpu().tolist(), ln.cpu().tolist()
    return [_lcp([tok[b][r][:ln[b][r]] for r in range(len(ln[b])) if ln[b][r] >= 0]) for b in range(len(ln))]


@pytest.mark.parametrize("peak", [3.0, 0.3], ids=["peaky", "flat"])
@pytest.mark.parametrize("beam,k", [(1, 5), (4, 5), (10, 5), (16, 3)])
def test_chunk_kernel_equals_offline_kernel_under_every_cutting(K, beam, k, peak):
    logits, vals, ids, blank_lp, ref = _lattice(K, beam, k, peak)
    for name, chunks in _cuttings().items():
        st = K.ctc_prefix_beam_state(B, beam, T, DEV)
        done, last_stable = 0, [0] * B
        for C, c0 in chunks:
            nv = [0] * B if c0 is None else [max(0, min(C, l - c0)) for l in LENS]
            c0 = 0 if c0 is None else c0
            before = (st.state.clone(), st.ws.clone()) if not any(nv) else None
            tok, ln, sc, stable = K.ctc_prefix_beam_chunk(st, _rows(vals, c0, C), _rows(ids, c0, C), _rows(blank_lp, c0, C), nv, C, beam, 0,
                                                          max_len=T)
            if before is not None:      # a chunk that consumes nothing changes no byte of the state (nor of the trie)
                assert torch.equal(st.state, before[0]) and torch.equal(st.ws, before[1]), name
            done = max(done, c0 + max(nv)) if any(nv) else done
            if done == 0:               # nothing consumed yet: the empty prefix alone, probability one
                assert ln[:, 0].tolist() == [0] * B and sc[:, 0].tolist() == [0.0] * B and stable.tolist() == [0] * B
                assert beam == 1 or (ln[:, 1:] == -1).all()
                continue
            wt, wl, ws_ = ref[done]     # the offline kernel on the frames consumed so far: equal, not close
            assert torch.equal(ln, wl), (name, done, ln, wl)
            assert torch.equal(tok, wt), (name, done)
            assert torch.equal(sc, ws_), (name, done, sc, ws_)
            want_stable = _stable_of(wt, wl)
            got_stable = stable.tolist()
            assert got_stable == want_stable, (name, done, got_stable, want_stable)
            assert all(g >= p for g, p in zip(got_stable, last_stable)), (name, done, got_stable, last_stable)      # never retracted
            if beam == 1:
                assert got_stable == ln[:, 0].tolist()
            last_stable = got_stable
        assert done == T and st.frames == LENS, name
    # the final lists against the fp64 host restatement, the gate of test_ctc_prefix_beam_kernel_matches_host_restatement
    tok, ln, sc = (x.cpu() for x in (tok, ln, sc))
    logp = torch.log_softmax(logits.double(), -1).numpy()
    ids_h = ids.cpu().numpy()
    for b in range(B):
        want = D.ctc_prefix_beam_search(logp[b, :LENS[b]], beam, candidates=[list(ids_h[b, t]) for t in range(LENS[b])])[:beam]
        want = [(p, s_) for p, s_ in want if s_ > -1e300]
        got = [(tuple(tok[b, r, : int(ln[b, r])].tolist()), float(sc[b, r])) for r in range(beam) if int(ln[b, r]) >= 0]
        assert [p for p, _ in got] == [p for p, _ in want], (b, got, want)
        for (_, a), (_, w) in zip(got, want):
            assert abs(a - w) < 1e-5 * max(1.0, abs(w)), (a, w)


def test_chunk_past_the_trie_capacity_raises_before_any_launch(K):
    """T_cap = 8 frames: 5 fit, 5 more do not - refused in Python, state, trie and frame count untouched - and 3 more still fit."""
    beam, k, C = 4, 5, 5
    _, vals, ids, blank_lp, _ = _lattice(K, beam, k, 3.0)
    st = K.ctc_prefix_beam_state(B, beam, 8, DEV)
    args = lambda c0: (_rows(vals, c0, C), _rows(ids, c0, C), _rows(blank_lp, c0, C))      # noqa: E731
    K.ctc_prefix_beam_chunk(st, *args(0), [5, 5, 5], C, beam, 0)
    before = (st.state.clone(), st.ws.clone())
    with pytest.raises(ValueError, match="trie holds 8"):
        K.ctc_prefix_beam_chunk(st, *args(5), [0, 5, 0], C, beam, 0)
    with pytest.raises(ValueError, match="n_valid"):
        K.ctc_prefix_beam_chunk(st, *args(5), [0, 6, 0], C, beam, 0)
    assert torch.equal(st.state, before[0]) and torch.equal(st.ws, before[1]) and st.frames == [5, 5, 5]
    tok, ln, sc, _ = K.ctc_prefix_beam_chunk(st, *args(5), [3, 3, 0], C, beam, 0, max_len=T)
    assert st.frames == [8, 8, 5]
    cut = torch.tensor([8, 8, 5], dtype=torch.int32, device=DEV)
    wt, wl, ws_ = K.ctc_prefix_beam(vals.reshape(B * T, k), ids.reshape(B * T, k), blank_lp.reshape(B * T), cut, B, T, beam, beam, 0)
    assert torch.equal(tok, wt) and torch.equal(ln, wl) and torch.equal(sc, ws_)
    from asr_chinese_e2e_amd._lib import AsrHipError
    with pytest.raises(AsrHipError):      # 8 * 11 > 64 slots: refused by the library, as the offline entry point refuses it
        K.ctc_prefix_beam_chunk(K.ctc_prefix_beam_state(1, 8, 8, DEV), torch.zeros(4, 10, device=DEV), torch.zeros(4, 10, dtype=torch.int32, device=DEV),
                                torch.zeros(4, device=DEV), [4], 4, 1, 0)


# ------------------------------------------------------------------------------------------------------------ the stream
def _stream_model(dtype, cls_name, C=4):
    """The small streaming models of tests/test_chunk_gpu.py (joint and CTC-only), with sos / eos kept out of the CTC head's reach
    (a trained head never emits them; the decoder's target preparation gives them a meaning of their own)."""
    from tests.test_chunk_gpu import _build, _case
    over = dict(d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, ctc_weight=0.5 if cls_name == "TransformerOffical" else 1.0)
    if cls_name == "TransformerCTC":
        over["use_decoder"] = False
    cfg, sd, _ = _case(1, 8, 16, 30, 4, over, seed=11)
    sd["ctc_lo.bias"] = sd["ctc_lo.bias"].clone()
    sd["ctc_lo.bias"][[SOS, EOS]] = -30.0
    model = _build(cfg, 30, cls_name, dtype=dtype, chunk_size=C, left_chunks=-1, cross_mask="wave_len").cuda().eval()
    model.load_state_dict(sd)
    return model


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("cls_name", ["TransformerOffical", "TransformerCTC"], ids=["joint", "ctc_only"])
def test_stream_prefix_beam_matches_offline_kernel_and_commits_a_prefix(K, monkeypatch, cls_name, dtype):
    C, Bm, beam, topk = 4, 3, 4, 5
    lens = [19, 14, 6]
    Tm = 20
    model = _stream_model(dtype, cls_name, C)
    torch.manual_seed(7)
    feats = torch.randn(Bm, Tm, 16, device=DEV).to(torch.float32 if dtype == "fp32" else torch.bfloat16)
    fed = []
    real = K.ctc_frame_topk

    def recording(logits, k, blank=0):
        out = real(logits, k, blank)
        fed.append(tuple(t.clone() for t in out))
        return out
    monkeypatch.setattr(K, "ctc_frame_topk", recording)
    st = model.stream(Bm, search="prefix_beam", beam_size=beam, frame_topk=topk)
    assert st.nbest() == [[{"yseq": [], "score": 0.0}]] * Bm
    said = [[] for _ in range(Bm)]
    for c0 in range(0, Tm, C):
        nv = [max(0, min(C, l - c0)) for l in lens]
        for b, ids in enumerate(st.push(feats[:, c0:c0 + C].contiguous(), nv)):
            said[b] += ids
        part = st.partial()
        for b in range(Bm):      # what push handed out so far is the stable part of the revisable hypothesis
            assert part[b]["stable_len"] == len(said[b]) and part[b]["ids"][:part[b]["stable_len"]] == said[b], (c0, b, part[b], said[b])
            assert part[b]["ids"] == st.nbest()[b][0]["yseq"] and part[b]["score"] == st.nbest()[b][0]["score"]
    monkeypatch.setattr(K, "ctc_frame_topk", real)
    assert len(fed) == Tm // C
    vals, ids, blank_lp = (torch.cat([f[i].view(Bm, C, -1) for f in fed], dim=1) for i in range(3))
    tok, ln, sc = K.ctc_prefix_beam(vals.reshape(Bm * Tm, topk).contiguous(), ids.reshape(Bm * Tm, topk).contiguous(), blank_lp.reshape(Bm * Tm).contiguous(),
                                    torch.tensor(lens, dtype=torch.int32, device=DEV), Bm, Tm, beam, beam, 0)
    tok, ln, sc = tok.cpu().tolist(), ln.cpu().tolist(), sc.cpu().tolist()
    want = [[{"yseq": tok[b][r][:ln[b][r]], "score": sc[b][r]} for r in range(beam) if ln[b][r] >= 0] for b in range(Bm)]
    assert st.nbest() == want
    assert any(len(s) > 0 for s in said)      # something was committed before the end
    nbest = st.nbest()
    fin = st.finish(joint="ctc_rescore")
    from asr_chinese_e2e_amd.Utils import Pack
    pack = Pack(wave=feats, wave_len=torch.tensor(lens, dtype=torch.int32, device=DEV))
    assert [set(f) for f in fin] == [set(w) for w in model.transcribe(pack, beam_size=2)]
    for b in range(Bm):
        assert fin[b]["ids"][:len(said[b])] == said[b], (b, fin[b]["ids"], said[b])
        assert fin[b]["ids"] in [h["yseq"] for h in nbest[b]]
        assert len(fin[b]["tokens"]) == len(fin[b]["ids"])
        # a hypothesis of the CTC search has non-zero CTC probability on these frames: it is alignable, so every token carries times
        assert all(t["start_frame"] is not None and t["end_s"] is not None for t in fin[b]["tokens"]), (b, fin[b])
        if cls_name == "TransformerCTC":      # no decoder: the CTC best, not rescored
            assert fin[b]["ids"] == nbest[b][0]["yseq"] and fin[b]["score"] == nbest[b][0]["score"]
    assert st.finish(joint="ctc_rescore", timestamps=False)[0]["tokens"] is None
    # the greedy stream is what it was: lists of ids per push; it has no n-best to rescore
    gr = model.stream(Bm)
    out = gr.push(feats[:, :C].contiguous(), [C] * Bm)
    assert len(out) == Bm and all(isinstance(o, list) for o in out)
    with pytest.raises(ValueError, match="prefix_beam"):
        gr.finish(joint="ctc_rescore")
    with pytest.raises(ValueError, match="prefix_beam"):
        gr.nbest()
    with pytest.raises(ValueError):
        model.stream(Bm, search="viterbi")
    with pytest.raises(ValueError, match="64"):
        model.stream(Bm, search="prefix_beam", beam_size=8, frame_topk=10)


# ------------------------------------------------------------------------------------------------------------ the second pass
def _rescore_model(dtype, lam=0.4):
    over = dict(d_model=64, hidden_size=64 if dtype == "bf16" else 16, num_head=2 if dtype == "bf16" else 4, ff_size=128, layer_num=2,
                ctc_weight=lam)
    cfg, sd, batch = oracle_case(3, 18, 16, 24, 5, over, seed=9)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 3.0      # a decoder with opinions
    if "decoder.tgt_word_prj.weight" in sd:
        sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    sd["ctc_lo.weight"] = sd["ctc_lo.weight"] * 4.0
    sd["ctc_lo.bias"] = sd["ctc_lo.bias"].clone()
    sd["ctc_lo.bias"][[SOS, EOS]] = -30.0      # as a trained CTC head: sos / eos are never spelled
    model = build(cfg, 24, dtype=dtype, cross_mask="wave_len").cuda()
    model.load_state_dict(sd)
    model.eval()
    return cfg, sd, batch, model


def _close(a, b, tol):
    if a == -math.inf or b == -math.inf:
        return a == b
    return abs(a - b) <= tol * max(1.0, abs(b))


def _forced_att_scores(model, pack, hyps):
    """sum_i log p(target_i | sos, y_<i) through the searches' own step decoder (_DecoderSteps, beam 1), forced along the tokens of
    hyps[b] (one hypothesis per utterance), target = y + [eos].  Same model, same encoder."""
    from asr_chinese_e2e_amd import decode
    eng = model._ensure_engine(pack.wave.device)
    Bm = len(hyps)
    Lmax = max(len(y) for y in hyps) + 1
    was, eng.training = eng.training, False
    try:
        with torch.no_grad():
            dec = decode._DecoderSteps(model, eng, pack, 1, Lmax)
            tot = [0.0] * Bm
            for i in range(Lmax):
                last = torch.tensor([[([SOS] + y + [EOS] * Lmax)[i]] for y in hyps], dtype=torch.int32, device=DEV)
                lp = torch.log_softmax(dec.logits(i, last).double(), -1).cpu()
                for b, y in enumerate(hyps):
                    if i <= len(y):
                        tot[b] += float(lp[b, (y + [EOS])[i]])
    finally:
        eng.training = was
    return tot


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ctc_rescore_scores_are_consistent_and_match_the_step_decoder(dtype):
    """beam_search(joint="ctc_rescore"): ctc_score = the prefix beam search's score of that hypothesis, att_score = the step decoder
    forced along it (1e-4 in fp32, 0.3 in bf16, relative to max(1, |score|): the form and the figures of the rescoring and beam-search
    tests of tests/test_model_gpu.py) and, in fp32, the oracle decoder's teacher-forced log-probabilities (1e-4); score = the stated mix,
    the list sorted by it."""
    lam, beam = 0.4, 4
    cfg, sd, batch, model = _rescore_model(dtype, lam)
    pack = to_pack({k: batch[k] for k in ("wave", "wave_len")} | {"tgt_for_input": batch["tgt_for_input"]})
    got = model.beam_search(pack, beam, beam, ctc_weight=lam, joint="ctc_rescore")
    ctc = model.ctc_prefix_beam_search(pack, beam, beam)
    tol = 1e-4 if dtype == "fp32" else 0.3
    enc_ref = R.encoder_forward(sd, cfg, batch["wave"], batch["wave_len"]) if dtype == "fp32" else None
    assert all(len(g) == len(c) > 1 for g, c in zip(got, ctc))
    for r in range(beam):      # the r-th hypothesis of every utterance in one forced run
        hyps = [g[min(r, len(g) - 1)]["yseq"] for g in got]
        forced = _forced_att_scores(model, pack, hyps)
        for b, g in enumerate(got):
            h = g[min(r, len(g) - 1)]
            assert _close(h["att_score"], forced[b], tol), (b, r, h, forced[b])
    for b, g in enumerate(got):
        assert {tuple(h["yseq"]): h["ctc_score"] for h in g} == {tuple(h["yseq"]): h["score"] for h in ctc[b]}
        assert all(SOS not in h["yseq"] and EOS not in h["yseq"] and 0 not in h["yseq"] for h in g)
        for h in g:
            assert abs(h["score"] - (lam * h["ctc_score"] + (1 - lam) * h["att_score"])) <= 1e-6 * max(1.0, abs(h["score"]))
        assert all(g[i]["score"] >= g[i + 1]["score"] for i in range(len(g) - 1))
        if enc_ref is not None:
            Tb = int(batch["wave_len"][b])
            for h in g:
                pred, ys_out = R.decoder_forward(sd, cfg, torch.tensor([h["yseq"]], dtype=torch.long).reshape(1, -1), enc_ref[b:b + 1, :Tb],
                                                 torch.tensor([Tb]))
                lp = torch.log_softmax(pred.double(), -1)[0]
                want = float(sum(lp[i, int(ys_out[0, i])] for i in range(len(h["yseq"]) + 1)))
                assert _close(h["att_score"], want, 1e-4), (b, h, want)
    # nbest cuts the re-ranked list; transcribe returns its head without sos / eos handling
    top = model.beam_search(pack, beam, 1, ctc_weight=lam, joint="ctc_rescore")
    assert [t[0] for t in top] == [g[0] for g in got]
    tr = model.transcribe(pack, beam_size=beam, ctc_weight=lam, joint="ctc_rescore")
    assert [t["ids"] for t in tr] == [g[0]["yseq"] for g in got] and all(t["tokens"] is not None for t in tr)


def test_attention_rescore_reorders_and_handles_the_edges():
    """A decoder whose preference differs from the CTC ranking: with the cross-attention output projection zeroed (the audio-blinded
    decoder of tests/test_joint_one_pass_gpu.py) and a tiny tied embedding, every token costs about log V, so the decoder prefers the
    shorter hypothesis whatever CTC says.  ctc_weight near 1 keeps the CTC order, near 0 the second CTC hypothesis wins.  Also: missing
    ranks, the empty hypothesis (log p(eos | sos)), a hypothesis longer than the positional table, a model without a decoder."""
    from asr_chinese_e2e_amd import decode
    cfg, sd, batch, model = _rescore_model("fp32")
    sd = {k: (torch.zeros_like(v) if ".enc_attn.fc." in k else v) for k, v in model.state_dict().items()}
    for k in ("decoder.tgt_word_emb.weight", "decoder.tgt_word_prj.weight"):
        if k in sd:
            sd[k] = sd[k] * 1e-3
    model.load_state_dict(sd)
    pack = to_pack({k: batch[k] for k in ("wave", "wave_len")} | {"tgt_for_input": batch["tgt_for_input"]})
    with torch.no_grad():
        enc = model.forward(pack).encoder_out
    eng = model._engine
    long_hyp = [5] * eng.pe.shape[0]
    lists = [[{"yseq": [5, 6, 7], "score": -1.0}, {"yseq": [5, 6], "score": -2.0}, {"yseq": long_hyp, "score": -2.5}],
             [{"yseq": [], "score": -0.5}],
             []]
    logV = math.log(24)
    keep = decode.attention_rescore(model, enc, pack.wave_len, lists, 0.999)
    flip = decode.attention_rescore(model, enc, pack.wave_len, lists, 0.001)
    assert [h["yseq"] for h in keep[0]] == [[5, 6, 7], [5, 6], long_hyp]
    assert [h["yseq"] for h in flip[0]] == [[5, 6], [5, 6, 7], long_hyp]      # the second CTC hypothesis wins
    for res in (keep, flip):
        assert [len(r) for r in res] == [3, 1, 0]
        by = {tuple(h["yseq"]): h for h in res[0]}
        assert abs(by[(5, 6, 7)]["att_score"] + 4 * logV) < 0.05 and abs(by[(5, 6)]["att_score"] + 3 * logV) < 0.05
        assert by[tuple(long_hyp)]["att_score"] == -math.inf and by[tuple(long_hyp)]["score"] == -math.inf
        assert by[tuple(long_hyp)]["ctc_score"] == -2.5
        assert abs(res[1][0]["att_score"] + logV) < 0.05 and res[1][0]["ctc_score"] == -0.5      # log p(eos | sos)
    with pytest.raises(ValueError):
        decode.attention_rescore(model, enc, pack.wave_len, lists[:2], 0.5)
    # models that lack a head
    ctc_only = build(R.default_cfg(n_mels=16, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1, ctc_weight=1.0), 24,
                     "TransformerCTC", dtype="fp32").cuda().eval()
    with pytest.raises(RuntimeError):
        ctc_only.beam_search(pack, 2, 1, joint="ctc_rescore")
    with pytest.raises(RuntimeError):
        ctc_only.transcribe(pack, beam_size=2, joint="ctc_rescore")
    with pytest.raises(ValueError, match="ctc_rescore"):
        model.beam_search(pack, 2, 1, joint="three_pass")
    with pytest.raises(ValueError, match="ctc_rescore"):
        model.transcribe(pack, joint="three_pass")


# ------------------------------------------------------------------------------------------------------------ the command line
def test_transcribe_cli_ctc_rescore_and_streamed_prefix_beam(tmp_path, capsys):
    """transcribe.py --joint=ctc_rescore, and --stream=1 --stream_search=prefix_beam: per chunk {"file", "chunk", "partial", "stable"}
    with a stable text that only grows and that the final text starts with (one-character tokens: text prefixes are id prefixes).
    Run in this process (transcribe.transcribe is the script's whole body): no second interpreter to start."""
    import json
    import sys
    from asr_chinese_e2e_amd.data_handler import Vocab
    from tests.helpers import ROOT
    from tests.test_ctc_align_gpu import _write_wav
    sys.path.insert(0, ROOT)
    import transcribe as T_
    from train import TrainConfig, get_model_class, parse_flags
    flags = dict(model_name="TransformerOffical", d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1, dtype="fp32",
                 ctc_weight=0.3, decoding_chunk_size=4)
    config = TrainConfig()
    config.fn_build(dict(flags))
    Model, MC = get_model_class(config.model_name)
    config.fn_combine(MC())
    config.fn_build(dict(flags))
    vocab = Vocab.synthetic(40)
    vocab.save(str(tmp_path / "vocab.t"))
    torch.manual_seed(0)
    Model(config, vocab).save(str(tmp_path / "m.model"))
    wavs = [tmp_path / "a.wav", tmp_path / "b.wav"]
    for i, (p, s) in enumerate(zip(wavs, [1.1, 0.6])):
        _write_wav(p, s, i)
    argv = [f"--{k}={v}" for k, v in flags.items()] + [f"--ckpt={tmp_path / 'm.model'}", f"--vocab_path={tmp_path / 'vocab.t'}",
                                                       "--wavs=" + ",".join(map(str, wavs)), "--beam_size=3"]
    capsys.readouterr()
    T_.transcribe(**parse_flags(argv + ["--joint=ctc_rescore"]))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["file"] for l in lines] == [str(p) for p in wavs]
    assert all(isinstance(l["text"], str) and isinstance(l["ids"], list) and l["tokens"] is not None for l in lines)
    T_.transcribe(**parse_flags(argv + ["--stream=1", "--stream_search=prefix_beam", "--frame_topk=5"]))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    final = {l["file"]: l for l in lines if "text" in l}
    assert sorted(final) == sorted(str(p) for p in wavs)
    for p in map(str, wavs):
        chunks = [l for l in lines if l["file"] == p and "chunk" in l]
        assert len(chunks) >= 2 and [l["chunk"] for l in chunks] == sorted(l["chunk"] for l in chunks)
        stable = ""
        for l in chunks:
            assert set(l) == {"file", "chunk", "partial", "stable"}
            assert l["partial"].startswith(l["stable"]) and l["stable"].startswith(stable), l
            stable = l["stable"]
        assert final[p]["text"].startswith(stable)
    with pytest.raises(SystemExit):
        T_.transcribe(**parse_flags(argv + ["--stream_search=prefix_beam"]))      # without --stream=1
