"""Token times of CTC prefix beam hypotheses on the GPU: asr_ctc_prefix_beam_timed / asr_ctc_prefix_beam_chunk_timed against the plain
kernels (tokens, lengths, scores, stable prefix: equal) and against tests/beam_times_ref.py on the kernel's own candidates (records,
Viterbi scores, final counts: equal), then model.stream / model.sessions / model.ctc_prefix_beam_search with beam_times=True.

Every comparison is ==: integers, copied floats, float32 sums in a fixed order, fp64 sums in a fixed order."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import beam_times_ref as BT  # noqa: E402

DEV = "cuda"
B, V = 3, 12
TS = [1, 2, 17, 64, 65]
BEAMS = [(1, 10), (2, 10), (5, 10), (16, 3)]


def _lens(T):
    return [T, (2 * T + 1) // 3, T // 2]      # ragged; T = 1 leaves one utterance without a frame


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _host(ts):
    return tuple(t.cpu().numpy() for t in ts)


_LATTICE = {}


def _lattice(K, T, beam, k, peak):
    """One random lattice (drawn as tests/test_stream_beam_gpu.py draws its own), its candidates, and computed once: the plain and the timed
    offline kernels' full beams after t = 1 .. T frames (every utterance cut at min(len, t)) and the reference's snapshots after every
    frame of every utterance: snap[b][t] = (hypotheses, final count)."""
    key = (T, beam, k, peak)
    if key not in _LATTICE:
        lens = _lens(T)
        g = torch.Generator().manual_seed(B * 1000 + T)
        logits = torch.randn(B, T, V, generator=g) * peak
        vals, ids, blank_lp = K.ctc_frame_topk(logits.reshape(B * T, V).to(DEV), k, 0)
        plain, timed = {}, {}
        for t in range(1, T + 1):
            cut = torch.tensor([min(l, t) for l in lens], dtype=torch.int32, device=DEV)
            plain[t] = _host(K.ctc_prefix_beam(vals, ids, blank_lp, cut, B, T, beam, beam, 0))
            timed[t] = _host(K.ctc_prefix_beam(vals, ids, blank_lp, cut, B, T, beam, beam, 0, times=True))
        v_h, i_h, b_h = vals.view(B, T, k).cpu().numpy(), ids.view(B, T, k).cpu().numpy(), blank_lp.view(B, T).cpu().numpy()
        snap = []
        for b in range(B):
            s = BT.BeamTimes(beam)
            rows = [(s.hyps(), s.final_count())]
            for t in range(lens[b]):
                s.step(b_h[b, t], list(zip(i_h[b, t].tolist(), v_h[b, t])))
                rows.append((s.hyps(), s.final_count()))
            snap.append(rows)
        _LATTICE[key] = (vals.view(B, T, k), ids.view(B, T, k), blank_lp.view(B, T), plain, timed, snap)
    return _LATTICE[key]


def _check_against_reference(out, hyps, b, beam, Lcap, what):
    """The kernel's rows of utterance b (tokens, lengths, scores, vit, start, end, mx, mn, sm) against the reference's hypotheses."""
    tok, ln, sc, vit, start, end, mx, mn, sm = out[:9]
    assert [int(x) for x in ln[b] if x >= 0] == [len(h["prefix"]) for h in hyps], (what, b, ln[b], hyps)
    assert (ln[b, len(hyps):] == -1).all() and (vit[b, len(hyps):] == -math.inf).all(), (what, b)
    for r, h in enumerate(hyps):
        n = min(len(h["prefix"]), Lcap)
        assert tuple(tok[b, r, :n].tolist()) == h["prefix"][:n], (what, b, r)
        assert vit[b, r] == h["viterbi_score"], (what, b, r, vit[b, r], h["viterbi_score"])
        got = list(zip(start[b, r, :n].tolist(), end[b, r, :n].tolist(), mx[b, r, :n], mn[b, r, :n], sm[b, r, :n]))
        assert got == list(h["records"][:n]), (what, b, r, got, h["records"])
        for x in (start, end, mx, mn, sm):      # nothing is written past the hypothesis
            assert (x[b, r, n:] == 0).all(), (what, b, r)


@pytest.mark.parametrize("beam,k", BEAMS)
@pytest.mark.parametrize("T", TS)
def test_offline_timed_kernel_equals_plain_kernel_and_reference(K, T, beam, k):
    for peak in (3.0, 0.3):
        _, _, _, plain, timed, snap = _lattice(K, T, beam, k, peak)
        lens = _lens(T)
        for t in range(1, T + 1):
            for got, want in zip(timed[t][:3], plain[t]):      # tokens, lengths, scores: the plain kernel's bits
                assert np.array_equal(got, want), (peak, t)
            for b in range(B):
                _check_against_reference(timed[t], snap[b][min(lens[b], t)][0], b, beam, T, (peak, t))


def _cuttings(T):
    """name -> list of (C, c0 or None): the chunk covers frames [c0, c0 + C) of every utterance, None = a chunk that consumes nothing."""
    by5 = [(5, c0) for c0 in range(0, T, 5)]
    gaps = [(5, None)]
    for ch in by5:
        gaps += [ch, (5, None)]
    return {"whole": [(T, 0)], "frames": [(1, t) for t in range(T)], "C5": by5, "C16": [(16, c0) for c0 in range(0, T, 16)], "C5_gaps": gaps}


def _rows(x, c0, C):
    part = x[:, c0:c0 + C]
    if part.shape[1] < C:
        part = torch.cat([part, torch.zeros(B, C - part.shape[1], *x.shape[2:], dtype=x.dtype, device=x.device)], dim=1)
    return part.reshape(B * C, *x.shape[2:]).contiguous()


@pytest.mark.parametrize("beam,k", BEAMS)
@pytest.mark.parametrize("T", TS)
def test_chunk_timed_kernel_under_every_cutting(K, T, beam, k):
    """The resumable kernel: the plain chunk kernel's tokens, lengths, scores and stable prefix; the offline timed kernel's records on the
    frames so far; the reference's final count, which never decreases."""
    peak = 3.0 if (T + beam) % 2 else 0.3
    vals, ids, blank_lp, _, timed, snap = _lattice(K, T, beam, k, peak)
    lens = _lens(T)
    for name, chunks in _cuttings(T).items():
        st = K.ctc_prefix_beam_state(B, beam, T, DEV, times=True)
        st_plain = K.ctc_prefix_beam_state(B, beam, T, DEV)
        done, last_final = 0, [0] * B
        for C, c0 in chunks:
            nv = [0] * B if c0 is None else [max(0, min(C, l - c0)) for l in lens]
            c0 = 0 if c0 is None else c0
            args = (_rows(vals, c0, C), _rows(ids, c0, C), _rows(blank_lp, c0, C), nv, C, beam, 0)
            before = (st.state.clone(), st.ws.clone()) if not any(nv) else None
            out = K.ctc_prefix_beam_chunk(st, *args, max_len=T)
            if before is not None:      # a chunk that consumes nothing changes no byte of the state nor of the tries
                assert torch.equal(st.state, before[0]) and torch.equal(st.ws, before[1]), name
            want_plain = K.ctc_prefix_beam_chunk(st_plain, *args, max_len=T)
            for got, want in zip(out[:4], want_plain):
                assert torch.equal(got, want), (name, done)
            out = _host(out)
            done = max(done, c0 + max(nv)) if any(nv) else done
            final = out[10].tolist()
            assert final == [snap[b][min(lens[b], done)][1] for b in range(B)], (name, done, final)
            assert all(f >= p for f, p in zip(final, last_final)) and all(f <= max(int(out[1][b, 0]), 0) for b, f in enumerate(final)), (name, done)
            last_final = final
            if done == 0:
                assert out[1][:, 0].tolist() == [0] * B and out[4][:, 0].tolist() == [0.0] * B and final == [0] * B
                continue
            for got, want in zip(out[4:10], timed[done][3:]):      # vit and the five record arrays: the offline timed kernel's bits
                assert np.array_equal(got, want), (name, done)
        assert done == T and st.frames == lens, name
        for b in range(B):      # the end of the cutting against the reference itself
            _check_against_reference(out[:3] + out[4:10], snap[b][lens[b]][0], b, beam, T, name)


def test_reset_slot_starts_from_frame_zero_and_neighbours_keep_every_byte(K):
    C, beam, k, T_cap = 8, 4, 5, 64
    g = torch.Generator().manual_seed(21)
    chunks = [torch.randn(B * C, V, generator=g).to(DEV) * 2 for _ in range(6)]
    st = K.ctc_prefix_beam_state(B, beam, T_cap, DEV, times=True)
    for x in chunks[:3]:
        K.ctc_prefix_beam_chunk(st, *K.ctc_frame_topk(x, k, 0), [C, C - 3, C], C, beam)
    state0, ws0 = st.state.clone(), st.ws.clone()
    K.ctc_prefix_beam_state_reset(st, torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV), [1])
    per = st.state.numel() // B
    cap = T_cap * beam + 1
    words, words0 = st.ws.view(torch.int32), ws0.view(torch.int32)
    tries = lambda w, b: (w[:B * 2 * cap].view(B, -1)[b], w[B * 2 * cap:].view(B, -1)[b])      # noqa: E731  (the prefix trie and the time trie of utterance b)
    for b in (0, 2):
        assert torch.equal(st.state.view(B, per)[b], state0.view(B, per)[b])
        assert all(torch.equal(x, y) for x, y in zip(tries(words, b), tries(words0, b)))
    fresh = K.ctc_prefix_beam_state(B, beam, T_cap, DEV, times=True)
    assert torch.equal(st.state.view(B, per)[1], fresh.state.view(B, per)[1])      # byte for byte the initialised state
    assert st.frames == [3 * C, 0, 3 * C]
    for x in chunks[3:]:
        cand = K.ctc_frame_topk(x, k, 0)
        got = K.ctc_prefix_beam_chunk(st, *cand, [C, C, 0], C, beam, max_len=T_cap)
        want = K.ctc_prefix_beam_chunk(fresh, *cand, [0, C, 0], C, beam, max_len=T_cap)
        assert all(torch.equal(x[1], y[1]) for x, y in zip(got, want))
    assert int(got[1][1, 0]) > 0 and int(got[6][1].max()) < 3 * C      # frames count from the reset: no run ends past the 3 chunks since


def test_hypothesis_longer_than_the_row_keeps_its_first_records(K):
    T, beam, k = 64, 5, 10
    vals, ids, blank_lp, _, timed, _ = _lattice(K, T, beam, k, 3.0)
    full = timed[T]
    Lcap = 3
    assert int(full[1][0, 0]) > Lcap
    cut = torch.tensor(_lens(T), dtype=torch.int32, device=DEV)
    short = _host(K.ctc_prefix_beam(vals.reshape(B * T, k), ids.reshape(B * T, k), blank_lp.reshape(B * T), cut, B, T, beam, beam, 0, max_len=Lcap, times=True))
    st = K.ctc_prefix_beam_state(B, beam, T, DEV, times=True)
    chunk = _host(K.ctc_prefix_beam_chunk(st, vals.reshape(B * T, k), ids.reshape(B * T, k), blank_lp.reshape(B * T), _lens(T), T, beam, 0, max_len=Lcap))
    for got in (short, chunk[:3] + chunk[4:10]):
        assert np.array_equal(got[1], full[1]) and np.array_equal(got[2], full[2]) and np.array_equal(got[3], full[3])
        for i in (0, 4, 5, 6, 7, 8):
            want = full[i][:, :, :Lcap].copy()
            want[np.broadcast_to(np.arange(Lcap), want.shape) >= np.maximum(full[1], 0)[:, :, None]] = 0
            assert got[i].shape[-1] == Lcap and np.array_equal(got[i], want), i


def test_repeat_wins_the_tie(K):
    """Frame 0: blank and class 1 are equally likely, so after frame 1 the prefix (1,) reaches its best non-blank alignment both as 1 1
    (its own repeat) and as blank 1 (its parent's extension, merged into its stay slot) with the same value.  The repeat wins: one run
    over both frames.  Class 1 beats the blank in frame 1, so that alignment is the reported one."""
    f = np.float32
    p = [[0.4, 0.4, 0.2], [0.3, 0.6, 0.1]]      # blank, 1, 2
    vals = torch.tensor([[f(math.log(r[1])), f(math.log(r[0])), f(math.log(r[2]))] for r in p], device=DEV)
    ids = torch.tensor([[1, 0, 2], [1, 0, 2]], dtype=torch.int32, device=DEV)
    blank_lp = vals[:, 1].contiguous()
    out = _host(K.ctc_prefix_beam(vals, ids, blank_lp, None, 1, 2, 4, 4, 0, times=True))
    s = BT.BeamTimes(4)
    for t in range(2):
        s.step(blank_lp[t].item(), list(zip(ids[t].tolist(), vals[t].cpu().numpy())))
    assert s.beam[(1,)].rep
    _check_against_reference(out, s.hyps(), 0, 4, 2, "tie")
    r = [tuple(out[0][0, i, :out[1][0, i]].tolist()) for i in range(4)].index((1,))
    assert (out[4][0, r, 0], out[5][0, r, 0]) == (0, 1) and out[6][0, r, 0] == f(math.log(0.6)) and out[7][0, r, 0] == f(math.log(0.4))
    assert out[3][0, r] == float(f(math.log(0.4))) + float(f(math.log(0.6)))
    st = K.ctc_prefix_beam_state(1, 4, 2, DEV, times=True)
    for t in range(2):
        chunk = _host(K.ctc_prefix_beam_chunk(st, vals[t:t + 1].contiguous(), ids[t:t + 1].contiguous(), blank_lp[t:t + 1].contiguous(), [1], 1, 4, 0, max_len=2))
    assert all(np.array_equal(a, b) for a, b in zip(chunk[:3] + chunk[4:10], out))


# ------------------------------------------------------------------------------------------------------------ the model
def _tokens_of(K, fed, lens, Bm, C, beam, topk, model, which):
    """What tokens() must say after the chunks in `fed`: the offline timed kernel over the recorded candidates."""
    from asr_chinese_e2e_amd.confidence import beam_tokens
    Tm = len(fed) * C
    vals, ids, blank_lp = (torch.cat([f[i].view(Bm, C, -1) for f in fed], dim=1) for i in range(3))
    cut = torch.tensor([min(l, Tm) for l in lens], dtype=torch.int32, device=DEV)
    out = _host(K.ctc_prefix_beam(vals.reshape(Bm * Tm, topk).contiguous(), ids.reshape(Bm * Tm, topk).contiguous(), blank_lp.reshape(Bm * Tm).contiguous(),
                                  cut, Bm, Tm, beam, beam, 0, times=True))
    tok, ln = out[0], out[1]
    return [[beam_tokens(tok[b, r, :ln[b, r]], *(x[b, r, :ln[b, r]] for x in out[4:9]), which, model.vocab._id2token, model.frame_seconds())
             for r in range(beam) if ln[b, r] >= 0] for b in range(Bm)], out


def test_stream_and_sessions_report_the_kernels_records(K, monkeypatch):
    from tests.test_stream_beam_gpu import _stream_model
    C, Bm, beam, topk = 4, 3, 4, 5
    lens, Tm = [19, 14, 6], 20
    model = _stream_model("fp32", "TransformerCTC", C)
    torch.manual_seed(7)
    feats = torch.randn(Bm, Tm, 16, device=DEV)
    fed = []
    real = K.ctc_frame_topk

    def recording(logits, k, blank=0):
        out = real(logits, k, blank)
        fed.append(tuple(t.clone() for t in out))
        return out
    monkeypatch.setattr(K, "ctc_frame_topk", recording)
    st = model.stream(Bm, search="prefix_beam", beam_size=beam, frame_topk=topk, beam_times=True, confidence="post_mean")
    plain = model.stream(Bm, search="prefix_beam", beam_size=beam, frame_topk=topk)
    assert st.tokens() == [[]] * Bm
    was_final = [[] for _ in range(Bm)]
    per_push = []
    for c0 in range(0, Tm, C):
        nv = [max(0, min(C, l - c0)) for l in lens]
        x = feats[:, c0:c0 + C].contiguous()
        got = st.push(x, nv)
        n_fed = len(fed)
        assert got == plain.push(x, nv)      # push returns what it returns
        del fed[n_fed:]
        want, raw = _tokens_of(K, fed, lens, Bm, C, beam, topk, model, "post_mean")
        toks, part, nb, nb_plain = st.tokens(), st.partial(), st.nbest(), plain.nbest()
        per_push.append(toks)
        for b in range(Bm):
            assert [{k_: v for k_, v in t.items() if k_ != "final"} for t in toks[b]] == want[b][0], (c0, b)
            assert [h["tokens"] for h in nb[b]] == want[b] and [h["viterbi_score"] for h in nb[b]] == raw[3][b, :len(nb[b])].tolist()
            assert [{k_: h[k_] for k_ in ("yseq", "score")} for h in nb[b]] == nb_plain[b]
            assert [t["id"] for t in part[b]["tokens"]] == part[b]["ids"] and part[b]["tokens"] == nb[b][0]["tokens"]
            assert all(t["confidence"] == t["measures"]["post_mean"] and t["end_s"] == (t["end_frame"] + 1) * model.frame_seconds() for t in toks[b])
            flags = [t["final"] for t in toks[b]]
            assert flags == sorted(flags, reverse=True)      # the final records lead
            n_was = len(was_final[b])
            assert flags[:n_was] == [True] * n_was and toks[b][:n_was] == was_final[b]      # they only ever turn on, and what was final stays as it is
            was_final[b] = [t for t in toks[b] if t["final"]]
    monkeypatch.setattr(K, "ctc_frame_topk", real)
    assert any(was_final) and any(len(t) > len(f) for t, f in zip(toks, was_final))
    # the offline search over the same features: the same call with beam_times gains the two fields and changes nothing else
    from asr_chinese_e2e_amd.Utils import Pack
    pack = Pack(wave=feats, wave_len=torch.tensor(lens, dtype=torch.int32, device=DEV))
    off, off_plain = model.ctc_prefix_beam_search(pack, beam, beam, topk, beam_times=True, confidence="post_min"), model.ctc_prefix_beam_search(pack, beam, beam, topk)
    for b in range(Bm):
        assert [{k_: h[k_] for k_ in ("yseq", "score")} for h in off[b]] == off_plain[b] and all(set(h) == {"yseq", "score", "viterbi_score", "tokens"} for h in off[b])
        for h in off[b]:
            assert [t["id"] for t in h["tokens"]] == h["yseq"] and all(t["confidence"] == t["measures"]["post_min"] for t in h["tokens"])
            assert all(a["end_frame"] < c["start_frame"] for a, c in zip(h["tokens"], h["tokens"][1:])) and h["viterbi_score"] <= h["score"] + 1e-6
    # finish() is what it is, and drops the records
    fin, fin_plain = st.finish(joint="ctc_rescore"), plain.finish(joint="ctc_rescore")
    assert fin == fin_plain and st.tokens() == [[]] * Bm and all("tokens" not in h for h in st.nbest()[0])
    # sessions in lock-step: the stream's tokens slot by slot; a finished slot has none, a reopened one starts from frame 0
    ss = model.sessions(Bm, search="prefix_beam", beam_size=beam, frame_topk=topk, beam_times=True, confidence="post_mean")
    for b in range(Bm):
        ss.open(b)
        assert ss.tokens(b) == []
    for i, c0 in enumerate(range(0, Tm, C)):
        nv = [max(0, min(C, l - c0)) for l in lens]
        ss.push(feats[:, c0:c0 + C].contiguous(), nv, [ss.state[b] == "open" and c0 + C >= lens[b] for b in range(Bm)])
        assert [ss.tokens(b) for b in range(Bm)] == per_push[i], i
        assert all(ss.partial(b)["tokens"] == ss.nbest(b)[0]["tokens"] for b in range(Bm))
    ss.finish(1)
    assert ss.tokens(1) == []
    ss.open(1)
    assert ss.tokens(1) == [] and "tokens" not in ss.nbest(1)[0]
    x = torch.zeros(Bm, C, 16, device=DEV)
    x[1] = feats[1, :C]
    ss.push(x, [0, C, 0], [False] * Bm)
    assert ss.tokens(1) == per_push[0][1] and ss.tokens(0) == per_push[-1][0]
    ss.drop(1)
    assert ss.tokens(1) == []


def test_transcribe_cli_streams_beam_times(tmp_path, capsys):
    """transcribe.py --stream=1 --stream_search=prefix_beam --beam_times=1: the chunk lines gain "tokens" that spell the partial text.
    Run in this process, as tests/test_stream_beam_gpu.py runs the script."""
    import json
    import sys
    from asr_chinese_e2e_amd.data_handler import Vocab
    from tests.helpers import ROOT
    from tests.test_ctc_align_gpu import _write_wav
    sys.path.insert(0, ROOT)
    import transcribe as T_
    from train import TrainConfig, get_model_class, parse_flags
    flags = dict(model_name="TransformerOffical", d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1, dtype="fp32", ctc_weight=0.3,
                 decoding_chunk_size=4)
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
    argv = [f"--{k}={v}" for k, v in flags.items()] + [f"--ckpt={tmp_path / 'm.model'}", f"--vocab_path={tmp_path / 'vocab.t'}", "--wavs=" + ",".join(map(str, wavs)),
                                                       "--beam_size=3", "--stream=1", "--stream_search=prefix_beam", "--frame_topk=5"]
    capsys.readouterr()
    T_.transcribe(**parse_flags(argv + ["--beam_times=1"]))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    chunks = [l for l in lines if "chunk" in l]
    assert len(chunks) >= 4 and all(set(l) == {"file", "chunk", "partial", "stable", "tokens"} for l in chunks)
    for l in chunks:
        assert "".join(t["token"] for t in l["tokens"] if t["id"] not in (0, 2, 3)) == l["partial"]
        assert all(set(t) == {"id", "token", "start_frame", "end_frame", "start_s", "end_s", "measures", "confidence", "final"} for t in l["tokens"])
    with pytest.raises(SystemExit):
        T_.transcribe(**parse_flags(argv[:-2] + ["--beam_times=1"]))      # without the prefix beam search
    with pytest.raises(SystemExit):
        T_.transcribe(**parse_flags(argv + ["--beam_times=1", "--confidence=ent_min"]))
