"""Token confidence and streamed token times on the GPU (csrc/confidence.hip) against tests/confidence_ref.py: the frame statistics
against their two sibling kernels bit for bit and against the float64 definition within the derived bounds, the token measures over
asr_ctc_align's spans, the timed session step under every cutting bit for bit, the streamed greedy records against the offline Viterbi
ones, and model.stream / model.sessions / finish / transcribe.py end to end."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import confidence_ref as CR  # noqa: E402

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
NINF = float("-inf")
SILENCE_LP = math.log(0.8)


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _np(t):
    return t.detach().cpu().double().numpy()


def _ratio(got, want, bound):
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
    return float((np.abs(got[fin] - want[fin]) / bound[fin]).max()) if fin.any() else 0.0


# ================================================================================================ frame statistics
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V", [2, 63, 64, 65, 4232, 4233])
def test_frame_stats_match_their_siblings_and_the_definition(K, V, dtype):
    """(B, T) = (2, 19) frames, the second utterance 11 long, rows padded to a stride of V + 8 whose padding holds 3e38.  Edge rows:
    one-hot at +-1e4, constant, all -inf but two entries."""
    B, T, ld = 2, 19, V + 8
    g = torch.Generator().manual_seed(V)
    x = torch.randn(B * T, V, generator=g) * torch.tensor([0.1, 1.0, 4.0, 12.0])[torch.randint(0, 4, (B * T, 1), generator=g)]
    x[0], x[1] = -1e4, 0.25
    x[0, V // 2] = 1e4
    x[2] = NINF
    x[2, 0], x[2, V - 1] = 0.5, -0.75
    x[3] = torch.randint(0, 3, (V,), generator=g).float()      # ties in the maximum: the first wins
    x[4, V - 1] = x[4].max() + 1                                # the maximum in the scalar tail / last vector
    x = x.to(DT[dtype])
    buf = torch.full((B * T, ld), 3.0e38).to(DT[dtype])
    buf[:, :V] = x
    xd = buf.to(DEV)[:, :V].view(B, T, V)
    lens = _i32([T, 11])
    path, best_lp, blank_lp, lse, ent = K.ctc_frame_stats(xd, lens, 0)
    assert torch.equal(path, K.ctc_frame_argmax(xd, lens, 0))
    want_path, want_blank = K.ctc_frame_best_blank(xd, lens, 0)
    assert torch.equal(path, want_path) and torch.equal(blank_lp.view(torch.int32), want_blank.view(torch.int32))      # bit for bit
    live = (torch.arange(T)[None, :] < torch.tensor([[T], [11]])).view(-1).numpy()
    for t in (path, best_lp, blank_lp, lse, ent):      # rows past in_len: the blank and zeros
        assert (t.view(-1).cpu().numpy()[~live] == 0).all()
    x64 = x.double().numpy()[live]
    want, bound = CR.frame_stats(x64, 0), CR.frame_bounds(x64)
    assert np.array_equal(path.view(-1).cpu().numpy()[live], want["path"])
    rows = np.arange(len(x64))
    worst = {}
    for key, got, b in (("lse", lse, bound["lse"]), ("best_lp", best_lp, bound["lp"][rows, want["path"]]), ("blank_lp", blank_lp, bound["lp"][:, 0]),
                        ("ent", ent, bound["ent"])):
        worst[key] = _ratio(_np(got).reshape(-1)[live], want[key], b)
    print(f"frame_stats V={V} {dtype}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    e = _np(ent).reshape(-1)
    assert not np.isnan(e).any() and e.min() >= 0.0 and e.max() <= 1.0
    assert e[0] == 1.0 and e[1] == 0.0      # one-hot: exactly 1, constant: exactly 0
    assert _np(best_lp).reshape(-1)[0] == 0.0 and int(path.view(-1)[0]) == V // 2 and int(path.view(-1)[1]) == 0
    if V > 2:
        assert _np(blank_lp).reshape(-1)[2] != NINF and int(path.view(-1)[2]) == 0 and 0.0 < e[2] < 1.0
    assert max(worst.values()) <= 1.0, worst


# ================================================================================================ token measures
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("Lmax", [0, 1, 7])
def test_token_measures_over_the_alignments_spans(K, Lmax, dtype):
    """B = 3 ragged, T = 40, V = 50: utterance 0 has Lmax labels, utterance 1 cannot be aligned (more labels with repeats than its 3
    frames hold) and utterance 2 has no labels."""
    B, T, V = 3, 40, 50
    g = torch.Generator().manual_seed(100 + Lmax)
    x = (torch.randn(B, T, V, generator=g) * 3).to(DT[dtype])
    in_len = [40, 3, 29]
    labs = [[5, 5, 9, 1, 49, 7, 7][:Lmax], [4, 4, 4, 4, 4, 4, 4][:Lmax], []]
    lab = torch.zeros(B, Lmax, dtype=torch.int32)
    for b, l in enumerate(labs):
        lab[b, :len(l)] = torch.tensor(l, dtype=torch.int32)
    xd, lab_d, ll_d, il_d = x.to(DEV), lab.to(DEV), _i32([len(l) for l in labs]), _i32(in_len)
    _, spans, tlp, score = K.ctc_align(xd, il_d, lab_d, ll_d)
    _, _, _, lse, ent = K.ctc_frame_stats(xd, il_d, 0)
    conf = K.ctc_token_conf(xd, lab_d, ll_d, spans, lse, ent)
    assert conf.shape == (B, Lmax, 5)
    conf, spans_h, tlp_h, score_h = _np(conf), spans.cpu().numpy(), _np(tlp), _np(score)
    if Lmax >= 2:
        assert score_h[1] == NINF and (spans_h[1] == -1).all() and np.isnan(conf[1]).all()      # infeasible: NaN in all five
    assert np.all(conf[2] == 0.0)                                                          # past lab_len: 0
    worst, worst_lp = 0.0, 0.0
    for b in range(B):
        if score_h[b] == NINF:
            continue
        n_b = in_len[b]
        x64 = x[b, :n_b].double().numpy()
        st, fb = CR.frame_stats(x64, 0), CR.frame_bounds(x64)
        for i, y in enumerate(labs[b]):
            s, e = int(spans_h[b, i, 0]), int(spans_h[b, i, 1])
            assert 0 <= s <= e < n_b
            want, bound = CR.token_measures(st["logp"], st["ent"], y, s, e), CR.token_bounds(st["logp"], st["ent"], fb["lp"], fb["ent"], y, s, e)
            got = dict(zip(CR.MEASURES, conf[b, i]))
            for k in CR.MEASURES:
                worst = max(worst, abs(got[k] - want[k]) / bound[k])
            assert got["post_max"] >= got["post_mean"] >= got["post_min"] and got["ent_mean"] >= got["ent_min"]
            # the geometric mean against ctc_align's summed log-probability: each side within its derived distance of the exact sum
            n = e - s + 1
            lp = st["logp"][s:e + 1, y]
            tol = n * bound["post_mean"] / want["post_mean"] + CR.SLACK * (fb["lp"][s:e + 1, y].sum() + (n - 1) * CR.EPS * np.abs(lp).sum())
            worst_lp = max(worst_lp, abs(math.log(got["post_mean"]) * n - tlp_h[b, i]) / tol)
    print(f"token_conf Lmax={Lmax} {dtype}: largest err / bound {worst:.3f}, log(post_mean) n against token_logp {worst_lp:.3f}")
    assert worst <= 1.0 and worst_lp <= 1.0


# ================================================================================================ the timed step
_STEP = {}


def _step_input():
    if not _STEP:
        x = CR.step_logits()
        _STEP["x"], _STEP["xd"] = x, torch.from_numpy(x).to(DEV)
        _STEP["ref"] = [CR.stream_tokens(x[b, :n].astype(np.float64), 0) for b, n in enumerate(CR.STEP_LENS)]
    return _STEP


def _records(words, C, b):
    """Slot b of a host (slots, 13 + 9 C) int32 buffer -> ([closed records as 8-word tuples], the open record or None)."""
    row = words[b]
    n, base = row[4 + C], 5 + C
    closed = [tuple(row[base + 8 * r:base + 8 * r + 8]) for r in range(n)]
    assert all(v == 0 for v in row[base + 8 * n:base + 8 * C])      # zeros behind the last record
    op = tuple(row[base + 8 * C:base + 8 * C + 8])
    return closed, (op if op[0] >= 0 else None)


def _play(K, xd, tapes, C, sit):
    """tapes[b]: the utterances (index, length) slot b plays one after the other, each a session of its own (reset on its first tick).
    Every tick a slot takes its next C frames or sits out.  -> {utterance: (ids, records)}, the open run closed by the host at the end.
    Beside it asr_session_ctc_step runs on a state of its own: the first 4 + C words and the state must be the same."""
    S, V = len(tapes), xd.shape[2]
    state, run, state2 = (torch.zeros(S, n, dtype=torch.int32, device=DEV) for n in (4, 8, 4))
    state += 77      # garbage that the reset has to clear
    run += 77
    state2 += 77
    cur, pos = [0] * S, [0] * S
    out = {}
    acc = [([], []) for _ in range(S)]
    for tick in range(2000):
        if all(cur[b] >= len(tapes[b]) for b in range(S)):
            break
        nv, rs = [0] * S, [0] * S
        chunk = torch.zeros(S, C, V, device=DEV)
        for b in range(S):
            if cur[b] >= len(tapes[b]) or (sit and (tick * 7 + b * 13 + 5) % 3 == 0):
                continue
            u, n = tapes[b][cur[b]]
            nv[b], rs[b] = min(C, n - pos[b]), int(pos[b] == 0)
            chunk[b, :nv[b]] = xd[u, pos[b]:pos[b] + nv[b]]
        nv_d, rs_d = _i32(nv), _i32(rs)
        path, best_lp, blank_lp, _, ent = K.ctc_frame_stats(chunk, nv_d, 0)
        buf = K.session_ctc_step_tokens(path, blank_lp, best_lp, ent, nv_d, rs_d, state, run, C, SILENCE_LP, 0)
        plain = K.session_ctc_step(path, blank_lp, nv_d, rs_d, state2, C, SILENCE_LP, 0)
        touched = [b for b in range(S) if nv[b] > 0]
        assert torch.equal(buf[touched, :4 + C], plain[touched]) and torch.equal(state[touched], state2[touched]), tick
        words = buf.cpu().tolist()
        for b in touched:
            u, n = tapes[b][cur[b]]
            closed, op = _records(words, C, b)
            acc[b][0].extend(words[b][4:4 + words[b][0]])
            acc[b][1].extend(closed)
            pos[b] += nv[b]
            if pos[b] >= n:      # the session's input has ended: the host closes the open run
                out[u if cur[b] == 0 else (u, "again")] = (acc[b][0], acc[b][1] + ([op] if op else []))
                acc[b], cur[b], pos[b] = ([], []), cur[b] + 1, 0
    assert all(cur[b] >= len(tapes[b]) for b in range(S))
    return out


def _whole(K):
    st = _step_input()
    if "whole" not in st:
        T = CR.STEP_T
        st["whole"] = _play(K, st["xd"], [[(b, n)] for b, n in enumerate(CR.STEP_LENS)], T, sit=False)
    return st["whole"]


def _f32(word):
    return float(np.array([word], dtype=np.int32).view(np.float32)[0])


def test_timed_step_whole_input_matches_the_definition(K):
    st = _step_input()
    whole = _whole(K)
    worst = 0.0
    for b, n in enumerate(CR.STEP_LENS):
        ids, recs = whole[b]
        ref = st["ref"][b]
        assert ids == [r["id"] for r in ref] and [(r[0], r[1], r[2]) for r in recs] == [(r["id"], r["start_frame"], r["end_frame"]) for r in ref]
        x64 = st["x"][b, :n].astype(np.float64)
        fs, fb = CR.frame_stats(x64, 0), CR.frame_bounds(x64)
        for rec, r in zip(recs, ref):
            bound = CR.token_bounds(fs["logp"], fs["ent"], fb["lp"], fb["ent"], r["id"], r["start_frame"], r["end_frame"])
            for j, k in enumerate(CR.MEASURES):
                worst = max(worst, abs(_f32(rec[3 + j]) - r["measures"][k]) / bound[k])
    lengths = {r[2] - r[1] + 1 for b in range(3) for r in whole[b][1]}
    assert 1 in lengths and 2 in lengths and max(lengths) > 64
    assert whole[2][1][-1][2] == CR.STEP_LENS[2] - 1      # slot 2 ended on an open run, which the host closed
    print(f"timed step: largest err / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("C", [1, 5, 16, 64, 65])
def test_timed_step_is_the_same_under_every_cutting(K, C):
    """Chunks of C with ticks sat out; slot 0 plays utterance 0 and then, reset, utterance 1 again as a second session: every record
    has the whole-input run's bits, the second session those of utterance 1 run alone."""
    st = _step_input()
    whole = _whole(K)
    lens = CR.STEP_LENS
    got = _play(K, st["xd"], [[(0, lens[0]), (1, lens[1])], [(1, lens[1])], [(2, lens[2])]], C, sit=True)
    assert sorted(map(str, got)) == sorted(map(str, [0, 1, 2, (1, "again")]))
    for u in range(3):
        assert got[u] == whole[u], (C, u)
    assert got[(1, "again")] == whole[1]
    for u in range(3):      # a run lies across a cut of this chunking
        assert any(r[1] < k <= r[2] for r in whole[u][1] for k in range(C, lens[u], C))


def test_streamed_greedy_records_equal_the_offline_viterbi_ones(K):
    """ctc_align + ctc_token_conf of the final greedy ids against the streamed records: the same spans, the same bits.  Every frame's
    two largest log-probabilities differ by more than 1e-3 in float64 (asserted for every frame), so the greedy path is the one best
    path and no fp32 rounding can make the Viterbi recursion prefer another.  fp32 on purpose: in bf16 equal maxima are common, and
    the Viterbi tie rule may then pick another path of the same score."""
    st = _step_input()
    whole = _whole(K)
    lens = CR.STEP_LENS
    for b, n in enumerate(lens):
        assert CR.top2_gap(st["x"][b, :n]).min() > 1e-3
    Lmax = max(len(whole[b][0]) for b in range(3))
    assert 0 < Lmax <= 255
    lab = torch.zeros(3, Lmax, dtype=torch.int32)
    for b in range(3):
        lab[b, :len(whole[b][0])] = torch.tensor(whole[b][0], dtype=torch.int32)
    lab_d, ll_d, il_d = lab.to(DEV), _i32([len(whole[b][0]) for b in range(3)]), _i32(list(lens))
    _, spans, _, score = K.ctc_align(st["xd"], il_d, lab_d, ll_d)
    _, _, _, lse, ent = K.ctc_frame_stats(st["xd"], il_d, 0)
    conf = K.ctc_token_conf(st["xd"], lab_d, ll_d, spans, lse, ent).view(torch.int32).cpu().tolist()
    spans = spans.cpu().tolist()
    assert torch.isfinite(score).all()
    for b in range(3):
        for i, rec in enumerate(whole[b][1]):
            assert (rec[0], rec[1], rec[2]) == (int(lab[b, i]), spans[b][i][0], spans[b][i][1]), (b, i)
            assert list(rec[3:]) == conf[b][i], (b, i)


# ================================================================================================ end to end
_E2E = {}


def _ctc_model():
    """tests/test_sessions_gpu.py's small streaming model, CTC only, fp32, C = 8; the CTC head's weights are scaled by 30 so that its
    posteriors are peaked and the beam-1 prefix search is the greedy search."""
    if "m" not in _E2E:
        from tests.test_chunk_gpu import _stream_model
        model = _stream_model("fp32", 2, "TransformerCTC", C=8)
        sd = model.state_dict()
        for k in sd:
            if k.endswith("ctc_lo.weight") or k.endswith("ctc_lo.bias"):
                sd[k] = sd[k] * 30.0
        model.load_state_dict(sd)
        _E2E["m"] = model
    return _E2E["m"]


def _utts(lens, seed=5, F=16):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, F, generator=g).to(DEV) for n in lens]


def _chunk(utts, c0, C, F=16):
    x = torch.zeros(len(utts), C, F, device=DEV)
    nv = []
    for i, u in enumerate(utts):
        n = max(0, min(C, u.shape[0] - c0))
        if n:
            x[i, :n] = u[c0:c0 + n]
        nv.append(n)
    return x, nv


def test_timed_sessions_equal_the_timed_stream_and_finish():
    model, C = _ctc_model(), 8
    utts = _utts([37, 21])
    st = model.stream(2, timed=True)
    ss = model.sessions(2, timed=True)
    plain = model.sessions(2)
    for b in range(2):
        ss.open(b)
        plain.open(b)
    ids = [[], []]
    for c0 in range(0, 40, C):
        x, nv = _chunk(utts, c0, C)
        fin = [c0 + C >= u.shape[0] and n > 0 for u, n in zip(utts, nv)]
        got_st = st.push(x, nv)
        got_ss = ss.push(x, nv, fin)
        assert got_ss == got_st == plain.push(x, nv, fin)      # push returns what it returns without timed
        toks_st = st.tokens()
        for b in range(2):
            ids[b] += got_ss[b]
            assert ss.tokens(b) == toks_st[b], (c0, b)
            assert [t["id"] for t in toks_st[b]] == ids[b]
            assert all(t["final"] for t in toks_st[b][:-1])
    assert any(ids)
    d = model.frame_seconds()
    for b in range(2):
        toks = ss.tokens(b)
        assert all(t["final"] for t in toks) and ss.status(b)["state"] == "ended"
        for t in toks:
            assert t["start_s"] == t["start_frame"] * d and t["end_s"] == (t["end_frame"] + 1) * d
            assert t["confidence"] == t["measures"]["post_max"] and 0.0 < t["measures"]["post_min"] <= t["measures"]["post_mean"] <= t["measures"]["post_max"] <= 1.0
            assert 0.0 <= t["measures"]["ent_min"] <= t["measures"]["ent_mean"] <= 1.0
        r = ss.finish(b, beam_size=1, confidence="post_max")
        assert r["ids"] == ids[b]      # the final search is greedy-equivalent
        assert [(t["id"], t["start_frame"], t["end_frame"]) for t in r["tokens"]] == [(t["id"], t["start_frame"], t["end_frame"]) for t in toks]
        assert r["confidence"] == CR.utterance(t["confidence"] for t in r["tokens"])
        assert ss.tokens(b) == toks      # the list stays until the slot is reopened
        ss.open(b)
        assert ss.tokens(b) == []
    fin_st = st.finish(beam_size=1, confidence="ent_mean")
    for b in range(2):
        assert fin_st[b]["ids"] == ids[b] and all(t["confidence"] == t["measures"]["ent_mean"] for t in fin_st[b]["tokens"])
    off = model.sessions(1)
    off.open(0)
    off.push(*_chunk(utts[:1], 0, C), [False])
    r = off.finish(0, beam_size=1)
    assert "confidence" not in r and all("confidence" not in t and "measures" not in t for t in r["tokens"])      # off by default


def test_model_ctc_align_and_transcribe_carry_confidence():
    from asr_chinese_e2e_amd.Utils import Pack
    model = _ctc_model()
    utts = _utts([24, 16], seed=9)
    wave = torch.zeros(2, 24, 16, device=DEV)
    for b, u in enumerate(utts):
        wave[b, :u.shape[0]] = u
    pack = Pack(wave=wave, wave_len=_i32([24, 16]))
    base = model.transcribe(pack, beam_size=2)
    got = model.transcribe(pack, beam_size=2, confidence=True)
    for r0, r in zip(base, got):
        assert r["ids"] == r0["ids"] and "confidence" not in r0
        assert [{k: v for k, v in t.items() if k not in ("confidence", "measures")} for t in r["tokens"]] == r0["tokens"]
        for t in r["tokens"]:
            assert t["confidence"] == t["measures"]["post_max"]
        assert r["confidence"] == CR.utterance(t["confidence"] for t in r["tokens"])
    al = model.ctc_align(pack, labels=[[5, 6], [4] * 20], confidence="post_min")
    assert al[0]["confidence"] is not None and all(t["confidence"] == t["measures"]["post_min"] for t in al[0]["tokens"])
    assert al[1]["confidence"] is None and all(t["confidence"] is None and t["measures"] is None for t in al[1]["tokens"])      # 20 repeats in 16 frames
    assert all("confidence" not in t for t in model.ctc_align(pack, labels=[[5, 6], [4]])[0]["tokens"])


def test_transcribe_cli_confidence_and_timed(tmp_path, capsys):
    """transcribe.py --confidence offline, --stream=1 --timed=1 and --sessions=2 with both, in this process."""
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
    capsys.readouterr()
    runs = {}
    for name, extra in (("plain", []), ("offline", ["--confidence=post_max"]), ("stream", ["--stream=1", "--timed=1"]),
                        ("sessions", ["--stream=1", "--timed=1", "--sessions=2", "--confidence=ent_mean"])):
        T_.transcribe(**parse_flags(argv + extra))
        runs[name] = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    final = {name: {l["file"]: l for l in lines if "ids" in l} for name, lines in runs.items()}
    for name in runs:
        assert sorted(final[name]) == sorted(map(str, wavs)), name
    assert all("confidence" not in l and all("confidence" not in t for t in l["tokens"]) for l in final["plain"].values())
    assert all("tokens" not in l for l in runs["plain"] if "chunk" in l)
    for f, l in final["offline"].items():
        assert l["ids"] == final["plain"][f]["ids"] and "confidence" in l
        assert all(t["confidence"] == t["measures"]["post_max"] for t in l["tokens"] if t["measures"])
    assert all("confidence" not in l for l in final["stream"].values())
    for f, l in final["sessions"].items():
        assert all(t["confidence"] == t["measures"]["ent_mean"] for t in l["tokens"] if t["measures"])
    for name, which in (("stream", "post_max"), ("sessions", "ent_mean")):
        chunks = [l for l in runs[name] if "chunk" in l]
        assert chunks and all("tokens" in l for l in chunks)
        for l in chunks:
            assert "".join(t["token"] for t in l["tokens"]) == l["partial"]
            assert all(t["confidence"] == t["measures"][which] for t in l["tokens"]) and all(t["final"] for t in l["tokens"][:-1])
    with pytest.raises(SystemExit, match="--timed"):
        T_.transcribe(**parse_flags(argv + ["--timed=1"]))
    with pytest.raises(SystemExit, match="--confidence"):
        T_.transcribe(**parse_flags(argv + ["--confidence=entropy"]))
