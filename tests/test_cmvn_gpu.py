"""Global CMVN and the streaming waveform front end on the GPU: the statistics and apply kernels against the float64 definition
(tests/cmvn_ref.py), streamed features against offline ones bit for bit under every way of cutting the audio into blocks, and
model.stream().push_audio against push() of the offline features."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cmvn_ref as CR  # noqa: E402

DEV = "cuda"
LENS = [0, 150, 4000, 12345]
SMAX = 12345
AMP = [1.0, 0.05, 0.3, 3.0]      # loudness differs by utterance: no utterance's normalised mean sits near zero


def _waves(seed):
    rng = np.random.RandomState(seed)
    wav = np.zeros((len(LENS), SMAX), dtype=np.float32)
    for b, l in enumerate(LENS):
        wav[b, :l] = (AMP[b] * rng.randn(l)).astype(np.float32)
    return wav


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def logmels(K):
    """n_mels -> (parser, wav (B, S) cuda, lens cuda int32, [log-mel of two batches] as the kernel gives them, numpy copies)."""
    from asr_chinese_e2e_amd.data_handler import AudioParser
    out = {}
    for n_mels in (40, 80):
        parser = AudioParser(n_mels=n_mels, device=DEV)
        wl = torch.tensor(LENS, dtype=torch.int32, device=DEV)
        wavs = [torch.from_numpy(_waves(seed)).to(DEV) for seed in (0, 1)]
        feats = [K.logmel(w, wl, parser.window, parser.melfb, 1 + SMAX // 160) for w in wavs]
        out[n_mels] = (parser, wavs, wl, feats, [f.cpu().numpy() for f in feats])
    return out


@pytest.fixture(scope="module")
def stats40(logmels):
    """Statistics of the first 40-bin batch (float64, from the reference) - what the apply and streaming tests normalise with."""
    return CR.finalize(*CR.accumulate(logmels[40][4][0], LENS))[:2]


# ------------------------------------------------------------------------------------ 1. statistics
@pytest.mark.parametrize("n_mels", [40, 80])
def test_statistics_kernel_matches_reference(K, logmels, n_mels):
    from asr_chinese_e2e_amd.data_handler import cmvn
    parser, wavs, wl, feats, feats_np = logmels[n_mels]
    acc = torch.zeros(2 * n_mels + 1, dtype=torch.float64, device=DEV)
    ref = None
    for k in range(2):      # two batches into the same accumulators
        K.cmvn_accumulate(feats[k], wl, acc)
        ref = CR.accumulate(feats_np[k], LENS, ref)
        a = acc.cpu().numpy()
        mean, istd, count = cmvn.finalize_stats(a[:n_mels], a[n_mels:2 * n_mels], a[2 * n_mels])
        rmean, ristd, rcount = CR.finalize(*ref)
        e_mean, e_std = np.abs(mean / rmean - 1).max(), np.abs(ristd / istd - 1).max()
        print(f"n_mels {n_mels} after batch {k}: count {count}, mean rel err {e_mean:.3g}, std rel err {e_std:.3g}")
        assert count == rcount == (k + 1) * (1 + 26 + 78) and a[2 * n_mels] == rcount
        assert e_mean <= 1e-9 and e_std <= 1e-9
    # the accumulator class takes the same path from the waveforms
    accu = cmvn.CmvnAccumulator(parser)
    for w in wavs:
        accu.update(w, wl)
    m2, i2, c2 = accu.finalize()
    assert c2 == count and np.abs(m2 / rmean - 1).max() <= 1e-9 and np.abs(ristd / i2 - 1).max() <= 1e-9


# ------------------------------------------------------------------------------------ 2. apply
def _parser(n_mels, stats, m, n):
    from asr_chinese_e2e_amd.data_handler import AudioParser
    return AudioParser(n_mels=n_mels, lfr_m=m, lfr_n=n, device=DEV, norm="global", cmvn=stats)


@pytest.mark.parametrize("m,n", [(4, 3), (1, 1)])
def test_apply_kernel_matches_reference(K, logmels, stats40, m, n):
    _, wavs, wl, feats, feats_np = logmels[40]
    mean, istd = (torch.from_numpy(v.astype(np.float32)).to(DEV) for v in stats40)
    Tmax = feats[0].shape[1]
    Tl = -(-Tmax // n) + 2                                   # two rows more than any utterance has: padding rows
    want, want_len, _ = CR.apply(feats_np[0], LENS, *stats40, m, n, Tl)
    got, got_len = K.global_norm_lfr(feats[0], wl, mean, istd, m, n, Tl, torch.float32)
    assert got_len.tolist() == want_len.tolist() == [-(-CR.total_frames(l) // n) for l in LENS]
    g = got.cpu().numpy()
    err = np.abs(g - want) - 3e-7 * np.abs(want)
    print(f"LFR {m}/{n}: fp32 max excess over rtol 3e-7: {err.max():.3g}, bit-identical: {np.array_equal(g, want)}")
    assert err.max() <= 0
    for b, l in enumerate(want_len):
        assert not g[b, l:].any()                            # padding rows are zero
    if (m, n) == (4, 3):                                     # tail repeat: the last row of the 12345-sample utterance (78 frames) stacks 75, 76, 77, 77
        assert np.array_equal(g[3, 25, 2 * 40:3 * 40], g[3, 25, 3 * 40:]) and not np.array_equal(g[3, 25, 40:80], g[3, 25, 80:120])
    bf, bf_len = K.global_norm_lfr(feats[0], wl, mean, istd, m, n, Tl, torch.bfloat16)
    assert bf_len.tolist() == want_len.tolist()
    d = (bf.float() - got).abs()
    ulp = torch.exp2(torch.floor(torch.log2(got.abs().clamp_min(1e-30))) - 7)      # bf16: 8 significant bits
    assert bool((d <= ulp).all()), float((d / ulp).max())
    # the parser's global path is this kernel
    p_out, p_len = _parser(40, stats40, m, n).parse_batch(wavs[0], wl)
    assert torch.equal(p_out[:, :p_out.shape[1]], got[:, :p_out.shape[1]]) and p_len.tolist() == want_len.tolist()


def test_apply_kernel_with_masks(K, logmels, stats40):
    _, _, wl, feats, feats_np = logmels[40]
    mean, istd = (torch.from_numpy(v.astype(np.float32)).to(DEV) for v in stats40)
    masks = [[0, 0, 0, 0], [0, 1, 3, 9], [5, 17, 30, 40], [70, 90, 0, 11]]      # one past the end of the utterance: clamped
    Tmax = feats[0].shape[1]
    plain, _ = K.global_norm_lfr(feats[0], wl, mean, istd, 1, 1, Tmax, torch.float32)
    for m, n in ((1, 1), (4, 3)):
        Tl = -(-Tmax // n)
        want, want_len, fills = CR.apply(feats_np[0], LENS, *stats40, m, n, Tl, masks=masks)
        got, got_len = K.global_norm_lfr(feats[0], wl, mean, istd, m, n, Tl, torch.float32, masks=torch.tensor(masks, dtype=torch.int32, device=DEV))
        assert got_len.tolist() == want_len.tolist()
        g = got.cpu().numpy()
        for b in (1, 2, 3):
            t0, t1, f0, f1 = masks[b]
            Tb = CR.total_frames(LENS[b])
            t1 = min(t1, Tb)
            first = g[b, :want_len[b]].reshape(want_len[b], m, 40)[:, 0]      # the first stacked frame of every row: frames 0, n, 2 n, ..
            rows = np.arange(want_len[b]) * n
            in_t = (rows >= t0) & (rows < t1)
            mel = first[:, f0:f1]
            tim = np.delete(first[in_t], np.s_[f0:f1], axis=1)
            assert mel.size and np.all(mel == mel.flat[0])                     # masked regions: one value, exactly
            e_f = abs(mel.flat[0] - fills[b, 1]) / abs(fills[b, 1])
            e_t = None
            if tim.size:
                assert np.all(tim == tim.flat[0])
                e_t = abs(tim.flat[0] - fills[b, 0]) / abs(fills[b, 0])
                assert e_t <= 1e-5
            print(f"LFR {m}/{n} utterance {b}: mel fill {mel.flat[0]:.6f} (ref {fills[b, 1]:.6f}, rel {e_f:.3g}), time fill rel err {e_t}")
            assert e_f <= 1e-5
            if (m, n) == (1, 1):                                               # outside the masks nothing changes
                keep = np.ones((Tb, 40), dtype=bool)
                keep[t0:t1] = False
                keep[:, f0:f1] = False
                assert np.array_equal(g[b, :Tb][keep], plain[b, :Tb].cpu().numpy()[keep])
        assert not g[0].any()


# ------------------------------------------------------------------------------------ 3. streamed == offline
def _stream(fe, wav, lens, plan):
    """plan: list of per-utterance (n_samples, final) lists, one entry per push.  -> rows per utterance, n_valid sums."""
    B = len(lens)
    pos, rows, tot = [0] * B, [[] for _ in range(B)], [0] * B
    for step in plan:
        ns = [s[0] for s in step]
        S = max(max(ns), 1)
        pcm = torch.zeros(B, S)
        for b in range(B):
            pcm[b, :ns[b]] = wav[b, pos[b]:pos[b] + ns[b]]
            pos[b] += ns[b]
        for feats, nv in fe.push_audio(pcm, ns, [s[1] for s in step]):
            assert feats.shape[:2] == (B, fe.C) and len(nv) == B
            for b in range(B):
                rows[b].append(feats[b, :nv[b]])
                tot[b] += nv[b]
                assert not feats[b, nv[b]:].any()
    assert pos == list(lens)
    return [torch.cat(r) if r else None for r in rows], tot


def _blocks(length, sizes):
    """(n, final) pushes that cut `length` samples into blocks of the given sizes (the last size repeats); final rides on the last block."""
    out, pos, i = [], 0, 0
    while pos < length:
        n = min(sizes[min(i, len(sizes) - 1)], length - pos)
        pos += n
        i += 1
        out.append((n, pos == length))
    return out or [(0, True)]


def _splits(length):
    rng = random.Random(length)
    plans = {"at_once": [(length, True)], "blocks_160": _blocks(length, [160]),
             "random": _blocks(length, [rng.randint(1, 3000) for _ in range(64)])}
    if length == 150:
        plans["blocks_7"] = _blocks(length, [7])
    for t in (2, 32):
        for d in (-1, 0, 1):
            k = 160 * t + 200 + d
            if k < length:
                plans[f"cut_{t}_{d:+d}"] = [(k, False), (length - k, True)]
    z = []
    for s in _blocks(length, [rng.randint(100, 900) for _ in range(64)]):      # zero-sample pushes in between, and final on its own
        z += [(s[0], False), (0, False)]
    plans["zeros_then_final"] = z + [(0, True)]
    return plans


def _offline(parser, wav, lens):
    if wav.shape[1] < 256:      # the offline kernel wants rows longer than half a window
        wav = np.pad(wav, ((0, 0), (0, 256 - wav.shape[1])))
    out, out_len = parser.parse_batch(torch.from_numpy(wav).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV))
    return out, out_len.tolist()


@pytest.mark.parametrize("length", [150, 201, 4000, 12345])
def test_streamed_features_equal_offline_bit_for_bit(stats40, length):
    from asr_chinese_e2e_amd.data_handler import StreamingFrontEnd
    parser = _parser(40, stats40, 4, 3)
    wav = (0.5 * np.random.RandomState(length).randn(1, length)).astype(np.float32)
    want, want_len = _offline(parser, wav, [length])
    assert want_len == [-(-CR.total_frames(length) // 3)]
    for name, plan in _splits(length).items():
        fe = StreamingFrontEnd(parser, 1, 4, sample_cap=1024 if name == "at_once" else 4096)      # at once: worked through in pieces of 512
        rows, tot = _stream(fe, torch.from_numpy(wav), [length], [[s] for s in plan])
        assert tot == want_len, (name, tot, want_len)
        assert torch.equal(rows[0], want[0, :want_len[0]]), name


def test_streamed_features_lock_step_batch_and_plain_stacking(stats40):
    from asr_chinese_e2e_amd.data_handler import StreamingFrontEnd
    lens = [150, 4000, 12345]
    wav = _waves(0)[1:]
    rng = random.Random(7)
    for m, n in ((4, 3), (1, 1)):
        parser = _parser(40, stats40, m, n)
        want, want_len = _offline(parser, wav, lens)
        # every utterance cut its own way: the shortest closes early, the others wait for one another's rows
        per = [_blocks(l, [rng.randint(1, 3000) for _ in range(64)]) for l in lens]
        per[1] = [(0, False)] * 3 + per[1]
        steps = max(len(p) for p in per)
        plan = [[p[i] if i < len(p) else (0, True) for p in per] for i in range(steps)]
        fe = StreamingFrontEnd(parser, 3, 4, sample_cap=2048)
        rows, tot = _stream(fe, torch.from_numpy(wav), lens, plan)
        assert tot == want_len
        for b in range(3):
            assert torch.equal(rows[b], want[b, :want_len[b]]), (m, n, b)
    with pytest.raises(ValueError, match="closed"):
        fe.push_audio(torch.zeros(3, 8), [0, 8, 0], [False] * 3)


def test_frame_ring_grows_behind_a_stalled_utterance_beside_a_finished_one(stats40):
    """Lock-step: utterance 0 (4000 samples: 26 frames, 9 rows, so its next row's first frame, 27, lies past its last one) closes and
    drains; utterance 1 then gets no audio for a long while, so no chunk can leave, and utterance 2 keeps receiving: its frames pile up
    and the frame rings are re-laid twice (64 -> 128 -> 256).  Every row must still equal the offline one."""
    from asr_chinese_e2e_amd.data_handler import StreamingFrontEnd
    lens = [4000, 12345, 30000]
    rng = np.random.RandomState(9)
    wav = np.zeros((3, 30000), dtype=np.float32)
    for b, l in enumerate(lens):
        wav[b, :l] = (0.5 * rng.randn(l)).astype(np.float32)
    parser = _parser(40, stats40, 4, 3)
    want, want_len = _offline(parser, wav, lens)
    fe = StreamingFrontEnd(parser, 3, 4, sample_cap=1024)
    cap0 = fe.fcap
    plan = [[(4000, True), (6500, False), (6500, False)]]                       # all three advance: utterance 0 drains
    plan += [[(0, True), (0, False), (1000, False)] for _ in range(23)]         # utterance 1 stalls the chunk, utterance 2 runs ahead
    plan += [[(0, True), (5845, True), (500, True)]]                            # the rest: everything drains
    rows, tot = _stream(fe, torch.from_numpy(wav), lens, plan)
    assert cap0 == 64 and fe.fcap == 256                                        # the rings were re-laid, twice
    assert tot == want_len
    for b in range(3):
        assert torch.equal(rows[b], want[b, :want_len[b]]), b
    # the limit: an utterance may not run ahead without bound, and a refused call changes nothing
    fe = StreamingFrontEnd(parser, 2, 4, sample_cap=1024, max_frames=100)
    x = torch.from_numpy(wav[1:, :12000])
    fe.push_audio(x, [0, 12000], [False, False])                                # 74 frames wait for utterance 0
    state = (list(fe.received), list(fe.next_frame), list(fe.next_row), fe.fcap)
    with pytest.raises(ValueError, match="lock-step"):
        fe.push_audio(x, [0, 12000], [False, False])
    assert state == (list(fe.received), list(fe.next_frame), list(fe.next_row), fe.fcap)
    last = np.zeros((2, 12345), dtype=np.float32)
    last[0], last[1, :345] = wav[1, :12345], wav[2, 12000:12345]
    got = fe.push_audio(torch.from_numpy(last), [12345, 345], [True, True])     # utterance 0 arrives: everything leaves
    want2, want2_len = _offline(parser, wav[2:, :12345], [12345])
    assert torch.equal(torch.cat([f[0, :nv[0]] for f, nv in got]), want[1, :want_len[1]])
    assert torch.equal(torch.cat([f[1, :nv[1]] for f, nv in got]), want2[0, :want2_len[0]])


# ------------------------------------------------------------------------------------ 4. end to end
def _model(d_in, C, dtype="fp32"):
    from oracle import ref_model as R
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    V = 30
    cfg = R.default_cfg(n_mels=d_in, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, ctc_weight=0.5)
    sd = R.init_state_dict(cfg, V, seed=11)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
    sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    M = Models.TransformerOffical
    mc = M.get_default_config()()
    d = dict(vars(cfg))
    d.pop("use_decoder", None)
    d.update(dtype=dtype, decoding_chunk_size=C, decoding_left_chunks=-1, cross_mask="wave_len")
    mc.fn_build(d)
    model = M(mc, Vocab.synthetic(V)).cuda().eval()
    model.load_state_dict(sd)
    return model


@pytest.fixture(scope="module")
def model4():
    return _model(160, 4)


def test_push_audio_equals_push_of_offline_features(model4, stats40):
    C = 4
    parser = _parser(40, stats40, 4, 3)
    lens = [4000, 12345]
    wav = _waves(0)[2:]
    want, want_len = _offline(parser, wav, lens)
    off = model4.stream(2)
    off_ids = []
    for c0 in range(0, max(want_len), C):
        x = want[:, c0:c0 + C]
        if x.shape[1] < C:
            x = torch.nn.functional.pad(x, (0, 0, 0, C - x.shape[1]))
        off_ids.append(off.push(x.contiguous(), [max(0, min(C, l - c0)) for l in want_len]))
    st = model4.stream(2, parser=parser)
    rng = random.Random(3)
    per = [_blocks(l, [rng.randint(1, 3000) for _ in range(64)]) for l in lens]
    pos, got_ids, total = [0, 0], [], [[], []]
    for i in range(max(len(p) for p in per)):
        step = [p[i] if i < len(p) else (0, True) for p in per]
        ns = [s[0] for s in step]
        pcm = torch.zeros(2, max(max(ns), 1))
        for b in range(2):
            pcm[b, :ns[b]] = torch.from_numpy(wav[b, pos[b]:pos[b] + ns[b]])
            pos[b] += ns[b]
        for nv, ids in st.push_audio_chunks(pcm if i % 2 else pcm.to(DEV), ns, [s[1] for s in step]):      # host and device blocks alike
            got_ids.append(ids)
            for b in range(2):
                total[b] += ids[b]
    assert got_ids == off_ids and any(any(i) for i in got_ids)
    enc, enc_len = st.encoder_output()
    enc_off, off_len = off.encoder_output()
    assert enc_len.tolist() == off_len.tolist() == want_len and torch.equal(enc, enc_off)
    a, b_ = st.finish(beam_size=3), off.finish(beam_size=3)
    assert [r["ids"] for r in a] == [r["ids"] for r in b_] and [r["score"] for r in a] == [r["score"] for r in b_]
    assert [r["text"] for r in a] == [r["text"] for r in b_]
    # push_audio is the same loop, ids joined per utterance
    st2 = model4.stream(2, parser=parser)
    ids2 = st2.push_audio(torch.from_numpy(wav), lens, [True, True])
    assert ids2 == total


# ------------------------------------------------------------------------------------ 5. errors
def test_push_audio_errors_and_plain_push(model4, stats40):
    from asr_chinese_e2e_amd.data_handler import AudioParser
    with pytest.raises(ValueError, match="global"):
        model4.stream(1, parser=AudioParser(n_mels=40, device=DEV)).push_audio(torch.zeros(1, 400), [400], [False])
    with pytest.raises(ValueError, match="parser"):
        model4.stream(1).push_audio(torch.zeros(1, 400), [400], [False])
    st = model4.stream(1, parser=_parser(40, stats40, 4, 3))
    st.push_audio(torch.randn(1, 3000), [3000], [True])
    with pytest.raises(ValueError, match="closed"):
        st.push_audio(torch.zeros(1, 10), [10], [False])
    assert st.push_audio(torch.zeros(1, 10), [0], [True]) == [[]]       # closing again, with nothing, is no audio
    plain = model4.stream(2)                                            # without a parser: the stream of before
    ids = plain.push(torch.randn(2, 4, 160, device=DEV), [4, 2])
    assert len(ids) == 2 and plain.offset == 4 and plain.ended == [False, True]
