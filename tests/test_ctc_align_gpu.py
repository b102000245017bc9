"""CTC forced alignment on the device (asr_ctc_align / kernels.ctc_align / model.ctc_align / model.transcribe / transcribe.py) against
the fp64 Viterbi restatement of tests/test_ctc_align_cpu.py (itself pinned by brute-force enumeration)."""
import json
import math
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import ROOT, golden_model_case  # noqa: E402
from tests.test_ctc_align_cpu import align_outputs, collapse, log_softmax, rescore, viterbi_ref  # noqa: E402

DEV = "cuda"


def _logits(B, T, V, dtype, ld=None, seed=0, scale=2.0, want_logp=True):
    """(B, T, V) logits on the device, dense or as rows `ld` elements apart; also their fp64 log-softmax as the kernel sees them."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = (torch.randn(B * T, ld or V, generator=g, device=DEV) * scale).to(dtype)
    logits = buf[:, :V].view(B, T, V)
    logp = log_softmax(logits.double().cpu().numpy()) if want_logp else None
    return logits, logp


def _labels(lists, Lmax=None):
    Lmax = max([len(l) for l in lists] + [0]) if Lmax is None else Lmax
    lab = torch.zeros(len(lists), Lmax, dtype=torch.int32)
    for b, l in enumerate(lists):
        lab[b, : len(l)] = torch.tensor(l, dtype=torch.int32)
    return lab.to(DEV), torch.tensor([len(l) for l in lists], dtype=torch.int32, device=DEV)


def _run(logits, in_len, lists, Lmax=None):
    from asr_chinese_e2e_amd import kernels as K
    lab, lab_len = _labels(lists, Lmax)
    il = torch.tensor(in_len, dtype=torch.int32, device=DEV)
    path, spans, tlp, score = K.ctc_align(logits, il, lab, lab_len)
    torch.cuda.synchronize()
    return path.cpu().numpy(), spans.cpu().numpy(), tlp.cpu().numpy(), score.cpu().numpy()


def _random_labels(rng, L, V, repeats=True):
    lab = list(rng.integers(1, V, L))
    if repeats and L >= 3:
        lab[1] = lab[0]                 # an adjacent repeat: needs a blank in between
    return [int(x) for x in lab]


def _plant(rng, T, labels, V, margin, base):
    """A valid alignment of `labels` over T frames and logits that favour it by `margin` nats per frame."""
    L = len(labels)
    reps = sum(a == b for a, b in zip(labels, labels[1:]))
    extra = T - L - reps
    path = []
    for i, c in enumerate(labels):
        if i > 0 and labels[i - 1] == c:
            path.append(0)
        n = int(rng.integers(0, max(1, extra // max(L, 1)) + 1)) if extra > 0 else 0
        n = min(n, extra)
        extra -= n
        path += [0] * n + [c]
    path += [0] * (T - len(path))
    x = base.copy()
    for t, c in enumerate(path):
        x[t, c] = x[t].max() + margin
    return x, path


def _check_against_oracle(logits, logp, in_len, lists, Lmax, planted=None):
    path, spans, tlp, score = _run(logits, in_len, lists, Lmax)
    T = logits.shape[1]
    for b, labels in enumerate(lists):
        Tb = in_len[b]
        wp, ws, wt, wsc = align_outputs(logp[b, :Tb], labels, T, Lmax=Lmax)
        if wsc == -math.inf:
            assert score[b] == -math.inf and (spans[b] == -1).all(), b
            assert (path[b, :Tb] == 0).all() and (path[b, Tb:] == -1).all(), b
            continue
        assert abs(score[b] - wsc) <= 1e-5 * max(1.0, abs(wsc)), (b, score[b], wsc)
        assert (path[b, Tb:] == -1).all()
        assert collapse(path[b, :Tb].tolist()) == labels, b
        # the kernel's path, re-scored in fp64, is a best path
        assert abs(rescore(logp[b, :Tb], path[b, :Tb]) - wsc) <= 1e-5 * max(1.0, abs(wsc)), b
        if planted is not None:
            assert path[b, :Tb].tolist() == planted[b], b
            assert (spans[b] == ws).all(), b
            assert np.allclose(tlp[b], wt, rtol=1e-5, atol=1e-4), b
        assert (spans[b, len(labels):] == -1).all() and (tlp[b, len(labels):] == 0).all()
    return path, spans, tlp, score


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("T,V,Lmax", [(60, 30, 12), (300, 40, 100), (500, 24, 200), (2000, 64, 60)])
def test_ctc_align_random_logits_match_oracle(dtype, padded, T, V, Lmax):
    """Random logits: score and the fp64 re-scoring of the kernel's path equal the oracle's best.  Lmax 12 / 60 / 100 / 200 cover
    one, two and four registers per lane (W = 32 .. 256); T = 2000 and (500, Lmax 200) keep the back-pointers in the workspace."""
    rng = np.random.default_rng(T + Lmax)
    B = 3
    ld = (V + 63) // 64 * 64 + 64 if padded else None
    logits, logp = _logits(B, T, V, dtype, ld, seed=T)
    in_len = [T, T - 7, max(1, T // 3)]
    lists = [_random_labels(rng, min(Lmax, in_len[b] // 2), V) for b in range(B)]
    lists[2] = lists[2][: max(0, min(len(lists[2]), Lmax - 1))]
    _check_against_oracle(logits, logp, in_len, lists, Lmax)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("T,L", [(40, 9), (400, 150), (2000, 40)])
def test_ctc_align_planted_alignment_exact(dtype, padded, T, L):
    """Logits that favour a planted alignment by >= 1 nat per frame: path, spans and token_logp equal the oracle exactly."""
    rng = np.random.default_rng(L)
    B, V = 2, 32
    base = rng.normal(0, 1.0, (B, T, V))
    lists, planted, x = [], [], np.zeros((B, T, V))
    for b in range(B):
        Tb = T - 3 * b
        labels = _random_labels(rng, L - b, V)
        x[b] = base[b]
        x[b, :Tb], p = _plant(rng, Tb, labels, V, 1.5, base[b, :Tb])
        lists.append(labels)
        planted.append(p)
    ld = ((V + 63) // 64) * 64 if padded else V
    buf = torch.zeros(B * T, ld, dtype=torch.float64)
    buf[:, :V] = torch.from_numpy(x.reshape(B * T, V))
    buf = buf.to(dtype).to(DEV)
    logits = buf[:, :V].view(B, T, V)
    logp = log_softmax(logits.double().cpu().numpy())
    _check_against_oracle(logits, logp, [T, T - 3], lists, L, planted=planted)


def test_ctc_align_edge_cases():
    """One-frame utterances, L = 0, in_len = 0, infeasible repeats, and exact ties (uniform logits)."""
    T, V = 8, 6
    logits, logp = _logits(6, T, V, torch.float32, seed=3)
    in_len = [1, 1, 0, 0, 3, 5]
    lists = [[2], [], [], [1], [4, 4], [1, 2]]
    path, spans, tlp, score = _check_against_oracle(logits, logp, in_len, lists, 2)
    assert score[2] == 0.0 and (path[2] == -1).all()                      # in_len = 0, L = 0
    assert score[3] == -math.inf and (path[3] == -1).all()                # in_len = 0, L > 0
    assert score[4] > -math.inf                                           # 'aa' in 3 frames: the only path
    assert path[4, :3].tolist() == [4, 0, 4]
    # infeasible: 'aa' in 2 frames
    _, spans2, tlp2, score2 = _run(logits[:1], [2], [[3, 3]], 3)
    assert score2[0] == -math.inf and (spans2 == -1).all() and tlp2[0, :2].tolist() == [-math.inf] * 2 and tlp2[0, 2] == 0
    # uniform posteriors: every alignment ties, the tie rules decide (labels as early as possible)
    uni = torch.zeros(2, 7, 5, device=DEV)
    path, _, _, _ = _run(uni, [7, 7], [[1, 2, 3], [1, 1]], 3)
    assert path[0].tolist() == [1, 2, 3, 0, 0, 0, 0]
    assert path[1].tolist() == [1, 0, 1, 0, 0, 0, 0]


def test_ctc_align_full_size_invariants():
    """configs[2] shapes (B = 32, T = 500, V = 4232, bf16, engine row padding): the path spells the labels, spans are ordered and
    inside the utterance, the best path is at most the total probability, token_logp + blank frames = score, bit-identical reruns."""
    from asr_chinese_e2e_amd import kernels as K
    B, T, V = 32, 500, 4232
    ld = (V + 63) // 64 * 64
    rng = np.random.default_rng(7)
    logits, _ = _logits(B, T, V, torch.bfloat16, ld, seed=11, scale=3.0, want_logp=False)
    in_len = [int(x) for x in rng.integers(300, T + 1, B)]
    in_len[0] = T
    lists = [_random_labels(rng, int(rng.integers(15, 30)), V) for _ in range(B)]
    lab, lab_len = _labels(lists)
    il = torch.tensor(in_len, dtype=torch.int32, device=DEV)
    out1 = [t.clone() for t in K.ctc_align(logits, il, lab, lab_len)]
    out2 = K.ctc_align(logits, il, lab, lab_len)
    for a, b in zip(out1, out2):
        assert torch.equal(a, b)
    ws = K.Workspace(DEV)
    nll, _ = K.ctc_fwd_bwd(logits, il, lab, lab_len, ws, want_grad=False)
    path, spans, tlp, score = (t.cpu().numpy() for t in out1)
    nll = nll.cpu().numpy()
    lp_blank = torch.log_softmax(logits.double(), -1)[..., 0].cpu().numpy()
    for b in range(B):
        Tb, L = in_len[b], len(lists[b])
        assert collapse(path[b, :Tb].tolist()) == lists[b], b
        assert (path[b, Tb:] == -1).all()
        sp = spans[b, :L]
        assert (sp[:, 0] <= sp[:, 1]).all() and (sp[1:, 0] > sp[:-1, 1]).all() and sp[0, 0] >= 0 and sp[-1, 1] < Tb, b
        assert score[b] <= -nll[b] + 1e-5 * abs(nll[b]), (b, score[b], nll[b])
        total = float(tlp[b, :L].astype(np.float64).sum() + lp_blank[b, :Tb][path[b, :Tb] == 0].sum())
        assert abs(total - score[b]) <= 1e-4 * abs(score[b]), (b, total, score[b])


# ---------------------------------------------------------------------------------------------------------- model level
def _golden_model(kind):
    """The small golden config with a CTC head (seeded, scaled up for peaky posteriors): 'ctc' = TransformerCTC, 'joint' = joint
    CTC / attention, 'att' = attention only."""
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    from asr_chinese_e2e_amd.Utils import Pack
    cfg, sd, batch, z = golden_model_case("model_small_ragged.npz")
    V = int(z["cfg/V"])
    g = torch.Generator().manual_seed(23)
    sd = dict(sd)
    sd["ctc_lo.weight"] = torch.randn(V, cfg.d_model, generator=g) * 0.8
    sd["ctc_lo.bias"] = torch.randn(V, generator=g) * 0.5
    M = Models.TransformerCTC if kind == "ctc" else Models.TransformerOffical
    mc = M.get_default_config()()
    d = dict(vars(cfg))
    d.pop("use_decoder", None)
    d.update(dtype="fp32", ctc_weight=0.0 if kind == "att" else 0.3)
    mc.fn_build(d)
    model = M(mc, Vocab.synthetic(V))
    keys = set(model.state_dict())
    model.load_state_dict({k: v for k, v in sd.items() if k in keys})
    model = model.cuda().eval()
    full = Pack({k: v.to(DEV) for k, v in batch.items()})
    audio = Pack(wave=full.wave, wave_len=full.wave_len)
    return model, full, audio, batch


@pytest.mark.parametrize("kind", ["ctc", "joint"])
def test_model_ctc_align_matches_oracle(kind):
    from asr_chinese_e2e_amd import kernels as K
    model, full, audio, batch = _golden_model(kind)
    got = model.ctc_align(full)
    with torch.no_grad():
        logits = model.forward(full).ctc_logits
    logp = log_softmax(logits.double().cpu().numpy())
    prep = K.dec_preprocess(full.tgt_for_input.contiguous(), 2, 3)
    lab, lens = prep[2].cpu(), prep[4].cpu().tolist()
    d = model.frame_seconds()
    assert abs(d - 0.03) < 1e-12
    for b in range(logits.shape[0]):
        labels = lab[b, : lens[b]].tolist()
        Tb = int(batch["wave_len"][b])
        wsc, states = viterbi_ref(logp[b, :Tb], labels)
        r = got[b]
        assert [t["id"] for t in r["tokens"]] == labels
        if states is None:
            assert r["score"] == -math.inf and all(t["start_frame"] is None for t in r["tokens"])
            continue
        assert abs(r["score"] - wsc) <= 1e-5 * max(1.0, abs(wsc)), (b, r["score"], wsc)
        _, ws, wt, _ = align_outputs(logp[b, :Tb], labels, Tb)
        for i, t in enumerate(r["tokens"]):
            assert (t["start_frame"], t["end_frame"]) == (ws[i, 0], ws[i, 1]), (b, i)
            assert abs(t["start_s"] - ws[i, 0] * d) < 1e-9 and abs(t["end_s"] - (ws[i, 1] + 1) * d) < 1e-9
            assert abs(t["logp"] - wt[i]) <= 1e-4 * max(1.0, abs(wt[i]))
            assert t["token"] == model.vocab._id2token[t["id"]]
    # explicit labels, audio-only batch: same result
    again = model.ctc_align(audio, labels=[lab[b, : lens[b]].tolist() for b in range(len(lens))])
    assert [[(t["start_frame"], t["end_frame"]) for t in r["tokens"]] for r in again] == \
        [[(t["start_frame"], t["end_frame"]) for t in r["tokens"]] for r in got]


@pytest.mark.parametrize("kind", ["ctc", "joint"])
def test_transcribe_audio_only_matches_decoders(kind):
    model, full, audio, batch = _golden_model(kind)
    got = model.transcribe(audio, beam_size=4)
    if kind == "ctc":
        want = [h[0]["yseq"] for h in model.ctc_prefix_beam_search(full, beam_size=4, nbest=1)]
    else:
        want = [h[0]["yseq"][1:-1] if h[0]["yseq"][-1] == 3 else h[0]["yseq"][1:]
                for h in model.beam_search(full, beam_size=4, nbest=1, ctc_weight=0.3)]
    assert [r["ids"] for r in got] == want
    id2tok = model.vocab._id2token
    for r in got:
        assert r["text"] == "".join(id2tok[x] for x in r["ids"] if x not in (0, 2, 3))
        assert [t["id"] for t in r["tokens"]] == r["ids"]
        times = [(t["start_s"], t["end_s"]) for t in r["tokens"] if t["start_s"] is not None]
        assert all(a < b for a, b in times) and all(times[i][1] <= times[i + 1][0] + 1e-9 for i in range(len(times) - 1))
    # the audio-only forward pass: encoder and CTC head only
    with torch.no_grad():
        out = model.forward(audio)
    assert out.pred is None and out.ctc_logits is not None


def test_transcribe_attention_only_refuses_timestamps():
    model, full, audio, batch = _golden_model("att")
    with pytest.raises(ValueError):
        model.transcribe(audio, timestamps=True)
    with pytest.raises(RuntimeError):
        model.ctc_align(full)
    got = model.transcribe(audio, beam_size=3, timestamps=False)
    want = model.beam_search(full, beam_size=3, nbest=1)
    assert [r["ids"] for r in got] == [h[0]["yseq"][1:-1] if h[0]["yseq"][-1] == 3 else h[0]["yseq"][1:] for h in want]


# ---------------------------------------------------------------------------------------------------------- CLI
def _write_wav(path, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(16000 * seconds)
    t = np.arange(n) / 16000.0
    x = 0.3 * np.sin(2 * np.pi * 220 * t) * (1 + np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.normal(size=n)
    pcm = (np.clip(x, -1, 1) * 32000).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.tobytes())


def test_transcribe_cli(tmp_path):
    from asr_chinese_e2e_amd.data_handler import Vocab
    sys.path.insert(0, ROOT)
    from train import TrainConfig, get_model_class
    flags = dict(model_name="TransformerCTC", d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=1, dtype="fp32")
    config = TrainConfig()
    config.fn_build(flags)
    Model, MC = get_model_class(config.model_name)
    config.fn_combine(MC())
    config.fn_build(flags)
    vocab = Vocab.synthetic(40)
    vocab.save(str(tmp_path / "vocab.t"))
    torch.manual_seed(0)
    Model(config, vocab).save(str(tmp_path / "m.model"))
    durs = [1.3, 0.7]
    wavs = [tmp_path / "a.wav", tmp_path / "b.wav"]
    for i, (p, s) in enumerate(zip(wavs, durs)):
        _write_wav(p, s, i)
    cmd = [sys.executable, os.path.join(ROOT, "transcribe.py")] + [f"--{k}={v}" for k, v in flags.items()] + \
        [f"--ckpt={tmp_path / 'm.model'}", f"--vocab_path={tmp_path / 'vocab.t'}", "--wavs=" + ",".join(map(str, wavs)), "--beam_size=3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for line, p, dur in zip(lines, wavs, durs):
        assert line["file"] == str(p) and abs(line["duration_s"] - dur) < 1e-3
        assert isinstance(line["text"], str) and [t["id"] for t in line["tokens"]] == line["ids"]
        last = 0.0
        for t in line["tokens"]:
            assert t["start_s"] is not None and last <= t["start_s"] <= t["end_s"] <= dur + 1e-9
            last = t["end_s"]
    # a missing checkpoint is an error
    bad = [c if not c.startswith("--ckpt=") else f"--ckpt={tmp_path / 'none.model'}" for c in cmd]
    r = subprocess.run(bad, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode != 0 and "checkpoint not found" in r.stderr
