"""asr_ctc_align_long on the device against its definition (tests/align_long_ref.py), bit for bit: score (fp64), path, spans and the
token sums / extremes - no tolerance anywhere in the kernel tests.  Then against the existing one-wave kernel (asr_ctc_align) on lattices
whose margin is asserted first, and end to end through model.align_long and align.py.

Which instantiation (pairs per thread P, workgroup of 64 / 128 / 256 / 1024 threads) a label count reaches:
    L = 1, 2, 63, 64        P = 1 (one wave, no barrier in the frame loop); 63 / 64 / 65 straddle the wave and the P = 1 | 2 threshold
    L = 65, 255, 256        P = 2 (two waves); 256 | 257 is the P = 2 | 4 threshold
    L = 257, 1023, 1024     P = 4 (four waves); 300 (the V = 4232 case) too
    L = 1025, 8192          P = 8 (sixteen waves, three of them with pairs at 1025; every register pair used at 8192, the limit)"""
import functools
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import align_long_ref as A  # noqa: E402

DEV = "cuda"


def classes(L):
    return 1 if L <= 64 else 2 if L <= 256 else 4 if L <= 1024 else 8


def _labels(rng, L, V, repeats=True):
    lab = rng.randint(1, V, L)
    if repeats and L >= 3:
        lab[1] = lab[0]             # at least one adjacent repeat: it needs a blank in between
    return lab


@functools.lru_cache(maxsize=None)
def case(T, L, V, seed, few_repeats=False, extra=None):
    """(rows (T, V) float32, labels); extra: T = L + repeats + extra instead of the given T.  few_repeats: the draws are repaired so that
    no token repeats its neighbour, then every 1000th is made to."""
    rng = np.random.RandomState(seed)
    lab = _labels(rng, L, V)
    if few_repeats:
        for i in range(1, L):
            if lab[i] == lab[i - 1]:
                lab[i] = 1 + lab[i] % (V - 1)
        lab[1000::1000] = lab[999::1000][:len(lab[1000::1000])]
    if extra is not None:
        T = L + A.repeats(lab) + extra
    rows = (rng.normal(0.0, 2.0, (T, V))).astype(np.float32)
    return rows, lab


def as_dtype(rows, dtype):
    """The rows as the device will hold them, back in float32 (bf16 -> float32 is exact)."""
    return torch.from_numpy(np.ascontiguousarray(rows)).to(dtype).float().numpy()


def run(recs, dtype=torch.float32, ld=None, blank=0):
    """recs: [(rows float32 as the device holds them, lse, labels)] -> per recording dict(score, path, spans, tok) from ONE launch."""
    from asr_chinese_e2e_amd import kernels as K
    V = recs[0][0].shape[1]
    Ts, Ls = [r[0].shape[0] for r in recs], [len(r[2]) for r in recs]
    buf = torch.zeros(max(sum(Ts), 1), ld or V, dtype=dtype, device=DEV)
    if sum(Ts):
        buf[:sum(Ts), :V] = torch.from_numpy(np.concatenate([r[0] for r in recs])).to(DEV).to(dtype)
    lse = torch.from_numpy(np.concatenate([np.asarray(r[1], np.float32) for r in recs])).to(DEV)
    ro, lo = np.concatenate(([0], np.cumsum(Ts))), np.concatenate(([0], np.cumsum(Ls)))
    lab = np.concatenate([np.asarray(r[2], np.int64).reshape(-1) for r in recs])
    path, spans, tok, score = K.ctc_align_long(buf[:sum(Ts), :V], lse, ro, lab, lo, blank=blank)
    torch.cuda.synchronize()
    path, spans, tok, score = path.cpu().numpy(), spans.cpu().numpy(), tok.cpu().numpy(), score.cpu().numpy()
    return [dict(score=score[r], path=path[ro[r]:ro[r + 1]], spans=spans[lo[r]:lo[r + 1]], tok=tok[lo[r]:lo[r + 1]]) for r in range(len(recs))]


def same_bits(got, want, what=""):
    assert np.float64(got["score"]).view(np.int64) == np.float64(want["score"]).view(np.int64), (what, got["score"], want["score"])
    assert np.array_equal(got["path"], want["path"]), what
    assert np.array_equal(got["spans"], want["spans"]), what
    assert np.array_equal(np.ascontiguousarray(got["tok"], np.float32).view(np.uint32), np.ascontiguousarray(want["tok"], np.float32).view(np.uint32)), what


def check(rows, lab, dtype=torch.float32, ld=None, blank=0):
    x = as_dtype(rows, dtype)
    lse = A.lse_of(x) if x.shape[0] else np.zeros(0, np.float32)
    want = A.align(x, lse, lab, blank)
    got = run([(x, lse, lab)], dtype, ld, blank)[0]
    same_bits(got, want, (x.shape, len(lab), dtype, ld))
    return got, want


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_kernel_is_the_definition(L):
    """T = L + repeats + 37, V = 12; f32 and bf16 rows, ld = V and a padded ld."""
    rows, lab = case(0, L, 12, 100 + L, extra=37)
    assert classes(L) == {1: 1, 2: 1, 63: 1, 64: 1, 65: 2, 255: 2, 256: 2, 257: 4, 1023: 4, 1024: 4, 1025: 8}[L]
    for dtype, ld in ((torch.float32, None), (torch.float32, 24), (torch.bfloat16, None), (torch.bfloat16, 16)):
        got, _ = check(rows, lab, dtype, ld)
        assert np.isfinite(got["score"]) and (got["spans"] >= 0).all()


def test_kernel_at_the_limit():
    """L = 8192 (P = 8, every pair of all 1024 threads), T = L + repeats + 300, V = 16, uniform draws."""
    rows, lab = case(0, 8192, 16, 7, extra=300)
    got, _ = check(rows, lab, torch.float32, None)
    assert np.isfinite(got["score"])


def test_kernel_at_the_limit_few_repeats():
    """L = 8192 with labels repaired so that adjacent repeats are few (counted), T = L + repeats + 8, bf16 rows in a padded buffer."""
    rows, lab = case(0, 8192, 16, 8, few_repeats=True, extra=8)
    reps = A.repeats(lab)
    assert 8 <= reps <= 16 and rows.shape[0] == 8192 + reps + 8
    got, _ = check(rows, lab, torch.bfloat16, 24)
    assert np.isfinite(got["score"])


def test_empty_sides_and_feasibility_edge():
    rows, lab = case(9, 0, 12, 3)
    got, _ = check(rows, lab)                                                   # L = 0: every frame blank, the score their sum
    assert np.isfinite(got["score"]) and (got["path"] == -1).all()
    got, _ = check(np.zeros((0, 12), np.float32), np.zeros(0, np.int64))       # T = 0, L = 0
    assert got["score"] == 0.0
    got, _ = check(np.zeros((0, 12), np.float32), np.array([3, 4, 4]))         # T = 0, L = 3
    assert got["score"] == -np.inf and (got["spans"] == -1).all()
    for L in (5, 70, 300):
        rows, lab = case(0, L, 12, 40 + L, extra=0)                            # T exactly at feasibility: no frame to spare
        got, _ = check(rows, lab)
        assert np.isfinite(got["score"]) and (got["spans"][:, 0] == got["spans"][:, 1]).all()
        got, _ = check(rows[:-1], lab)                                          # one below
        assert got["score"] == -np.inf and (got["spans"] == -1).all() and (got["path"] == -1).all() and np.isneginf(got["tok"]).all()


def test_full_vocabulary():
    rows, lab = case(700, 300, 4232, 11)
    check(rows, lab, torch.bfloat16, None)
    lab2 = lab - 1                                                             # another blank id: labels in [0, V - 1)
    check(rows, lab2, torch.float32, 4240, blank=4231)


def test_ragged_launch_and_determinism():
    """R = 3: a long recording (P = 4), an infeasible one (P = 1) and an empty one share a launch; each has the bits it has alone, and a
    second run gives the same bits."""
    recs = []
    for (T, L, seed) in ((900, 600, 21), (6, 9, 22), (0, 0, 23), (300, 70, 24)):
        rows, lab = case(T, L, 12, seed)
        recs.append((rows, A.lse_of(rows) if T else np.zeros(0, np.float32), lab))
    alone = [run([r])[0] for r in recs]
    together, again = run(recs), run(recs)
    for r, (a, b, c) in enumerate(zip(alone, together, again)):
        same_bits(b, a, r)
        same_bits(c, a, r)
        same_bits(a, A.align(*recs[r]), r)
    assert np.isfinite(alone[0]["score"]) and alone[1]["score"] == -np.inf and alone[2]["score"] == 0.0


def test_ties_and_minus_infinity():
    lab = _labels(np.random.RandomState(5), 70, 12)
    got, _ = check(np.zeros((200, 12), np.float32), lab)                       # all-equal rows: every cell a tie
    assert np.isfinite(got["score"])
    rows, lab = case(400, 130, 12, 31)
    rows = rows.copy()
    rng = np.random.RandomState(32)
    rows[rng.uniform(size=rows.shape) < 0.3] = -np.inf
    rows[:, 0] = 0.0                                                           # the blank stays finite: no row is -inf throughout
    for dtype in (torch.float32, torch.bfloat16):
        got, want = check(rows, lab, dtype)
        assert not np.isnan(got["score"]) and not np.isnan(got["tok"]).any()


@pytest.mark.parametrize("T,L,V,peak,seed", [(60, 20, 12, 3.0, 0), (300, 100, 12, 4.0, 1), (512, 255, 16, 4.0, 2)])
def test_against_the_one_wave_kernel(T, L, V, peak, seed):
    """Path and spans equal asr_ctc_align's on peaky lattices whose margin (checked first) is far above what the two domains can differ
    by.  The scores: the old kernel takes its log-softmax in fp64 and reports f32; the new one sums emissions made of an f32 lse (within
    2^-24 |lse| of the fp64 value) and one f32 subtraction (within 2^-24 |lp|) - the bound below is T of those plus half an f32 ulp of
    the score for the old kernel's own rounding."""
    from asr_chinese_e2e_amd import kernels as K
    rows, lse, lab = A.peaky_case(T, L, V, peak, seed)
    want = A.align(rows, lse, lab, want_margin=True)
    assert want["margin"] > 1e-6
    got = run([(rows, lse, lab)])[0]
    same_bits(got, want)
    logits = torch.from_numpy(rows).to(DEV).view(1, T, V)
    il, ll = torch.tensor([T], dtype=torch.int32, device=DEV), torch.tensor([L], dtype=torch.int32, device=DEV)
    path, spans, tlp, score = K.ctc_align(logits, il, torch.from_numpy(lab.astype(np.int32)).to(DEV).view(1, L), ll)
    path, spans, score = path.cpu().numpy()[0], spans.cpu().numpy()[0], float(score.cpu()[0])
    assert np.array_equal(spans, got["spans"])
    assert np.array_equal(path, np.where(got["path"] >= 0, lab[np.maximum(got["path"], 0)], 0))
    lp = A.emissions(rows, lse)
    bound = T * 2.0 ** -24 * float(np.abs(lp).max() + np.abs(lse).max()) + 0.5 * float(np.spacing(np.float32(abs(score))))
    assert abs(score - got["score"]) <= bound, (score, got["score"], bound)


# ------------------------------------------------------------------------------------ end to end
def _model(dtype):
    """The tiny joint model of tests/test_vad_gpu.py (a peaky CTC head, so the CTC search spells tokens), in fp32 or bf16."""
    from oracle import ref_model as RM
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    V = 30
    cfg = RM.default_cfg(n_mels=320, lfr_m=1, d_model=64, hidden_size=64 if dtype == "bf16" else 16, num_head=2 if dtype == "bf16" else 4, ff_size=128,
                         layer_num=2, ctc_weight=0.5)
    sd = RM.init_state_dict(cfg, V, seed=11)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
    sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    g = torch.Generator().manual_seed(23)
    sd["ctc_lo.weight"] = torch.randn(V, cfg.d_model, generator=g) * 0.8
    sd["ctc_lo.bias"] = torch.randn(V, generator=g) * 0.5
    sd["ctc_lo.bias"][[2, 3]] = -30.0
    M = Models.TransformerOffical
    mc = M.get_default_config()()
    d = dict(vars(cfg))
    d.pop("use_decoder", None)
    d.update(dtype=dtype, cross_mask="wave_len")
    mc.fn_build(d)
    model = M(mc, Vocab.synthetic(V)).cuda().eval()
    model.load_state_dict(sd)
    return model


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def long_setup(request):
    from asr_chinese_e2e_amd.data_handler import AudioParser
    from tests import vad_cases as C
    model = _model(request.param)
    parser = AudioParser(n_mels=80, lfr_m=4, lfr_n=3, device=DEV, frontend="kaldi")
    x = C.long_case()
    wav = torch.from_numpy(x[None]).to(DEV)
    tr = model.transcribe_long(parser, wav, [len(x)], batch_size=2, beam_size=3, joint="ctc_rescore", **C.LONG_OPTS)[0]
    return model, parser, x, wav, tr, C


def host_rows(model, parser, x, segs, batch_size):
    """The recording's concatenated CTC rows and lse as align_long lays them out, built batch by batch on the host side of the kernels:
    (rows (T, V) float32, lse (T,) float32, rows per segment)."""
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.Utils import Pack
    rows, lse, counts = [], [], []
    for i in range(0, len(segs), batch_size):
        part = segs[i:i + batch_size]
        S = max(1, max(b - a for a, b in part))
        wav = np.zeros((len(part), S), dtype=np.float32)
        for r, (a, b) in enumerate(part):
            wav[r, :b - a] = x[a:b]
        feats, flen = parser.parse_batch(torch.from_numpy(wav).cuda(), torch.tensor([b - a for a, b in part], dtype=torch.int32).cuda())
        logits = model._ctc_logits(Pack(wave=feats, wave_len=flen))
        _, _, _, l, _ = K.ctc_frame_stats(logits, flen.to(torch.int32), 0)
        for r, n in enumerate(flen.tolist()):
            rows.append(logits[r, :n].float().cpu().numpy())
            lse.append(l[r, :n].cpu().numpy())
            counts.append(int(n))
    return np.concatenate(rows), np.concatenate(lse), counts


def test_align_long_end_to_end(long_setup):
    """The 12 s, five-burst recording; the transcript is transcribe_long's own ids as two lines.  Tokens and score are the definition's on
    the same concatenated rows and lse, bit for bit; the segments are transcribe_long's; lines enclose their tokens; a transcript one
    token too long for the frames is infeasible with None times."""
    model, parser, x, wav, tr, C = long_setup
    ids = [i for i in tr["ids"] if i != 0]
    assert len(tr["segments"]) == C.LONG_SEGMENTS and len(ids) >= 4
    h = len(ids) // 2
    res = model.align_long(parser, wav, [len(x)], [[ids[:h], ids[h:]]], batch_size=2, **C.LONG_OPTS)
    assert len(res) == 1
    res = res[0]
    assert res["segments"] == [(s["start_s"], s["end_s"]) for s in tr["segments"]] and res["duration_s"] == C.LONG_SECONDS
    segs = [(s["start_sample"], int(round(s["end_s"] * 16000))) for s in tr["segments"]]
    rows, lse, counts = host_rows(model, parser, x, segs, 2)
    want = A.align(rows, lse, ids)
    assert res["frames"] == rows.shape[0] == sum(counts) and np.isfinite(want["score"])
    assert np.float64(res["score"]).view(np.int64) == np.float64(want["score"]).view(np.int64)
    d, first = model.frame_seconds(), np.concatenate(([0], np.cumsum(counts)))
    assert [t["id"] for t in res["tokens"]] == ids and [t["line"] for t in res["tokens"]] == [0] * h + [1] * (len(ids) - h)
    for i, t in enumerate(res["tokens"]):
        a, b = (int(v) for v in want["spans"][i])
        sm, mx, mn = (float(v) for v in want["tok"][i])
        assert (t["start_frame"], t["end_frame"], t["logp"]) == (a, b, sm)
        assert t["measures"] == {"post_max": math.exp(mx), "post_min": math.exp(mn), "post_mean": math.exp(sm / (b - a + 1))} and t["confidence"] == t["measures"]["post_mean"]
        sa, sb = int(np.searchsorted(first, a, side="right")) - 1, int(np.searchsorted(first, b, side="right")) - 1
        assert t["segment"] == sa and t["start_s"] == segs[sa][0] / 16000.0 + (a - first[sa]) * d and t["end_s"] == segs[sb][0] / 16000.0 + (b - first[sb] + 1) * d
    at = 0
    for l, want_ids in zip(res["lines"], (ids[:h], ids[h:])):
        mine = res["tokens"][at:at + len(want_ids)]
        at += len(want_ids)
        assert l["ids"] == want_ids and l["start_s"] <= min(t["start_s"] for t in mine) and l["end_s"] >= max(t["end_s"] for t in mine)
        assert l["frames"] == sum(t["end_frame"] - t["start_frame"] + 1 for t in mine) and l["confidence"] == math.exp(l["logp"] / l["frames"])
    # one token more than the frames can hold (no adjacent repeats: exactly T tokens fit)
    T = rows.shape[0]
    fits, over = [4 + (i % 2) for i in range(T)], [4 + (i % 2) for i in range(T + 1)]
    ok, bad = model.align_long(parser, torch.cat([wav, wav]), [len(x), len(x)], [[fits], [over]], batch_size=2, **C.LONG_OPTS)
    assert np.isfinite(ok["score"]) and all(t["start_frame"] == t["end_frame"] == i for i, t in enumerate(ok["tokens"]))
    assert bad["score"] == -np.inf and bad["frames"] == T and len(bad["tokens"]) == T + 1
    assert all(t["start_s"] is None and t["end_s"] is None and t["logp"] is None for t in bad["tokens"]) and bad["lines"][0]["start_s"] is None


def test_align_py_writes_what_train_py_reads(long_setup, tmp_path, capsys):
    """align.py's file loop on the real model: the wavs hold the recording's own samples at the reported ranges, and build_dataloader
    loads the collector file."""
    import wave
    import align
    from asr_chinese_e2e_amd.data_handler import build_dataloader
    from asr_chinese_e2e_amd.vad import EnergyVad
    model, parser, x, wav, tr, C = long_setup
    pcm = np.round(np.clip(x, -1, 1) * 32767).astype("<i2")
    path = str(tmp_path / "rec.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(pcm.tobytes())
    ids = [i for i in tr["ids"] if i > 3]
    h = len(ids) // 2
    tok = model.vocab._id2token
    texts = ["".join(tok[i] for i in ids[:h]), " ".join(tok[i] for i in ids[h:])]
    pfx = str(tmp_path / "cut" / "rec")
    lines = align.align_file(model, parser, path, texts, EnergyVad(), dict(C.LONG_OPTS), 2, False, 16000, "post_mean", 0.0, pfx, "train")
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert len(out) == 3 and out[2]["kept"] == 2 and out[2]["lines"] == 2 and out[2]["score"] is not None
    man = [json.loads(l) for l in open(pfx + "_train.json", encoding="utf-8")]
    assert [m["tgt"] for m in man] == ["".join(t.split()) for t in texts]
    for m, l in zip(man, out[:2]):
        assert l["kept"] and l["ids"] == model.vocab.convert_str(m["tgt"], use_bos=False, use_eos=False) and 0 <= l["start_sample"] < l["end_sample"] <= len(pcm)
        assert l["start_sample"] == int(round(l["start_s"] * 16000))
        with wave.open(m["wave"], "rb") as w:
            got = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        assert np.array_equal(got, pcm[l["start_sample"]:l["end_sample"]])
    packs = [p for p in build_dataloader(pfx, model.vocab, 2, part="train", dtype=torch.float32, n_mels=80)]
    assert len(packs) == 1 and packs[0]["wave"].shape[0] == 2
    assert sorted(int(n) for n in packs[0]["tgt_len"]) == sorted(len(l["ids"]) for l in out[:2])
