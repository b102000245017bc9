"""asr_vad_energy / asr_vad_decide / asr_segment_gather and model.transcribe_long against tests/vad_ref.py.  Every output buffer starts
full of NaN (or of 7 for the mask), so a cell nobody writes shows.

Energy: every frame within vad_ref.frame_bounds (fp32 arithmetic alone) of the float64 definition, in the linear domain; all-zero frames
bit for bit logf(FLT_EPSILON); a frame's bits independent of batch, tile and position.  Decision: the reference rule applied to the kernel's
own E, bit for bit, after asserting that no frame lies within 1e-6 of its threshold (so no frame is excluded).  Gather: bit-exact.
End to end: transcribe_long's segments are the reference segmenter's on the kernel's mask, and every segment's result is
model.transcribe's on the same batches built on the host."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import vad_cases as C  # noqa: E402
from tests import vad_ref as R  # noqa: E402

DEV = "cuda"
GARBAGE = 1e3            # what lies in a row past its recording


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def energy(K, wav, lens, Tmax):
    """wav (B, S) float32 numpy -> E (B, Tmax) float32 numpy, the kernel writing into a buffer full of NaN."""
    E = torch.full((wav.shape[0], Tmax), float("nan"), dtype=torch.float32, device=DEV)
    out = K.vad_energy(torch.from_numpy(np.ascontiguousarray(wav)).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), Tmax, E=E)
    assert out.data_ptr() == E.data_ptr()
    return E.cpu().numpy()


def ragged(lens, S, seed):
    """(B, S) float32: recording b = noise of amplitude 0.1 with a stretch of exact zeros (samples 1000 .. 1999), GARBAGE behind it."""
    rng = np.random.RandomState(seed)
    wav = np.full((len(lens), S), GARBAGE, dtype=np.float32)
    for b, l in enumerate(lens):
        wav[b, :l] = 0.1 * rng.randn(l)
        wav[b, 1000:min(2000, l)] = 0.0
    return wav


_floor = []


def is_floor(K, x):
    """x holds the device's logf(FLT_EPSILON) and nothing else, bit for bit: the value every frame of a silent recording holds, itself
    within 2 ulp of the float32 nearest to log(2^-23) (tests/test_fbank_gpu.py is_floor's argument: the hardware's log2 to 1 ulp, times
    ln 2, one rounding)."""
    if not _floor:
        got = bits(energy(K, np.zeros((1, 3000), dtype=np.float32), [3000], 17))
        assert np.all(got == got.flat[0]), "silent frames differ among themselves"
        assert abs(int(got.flat[0]) - int(bits(np.array([R.LOG_FLOOR32]))[0])) <= 2, got.flat[0]
        _floor.append(got.flat[0])
    return bool(np.all(bits(x) == _floor[0]))


def check_row(K, got, wav, what):
    """One row (Tmax,) against the recording wav (len,): the bound on its frames, exact floor, exact zeros behind.  -> err / bound."""
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} frames never written"
    T = R.num_frames(len(wav))
    assert np.array_equal(bits(got[T:]), np.zeros_like(bits(got[T:]))), f"{what}: frames past {T} are not zero"
    if T == 0:
        return 0.0
    zero = R.zero_frames(wav)
    assert is_floor(K, got[:T][zero]), f"{what}: all-zero frames are not logf(FLT_EPSILON)"
    ratio, at = R.error_ratio(got[:T], wav)
    assert ratio <= 1.0, f"{what}: err / bound {ratio:.3e} at frame {at}"
    err = np.abs(got[:T].astype(np.float64) - R.energy64(wav))
    assert np.all(err[~zero] <= R.log_bound(wav)[~zero]), f"{what}: log domain"
    return ratio


# ------------------------------------------------------------------------------------ energy
# T = 0, 1, 63, 64, 65 and 257 frames over two batches; the second batch's row stride is no multiple of four (the scalar load path)
BATCHES = [([399, 10480, 41360], 41360), ([400, 10320, 10640], 10641)]


@pytest.fixture(scope="module")
def energy_runs(K):
    out = []
    for i, (lens, S) in enumerate(BATCHES):
        wav = ragged(lens, S, seed=20 + i)
        out.append((wav, lens, energy(K, wav, lens, R.num_frames(S) + 3)))      # three rows of padding behind the longest
    return out


def test_energy_against_float64(K, energy_runs):
    assert sorted(R.num_frames(l) for lens, _ in BATCHES for l in lens) == [0, 1, 63, 64, 65, 257] and BATCHES[1][1] % 4 != 0
    worst = 0.0
    for wav, lens, E in energy_runs:
        for b, l in enumerate(lens):
            ratio = check_row(K, E[b], wav[b, :l], f"len {l}")
            print(f"len {l:6d}  T {R.num_frames(l):4d}  row stride {wav.shape[1]}  err/bound {ratio:.3e}")
            worst = max(worst, ratio)
            if R.num_frames(l) > 13:
                assert R.zero_frames(wav[b, :l]).sum() == 4       # frames 7 .. 10 lie inside the zeroed stretch
    print(f"largest err / bound {worst:.3e}")
    assert 0.0 < worst <= 1.0


def test_energy_silence_and_emulation(K):
    assert is_floor(K, energy(K, np.zeros((2, 3000), dtype=np.float32), [3000, 2999], 17)[:, :16])
    # the float32 restatement states the kernel's summation order: the same bits up to what logf may differ by
    x = C.bursts(10480, [(2000, 6000)], seed=1)
    got, emu = energy(K, x[None], [10480], 64)[0], R.emulate32(x)
    print(f"kernel against the float32 restatement: largest difference {np.abs(got - emu).max():.3e}")
    assert np.abs(got.astype(np.float64) - emu).max() <= 6 * 2.0 ** -19          # two logf implementations, 2.5 ulp of 2^-19 each below 32, and slack of one


def test_energy_bits_do_not_depend_on_batch_tile_or_position(K, energy_runs):
    wav, lens, E = energy_runs[0]
    alone = energy(K, wav[2:3, :41360], [41360], 257)
    assert np.array_equal(bits(alone[0]), bits(E[2, :257]))                      # alone = inside the ragged batch
    alone = energy(K, wav[1:2, :10480].copy(), [10480], 64)
    assert np.array_equal(bits(alone[0]), bits(E[1, :64]))
    # without its first 160 samples every frame moves one row up (another place in the tile, another tile at the seams)
    shifted = energy(K, wav[2:3, 160:41360].copy(), [41200], 256)
    assert np.array_equal(bits(shifted[0]), bits(E[2, 1:257]))
    # the scalar load path (row stride 41357) gives the bits of the 16-byte path
    odd = energy(K, wav[2:3, :41357].copy(), [41357], 256)
    assert R.num_frames(41357) == 256 and np.array_equal(bits(odd[0]), bits(E[2, :256]))
    # a length past the row is clamped, a negative one is an empty row
    got = energy(K, wav[:2], [41360 + 500, -3], 257)
    assert not np.isnan(got).any() and not got[1].any() and got[0].all()


# ------------------------------------------------------------------------------------ decision
def decide(K, E, lens, vad_kw, ctx):
    from asr_chinese_e2e_amd.vad import EnergyVad
    vad = EnergyVad(frames_context=ctx, **vad_kw)
    speech = torch.full(E.shape, 7, dtype=torch.uint8, device=DEV)
    thr = torch.full((E.shape[0],), float("nan"), dtype=torch.float64, device=DEV)
    K.vad_decide(E, torch.tensor(lens, dtype=torch.int32, device=DEV), vad.params(DEV), ctx, speech=speech, thr=thr)
    return speech.cpu().numpy(), thr.cpu().numpy()


@pytest.fixture(scope="module")
def decide_E(K):
    wav, lens = C.decide_case()
    return lens, K.vad_energy(torch.from_numpy(wav).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), 260)


@pytest.mark.parametrize("ctx", [0, 2, 5])
def test_decision_is_the_reference_rule_on_the_kernels_energies(K, decide_E, ctx):
    lens, dE = decide_E
    E = dE.cpu().numpy()
    for kw in C.DECIDE_OPTIONS:
        speech, thr = decide(K, dE, lens, kw, ctx)
        again, thr2 = decide(K, dE, lens, kw, ctx)
        assert np.array_equal(speech, again) and np.array_equal(thr.view(np.uint64), thr2.view(np.uint64))      # two runs: identical bits
        opt = dict(R.DEFAULTS, **kw)
        for b, l in enumerate(lens):
            T = R.num_frames(l)
            assert T == [257, 3, 8, 0][b]
            want_thr = R.threshold(E[b, :T], opt["energy_threshold"], opt["energy_mean_scale"])
            assert abs(thr[b] - want_thr) <= 1e-12 * abs(want_thr), (b, thr[b], want_thr)
            if T:
                gap = np.abs(E[b, :T].astype(np.float64) - want_thr).min()
                assert gap >= C.MARGIN, f"recording {b}: a frame lies {gap:.3e} from the threshold"      # no frame is excluded below
            want = R.decide(E[b, :T], want_thr, ctx, opt["proportion_threshold"])
            assert np.array_equal(speech[b, :T], want), (b, ctx, np.flatnonzero(speech[b, :T] != want)[:5])
            assert not speech[b, T:].any()                                       # rows past the frames are written, as zeros
        assert 0 < speech[0, :257].sum() < 257


def test_decision_over_many_partials(K):
    """Tmax = 2500: three partial sums per recording, ten workgroups of the final pass; the threshold and the mask do not depend on which
    workgroup formed them."""
    rng = np.random.RandomState(4)
    E = rng.uniform(6.0, 24.0, (2, 2500)).astype(np.float32)
    lens = [160 * 2499 + 400, 160 * 1030 + 400]
    E[1, 1031:] = 0.0
    speech, thr = decide(K, torch.from_numpy(E).to(DEV), lens, {}, 3)
    for b, T in enumerate((2500, 1031)):
        want_thr = R.threshold(E[b, :T])
        assert abs(thr[b] - want_thr) <= 1e-12 * abs(want_thr)
        assert np.abs(E[b, :T].astype(np.float64) - want_thr).min() >= C.MARGIN
        assert np.array_equal(speech[b, :T], R.decide(E[b, :T], want_thr, 3)) and not speech[b, T:].any()


# ------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("S,Smax", [(8000, 1600), (8001, 1600), (8000, 1601)], ids=["vector", "odd_row_stride", "odd_batch_stride"])
def test_gather_is_a_bit_exact_copy(K, S, Smax):
    rng = np.random.RandomState(S + Smax)
    wav = rng.randn(3, S).astype(np.float32)
    wav.view(np.uint32)[0, :8] = [0x7fc00001, 0xffc12345, 0x80000000, 0x00000001, 0x7f800000, 0xff800000, 0x7fa00000, 0x00800000]      # NaN payloads, -0, denormal, inf
    # at offset 0, at the end of a recording, of 400 samples, of different recordings in one launch, a start that is no multiple of four, empty
    segs = [(0, 0, 1600), (1, S - 1000, 1000), (2, 160, 400), (0, 4800, 1599), (2, 1602, 997), (1, 320, 0), (1, S - 400, 400)]
    rec, start, n = (list(v) for v in zip(*segs))
    out = torch.full((len(segs), Smax), float("nan"), dtype=torch.float32, device=DEV)
    got = K.segment_gather(torch.from_numpy(wav).to(DEV), rec, start, n, Smax, out=out).cpu().numpy()
    for i, (r, s, l) in enumerate(segs):
        assert np.array_equal(bits(got[i, :l]), bits(wav[r, s:s + l])), i
        assert np.array_equal(bits(got[i, l:]), np.zeros(Smax - l, dtype=np.uint32)), i      # exact zeros behind
    for bad in ((3, 0, 10), (-1, 0, 10), (0, -1, 10), (0, S - 5, 10), (0, 0, Smax + 1), (0, 0, -1)):
        with pytest.raises(ValueError, match="segment 0"):
            K.segment_gather(torch.from_numpy(wav).to(DEV), [bad[0]], [bad[1]], [bad[2]], Smax)


# ------------------------------------------------------------------------------------ end to end
def _model():
    """The tiny joint model of tests/test_fbank_gpu.py, full attention."""
    from oracle import ref_model as RM
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    V = 30
    cfg = RM.default_cfg(n_mels=320, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, ctc_weight=0.5)
    sd = RM.init_state_dict(cfg, V, seed=11)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
    sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    g = torch.Generator().manual_seed(23)                      # a peaky CTC head, as tests/test_ctc_align_gpu.py makes one: the CTC searches spell tokens
    sd["ctc_lo.weight"] = torch.randn(V, cfg.d_model, generator=g) * 0.8
    sd["ctc_lo.bias"] = torch.randn(V, generator=g) * 0.5
    sd["ctc_lo.bias"][[2, 3]] = -30.0                          # as a trained CTC head: sos / eos are never spelled
    M = Models.TransformerOffical
    mc = M.get_default_config()()
    d = dict(vars(cfg))
    d.pop("use_decoder", None)
    d.update(dtype="fp32", cross_mask="wave_len")
    mc.fn_build(d)
    model = M(mc, Vocab.synthetic(V)).cuda().eval()
    model.load_state_dict(sd)
    return model


@pytest.fixture(scope="module")
def long_setup():
    from asr_chinese_e2e_amd.data_handler import AudioParser
    from asr_chinese_e2e_amd.vad import EnergyVad, segment_frames
    model = _model()
    parser = AudioParser(n_mels=80, lfr_m=4, lfr_n=3, device=DEV, frontend="kaldi")
    x = C.long_case()
    wav = torch.from_numpy(x[None]).to(DEV)
    _, speech, _ = EnergyVad().frames(wav, torch.tensor([len(x)], dtype=torch.int32, device=DEV))
    want = R.segments(speech[0].cpu().numpy(), R.num_frames(len(x)), len(x), *segment_frames(**C.LONG_OPTS))      # the reference on the kernel's mask
    return model, parser, x, wav, want


def host_batches(model, parser, x, segs, batch_size, **kw):
    """model.transcribe on the batches built on the host from the segments, in order: transcribe.py's offline path."""
    from asr_chinese_e2e_amd.Utils import Pack
    out = []
    for i in range(0, len(segs), batch_size):
        part = segs[i:i + batch_size]
        S = max(1, max(b - a for a, b in part))
        wav = np.zeros((len(part), S), dtype=np.float32)
        for r, (a, b) in enumerate(part):
            wav[r, :b - a] = x[a:b]
        feats, flen = parser.parse_batch(torch.from_numpy(wav).cuda(), torch.tensor([b - a for a, b in part], dtype=torch.int32).cuda())
        out += model.transcribe(Pack(wave=feats, wave_len=flen), **kw)
    return out


@pytest.mark.parametrize("search", [dict(beam_size=3), dict(beam_size=3, joint="ctc_rescore", confidence="post_max")], ids=["rescore", "ctc_rescore_confidence"])
def test_transcribe_long_equals_transcribe_on_the_same_batches(long_setup, search):
    model, parser, x, wav, want = long_setup
    assert len(want) == C.LONG_SEGMENTS
    res = model.transcribe_long(parser, wav, [len(x)], batch_size=2, **C.LONG_OPTS, **search)
    assert len(res) == 1 and res[0]["duration_s"] == C.LONG_SECONDS
    segs = res[0]["segments"]
    assert [(s["start_sample"], s["start_s"], s["end_s"]) for s in segs] == [(a, a / 16000.0, b / 16000.0) for a, b in want]
    ref = host_batches(model, parser, x, want, 2, **search)
    assert len(ref) == len(segs) == 5
    d = model.frame_seconds()
    n_tokens = 0
    for s, r, (a, _) in zip(segs, ref, want):
        assert s["ids"] == r["ids"] and s["score"] == r["score"] and s["text"] == r["text"]
        assert len(s["tokens"]) == len(r["tokens"]) == len(s["ids"])
        for t, u in zip(s["tokens"], r["tokens"]):
            assert (t["id"], t["start_frame"], t["end_frame"], t["logp"]) == (u["id"], u["start_frame"], u["end_frame"], u["logp"])
            if u["start_s"] is None:
                assert t["start_s"] is None and t["end_s"] is None
                continue
            n_tokens += 1
            assert t["start_s"] == a / 16000.0 + u["start_s"] and t["end_s"] == a / 16000.0 + u["end_s"]      # the offset plus the relative time
            assert t["start_s"] == a / 16000.0 + t["start_frame"] * d
            if "confidence" in search:
                assert t["confidence"] == u["confidence"] and t["measures"] == u["measures"]
        if "confidence" in search:
            assert s["confidence"] == r["confidence"]
    print(f"{search}: {sum(len(s['ids']) for s in segs)} ids, {n_tokens} tokens with times in {len(segs)} segments")
    if search.get("joint") == "ctc_rescore":                   # the peaky CTC head spells tokens; what the attention beam of random weights emits is its business
        assert n_tokens > 0, "the CTC search emitted no token: the comparison of token times is empty"
    assert res[0]["text"] == "".join(r["text"] for r in ref) and res[0]["ids"] == [i for r in ref for i in r["ids"]]


def test_transcribe_long_resampled_silent_and_refused(long_setup):
    model, parser, x, wav, want = long_setup
    # 8 kHz: a decimated copy, converted in front; the segments exist and lie inside the recording
    x8 = np.ascontiguousarray(x[::2])
    res = model.transcribe_long(parser, torch.from_numpy(x8[None]).to(DEV), [len(x8)], batch_size=2, source_rate=8000, beam_size=3, **C.LONG_OPTS)[0]
    assert res["duration_s"] == C.LONG_SECONDS and len(res["segments"]) >= 3
    last = 0.0
    for s in res["segments"]:
        assert last - 240 / 16000.0 <= s["start_s"] < s["end_s"] <= res["duration_s"]      # the pieces of a split share the 240 samples by which their frames overlap
        last = s["end_s"]
        for t in s["tokens"]:
            if t["start_s"] is not None:
                assert s["start_s"] <= t["start_s"] <= t["end_s"] <= res["duration_s"] + model.frame_seconds()
    # silence, a recording too short for a frame, and a speaking one in one call
    batch = torch.zeros(3, len(x), device=DEV)
    batch[2] = wav[0]
    out = model.transcribe_long(parser, batch, [len(x), 300, len(x)], batch_size=2, beam_size=3, **C.LONG_OPTS)
    assert out[0] == {"text": "", "ids": [], "duration_s": 12.0, "segments": []} and out[1]["segments"] == [] and out[1]["duration_s"] == 300 / 16000.0
    assert [s["start_sample"] for s in out[2]["segments"]] == [a for a, _ in want] and len(want) == 5      # as alone: the batch does not matter
    # past the positional-encoding table: refused, the message names what fits
    table = model._ensure_engine(torch.device(DEV)).pe.shape[0]
    with pytest.raises(ValueError, match=f"largest admissible max_segment_s is {3 * table / 100.0}"):
        model.transcribe_long(parser, wav, [len(x)], max_segment_s=3 * table / 100.0 + 0.01)

