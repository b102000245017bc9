"""fbank_kernel / stream_fbank_kernel against the float64 Kaldi fbank definition (tests/fbank_ref.py) where they can go wrong: dynamic
range, silence, the frame count at every edge of snip_edges framing, padding rows and tiles, truncation, every mel width's lane layout,
tile independence, a length past the row; then everything that reads the frames - streaming (bit for bit the offline rows), both
normalisations with and without SpecAugment, the CMVN accumulator, model.stream and the waveform loader.  Every output buffer starts
full of NaN, so a row nobody writes shows.

Hard gate, every frame and bin: |exp(got) - max(mel64, FLT_EPSILON)| <= bound, the bound from fp32 arithmetic alone (fbank_ref.bound).
Floor cells (an all-zero frame, a filter without a weight) hold exactly logf(FLT_EPSILON): one value, within 2 ulp of the float32
nearest to log(2^-23) (test_logmel_gpu.is_floor's argument: the hardware's log2 to 1 ulp, times ln 2, one rounding)."""
import random
import wave as wave_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cmvn_ref as CR  # noqa: E402
from tests import fbank_ref as R  # noqa: E402

DEV = "cuda"
GARBAGE = 1e3            # what lies in a row past its utterance


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


_tables = {}


def tables(n_mels):
    if n_mels not in _tables:
        _tables[n_mels] = (torch.from_numpy(R.povey_window().astype(np.float32)).to(DEV),
                           torch.from_numpy(R.mel_filterbank(n_mels).astype(np.float32)).to(DEV))
    return _tables[n_mels]


def fbank(K, wav, lens, n_mels, Tmax):
    """wav (B, S) float32 numpy, lens -> (B, Tmax, n_mels) float32 numpy, the kernel writing into a buffer full of NaN."""
    window, fb = tables(n_mels)
    feat = torch.full((wav.shape[0], Tmax, n_mels), float("nan"), dtype=torch.float32, device=DEV)
    out = K.fbank(torch.from_numpy(np.ascontiguousarray(wav)).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), window, fb, Tmax,
                  R.WAV_SCALE, R.PREEMPH, feat=feat)
    assert out.data_ptr() == feat.data_ptr()
    return feat.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


_floor = []


def is_floor(K, x):
    """x holds logf(FLT_EPSILON) and nothing else, bit for bit: the value every cell of a silent utterance holds, itself within 2 ulp of
    the float32 nearest to log(2^-23)."""
    if not _floor:
        got = bits(fbank(K, np.zeros((1, 3000), dtype=np.float32), [3000], 80, R.num_frames(3000)))
        assert np.all(got == got.flat[0]), "silent cells differ among themselves"
        assert abs(int(got.flat[0]) - int(bits(np.array([R.LOG_FLOOR32]))[0])) <= 2, got.flat[0]
        _floor.append(got.flat[0])
    return bool(np.all(bits(x) == _floor[0]))


def ragged(lens, Smax, seed, amp=0.1):
    """(B, Smax) float32: noise of amplitude 0.1 in [0, len), GARBAGE behind it."""
    rng = np.random.RandomState(seed)
    wav = np.full((len(lens), Smax), GARBAGE, dtype=np.float32)
    for b, l in enumerate(lens):
        wav[b, :l] = amp * rng.randn(l)
    return wav


def check_row(K, got, wav, n_mels, what):
    """One batch row (Tmax, n_mels) against the utterance wav (len,): hard gate and exact floor cells on its frames (as many as Tmax
    leaves), exact zeros behind them, no NaN.  -> the largest err / bound."""
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} cells never written"
    T = min(R.num_frames(len(wav)), got.shape[0])
    assert np.array_equal(bits(got[T:]), np.zeros_like(bits(got[T:]))), f"{what}: rows past frame {T} are not zero"
    if T == 0:
        return 0.0
    floor = R.floor_cells(wav, n_mels)[:T]
    assert is_floor(K, got[:T][floor]), f"{what}: floor cells"
    ratio, at = R.error_ratio(got[:T], wav, n_mels)
    assert ratio <= 1.0, f"{what}: err / bound {ratio:.3e} at (frame, bin) {at}"
    return ratio


# ------------------------------------------------------------------------------------ accuracy against float64
@pytest.mark.parametrize("n_mels", [40, 80])
def test_accuracy_and_dynamic_range(K, n_mels):
    """48 frames per signal: one full tile and one ragged one.  Measured err / bound: README, "Kaldi fbank front end"."""
    sig = R.signals()
    names = list(sig)
    assert R.num_frames(R.N_SIG) == 48
    got = fbank(K, np.stack([sig[k] for k in names]), [R.N_SIG] * len(names), n_mels, 48)
    failed = []
    for b, name in enumerate(names):
        assert not np.isnan(got[b]).any(), name
        kern, at = R.error_ratio(got[b], sig[name], n_mels)
        emul, _ = R.error_ratio(R.emulate32(sig[name], n_mels), sig[name], n_mels)
        print(f"n_mels {n_mels:3d}  {name:24s} err/bound kernel {kern:.3e} at {at}  emulation {emul:.3e}")
        floor = R.floor_cells(sig[name], n_mels)
        if not is_floor(K, got[b][floor]):
            failed.append(f"{name}: floor cells are not logf(FLT_EPSILON)")
        if not kern <= 1.0:
            failed.append(f"{name}: hard gate, err / bound {kern:.3e} at {at}")
    assert not failed, failed


def test_silence(K):
    assert R.num_frames(3000) == 17
    assert is_floor(K, fbank(K, np.zeros((1, 3000), dtype=np.float32), [3000], 80, 17))
    wav = ragged([3000, 3000], 3000, seed=2, amp=0.9)
    wav[1] = 0.0
    got = fbank(K, wav, [3000, 3000], 80, 17)
    assert is_floor(K, got[1]) and np.all(got[0] > 0.0)


# ------------------------------------------------------------------------------------ frame count, tile and padding edges
EDGE_LENS = [0, 1, 399, 400, 559, 560, 5359, 5360, 5519, 5520, 10640]
EDGE_SMAX = 10640


@pytest.fixture(scope="module")
def edge_wav():
    return ragged(EDGE_LENS, EDGE_SMAX, seed=11)


@pytest.fixture(scope="module")
def edge_run65(K, edge_wav):
    return fbank(K, edge_wav, EDGE_LENS, 80, 65)


@pytest.mark.parametrize("Tmax", [65, 70])
def test_ragged_lengths_and_padding(K, edge_wav, edge_run65, Tmax):
    """Tmax = 70 puts padding rows behind every utterance, the tile 64..69 of the longest holding one frame and five padding rows."""
    assert [R.num_frames(l) for l in EDGE_LENS] == [0, 0, 0, 1, 1, 2, 31, 32, 32, 33, 65]
    got = edge_run65 if Tmax == 65 else fbank(K, edge_wav, EDGE_LENS, 80, Tmax)
    for b, l in enumerate(EDGE_LENS):
        ratio = check_row(K, got[b], edge_wav[b, :l], 80, f"len {l}, Tmax {Tmax}")
        print(f"len {l:6d}  Tmax {Tmax}  err/bound {ratio:.3e}")
    if Tmax != 65:
        assert np.array_equal(bits(got[:, :65]), bits(edge_run65))


def test_truncating_tmax(K, edge_wav, edge_run65):
    got = fbank(K, edge_wav, EDGE_LENS, 80, 20)
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(edge_run65[:, :20]))      # zeros behind the short utterances included
    assert np.all(got[EDGE_LENS.index(5359)] != 0.0)                # and 20 frames of the long ones


def test_length_past_the_row_is_clamped(K):
    """Row 0 claims more samples than a row holds (the overrun would stay inside the tensor: it would read row 1), and a negative
    length is an empty row."""
    Smax = 4000
    wav = ragged([Smax, Smax], Smax, seed=9)
    Tmax = R.num_frames(Smax + 500)
    want = fbank(K, wav, [Smax, Smax], 80, Tmax)
    got = fbank(K, wav, [Smax + 500, Smax], 80, Tmax)
    assert not np.isnan(got).any() and np.array_equal(bits(got), bits(want))
    assert not want[0, R.num_frames(Smax):].any() and want[0, :R.num_frames(Smax)].all()
    got = fbank(K, wav, [-3, Smax], 80, Tmax)
    assert not got[0].any() and np.array_equal(bits(got[1]), bits(want[1]))


# ------------------------------------------------------------------------------------ mel width
@pytest.mark.parametrize("n_mels", [23, 40, 80, 128, 160])
def test_mel_width(K, n_mels):
    """160: two mel tiles per wave; 23 and 40: lanes without a column; 128 and 160 have filters without a weight."""
    wav = ragged([5400], 5400, seed=n_mels)
    assert R.num_frames(5400) == 32
    got = fbank(K, wav, [5400], n_mels, 33)          # one row of padding behind 32 frames
    empty = ~R.mel_filterbank(n_mels).any(axis=0)
    assert int(empty.sum()) == {23: 0, 40: 0, 80: 0, 128: 1, 160: 3}[n_mels]
    ratio = check_row(K, got[0], wav[0], n_mels, f"n_mels {n_mels}")
    print(f"n_mels {n_mels:3d}  err/bound {ratio:.3e}  empty filters {int(empty.sum())}")
    assert is_floor(K, got[0, :32][:, empty])
    assert np.all(got[0, :32][:, ~empty] > R.LOG_FLOOR32 + 10.0)


# ------------------------------------------------------------------------------------ tile independence
def test_tile_independence(K):
    lens = [9000, 100, 6400]
    wav = ragged(lens, 9000, seed=5)
    batch = fbank(K, wav, lens, 80, 54)
    alone = fbank(K, wav[2:3, :6400], [6400], 80, 38)
    assert R.num_frames(6400) == 38 and R.num_frames(9000) == 54 and not np.isnan(alone).any()
    assert np.array_equal(bits(batch[2, :38]), bits(alone[0]))
    # nor does a frame know its row in the tile: without its first 160 samples every frame of the utterance moves one row up
    shifted = fbank(K, wav[2:3, 160:6400], [6240], 80, 37)
    assert np.array_equal(bits(shifted[0]), bits(alone[0, 1:]))


# ------------------------------------------------------------------------------------ streaming equals offline
STREAM_LENS = [8000, 5519, 300]


@pytest.fixture(scope="module")
def stream_case():
    """-> (parser: 80 bins, LFR 4/3, global CMVN, wav (3, 8000) float32, offline rows (3, Tl, 320), their lengths)."""
    from asr_chinese_e2e_amd.data_handler import AudioParser
    rng = np.random.RandomState(21)
    wav = np.zeros((3, 8000), dtype=np.float32)
    for b, l in enumerate(STREAM_LENS):
        wav[b, :l] = (0.3 * rng.randn(l)).astype(np.float32)
    f = R.fbank64(wav[0], 80)
    parser = AudioParser(n_mels=80, lfr_m=4, lfr_n=3, device=DEV, norm="global", cmvn=(f.mean(axis=0), 1.0 / f.std(axis=0)), frontend="kaldi")
    want, want_len = parser.parse_batch(torch.from_numpy(wav).to(DEV), torch.tensor(STREAM_LENS, dtype=torch.int32, device=DEV))
    assert want_len.tolist() == [-(-R.num_frames(l) // 3) for l in STREAM_LENS] == [16, 11, 0]
    return parser, wav, want, want_len.tolist()


def _cuts(name):
    rng = random.Random(5)
    if name == "random_with_zeros":
        return [[rng.choice([0, 0, rng.randint(1, 1500)]) for _ in range(200)] for _ in range(3)]
    size = {"one_block": 8000, "blocks_160": 160, "blocks_401": 401, "blocks_7": 7, "one_block_small_ring": 8000}[name]
    return [[size] * (8000 // size + 1)] * 3


@pytest.mark.parametrize("name", ["one_block", "blocks_160", "blocks_401", "blocks_7", "random_with_zeros", "one_block_small_ring"])
def test_streamed_rows_equal_offline_bit_for_bit(stream_case, name):
    from asr_chinese_e2e_amd.data_handler import StreamingFrontEnd
    parser, wav, want, want_len = stream_case
    fe = StreamingFrontEnd(parser, 3, 4, sample_cap=1024 if name == "one_block_small_ring" else 16384)
    cuts, pos, step = _cuts(name), [0, 0, 0], 0
    rows, tot = [[] for _ in range(3)], [0, 0, 0]
    src = torch.from_numpy(wav)
    while pos != STREAM_LENS:
        ns = [min(cuts[b][step] if step < len(cuts[b]) else 8000, STREAM_LENS[b] - pos[b]) for b in range(3)]
        pcm = torch.zeros(3, max(max(ns), 1))
        for b in range(3):
            pcm[b, :ns[b]] = src[b, pos[b]:pos[b] + ns[b]]
            pos[b] += ns[b]
        step += 1
        for feats, nv in fe.push_audio(pcm, ns, [pos[b] == STREAM_LENS[b] for b in range(3)]):
            assert feats.shape == (3, 4, 320) and len(nv) == 3
            for b in range(3):
                rows[b].append(feats[b, :nv[b]])
                tot[b] += nv[b]
                assert not feats[b, nv[b]:].any()
    assert tot == want_len and tot[2] == 0
    for b in range(2):
        assert torch.equal(torch.cat(rows[b]), want[b, :want_len[b]]), (name, b)
    assert fe.next_frame == [R.num_frames(l) for l in STREAM_LENS]


# ------------------------------------------------------------------------------------ normalisations
NORM_LENS = [0, 399, 2000, 5519, 8000]


def _log_err(wav, n_mels):
    """(T, n_mels): how far the kernel's log value may lie from the definition's, from the bound on the value under the log."""
    rel = R.bound(wav, n_mels) / np.maximum(R.mel_power64(wav, n_mels), R.FLT_EPSILON)
    return -np.log1p(-np.minimum(rel, 0.5))


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "specaug"])
@pytest.mark.parametrize("norm", ["utterance", "global"])
def test_parse_batch_against_the_float64_chain(K, norm, augment):
    """Definition -> normalisation (the utterance formula of oracle/logmel_ref.py, or tests/cmvn_ref.py) -> LFR, in float64, two ways:
    from the kernel's own frames with the tolerances the existing tests of these stages use (utterance: rtol = atol = 1e-4,
    test_logmel_gpu; global: rtol 3e-7, a masked cell 1e-5 of its fill, test_cmvn_gpu), and from the definition's frames with, on top of
    that, three roundings to float32 in front of the slope (the frame, the mean, their difference: half an ulp below 32, 1e-6 each) and the error the
    frames may carry: their log-domain bound times the slope of the normalisation (istd; for the utterance formula 2 / std, the factor 2
    for what the same errors do to the utterance's own mean and deviation), the largest of the utterance for a masked cell."""
    from asr_chinese_e2e_amd.data_handler import AudioParser, processor
    from oracle import logmel_ref as LM
    n_mels, m, n, S = 40, 4, 3, 8000
    rng = np.random.RandomState(3)
    wav = np.zeros((len(NORM_LENS), S), dtype=np.float32)
    for b, l in enumerate(NORM_LENS):
        wav[b, :l] = (0.2 * (b + 1) * rng.randn(l)).astype(np.float32)
    frames = [R.num_frames(l) for l in NORM_LENS]
    ref64 = [R.fbank64(wav[b, :l], n_mels) for b, l in enumerate(NORM_LENS)]
    allf = np.concatenate([f for f in ref64 if len(f)])
    stats = (allf.mean(axis=0), 1.0 / allf.std(axis=0))
    parser = AudioParser(n_mels=n_mels, lfr_m=m, lfr_n=n, device=DEV, norm=norm, cmvn=stats if norm == "global" else None, frontend="kaldi")
    dwav, dlen = torch.from_numpy(wav).to(DEV), torch.tensor(NORM_LENS, dtype=torch.int32, device=DEV)
    got, got_len = parser.parse_batch(dwav, dlen, augment=augment, rng=random.Random(4))
    masks = None
    if augment:
        r = random.Random(4)
        masks = [processor.sample_spec_augment(n_mels, f, r) for f in frames]
        assert any(t1 > t0 for t0, t1, _, _ in masks) and any(f1 > f0 for _, _, f0, f1 in masks)
    Tmax = parser.max_frames(S)
    assert Tmax == 48 and tuple(got.shape) == (5, 16, m * n_mels)
    assert got_len.tolist() == [-(-f // n) for f in frames] == [0, 0, 4, 11, 16]
    own = parser.features(dwav, dlen, Tmax).cpu().numpy()
    g = got.cpu().numpy().astype(np.float64)
    assert not np.isnan(g).any()

    def chain(feat_b, T, mask):
        """float64 rows (Tl, m n_mels) of one utterance from its frames feat_b (T, n_mels), which of their cells are masked, and the
        normalisation's slope per bin."""
        if norm == "utterance":
            x, slope = LM.utt_normalize(feat_b), np.full(n_mels, 2.0 / feat_b.std(ddof=1))
        else:
            x, slope = (feat_b - stats[0]) * stats[1], stats[1]
        x, masked = x.copy(), np.zeros(x.shape)
        if mask is not None:
            t0, t1, f0, f1 = mask
            t1 = min(t1, T)
            x[t0:t1] = x.mean()
            x[:, f0:f1] = x.mean()
            masked[t0:t1] = 1.0
            masked[:, f0:f1] = 1.0
        return LM.build_lfr(x, m, n), LM.build_lfr(masked, m, n) > 0, slope

    if norm == "global":
        stage_ref, stage_len, _ = CR.apply(own, [160 * (f - 1) + 1 if f else 0 for f in frames], *stats, m, n, 16, masks=masks)
        assert stage_len.tolist() == got_len.tolist()
    for b, T in enumerate(frames):
        rows = -(-T // n)
        assert not g[b, rows:].any()
        if T == 0:
            continue
        mask = masks[b] if augment else None
        # 1. the stage alone, from the kernel's own frames (global: cmvn_ref's fp32 subtraction and multiplication, as test_cmvn_gpu)
        ref, masked, slope = chain(own[b, :T].astype(np.float64), T, mask)
        if norm == "global":
            ref = stage_ref[b, :rows].astype(np.float64)
        stage = 1e-4 + 1e-4 * np.abs(ref) if norm == "utterance" else np.where(masked, 1e-5, 3e-7) * np.abs(ref)
        err = np.abs(g[b, :rows] - ref)
        assert np.all(err <= stage), (b, float((err - stage).max()))
        # 2. the whole chain, from the definition
        ref, masked, slope = chain(ref64[b], T, mask)
        carry = (_log_err(wav[b, :NORM_LENS[b]], n_mels) + 3e-6) * slope[None, :]
        if mask is not None:
            carry = np.full_like(carry, carry.max())
        stage = 1e-4 + 1e-4 * np.abs(ref) if norm == "utterance" else np.where(masked, 1e-5, 3e-7) * np.abs(ref)
        tol = stage + LM.build_lfr(carry, m, n)
        err = np.abs(g[b, :rows] - ref)
        print(f"{norm} utterance {b}: max err {err.max():.3e}, largest carried bound {carry.max():.3e}")
        assert np.all(err <= tol), (b, float((err - tol).max()))


def test_cmvn_accumulator(K):
    """Two ragged batches through CmvnAccumulator with a Kaldi parser against tests/cmvn_ref.py's float64 sums over the same frames (the
    existing statistics test's reference and its 1e-9), the frames counted by the fbank definition; and the statistics of the float64
    definition's frames: a bin's mean lies within the mean of its frames' log-domain bounds plus the rounding of a frame to float32
    (half an ulp below 32: 1e-6)."""
    from asr_chinese_e2e_amd.data_handler import AudioParser, CmvnAccumulator
    n_mels, lens, S = 40, [0, 399, 2000, 5519, 8000], 8000
    parser = AudioParser(n_mels=n_mels, device=DEV, frontend="kaldi")
    acc = CmvnAccumulator(parser)
    frames = [R.num_frames(l) for l in lens]
    ref = ref64 = None
    carried = np.zeros(n_mels)
    for seed in (0, 1):
        wav = ragged(lens, S, seed=seed, amp=0.3)
        dwav, dlen = torch.from_numpy(wav).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
        acc.update(dwav, dlen)
        own = parser.features(dwav, dlen, parser.max_frames(S)).cpu().numpy()
        equiv = [160 * (f - 1) + 1 if f else 0 for f in frames]
        ref = CR.accumulate(own, equiv, ref)
        d = np.zeros((len(lens), 48, n_mels))
        for b, l in enumerate(lens):
            d[b, :frames[b]] = R.fbank64(wav[b, :l], n_mels)
            if frames[b]:
                carried += _log_err(wav[b, :l], n_mels).sum(axis=0)
        ref64 = CR.accumulate(d, equiv, ref64)
    mean, istd, count = acc.finalize()
    rmean, ristd, rcount = CR.finalize(*ref)
    assert count == rcount == 2 * sum(frames) == 2 * (11 + 32 + 48)
    e_mean, e_std = np.abs(mean / rmean - 1).max(), np.abs(ristd / istd - 1).max()
    dmean, distd, _ = CR.finalize(*ref64)
    d_mean, d_tol = np.abs(mean - dmean), carried / count + 1e-6
    print(f"against the sums of the kernel's frames: mean rel err {e_mean:.3g}, std rel err {e_std:.3g}; against the definition's frames: "
          f"mean abs err {d_mean.max():.3g} (allowed {d_tol.min():.3g} .. {d_tol.max():.3g})")
    assert e_mean <= 1e-9 and e_std <= 1e-9
    assert np.all(d_mean <= d_tol)


# ------------------------------------------------------------------------------------ end to end
def _model(d_in, C):
    """The tiny model of tests/test_cmvn_gpu.py."""
    from oracle import ref_model as RM
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    V = 30
    cfg = RM.default_cfg(n_mels=d_in, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, ctc_weight=0.5)
    sd = RM.init_state_dict(cfg, V, seed=11)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
    sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    M = Models.TransformerOffical
    mc = M.get_default_config()()
    d = dict(vars(cfg))
    d.pop("use_decoder", None)
    d.update(dtype="fp32", decoding_chunk_size=C, decoding_left_chunks=-1, cross_mask="wave_len")
    mc.fn_build(d)
    model = M(mc, Vocab.synthetic(V)).cuda().eval()
    model.load_state_dict(sd)
    return model


def test_model_stream_push_audio_equals_transcribe(stream_case):
    """A tiny CTC / attention model: push_audio in 480 ms blocks, then finish(), gives the ids of model.transcribe on parse_batch's
    features; the 300-sample utterance, which has no frame, rides along and ends as the empty transcript.  Then a stream whose only
    utterance has no frame: one empty chunk, no error, the empty transcript."""
    from asr_chinese_e2e_amd.Utils import Pack
    parser, wav, want, want_len = stream_case
    model = _model(320, 4)
    lens = STREAM_LENS
    st = model.stream(3, parser=parser)
    pos, ids = [0, 0, 0], [[], [], []]
    while pos != lens:
        ns = [min(7680, lens[b] - pos[b]) for b in range(3)]
        pcm = torch.zeros(3, 7680)
        for b in range(3):
            pcm[b, :ns[b]] = torch.from_numpy(wav[b, pos[b]:pos[b] + ns[b]])
            pos[b] += ns[b]
        for b, new in enumerate(st.push_audio(pcm, ns, [pos[b] == lens[b] for b in range(3)])):
            ids[b] += new
    enc, enc_len = st.encoder_output()
    assert enc_len.tolist() == want_len == [16, 11, 0] and ids[2] == [] and bool(torch.isfinite(enc).all())
    a = st.finish(beam_size=3)
    b_ = model.transcribe(Pack(wave=want[:2].contiguous(), wave_len=torch.tensor(want_len[:2], dtype=torch.int32, device=DEV)), beam_size=3)
    assert [r["ids"] for r in a[:2]] == [r["ids"] for r in b_] and [r["text"] for r in a[:2]] == [r["text"] for r in b_]
    assert any(r["ids"] for r in b_)
    assert a[2]["ids"] == [] and a[2]["text"] == "" and a[2]["tokens"] == []
    # alone
    st = model.stream(1, parser=parser)
    assert st.push_audio(torch.from_numpy(wav[2:3, :300]), [300], [False]) == [[]]
    chunks = list(st.push_audio_chunks(torch.zeros(1, 1), [0], [True]))
    assert chunks == [([0], [[]])]
    assert st.encoder_output()[1].tolist() == [0]
    res = st.finish(beam_size=3)
    assert len(res) == 1 and res[0]["ids"] == [] and res[0]["text"] == ""
    with pytest.raises(ValueError, match="closed"):
        st.push_audio(torch.zeros(1, 8), [8], [False])


def _write_wav(path, x):
    with wave_module.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.round(np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())
    return str(path)


def test_loader_yields_parse_batch_features(tmp_path):
    """BucketedWaveLoader as build_dataloader(frontend="kaldi") builds it, over four short generated files, one of them too short for a frame."""
    from asr_chinese_e2e_amd.data_handler import AudioParser, BucketedWaveLoader, Vocab, WaveDataset, load_wav
    rng = np.random.RandomState(9)
    items = []
    for i, n in enumerate((8000, 5519, 300, 6400)):
        x = 0.3 * np.sin(2 * np.pi * (200 + 150 * i) * np.arange(n) / 16000) + 0.05 * rng.randn(n)
        items.append((_write_wav(tmp_path / f"utt{i}.wav", x), [4 + i] + list(range(10, 10 + i))))
    parser = AudioParser(sample_rate=16000, n_mels=40, lfr_m=4, lfr_n=3, device="cuda", frontend="kaldi")
    loader = BucketedWaveLoader(WaveDataset(items, Vocab.synthetic(30)), 4, parser=parser, augment=False, shuffle=False, drop_last=True, seed=0,
                                dtype=torch.float32)
    got = [{k: v.clone() for k, v in p.items() if torch.is_tensor(v)} for p in loader]
    assert len(got) == 1
    got = got[0]
    order = [int(v) - 4 for v in got["tgt_for_input"][:, 0]]
    assert sorted(order) == [0, 1, 2, 3]
    waves = [load_wav(items[i][0])[0] for i in order]
    wav = np.zeros((4, max(w.size for w in waves)), dtype=np.float32)
    for r, w in enumerate(waves):
        wav[r, :w.size] = w
    feat, feat_len = parser.parse_batch(torch.from_numpy(wav).to(DEV), torch.tensor([w.size for w in waves], dtype=torch.int32, device=DEV), torch.float32)
    assert torch.equal(got["wave"], feat) and torch.equal(got["wave_len"], feat_len.long())
    assert sorted(feat_len.tolist()) == sorted(-(-R.num_frames(n) // 3) for n in (8000, 5519, 300, 6400))
