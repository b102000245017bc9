"""Noise and reverberation on the GPU: both kernels against the float64 reference (tests/noise_ref.py) under derived bounds, their
invariants (zero padding, bit-exact copies, repeatability, aliasing), and the waveform loader with the augmentation on and off."""
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import noise_ref as NR  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def dev_i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def place(rows, smax, offset=0, fill=np.nan):
    """The rows as a (B, smax) device tensor whose first element sits `offset` floats behind a 16-byte boundary; `fill` beyond each row's end."""
    buf = np.full((len(rows), smax), fill, dtype=np.float32)
    for b, x in enumerate(rows):
        buf[b, :x.size] = x
    flat = torch.empty(len(rows) * smax + 4, dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    t = flat[offset:offset + len(rows) * smax].view(len(rows), smax)
    t.copy_(torch.from_numpy(buf))
    return t


# ------------------------------------------------------------------------------------------------ reverberation
@pytest.fixture(scope="module")
def reverb_case(K):
    """Every response length (1, 2, one tap chunk - 1, one chunk, one chunk + 1, 8192) with its peak at 0, in the middle and at L - 1,
    against every utterance length (0, 1, the tile edges, two tiles + 3: all shorter than the 8192-tap responses), plus the two
    out-of-range indices.  The reference is computed once."""
    T, C = K.REVERB_TILE, K.REVERB_CHUNK
    rng = np.random.RandomState(0)
    resp = [(L, p) for L in (1, 2, C - 1, C, C + 1, K.REVERB_MAX_TAPS) for p in sorted({0, L // 2, L - 1})]
    R = len(resp)
    table = np.full((R, K.REVERB_MAX_TAPS), np.nan, dtype=np.float32)          # what lies beyond a response's length must never be read
    for r, (L, p) in enumerate(resp):
        h = rng.randn(L) * np.exp(-np.arange(L) / max(L / 4.0, 1.0))
        table[r, :L] = (h / np.sqrt(np.sum(h * h))).astype(np.float32)
    lens = [0, 1, T - 1, T, T + 1, 2 * T + 3]
    rows, idx = [], []
    for r in range(R):
        for n in lens:
            rows.append(rng.uniform(-1.0, 1.0, size=n).astype(np.float32))
            idx.append(r)
    for bad in (-1, R, -7, R + 100):
        rows.append(rng.uniform(-1.0, 1.0, size=2 * T + 3).astype(np.float32))
        idx.append(bad)
    rows.append(rng.uniform(-1.0, 1.0, size=5).astype(np.float32))
    idx.append(-1)
    ref = [NR.reverb(x, table[r, :resp[r][0]], resp[r][1]) if 0 <= r < R else None for x, r in zip(rows, idx)]
    return dict(resp=resp, table=table, rows=rows, idx=idx, ref=ref)


@pytest.mark.parametrize("smax_extra,offset", [(2, 0), (2, 1), (5, 0)], ids=["odd_rows", "misaligned_buffer", "aligned_rows"])
def test_reverb_ragged_batch_against_the_reference(K, reverb_case, smax_extra, offset):
    """|out - ref| <= (L + 1) 2^-24 A[n], A[n] = sum_k |h[k]| |x[n + p - k]|: the worst case of an fp32 sum of L products in any order,
    with or without fused multiply-adds (tests/noise_ref.py).  Smax = 2 TILE + 5 is odd - rows start at every alignment -, the second
    run moves the whole buffer by one float, the third has Smax a multiple of 4 (the 16-byte copy path)."""
    c = reverb_case
    smax = 2 * K.REVERB_TILE + 3 + smax_extra
    assert (smax % 4 == 0) == (smax_extra == 5)
    B, R = len(c["rows"]), len(c["resp"])
    wav = place(c["rows"], smax, offset)
    out = place([np.zeros(0)] * B, smax, offset, fill=7.0)
    rl, rp = dev_i32([L for L, _ in c["resp"]]), dev_i32([p for _, p in c["resp"]])
    got = K.reverb(wav, dev_i32([x.size for x in c["rows"]]), dev_i32(c["idx"]), torch.from_numpy(c["table"]).to(DEV), rl, rp, out=out)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    worst = {}
    for b, (x, r) in enumerate(zip(c["rows"], c["idx"])):
        n = x.size
        assert not got[b, n:].any(), f"row {b}: not zero from wav_len = {n} on"
        if not 0 <= r < R:
            assert got[b, :n].tobytes() == x.tobytes(), f"row {b}: index {r} is not a copy"
            continue
        y, A = c["ref"][b]
        L = c["resp"][r][0]
        err, bound = np.abs(got[b, :n] - y), (L + 1) * 2.0 ** -24 * A
        assert np.isfinite(got[b, :n]).all()
        if n:
            worst[L] = max(worst.get(L, 0.0), float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (b, n, c["resp"][r], float((err - bound).max()))
    print("largest |out - ref| / bound per response length:", {L: round(v, 4) for L, v in worst.items()})


def test_reverb_refuses_more_than_max_taps(K):
    from asr_chinese_e2e_amd._lib import AsrHipError
    wav = torch.rand(2, 50, device=DEV)
    out = torch.full((2, 50), 7.0, device=DEV)
    rir = torch.rand(1, K.REVERB_MAX_TAPS + 1, device=DEV)
    with pytest.raises(AsrHipError, match="Lcap=8193"):
        K.reverb(wav, dev_i32([50, 50]), dev_i32([0, 0]), rir, dev_i32([3]), dev_i32([0]), out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ additive noise
def run_mix(K, rows, par, bank, smax, alias=False):
    wav = place(rows, smax)
    noise = torch.from_numpy(np.concatenate(bank)).to(DEV)
    off = dev_i32(np.concatenate([[0], np.cumsum([c.size for c in bank])]).tolist())
    out, gain = K.noise_mix(wav, dev_i32([x.size for x in rows]), dev_i32(par), noise, off, out=wav if alias else None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), gain.cpu().numpy()


def scale_bits(snr):
    from asr_chinese_e2e_amd.data_handler import noise
    return noise.snr_scale_bits(snr)


def test_mix_against_the_reference(K):
    """Clips of 1, 7 and more samples than the utterance, offsets 0 and nlen - 1, a 7-sample clip wrapping hundreds of times inside one
    tile and across tile edges; every case that must be a bit-exact copy with gain 0."""
    T = K.NOISE_MIX_TILE
    rng = np.random.RandomState(1)
    silent = np.zeros(3000, dtype=np.float32)
    silent[2500:] = 0.5                                                    # a stretch of silence longer than the utterance read from it
    bank = [np.array([0.25], dtype=np.float32), rng.randn(7).astype(np.float32), rng.randn(3 * T).astype(np.float32) * 0.3, silent]
    N = len(bank)
    cases = []                                                             # (samples, clip, offset, snr, copy expected)
    for n in (1, 5, T - 1, T, T + 1, 2 * T + 5):
        for j in range(3):
            for o in (0, bank[j].size - 1):
                cases.append((rng.uniform(-1, 1, size=n).astype(np.float32) * 0.2, j, o, float(rng.uniform(-5, 25)), False))
    cases.append((np.zeros(100, dtype=np.float32), 1, 3, 10.0, True))                                  # a silent utterance
    cases.append((rng.uniform(-1, 1, size=2000).astype(np.float32), 3, 10, 10.0, True))                # a silent stretch of noise: Ev = 0
    cases.append((np.zeros(0, dtype=np.float32), 1, 0, 10.0, True))                                    # len = 0
    cases.append((rng.uniform(-1, 1, size=T + 9).astype(np.float32), -1, 0, 10.0, True))               # no clip drawn
    cases.append((rng.uniform(-1, 1, size=77).astype(np.float32), N, 0, 10.0, True))                   # an index past the bank
    cases.append((rng.uniform(-1, 1, size=2000).astype(np.float32), 3, 2400, 15.0, False))             # the same clip where it is not silent
    rows = [c[0] for c in cases]
    par = [[j, o, scale_bits(snr), 0] for _, j, o, snr, _ in cases]
    smax = 2 * T + 7
    out, gain = run_mix(K, rows, par, bank, smax)
    out2, gain2 = run_mix(K, rows, par, bank, smax)
    assert out.tobytes() == out2.tobytes() and gain.tobytes() == gain2.tobytes(), "a second launch gives other bits"
    out3, gain3 = run_mix(K, rows, par, bank, smax, alias=True)
    assert out.tobytes() == out3.tobytes() and gain.tobytes() == gain3.tobytes(), "out = wav gives another result"
    worst_g = worst_o = 0.0
    for b, (x, j, o, snr, copy) in enumerate(cases):
        n = x.size
        assert not out[b, n:].any(), f"row {b}: not zero from wav_len = {n} on"
        if copy:
            assert gain[b] == 0.0 and out[b, :n].tobytes() == x.tobytes(), f"row {b}: not a copy with gain 0"
            continue
        scale = float(np.array(par[b][2], dtype=np.int32).view(np.float32))
        _, g_ref, v = NR.mix(x, bank[j], o, scale)
        assert g_ref > 0 and abs(float(gain[b]) - g_ref) <= 2.0 ** -23 * g_ref, (b, gain[b], g_ref)
        want = x.astype(np.float64) + float(gain[b]) * v
        err, bound = np.abs(out[b, :n] - want), 2.0 ** -23 * (np.abs(x) + np.abs(float(gain[b]) * v))
        assert (err <= bound).all(), (b, float((err - bound).max()))
        assert abs(NR.snr_db(x, out[b, :n].astype(np.float64) - x) - snr) < 1e-3       # and the mix has the signal-to-noise ratio asked for
        worst_g, worst_o = max(worst_g, abs(float(gain[b]) - g_ref) / g_ref * 2.0 ** 23), max(worst_o, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"largest gain error / bound {worst_g:.3f}, largest sample error / bound {worst_o:.3f}")


def test_mix_index_arithmetic_is_exact_near_2_31(K):
    """A clip of 2^31 - 64 samples read from its last three samples on: o + n runs up to and past the clip's end, just below 2^31."""
    nlen, n = 2 ** 31 - 64, 300
    noise = torch.zeros(nlen, dtype=torch.float32, device=DEV)
    rng = np.random.RandomState(2)
    head, tail = rng.randn(n).astype(np.float32), rng.randn(3).astype(np.float32)
    noise[:n] = torch.from_numpy(head).to(DEV)
    noise[nlen - 3:] = torch.from_numpy(tail).to(DEV)
    x = rng.uniform(-1, 1, size=n).astype(np.float32)
    wav = place([x], n + 1)
    out, gain = K.noise_mix(wav, dev_i32([n]), dev_i32([[0, nlen - 3, scale_bits(10.0), 0]]), noise, dev_i32([0, nlen]))
    torch.cuda.synchronize()
    v = np.concatenate([tail, head[:n - 3]]).astype(np.float64)
    scale = float(np.array(scale_bits(10.0), dtype=np.int32).view(np.float32))
    g_ref = scale * np.sqrt(np.sum(x.astype(np.float64) ** 2) / np.sum(v * v))
    g = float(gain[0])
    assert abs(g - g_ref) <= 2.0 ** -23 * g_ref
    got = out[0, :n].cpu().numpy()
    assert (np.abs(got - (x + g * v)) <= 2.0 ** -23 * (np.abs(x) + np.abs(g * v))).all() and float(out[0, n]) == 0.0


# ------------------------------------------------------------------------------------------------ loader
N_UTT = 20
N_NOISE, N_RIR = 3, 4


def write_wav(path, x):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype("<i2").tobytes())
    return str(path)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab, WaveDataset
    tmp = tmp_path_factory.mktemp("noise_reverb")
    rng = np.random.RandomState(3)
    items = []
    for i in range(N_UTT):
        n = int(rng.randint(int(0.3 * 16000), int(1.2 * 16000)))
        items.append(((rng.randn(n) * 0.1).astype(np.float32), [4 + i] + [int(t) for t in rng.randint(4, 30, size=rng.randint(1, 5))]))   # first label = utterance id
    noise_paths = [write_wav(tmp / f"noise{j}.wav", rng.randn(n) * 0.05) for j, n in enumerate((700, 9000, 30000))]
    rir_paths = []
    for j, n in enumerate((300, 900, 1500, 2500)):                              # exponentially decaying noise behind a direct path at sample 80 + j
        h = rng.randn(n) * np.exp(-np.arange(n) / (n / 6.0)) * 0.1
        h[:80 + j] *= 0.01
        h[80 + j] = 0.9
        rir_paths.append(write_wav(tmp / f"rir{j}.wav", h))
    vocab = Vocab.synthetic(30)
    return WaveDataset(items, vocab), AudioParser(n_mels=40, lfr_m=4, lfr_n=3, device=DEV), vocab, noise_paths, rir_paths


def epoch(loader):
    """{utterance index: (feature rows (T_b, F) on the host, wave_len)} of one epoch."""
    got = {}
    for pack in loader:
        for r in range(pack.wave.shape[0]):
            n = int(pack.wave_len[r])
            got[int(pack.tgt_for_input[r, 0]) - 4] = (pack.wave[r, :n].float().cpu().numpy(), n)
    return got


def test_loader_augments_per_epoch_and_reproducibly(corpus):
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader, load_wav, noise
    ds, parser, _, noise_paths, rir_paths = corpus
    mk = lambda **kw: BucketedWaveLoader(ds, 4, parser=parser, augment=False, shuffle=True, seed=7, bucket_size=8, dtype=torch.float32, **kw)
    on = dict(noise=noise_paths, rir=rir_paths, noise_prob=0.6, rir_prob=0.6, snr_db=(5, 20))
    loader = mk(**on)
    assert len(loader.noise) == N_NOISE and len(loader.rir) == N_RIR and len(loader) == len(mk()) == 5
    clean, e0, e1 = epoch(mk()), epoch(loader), epoch(loader)
    again = epoch(mk(**on))                                                     # the same seed reproduces the first epoch exactly
    assert all(again[i][1] == e0[i][1] and again[i][0].tobytes() == e0[i][0].tobytes() for i in range(N_UTT))
    draws = [noise.draw_augment(7, ep, N_UTT, 0.6, N_NOISE, loader.noise.lens, (5, 20), 0.6, N_RIR) for ep in (0, 1)]
    assert draws[0] != draws[1]
    for got, (nidx, noff, snr, ridx) in zip((e0, e1), draws):
        assert sorted(got) == list(range(N_UTT))
        for i in range(N_UTT):
            assert got[i][1] == clean[i][1]                                     # lengths never change
            if nidx[i] < 0 and ridx[i] < 0:
                assert got[i][0].tobytes() == clean[i][0].tobytes(), i         # nothing drawn: the clean features, bit for bit
            else:
                assert got[i][0].tobytes() != clean[i][0].tobytes(), i
    assert any(e0[i][0].tobytes() != e1[i][0].tobytes() for i in range(N_UTT))  # epochs differ
    # features of an utterance that drew both == the existing front end on the reference-augmented waveform.  The waveform differs from
    # the reference by at most (L + 1) 2^-24 A per sample after the room and 2^-23 relative after the mix (about 1e-4 of a sample's
    # scale at L = 2500); the tolerance is the one of the log-mel leg of test_bucketed_wave_loader_feeds_the_model, as for speed perturbation
    nidx, noff, snr, ridx = draws[0]
    both = [i for i in range(N_UTT) if nidx[i] >= 0 and ridx[i] >= 0]
    assert both
    for i in both[:2]:
        h, p = NR.rir_prepare(load_wav(rir_paths[ridx[i]])[0])
        y = NR.reverb(ds.wave(i), h.astype(np.float32), p)[0].astype(np.float32)
        scale = float(np.array(noise.snr_scale_bits(snr[i]), dtype=np.int32).view(np.float32))
        z = NR.mix(y, load_wav(noise_paths[nidx[i]])[0], noff[i], scale)[0].astype(np.float32)
        feat, feat_len = parser.parse_batch(torch.from_numpy(z)[None].to(DEV), torch.tensor([z.size], dtype=torch.int32, device=DEV), torch.float32)
        assert int(feat_len[0]) == e0[i][1]
        assert np.allclose(e0[i][0], feat[0, :e0[i][1]].cpu().numpy(), rtol=2e-3, atol=2e-3)


def test_loader_without_noise_and_reverberation_is_bit_identical(corpus):
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader
    ds, parser, _, noise_paths, rir_paths = corpus
    mk = lambda **kw: BucketedWaveLoader(ds, 4, parser=parser, augment=True, shuffle=True, seed=11, bucket_size=8, dtype=torch.float32, **kw)

    def packs(loader):
        return [{k: v.clone() for k, v in p.items() if torch.is_tensor(v)} for _ in range(2) for p in loader]
    a, b, c = packs(mk()), packs(mk(noise=None, rir=None)), packs(mk(noise=noise_paths, rir=rir_paths, noise_prob=0.0, rir_prob=0.0))
    assert len(a) == len(b) == len(c) == 10
    for x, y, z in zip(a, b, c):
        assert sorted(x) == sorted(y) == sorted(z)
        assert all(torch.equal(x[k], y[k]) and torch.equal(x[k], z[k]) for k in x)


def test_joint_model_trains_from_the_augmenting_loader(corpus):
    """Speed perturbation, reverberation and noise together, every utterance augmented, into a few training steps."""
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader
    from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
    ds, parser, vocab, noise_paths, rir_paths = corpus
    torch.manual_seed(0)
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=40, lfr_m=4, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, dropout=0.0, ctc_weight=0.3, dtype="fp32"))
    model = M(cfg, vocab).cuda()
    opt = NoamOpt(64, 1, 10, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
    # one batch holds the whole corpus: three epochs = three steps on the same utterances, each epoch augmented anew
    loader = BucketedWaveLoader(ds, N_UTT, parser=parser, augment=False, shuffle=True, seed=2, dtype=torch.float32, speed_perturb=(0.9, 1.0, 1.1),
                                noise=noise_paths, rir=rir_paths, noise_prob=1.0, rir_prob=1.0)
    losses = [float(model.iterate(pack, optimizer=opt)[0].loss) for _ in range(3) for pack in loader]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
