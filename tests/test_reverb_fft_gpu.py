"""FFT reverberation path on the GPU: the kernels against the float64 definition (tests/noise_ref.py) under the gate the float32
torch.fft restatement defines (tests/reverb_fft_ref.py), their invariants (zero padding, bit-exact copies, repeatability, a workspace
that holds anything), agreement with the direct kernel, the refusals, and the waveform loader with rir_method="fft"."""
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import noise_ref as NR  # noqa: E402
from tests import reverb_fft_cases as C  # noqa: E402
from tests import reverb_fft_ref as FR  # noqa: E402

DEV = "cuda"
BK = FR.BK


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


def launch(K, c, smax, offset=0, ws=None):
    B = len(c["rows"])
    wav = place(c["rows"], smax, offset)
    out = place([np.zeros(0)] * B, smax, offset, fill=7.0)
    rl, rp = dev_i32([L for L, _ in c["resp"]]), dev_i32([p for _, p in c["resp"]])
    got = K.reverb_fft(wav, dev_i32([x.size for x in c["rows"]]), dev_i32(c["idx"]), torch.from_numpy(c["table"]).to(DEV), rl, rp, out=out, ws=ws)
    torch.cuda.synchronize()
    return got.cpu().numpy()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("smax_extra,offset", [(2, 0), (2, 1), (5, 0)], ids=["odd_rows", "misaligned_buffer", "aligned_rows"])
def test_reverb_fft_ragged_batch_against_the_reference(K, smax_extra, offset):
    """|out - ref| <= c 2^-24 S_i on every sample of block i, c = 4 c_ref with c_ref the float32 torch.fft restatement's own largest ratio on
    these cases (tests/reverb_fft_ref.py).  Smax = 2 Bk + 5 is odd - rows start at every alignment -, the second run moves the whole
    buffer by one float, the third has Smax a multiple of 4."""
    c = C.cases()
    smax = 2 * BK + 3 + smax_extra
    assert (smax % 4 == 0) == (smax_extra == 5)
    R = len(c["resp"])
    got = launch(K, c, smax, offset)
    gate = FR.GATE_FACTOR * c["c_ref"]
    worst = {}
    for b, (x, r) in enumerate(zip(c["rows"], c["idx"])):
        n = x.size
        assert not got[b, n:].any(), f"row {b}: not zero from wav_len = {n} on"
        if not 0 <= r < R:
            assert got[b, :n].tobytes() == x.tobytes(), f"row {b}: index {r} is not a copy"
            continue
        y, S = c["ref"][b]
        L = c["resp"][r][0]
        assert np.isfinite(got[b, :n]).all(), (b, n, c["resp"][r])
        worst[L] = max(worst.get(L, 0.0), FR.worst_ratio(got[b, :n], y, S))
    print(f"c_ref {c['c_ref']:.3f} (per length {({L: round(v, 3) for L, v in c['c_ref_by_len'].items()})}), gate {gate:.3f}")
    print("largest |out - ref| / (2^-24 S_i) per response length:", {L: round(v, 3) for L, v in worst.items()})
    assert sorted(worst) == sorted(C.LENGTHS)
    assert all(v <= gate for v in worst.values()), (worst, gate)


def test_second_launch_and_a_workspace_full_of_nan_give_the_same_bits(K):
    c = C.cases()
    smax = 2 * BK + 5
    B, Lcap = len(c["rows"]), c["table"].shape[1]
    a = launch(K, c, smax)
    b = launch(K, c, smax)
    assert a.tobytes() == b.tobytes(), "a second launch gives other bits"
    ws = K.reverb_fft_workspace(B, smax, Lcap, DEV)
    assert ws.numel() * 4 == B * (3 + 1 + 32) * BK * 8
    ws.fill_(float("nan"))
    d = launch(K, c, smax, ws=ws)
    assert np.isfinite(d).all() and a.tobytes() == d.tobytes(), "a stale workspace is read"
    ws.fill_(3.0)
    assert a.tobytes() == launch(K, c, smax, ws=ws).tobytes()


def test_fft_and_direct_kernels_each_meet_their_own_bound(K):
    """L = 8192 and L = 100 in one batch through both kernels: the direct one within (L + 1) 2^-24 A[n], the FFT one within 4 c_ref 2^-24 S_i,
    both of the float64 reference - neither is the other's yardstick.  And the direct kernel still refuses 8193 taps where the FFT path
    takes them."""
    from asr_chinese_e2e_amd._lib import AsrHipError
    rng = np.random.RandomState(6)
    resp = [(8192, 70), (100, 3)]
    table = np.full((2, 8192), np.nan, dtype=np.float32)
    for r, (L, _) in enumerate(resp):
        table[r, :L] = C.response(rng, L)
    rows = [rng.uniform(-1, 1, size=n).astype(np.float32) for n in (2 * BK + 3, 2 * BK + 3, BK + 1, 777)]
    idx = [0, 1, 0, 1]
    smax = 2 * BK + 5
    args = lambda: (place(rows, smax), dev_i32([x.size for x in rows]), dev_i32(idx), torch.from_numpy(table).to(DEV), dev_i32([L for L, _ in resp]),
                    dev_i32([p for _, p in resp]))
    direct, fft = K.reverb(*args()).cpu().numpy(), K.reverb_fft(*args()).cpu().numpy()
    c_ref = 0.0
    checks = []
    for b, (x, r) in enumerate(zip(rows, idx)):
        L, p = resp[r]
        y, A = NR.reverb(x, table[r, :L], p)
        S = FR.block_scale(x, table[r, :L], p)
        c_ref = max(c_ref, FR.worst_ratio(FR.reverb_fft_f32(x, table[r, :L], p), y, S))
        checks.append((b, x.size, L, y, A, S))
    for b, n, L, y, A, S in checks:
        rd, rf = float((np.abs(direct[b, :n] - y) / ((L + 1) * 2.0 ** -24 * A)).max()), FR.worst_ratio(fft[b, :n], y, S)
        print(f"row {b} L = {L}: direct error / bound {rd:.4f}, fft error / (2^-24 S_i) {rf:.3f} (gate {4 * c_ref:.3f})")
        assert rd <= 1.0 and rf <= FR.GATE_FACTOR * c_ref, (b, rd, rf, c_ref)
        assert not direct[b, n:].any() and not fft[b, n:].any()
    wav, out = torch.rand(2, 50, device=DEV), torch.full((2, 50), 7.0, device=DEV)
    rir = torch.rand(1, K.REVERB_MAX_TAPS + 1, device=DEV)
    with pytest.raises(AsrHipError, match="Lcap=8193"):
        K.reverb(wav, dev_i32([50, 50]), dev_i32([0, 0]), rir, dev_i32([3]), dev_i32([0]), out=out)
    got = K.reverb_fft(wav, dev_i32([50, 50]), dev_i32([0, 0]), rir, dev_i32([3]), dev_i32([0]), out=out)
    torch.cuda.synchronize()
    h, x = rir[0, :3].double().cpu().numpy(), wav.double().cpu().numpy()
    assert np.allclose(got.cpu().numpy(), [np.convolve(x[b], h)[:50] for b in range(2)], rtol=0, atol=1e-5)


def test_runtime_refusals_leave_out_untouched_and_a_block_edge_is_data(K):
    from asr_chinese_e2e_amd._lib import AsrHipError
    wav, out = torch.rand(2, 50, device=DEV), torch.full((2, 50), 7.0, device=DEV)
    lens, idx, rl, rp = dev_i32([50, 50]), dev_i32([0, 0]), dev_i32([3]), dev_i32([0])
    with pytest.raises(AsrHipError, match="Lcap=65537"):
        K.reverb_fft(wav, lens, idx, torch.rand(1, K.REVERB_FFT_MAX_TAPS + 1, device=DEV), rl, rp, out=out, ws=K.reverb_fft_workspace(2, 50, 65536, DEV))
    rir = torch.rand(1, 8, device=DEV)
    with pytest.raises(AsrHipError, match="alias"):
        K.reverb_fft(wav, lens, idx, rir, rl, rp, out=wav)
    with pytest.raises(AsrHipError, match="workspace"):
        K.reverb_fft(wav, lens, idx, rir, rl, rp, out=out, ws=K.reverb_fft_workspace(1, 50, 8, DEV))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # len + p ends exactly on a block edge, with Smax = len: samples p .. p + len - 1 = 2 Bk - 1 of `full`; and one sample further
    rng = np.random.RandomState(8)
    L, p = BK + 40, 48
    h = C.response(rng, L)
    table = np.full((1, L), np.nan, dtype=np.float32)
    table[0] = h
    for n in (2 * BK - p, 2 * BK - p + 1):
        x = rng.uniform(-1, 1, size=n).astype(np.float32)
        got = K.reverb_fft(place([x], n), dev_i32([n]), dev_i32([0]), torch.from_numpy(table).to(DEV), dev_i32([L]), dev_i32([p]),
                           out=place([np.zeros(0)], n, fill=7.0)).cpu().numpy()
        y, S = NR.reverb(x, h, p)[0], FR.block_scale(x, h, p)
        c_ref = FR.worst_ratio(FR.reverb_fft_f32(x, h, p), y, S)
        ratio = FR.worst_ratio(got[0], y, S)
        print(f"len {n}: error / (2^-24 S_i) {ratio:.3f}, gate {4 * c_ref:.3f}")
        assert ratio <= FR.GATE_FACTOR * c_ref


# ------------------------------------------------------------------------------------------------ loader
N_UTT = 20
RIR_SAMPLES = (300, 2500, 9000, 20000)


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
    tmp = tmp_path_factory.mktemp("reverb_fft")
    rng = np.random.RandomState(3)
    items = []
    for i in range(N_UTT):
        n = int(rng.randint(int(0.3 * 16000), int(1.2 * 16000)))
        items.append(((rng.randn(n) * 0.1).astype(np.float32), [4 + i] + [int(t) for t in rng.randint(4, 30, size=rng.randint(1, 5))]))   # first label = utterance id
    rir_paths = []
    for j, n in enumerate(RIR_SAMPLES):                                        # exponentially decaying noise behind a direct path at sample 80 + j
        h = rng.randn(n) * np.exp(-np.arange(n) / (n / 6.0)) * 0.1
        h[:80 + j] *= 0.01
        h[80 + j] = 0.9
        rir_paths.append(write_wav(tmp / f"rir{j}.wav", h))
    vocab = Vocab.synthetic(30)
    return WaveDataset(items, vocab), AudioParser(n_mels=40, lfr_m=4, lfr_n=3, device=DEV), vocab, rir_paths


def epoch(loader):
    """{utterance index: (feature rows (T_b, F) on the host, wave_len)} of one epoch."""
    got = {}
    for pack in loader:
        for r in range(pack.wave.shape[0]):
            n = int(pack.wave_len[r])
            got[int(pack.tgt_for_input[r, 0]) - 4] = (pack.wave[r, :n].float().cpu().numpy(), n)
    return got


def test_loader_reverberates_with_long_responses_reproducibly(corpus):
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader, load_wav, noise
    ds, parser, _, rir_paths = corpus
    mk = lambda **kw: BucketedWaveLoader(ds, 4, parser=parser, augment=False, shuffle=True, seed=7, bucket_size=8, dtype=torch.float32, **kw)
    on = dict(rir=rir_paths, rir_prob=0.6, rir_method="fft", rir_max_taps=32768)
    loader = mk(**on)
    assert loader.rir.method == "fft" and loader.rir.max_taps == 32768
    assert loader.rir.lens.tolist() == [n - 16 - j for j, n in enumerate(RIR_SAMPLES)]      # the peak at 80 + j: 16 + j samples dropped, 9000 and 20000 kept whole
    assert mk(rir=rir_paths).rir.lens.tolist() == [300 - 16, 2500 - 17, 8192, 8192] and mk(rir=rir_paths).rir.method == "direct"
    assert mk(rir=rir_paths, rir_method="auto", rir_max_taps=32768).rir.method == "fft"
    ready = noise.RirBank(rir_paths, DEV, max_taps=32768, method="fft")       # a ready-made bank decides by its own method
    assert mk(rir=ready).rir is ready
    clean, e0 = epoch(mk()), epoch(loader)
    again, from_bank = epoch(mk(**on)), epoch(mk(rir=ready, rir_prob=0.6))
    assert all(again[i][1] == e0[i][1] and again[i][0].tobytes() == e0[i][0].tobytes() == from_bank[i][0].tobytes() for i in range(N_UTT))
    _, _, _, ridx = noise.draw_augment(7, 0, N_UTT, 0.5, 0, (), (5, 20), 0.6, len(rir_paths))
    assert sorted(e0) == list(range(N_UTT)) and {2, 3} & set(ridx)
    for i in range(N_UTT):
        assert e0[i][1] == clean[i][1]                                         # lengths never change
        assert (e0[i][0].tobytes() == clean[i][0].tobytes()) == (ridx[i] < 0), i      # nothing drawn: the clean features, bit for bit
    # features of two utterances that drew a long response == the front end on the reference-reverberated waveform (the waveform differs
    # from the reference by about 2^-24 S_i per sample; the tolerance is the one of tests/test_noise_reverb_gpu.py's loader test)
    drew = sorted((i for i in range(N_UTT) if ridx[i] >= 0), key=lambda i: -ridx[i])[:2]
    assert len(drew) == 2 and ridx[drew[0]] >= 2
    for i in drew:
        h, p = NR.rir_prepare(load_wav(rir_paths[ridx[i]])[0], 32768)
        assert h.size == RIR_SAMPLES[ridx[i]] - 16 - ridx[i]
        y = NR.reverb(ds.wave(i), h.astype(np.float32), p)[0].astype(np.float32)
        feat, feat_len = parser.parse_batch(torch.from_numpy(y)[None].to(DEV), torch.tensor([y.size], dtype=torch.int32, device=DEV), torch.float32)
        assert int(feat_len[0]) == e0[i][1]
        assert np.allclose(e0[i][0], feat[0, :e0[i][1]].cpu().numpy(), rtol=2e-3, atol=2e-3)


def test_loader_with_rir_method_direct_is_the_default_bit_for_bit(corpus):
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader
    ds, parser, _, rir_paths = corpus
    mk = lambda **kw: BucketedWaveLoader(ds, 4, parser=parser, augment=True, shuffle=True, seed=11, bucket_size=8, dtype=torch.float32, rir=rir_paths,
                                         rir_prob=0.7, **kw)

    def packs(loader):
        return [{k: v.clone() for k, v in p.items() if torch.is_tensor(v)} for _ in range(2) for p in loader]
    a, b, c = packs(mk()), packs(mk(rir_method="direct")), packs(mk(rir_method="direct", rir_max_taps=8192))
    assert len(a) == len(b) == len(c) == 10
    for x, y, z in zip(a, b, c):
        assert sorted(x) == sorted(y) == sorted(z)
        assert all(torch.equal(x[k], y[k]) and torch.equal(x[k], z[k]) for k in x)
    with pytest.raises(ValueError):
        mk(rir_method="direct", rir_max_taps=8193)
    with pytest.raises(ValueError):
        mk(rir_method="overlap-add")


def test_joint_model_trains_from_the_fft_reverberating_loader(corpus):
    """Speed perturbation and FFT reverberation, every utterance reverberated, into a few training steps."""
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader
    from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
    ds, parser, vocab, rir_paths = corpus
    torch.manual_seed(0)
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=40, lfr_m=4, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, dropout=0.0, ctc_weight=0.3, dtype="fp32"))
    model = M(cfg, vocab).cuda()
    opt = NoamOpt(64, 1, 10, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
    loader = BucketedWaveLoader(ds, N_UTT, parser=parser, augment=False, shuffle=True, seed=2, dtype=torch.float32, speed_perturb=(0.9, 1.0, 1.1),
                                rir=rir_paths, rir_prob=1.0, rir_method="fft", rir_max_taps=32768)
    losses = [float(model.iterate(pack, optimizer=opt)[0].loss) for _ in range(3) for pack in loader]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
