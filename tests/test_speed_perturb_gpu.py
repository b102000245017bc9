"""Speed perturbation on the GPU: the kernel against the float64 reference (tests/speed_ref.py) under a derived bound, its invariants
(lengths, zero padding, bit-exact factor 1, repeatability), and the waveform loader with the perturbation on and off."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import speed_ref as SR  # noqa: E402

DEV = "cuda"
FACTORS = (0.9, 1.0, 1.1)


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def run_kernel(K, wav, lens, fac, factors, smax_out):
    from asr_chinese_e2e_amd.data_handler import speed
    pq, taps = speed.build_tables(factors)
    out, out_len = K.speed_perturb(torch.from_numpy(wav).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV),
                                   torch.tensor(fac, dtype=torch.int32, device=DEV), torch.from_numpy(pq).to(DEV), torch.from_numpy(taps).to(DEV), smax_out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_len.cpu().numpy(), pq, taps


def gate(p, q, xmax):
    """|y_gpu - y_ref| <= (ntaps + 2) 2^-24 max_r sum_j |H[r][j]| max|x|: fp32 accumulation of ntaps products plus the one rounding of the
    table and of the store.  H is the factor's own float32 table (2 W + 1 taps: the zeros that centre it in a wider common table add
    exact zeros)."""
    from asr_chinese_e2e_amd.data_handler import speed
    H = speed.phase_table(p, q).astype(np.float32).astype(np.float64)
    return (H.shape[1] + 2) * 2.0 ** -24 * float(np.abs(H).sum(axis=1).max()) * xmax


def check_batch(K, lens, fac, factors, smax, extra, seed=0):
    from asr_chinese_e2e_amd.data_handler import speed
    rng = np.random.RandomState(seed)
    B = len(lens)
    wav = rng.uniform(-1.0, 1.0, size=(B, smax)).astype(np.float32)
    for b, l in enumerate(lens):
        wav[b, l:] = np.nan                                  # garbage beyond wav_len must never reach the output
    pq = [speed.parse_factor(s) for s in factors]
    n_outs = [speed.perturbed_len(l, *pq[f]) for l, f in zip(lens, fac)]
    smax_out = max(max(n_outs), 1) + extra
    out, out_len, _, taps = run_kernel(K, wav, lens, fac, factors, smax_out)
    again = run_kernel(K, wav, lens, fac, factors, smax_out)
    assert out.tobytes() == again[0].tobytes() and np.array_equal(out_len, again[1]), "a second launch gives other bits"
    assert out_len.tolist() == n_outs == [SR.n_out(l, *pq[f]) for l, f in zip(lens, fac)]
    bounds = {f: gate(*pq[f], 1.0) for f in set(fac) if pq[f][0] != pq[f][1]}
    worst = {f: 0.0 for f in bounds}
    for b in range(B):
        n = n_outs[b]
        assert not out[b, n:].any() and np.isfinite(out[b]).all(), f"row {b}: not zero at and beyond n_out = {n}"
        if pq[fac[b]][0] == pq[fac[b]][1]:
            assert out[b, :n].tobytes() == wav[b, :n].tobytes(), f"row {b}: factor 1 is not a copy"
        elif n:
            worst[fac[b]] = max(worst[fac[b]], float(np.abs(out[b, :n] - SR.perturb(wav[b, :lens[b]], *pq[fac[b]])).max()))
    for f in bounds:
        print(f"factor {pq[f][0]}/{pq[f][1]}: max |y_gpu - y_ref| = {worst[f]:.3g}, bound {bounds[f]:.3g}")
    assert all(worst[f] <= bounds[f] for f in bounds), (worst, bounds)
    return bounds


def test_ragged_batch_with_every_factor_and_edge_length(K):
    """Lengths 0, 1, 2, W, W + 1, the tile edges (input AND output side), one odd Smax (rows start at every alignment) and an Smax_out
    beyond every n_out; every length with every factor."""
    T, W = K.SPEED_TILE, 7
    base = [0, 1, 2, W, W + 1, T - 1, T, T + 1, 2 * T + 3, 1500, 333]
    # input lengths whose OUTPUT length sits on the tile edges for 9/10 and 11/10
    edge = [(T - 1) * 9 // 10, T * 9 // 10, (T * 9 + 9) // 10 + 1, (T * 11 + 9) // 10, (T * 11) // 10 + 2, ((2 * T + 3) * 11) // 10]
    lens = [l for l in base + edge for _ in FACTORS]
    fac = [i % 3 for i in range(len(lens))]
    bounds = check_batch(K, lens, fac, FACTORS, smax=(max(lens) + 1) | 1, extra=T + 5)      # odd Smax
    assert all(1.5e-6 < v < 2.5e-6 for v in bounds.values()), bounds      # about 1.9e-6 for |x| <= 1: computed from the table, checked against the estimate
    check_batch(K, lens[:12], fac[:12], FACTORS, smax=max(lens[:12]) + 4 - max(lens[:12]) % 4, extra=0, seed=1)   # Smax % 4 == 0, Smax_out = max n_out


def test_all_zero_length_batch_and_all_factor_one(K):
    check_batch(K, [0, 0, 0], [0, 1, 2], FACTORS, smax=9, extra=0)
    check_batch(K, [5, 2050, 0, 1024], [1, 1, 1, 1], FACTORS, smax=2051, extra=3)


def test_twenty_phases_and_a_wide_filter(K):
    T = K.SPEED_TILE
    check_batch(K, [T + 1, 2 * T + 3, 50, 0, 1999], [0, 0, 0, 0, 1], ("0.95", 1.0), smax=2 * T + 5, extra=2)
    # p/q = 2 and 1/2 with 0.9 in one table: 27 taps (the generic tap loop), narrower filters centred in it, several staging passes for 2
    check_batch(K, [3000, 700, 1025, 13], [0, 1, 2, 1], (2, 0.5, 0.9), smax=3001, extra=1)


# ------------------------------------------------------------------------------------------------ loader
N_UTT = 20


@pytest.fixture(scope="module")
def corpus():
    from asr_chinese_e2e_amd.data_handler import AudioParser, Vocab, WaveDataset
    rng = np.random.RandomState(3)
    items = []
    for i in range(N_UTT):
        n = int(rng.randint(int(0.3 * 16000), int(1.2 * 16000)))
        items.append(((rng.randn(n) * 0.1).astype(np.float32), [4 + i] + [int(t) for t in rng.randint(4, 30, size=rng.randint(1, 5))]))   # first label = utterance id
    vocab = Vocab.synthetic(30)
    return WaveDataset(items, vocab), AudioParser(n_mels=40, lfr_m=4, lfr_n=3, device=DEV), vocab


def epoch(loader):
    """{utterance index: (feature rows (T_b, F) on the host, wave_len)} of one epoch."""
    got = {}
    for pack in loader:
        for r in range(pack.wave.shape[0]):
            n = int(pack.wave_len[r])
            got[int(pack.tgt_for_input[r, 0]) - 4] = (pack.wave[r, :n].float().cpu().numpy(), n)
    return got


def test_loader_perturbs_per_epoch_and_reproducibly(corpus):
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader, speed
    ds, parser, _ = corpus
    mk = lambda **kw: BucketedWaveLoader(ds, 4, parser=parser, augment=False, shuffle=True, seed=7, bucket_size=8, dtype=torch.float32, **kw)
    loader = mk(speed_perturb=FACTORS)
    assert len(loader) == len(mk()) == 5
    pq = [speed.parse_factor(s) for s in FACTORS]
    e0, e1 = epoch(loader), epoch(loader)
    f0, f1 = speed.draw_factors(7, 0, N_UTT, 3), speed.draw_factors(7, 1, N_UTT, 3)
    assert f0 != f1 and len(set(f0)) == 3
    for got, fidx in ((e0, f0), (e1, f1)):
        assert sorted(got) == list(range(N_UTT))
        for i in range(N_UTT):
            n_out = speed.perturbed_len(ds.num_samples(i), *pq[fidx[i]])
            assert got[i][1] == -(-(1 + n_out // 160) // 3), (i, fidx[i])
    assert any(e0[i][1] != e1[i][1] for i in range(N_UTT))                      # frame counts change from epoch to epoch
    again = epoch(mk(speed_perturb=FACTORS))                                    # the same seed reproduces the first epoch exactly
    assert all(again[i][1] == e0[i][1] and again[i][0].tobytes() == e0[i][0].tobytes() for i in range(N_UTT))
    # features of one resampled utterance == the existing front end on the reference-perturbed waveform (tolerance of the log-mel leg of
    # test_bucketed_wave_loader_feeds_the_model)
    i = next(i for i in range(N_UTT) if f0[i] != 1)
    y = SR.perturb(ds.wave(i), *pq[f0[i]]).astype(np.float32)
    feat, feat_len = parser.parse_batch(torch.from_numpy(y)[None].to(DEV), torch.tensor([y.size], dtype=torch.int32, device=DEV), torch.float32)
    assert int(feat_len[0]) == e0[i][1]
    assert np.allclose(e0[i][0], feat[0, :e0[i][1]].cpu().numpy(), rtol=2e-3, atol=2e-3)


def test_loader_without_speed_perturbation_is_bit_identical(corpus):
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader
    ds, parser, _ = corpus
    mk = lambda **kw: BucketedWaveLoader(ds, 4, parser=parser, augment=True, shuffle=True, seed=11, bucket_size=8, dtype=torch.float32, **kw)

    def packs(loader):
        return [{k: v.clone() for k, v in p.items() if torch.is_tensor(v)} for _ in range(2) for p in loader]
    a, b, c = packs(mk()), packs(mk(speed_perturb=None)), packs(mk(speed_perturb=()))
    assert len(a) == len(b) == len(c) == 10
    for x, y, z in zip(a, b, c):
        assert sorted(x) == sorted(y) == sorted(z)
        assert all(torch.equal(x[k], y[k]) and torch.equal(x[k], z[k]) for k in x)


def test_joint_model_trains_from_the_perturbing_loader(corpus):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import BucketedWaveLoader
    from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
    ds, parser, vocab = corpus
    torch.manual_seed(0)
    M = Models.TransformerOffical
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=40, lfr_m=4, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=2, dropout=0.0, ctc_weight=0.3, dtype="fp32"))
    model = M(cfg, vocab).cuda()
    opt = NoamOpt(64, 1, 10, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
    # one batch holds the whole corpus: three epochs = three steps on the same utterances, each epoch at newly drawn speeds
    loader = BucketedWaveLoader(ds, N_UTT, parser=parser, augment=False, shuffle=True, seed=2, dtype=torch.float32, speed_perturb=FACTORS)
    losses = [float(model.iterate(pack, optimizer=opt)[0].loss) for _ in range(3) for pack in loader]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert losses[1] <= losses[0] and losses[2] <= losses[1]
