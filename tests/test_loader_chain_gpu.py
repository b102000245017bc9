"""The waveform loader with all four waveform stages on - sample-rate conversion, speed perturbation, reverberation, noise - against the
same kernels called here one after the other: pins the order of the stages and what each hands to the next, bit for bit."""
import wave as wave_module

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTORS = (0.9, 1.0, 1.1)
SEED = 2


def write_wav(path, x, fs):
    with wave_module.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(fs)
        f.writeframes(np.round(np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())
    return str(path)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """Four files of 0.3 to 0.6 s at 16, 44.1, 48 and 16 kHz (first label = utterance index + 4), two responses, two noise clips."""
    d = tmp_path_factory.mktemp("chain")
    rng = np.random.RandomState(9)
    items = []
    for i, (fs, sec) in enumerate([(16000, 0.5), (44100, 0.42), (48000, 0.61), (16000, 0.33)]):
        n = int(sec * fs)
        x = 0.3 * np.sin(2 * np.pi * (200 + 150 * i) * np.arange(n) / fs) + 0.05 * rng.randn(n)
        items.append((write_wav(d / f"utt{i}_{fs}.wav", x, fs), [4 + i] + list(range(10, 10 + i))))
    rirs = []
    for j, n in enumerate((300, 700)):
        h = rng.randn(n) * np.exp(-np.arange(n) / (n / 6.0)) * 0.1
        h[:40 + j] *= 0.01
        h[40 + j] = 0.9
        rirs.append(write_wav(d / f"rir{j}.wav", h, 16000))
    noises = [write_wav(d / f"noise{j}.wav", rng.randn(n) * 0.05, 16000) for j, n in enumerate((700, 9000))]
    return items, rirs, noises


@pytest.mark.parametrize("method", ["direct", "fft"])
def test_four_stages_chained_equal_the_kernels_called_in_order(corpus, method):
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.data_handler import AudioParser, BucketedWaveLoader, Vocab, WaveDataset, load_wav, noise, speed
    items, rirs, noises = corpus
    ds = WaveDataset(items, Vocab.synthetic(30), resample=True)
    parser = AudioParser(n_mels=40, lfr_m=4, lfr_n=3, device=DEV)
    loader = BucketedWaveLoader(ds, 4, parser=parser, augment=False, shuffle=True, seed=SEED, dtype=torch.float32, speed_perturb=FACTORS, noise=noises,
                                rir=rirs, noise_prob=1.0, rir_prob=1.0, rir_method=method, resample=True)
    assert loader.rir.method == method and len(loader) == 1
    pq_np, taps_np = speed.build_tables(FACTORS)
    pq = [tuple(int(v) for v in r) for r in pq_np]
    put = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(DEV)
    waves = [load_wav(p)[0] for p, _ in items]
    rates = [ds.rate(i) for i in range(4)]
    seen = []
    for epoch in (0, 1):
        got = [{k: v.clone() for k, v in p.items() if torch.is_tensor(v)} for p in loader]
        assert len(got) == 1
        got = got[0]
        order = [int(v) - 4 for v in got["tgt_for_input"][:, 0]]                 # the batch's row order, from the first label
        assert sorted(order) == [0, 1, 2, 3]
        fidx = speed.draw_factors(SEED, epoch, 4, len(pq))
        nidx, noff, snr, ridx = noise.draw_augment(SEED, epoch, 4, 1.0, len(loader.noise), loader.noise.lens, (5, 20), 1.0, len(loader.rir))
        assert any(pq[f][0] != pq[f][1] for f in fidx) and min(nidx) >= 0 and min(ridx) >= 0      # this seed: every stage runs in both epochs
        seen.append((fidx, nidx, noff, snr, ridx))
        # the staged batch: source samples, rows as wide as the longest
        sizes = [waves[i].size for i in order]
        wav = np.zeros((4, max(sizes)), dtype=np.float32)
        for r, i in enumerate(order):
            wav[r, :sizes[r]] = waves[i]
        win, rate_idx = loader.rate_table.windows(sizes, [rates[i] for i in order])
        len16 = [int(v) for v in win[:, 4]]
        x, n = K.resample(put(wav, np.float32), put(rate_idx), put(win), *loader.rate_table.dev, max(len16))
        fs = [fidx[i] for i in order]
        x, n = K.speed_perturb(x, n, put(fs), put(pq_np), put(taps_np, np.float32), max(speed.perturbed_len(m, *pq[f]) for m, f in zip(len16, fs)))
        rir = loader.rir
        x = (K.reverb_fft if method == "fft" else K.reverb)(x, n, put([ridx[i] for i in order]), rir.table, rir.lens, rir.peaks)
        par = [(nidx[i], noff[i], noise.snr_scale_bits(snr[i]), 0) for i in order]
        K.noise_mix(x, n, put(par), loader.noise.noise, loader.noise.noise_off, out=x)
        feat, feat_len = parser.parse_batch(x, n, torch.float32, augment=False)
        labels = [items[i][1] for i in order]
        tgt = torch.zeros(4, max(len(t) for t in labels), dtype=torch.int64)
        for r, t in enumerate(labels):
            tgt[r, :len(t)] = torch.tensor(t)
        assert torch.equal(got["wave"], feat)
        assert torch.equal(got["wave_len"], feat_len.long())
        assert torch.equal(got["tgt_for_input"].cpu(), tgt)
        assert torch.equal(got["tgt_len"].cpu(), torch.tensor([len(t) for t in labels]))
    assert seen[0] != seen[1]                                                    # the second epoch draws differently
