"""SpecAugment policies on the GPU: asr_utt_norm_specaug_lfr_fwd / asr_global_norm_specaug_lfr_fwd against the definition
(tests/specaug_ref.py), bit for bit.  The input of the definition is the existing kernels' own float32 output at m = n = 1 without masks
(the normalised frames), its bf16 expectation the torch cast of the float32 one.  Then the waveform loader with a policy against the
loader without one and the definition applied on the host."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import specaug_ref as SR  # noqa: E402

DEV = "cuda"
W = 5
COUNTS = (3, 2, 3)                                             # n_t, n_f, n_s of the crafted, random and hostile rows
POLICY = SR.Policy(warp=W, n_t=3, max_t=20, t_permille=500, n_f=2, max_f=10, n_s=3, sub_t=9)
# frames per utterance: 0 .. 5 and 67 inside ragged, padded batches, 2 W + 1 (one warp position) and 2 W (none)
BATCHES = (([0, 1, 2, 3], 5), ([4, 5, 67, 2 * W + 1], 70), ([2 * W, 67, 30, 67], 70))


def crafted(T, second):
    """Rows by hand for an utterance of T frames (mel ranges inside 23 bins)."""
    if T == 67 and not second:
        # wc = W with ww = 1; time masks that overlap, one empty; mel masks that overlap; substitutions with p = 0, with p = s, and one that
        # overlaps the one before it
        return [W, 1, 10, 20, 15, 30, 40, 40, 3, 9, 5, 12, 40, 45, 0, 50, 55, 50, 52, 60, 7]
    if T == 67:
        # ww = T - 1; a substitution whose frames lie in a time mask, one whose SOURCE frames do, one with p = s up to the last frame
        return [30, 66, 10, 20, 0, 0, 66, 67, 20, 23, 0, 0, 12, 18, 2, 22, 26, 8, 60, 67, 60]
    if T == 30:
        return [W, 2 * W, 0, 30, 3, 4, 0, 0, 0, 1, 0, 0, 5, 9, 2, 0, 0, 0, 0, 0, 0]      # a time mask over everything
    if T == 2 * W + 1:
        return [W, 2 * W, 2, 4, 3, 6, 0, 0, 0, 23, 0, 0, 6, 9, 0, 8, 10, 8, 7, 11, 3] if second else \
               [W, 1, 2, 4, 3, 6, 0, 0, 3, 9, 5, 12, 6, 9, 0, 8, 10, 8, 7, 11, 3]         # ww = T - 1 / ww = 1; a mel mask over everything
    # T = 0 .. 5 and 2 W: first frame, last frame, a warp by one frame where there is room; what does not fit is clamped away
    return [1, 2 if second else 1, 0, 1, T - 1, T, 0, 0, 0, 1, 22, 23, 1, 2, 1, 0, T, 0, T - 1, T, T - 1]


def hostile(T, rng):
    """Negative values, values past T, e < s, p > s, warp boundaries outside (0, T)."""
    pick = lambda: int(rng.choice([-2 ** 31, -100, -1, 0, 1, T - 1, T, T + 1, 200, 2 ** 31 - 1, int(rng.integers(-5, T + 6))]))
    return [pick() for _ in range(2 + 2 * COUNTS[0] + 2 * COUNTS[1] + 3 * COUNTS[2])]


def lengths_for(frames, equivalent):
    """Samples that make the kernels count `frames` frames: the Kaldi front end's equivalent lengths 160 (T - 1) + 1, or the longest
    length with that count."""
    return [0 if T == 0 else 160 * (T - 1) + 1 if equivalent else 160 * T - 1 for T in frames]


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


class Case:
    """One batch under one normalisation and bin count: the features, the existing kernels' normalised frames, and the launches."""

    def __init__(self, K, norm, F, frames, Tmax, seed):
        rng = np.random.default_rng(seed)
        self.K, self.norm, self.F, self.frames, self.Tmax, self.B = K, norm, F, frames, Tmax, len(frames)
        self.feat = torch.from_numpy((rng.standard_normal((self.B, Tmax, F)) * 3.0 - 7.0).astype(np.float32)).to(DEV)
        self.wl = torch.tensor(lengths_for(frames, equivalent=seed % 2 == 0), dtype=torch.int32, device=DEV)
        self.mean = torch.from_numpy((rng.standard_normal(F) - 7.0).astype(np.float32)).to(DEV)
        self.istd = torch.from_numpy(rng.uniform(0.2, 0.6, F).astype(np.float32)).to(DEV)
        x, xl = self.plain(1, 1, Tmax, torch.float32)
        assert xl.tolist() == frames
        self.x = x.cpu().numpy()                                   # normalised frames (B, Tmax, F); rows past an utterance's frames are 0
        self._applied = {}

    def plain(self, m, n, Tl, dtype):
        if self.norm == "global":
            return self.K.global_norm_lfr(self.feat, self.wl, self.mean, self.istd, m, n, Tl, dtype)
        return self.K.utt_norm_lfr(self.feat, self.wl, m, n, Tl, dtype)

    def spec(self, rows, counts, m, n, Tl, dtype, pad=0):
        rg = torch.full((self.B, len(rows[0]) + pad), 12345, dtype=torch.int32)
        rg[:, :len(rows[0])] = torch.tensor(rows, dtype=torch.int64).to(torch.int32)
        rg = rg.to(DEV)
        if self.norm == "global":
            return self.K.global_norm_specaug_lfr(self.feat, self.wl, rg, counts, self.mean, self.istd, m, n, Tl, dtype)
        return self.K.utt_norm_specaug_lfr(self.feat, self.wl, rg, counts, m, n, Tl, dtype)

    def applied(self, rows, counts):
        """The definition on every utterance's frames (computed once per row set)."""
        key = (tuple(map(tuple, rows)), counts)
        if key not in self._applied:
            self._applied[key] = [SR.apply(self.x[b, :T], rows[b], *counts) for b, T in enumerate(self.frames)]
        return self._applied[key]

    def expect(self, ys, m, n, Tl):
        out = np.stack([SR.stack(y, m, n, Tl)[0] for y in ys])
        return torch.from_numpy(out), [min(-(-T // n), Tl) for T in self.frames]


def same_bits(got, want):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    return torch.equal(got.view(view), want.view(view))


@pytest.fixture(scope="module")
def cases(K):
    return {(norm, F): [Case(K, norm, F, frames, Tmax, seed=10 * i + j) for i, (frames, Tmax) in enumerate(BATCHES)]
            for j, (norm, F) in enumerate((("utterance", 80), ("utterance", 23), ("global", 80), ("global", 23)))}


def row_sets(case, seed):
    rng = np.random.default_rng(seed)
    draws = SR.draw(seed, 0, case.B, POLICY)
    return {
        "crafted": [crafted(T, False) for T in case.frames],
        "crafted2": [crafted(T, True) for T in case.frames],
        "resolved": [SR.resolve(POLICY, draws[b], T, case.F).tolist() for b, T in enumerate(case.frames)],
        "hostile": [hostile(T, rng) for T in case.frames],
    }


@pytest.mark.parametrize("norm", ["utterance", "global"])
@pytest.mark.parametrize("F", [80, 23])
def test_kernels_equal_the_definition_bit_for_bit(cases, norm, F):
    touched = 0
    for ci, case in enumerate(cases[(norm, F)]):
        sets = row_sets(case, seed=ci)
        for m, n in ((4, 3), (1, 1)):
            Tl = -(-case.Tmax // n)
            plain_f32, plain_len = case.plain(m, n, Tl, torch.float32)
            want_plain, want_len = case.expect([case.x[b, :T] for b, T in enumerate(case.frames)], m, n, Tl)
            assert same_bits(plain_f32, want_plain) and plain_len.tolist() == want_len
            # the existing no-mask bf16 output is the torch cast of the float32 one: what lets the bf16 expectation be a cast
            assert same_bits(case.plain(m, n, Tl, torch.bfloat16)[0], want_plain.to(torch.bfloat16))
            for name, rows in sets.items():
                want, want_len = case.expect(case.applied(rows, COUNTS), m, n, Tl)
                for dtype in (torch.float32, torch.bfloat16):
                    got, got_len = case.spec(rows, COUNTS, m, n, Tl, dtype, pad=ci)      # rows further apart than their width, too
                    assert got_len.tolist() == want_len, (name, m, n)
                    assert same_bits(got, want.to(dtype)), (name, m, n, dtype, case.frames)
                    again, again_len = case.spec(rows, COUNTS, m, n, Tl, dtype, pad=ci)
                    assert same_bits(again, got.cpu()) and torch.equal(again_len, got_len), "a second launch gives other bits"
                touched += int(not torch.equal(want, want_plain))
    assert touched >= 12      # the rows do something: at least the crafted and resolved sets change the two long batches under both stackings


@pytest.mark.parametrize("norm", ["utterance", "global"])
def test_zero_rows_and_full_policies(cases, norm):
    """An all-zero row gives the bits of the entry points without masks, whatever the counts; eight ranges of every kind."""
    full = SR.Policy(warp=W, n_t=8, max_t=9, n_f=8, max_f=4, n_s=8, sub_t=5)
    for F in (80, 23):
        for ci, case in enumerate(cases[(norm, F)]):
            for m, n in ((4, 3), (1, 1)):
                Tl = -(-case.Tmax // n)
                for dtype in (torch.float32, torch.bfloat16):
                    plain, plain_len = case.plain(m, n, Tl, dtype)
                    for counts in ((0, 0, 0), COUNTS, (8, 8, 8)):
                        zero = [[0] * (2 + 2 * counts[0] + 2 * counts[1] + 3 * counts[2])] * case.B
                        got, got_len = case.spec(zero, counts, m, n, Tl, dtype)
                        assert same_bits(got, plain.cpu()) and torch.equal(got_len, plain_len), (F, ci, m, n, dtype, counts)
            draws = SR.draw(3, ci, case.B, full)
            rows = [SR.resolve(full, draws[b], T, F).tolist() for b, T in enumerate(case.frames)]
            want, want_len = case.expect(case.applied(rows, (8, 8, 8)), 4, 3, -(-case.Tmax // 3))
            got, got_len = case.spec(rows, (8, 8, 8), 4, 3, -(-case.Tmax // 3), torch.float32, pad=3)
            assert same_bits(got, want) and got_len.tolist() == want_len


def test_refusals_return_before_a_launch(K, cases):
    from asr_chinese_e2e_amd import _lib
    case = cases[("global", 23)][1]
    rg = torch.zeros(case.B, 19, dtype=torch.int32, device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.full((case.B, 24, 4 * 23), -1e30, dtype=dtype, device=DEV)
        out_len = torch.full((case.B,), -7, dtype=torch.int32, device=DEV)
        untouched = out.clone()
        p = lambda t: t.data_ptr()
        dt = K._dt(out)

        def utt(feat=p(case.feat), wl=p(case.wl), r=p(rg), ld=19, nt=2, nf=2, ns=3, o=p(out), ol=p(out_len), B=case.B, Tmax=70, F=23, m=4, n=3, Tl=24, d=dt):
            return _lib.fast.asr_utt_norm_specaug_lfr_fwd(feat, wl, r, ld, nt, nf, ns, o, ol, B, Tmax, F, m, n, Tl, d, None)

        def glob(feat=p(case.feat), wl=p(case.wl), r=p(rg), ld=19, nt=2, nf=2, ns=3, mean=p(case.mean), istd=p(case.istd), o=p(out), ol=p(out_len),
                 B=case.B, Tmax=70, F=23, m=4, n=3, Tl=24, d=dt):
            return _lib.fast.asr_global_norm_specaug_lfr_fwd(feat, wl, r, ld, nt, nf, ns, mean, istd, o, ol, B, Tmax, F, m, n, Tl, d, None)

        for f in (utt, glob):
            for kw in (dict(feat=None), dict(wl=None), dict(r=None), dict(o=None), dict(ol=None), dict(nt=9), dict(nf=9), dict(ns=9), dict(nt=-1),
                       dict(ld=18), dict(nt=8, nf=8, ns=8, ld=57), dict(B=0), dict(Tmax=0), dict(F=0), dict(m=0), dict(n=0), dict(Tl=0)):
                assert f(**kw) == -1, kw
            assert f(d=7) == -2
        assert glob(mean=None) == -1 and glob(istd=None) == -1 and glob(B=65536) == -1
        torch.cuda.synchronize()
        assert torch.equal(out, untouched) and bool((out_len == -7).all())      # nothing ran
        assert utt() == 0 and glob() == 0                                       # the same calls with every argument in range do
        torch.cuda.synchronize()
        assert out_len.tolist() == [2, 2, 23, 4] and not bool((out == untouched).any())
    for bad in (rg[:, :18], rg[:3], rg.long(), rg.t().contiguous().t()):
        with pytest.raises(ValueError):
            K.utt_norm_specaug_lfr(case.feat, case.wl, bad, (2, 2, 3), 4, 3, 24)
    with pytest.raises(ValueError):
        K.global_norm_specaug_lfr(case.feat, case.wl, rg, (2, 9, 3), case.mean, case.istd, 4, 3, 24)


# ------------------------------------------------------------------------------------------------ loader
N_UTT = 6
E2E_POLICY = "w5,t2x20,f2x10,s2x9,r500"


def corpus(rate, seed):
    from asr_chinese_e2e_amd.data_handler import Vocab, WaveDataset
    rng = np.random.RandomState(seed)
    items = []
    for i in range(N_UTT):
        n = int(rng.randint(3000, 9500)) * rate // 16000
        item = ((rng.randn(n) * 0.1).astype(np.float32), [4 + i, int(rng.randint(4, 30))])      # first label = utterance id
        items.append(item + (rate,) if rate != 16000 else item)
    return WaveDataset(items, Vocab.synthetic(30), resample=rate != 16000)


def epochs(loader, n=2):
    """[{utterance index: (rows (wave_len, width) on the host, wave_len, rows past wave_len all zero)}] of n epochs."""
    out = []
    for _ in range(n):
        got = {}
        for pack in loader:
            assert pack.wave.shape[0] == 3
            for r in range(3):
                k = int(pack.wave_len[r])
                got[int(pack.tgt_for_input[r, 0]) - 4] = (pack.wave[r, :k].cpu().clone(), k, not bool(pack.wave[r, k:].any()))
        assert sorted(got) == list(range(N_UTT))
        out.append(got)
    return out


@pytest.mark.parametrize("variant", ["speed", "kaldi_global_bf16", "resample48k_global"])
def test_loader_with_a_policy_equals_the_definition_on_the_loader_without(variant):
    from asr_chinese_e2e_amd.data_handler import AudioParser, BucketedWaveLoader, resample, speed
    from asr_chinese_e2e_amd.data_handler.specaug import SpecAugmentPolicy
    F, m, n, seed = 23, 4, 3, 5
    rate = 48000 if variant.startswith("resample") else 16000
    ds = corpus(rate, seed=1)
    rng = np.random.RandomState(2)
    pkw = dict(n_mels=F, device=DEV, frontend="kaldi" if variant.startswith("kaldi") else "reference")
    if "global" in variant:
        pkw.update(norm="global", cmvn=(rng.randn(F) - 9.0, rng.uniform(0.2, 0.5, F)))
    dtype = torch.bfloat16 if variant.endswith("bf16") else torch.float32
    lkw = dict(shuffle=True, seed=seed, bucket_size=6)
    if variant == "speed":
        lkw.update(speed_perturb=(0.9, 1.0, 1.1))
    if rate != 16000:
        lkw.update(resample=True)
    frames = epochs(BucketedWaveLoader(ds, 3, parser=AudioParser(lfr_m=1, lfr_n=1, **pkw), dtype=torch.float32, **lkw))
    parser = AudioParser(lfr_m=m, lfr_n=n, **pkw)
    loader = BucketedWaveLoader(ds, 3, parser=parser, dtype=dtype, spec_augment=E2E_POLICY, **lkw)
    assert loader.spec == SpecAugmentPolicy.from_string(E2E_POLICY)
    state = loader.rng.getstate()
    got = epochs(loader)
    pol = SR.Policy(warp=5, n_t=2, max_t=20, t_permille=500, n_f=2, max_f=10, n_s=2, sub_t=9)
    pq = [speed.parse_factor(s) for s in (0.9, 1.0, 1.1)]
    changed = 0
    for e in range(2):
        draws = SR.draw(seed, e, N_UTT, pol)
        fidx = speed.draw_factors(seed, e, N_UTT, 3)
        for i in range(N_UTT):
            x, T, _ = frames[e][i]
            # the host's frame count (from the lengths pack_meta decides) is the device's
            length = ds.num_samples(i)
            if rate != 16000:
                length = resample.plan(rate).n_out(length)
            if variant == "speed":
                length = speed.perturbed_len(length, *pq[fidx[i]])
            assert T == parser.num_frames(length) and 2 * 5 < T <= 70, (variant, e, i, T, length)
            row = SR.resolve(pol, draws[i], T, F)
            want, Tl = SR.stack(SR.apply(x.numpy(), row, pol.n_t, pol.n_f, pol.n_s), m, n, -(-T // n))
            rows, k, zero_tail = got[e][i]
            assert k == Tl == -(-T // n) and zero_tail, (variant, e, i)
            assert same_bits(rows, torch.from_numpy(want).to(dtype)), (variant, e, i, row.tolist())
            changed += int(not np.array_equal(want, SR.stack(x.numpy(), m, n, Tl)[0]))
    assert changed == 2 * N_UTT                                # every utterance of both epochs was augmented
    if variant != "speed":                                     # the same waveforms in both epochs: only the policy's draws make them differ
        assert not any(same_bits(got[0][i][0], got[1][i][0]) for i in range(N_UTT))
    # the loader's generator is the batch order's alone: a loader without a policy is in the same state after two epochs
    other = BucketedWaveLoader(ds, 3, parser=parser, dtype=dtype, **lkw)
    assert other.rng.getstate() == state
    epochs(other)
    assert other.rng.getstate() == loader.rng.getstate()
