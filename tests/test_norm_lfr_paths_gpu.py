"""The paths of the one normalise-augment-stack kernel (csrc/logmel.hip: norm_aug_lfr_kernel) that nothing else pins: empty reference
masks against none, what a reference mask may touch, the tiled grid past one pass of its largest launch, and the refusals the
utterance entries share with the global ones.

Fill values: under global CMVN they are held to tests/cmvn_ref.py within the relative 1e-5 of tests/test_cmvn_gpu.py.  Under utterance
normalisation the feature has mean 0 and deviation 1, so in the float64 definition (oracle/logmel_ref.py) the time fill is ~1e-17 and
the mel fill - the mean of what the time mask left - is 0 to 1e-2: an error relative to such a value measures the value, not the
kernel.  There the 1e-5 is taken relative to the feature's deviation, which is 1: an absolute 1e-5.  (The fp32 mean of ~5 carries ~1e-6
of relative error; divided by the deviation of 3 that moves every normalised value, and so both fills, by a few 1e-6.  Measured on
an MI355X: at most 1.7e-7 under either normalisation.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import logmel_ref as LM  # noqa: E402
from tests import cmvn_ref as CR  # noqa: E402
from tests import specaug_ref as SR  # noqa: E402

DEV = "cuda"
F = 40
LENS = [0, 1, 160 * 25, 160 * 77 + 159]                       # samples: no frame, one frame, a boundary, ragged
FRAMES = [CR.total_frames(l) for l in LENS]                   # 0, 1, 26, 78
TMAX = max(FRAMES)
MASKS = [[0, 0, 0, 0], [0, 1, 3, 9], [5, 17, 30, 40], [70, 90, 0, 11]]      # the last one runs past the end of its utterance
NORMS = ("utterance", "global")
DTYPES = (torch.float32, torch.bfloat16)
LFR = ((1, 1), (4, 3))


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def same_bits(got, want):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    return torch.equal(got.view(view), want.view(view))


class Batch:
    """Features (B, Tmax, n_mels), lengths in samples and global statistics, and the four calls on them."""

    def __init__(self, K, feat_np, lens, mean_np, istd_np):
        self.K, self.B, self.Tmax, self.feat_np, self.mean_np, self.istd_np = K, feat_np.shape[0], feat_np.shape[1], feat_np, mean_np, istd_np
        self.feat, self.mean, self.istd = (torch.from_numpy(v).to(DEV) for v in (feat_np, mean_np, istd_np))
        self.wl = torch.tensor(lens, dtype=torch.int32, device=DEV)

    @staticmethod
    def random(K, frames, lens, n_mels, seed):
        rng = np.random.RandomState(seed)
        feat = (rng.randn(len(frames), max(frames), n_mels) * 3 - 5).astype(np.float32)      # log-mel-like
        return Batch(K, feat, lens, (rng.randn(n_mels) - 5).astype(np.float32), rng.uniform(0.2, 0.6, n_mels).astype(np.float32))

    def run(self, norm, m, n, Tl, dtype, masks=None):
        masks = None if masks is None else torch.tensor(masks, dtype=torch.int32, device=DEV)
        if norm == "global":
            return self.K.global_norm_lfr(self.feat, self.wl, self.mean, self.istd, m, n, Tl, dtype, masks=masks)
        return self.K.utt_norm_lfr(self.feat, self.wl, m, n, Tl, dtype, masks=masks)

    def policy(self, norm, rows, counts, m, n, Tl, dtype):
        rg = torch.tensor(rows, dtype=torch.int32, device=DEV)
        if norm == "global":
            return self.K.global_norm_specaug_lfr(self.feat, self.wl, rg, counts, self.mean, self.istd, m, n, Tl, dtype)
        return self.K.utt_norm_specaug_lfr(self.feat, self.wl, rg, counts, m, n, Tl, dtype)


@pytest.fixture(scope="module")
def batch(K):
    return Batch.random(K, FRAMES, LENS, F, seed=5)          # the empty utterance's rows hold features too: none may come out


@pytest.mark.parametrize("norm", NORMS)
def test_empty_reference_masks_are_no_masks(batch, norm):
    for m, n in LFR:
        Tl = -(-TMAX // n)
        want_len = [-(-T // n) for T in FRAMES]
        for dtype in DTYPES:
            plain, plain_len = batch.run(norm, m, n, Tl, dtype)
            got, got_len = batch.run(norm, m, n, Tl, dtype, masks=[[0, 0, 0, 0]] * batch.B)
            zero, zero_len = batch.policy(norm, [[0] * 21] * batch.B, (3, 2, 3), m, n, Tl, dtype)
            assert plain_len.tolist() == want_len and got_len.tolist() == want_len and zero_len.tolist() == want_len
            assert same_bits(got, plain.cpu()) and same_bits(zero, plain.cpu()), (m, n, dtype)
            for out in (plain, got, zero):                     # the empty utterance: nothing but zero rows on every path
                assert not bool(out[0].any()), (m, n, dtype)
            assert bool(plain[3, :want_len[3]].ne(0).all()) and not bool(plain[2, want_len[2]:].any())


def fills_of_the_definition(batch, norm, b):
    """(time fill, mel fill, scale the 1e-5 is relative to) of utterance b in float64."""
    T = FRAMES[b]
    if norm == "global":
        _, _, fills = CR.apply(batch.feat_np, LENS, batch.mean_np.astype(np.float64), batch.istd_np.astype(np.float64), 1, 1, TMAX, masks=MASKS)
        return fills[b, 0], fills[b, 1], None
    x = LM.utt_normalize(batch.feat_np[b, :T].astype(np.float64))
    t0, t1, f0, f1 = MASKS[b]
    y = x.copy()
    y[t0:min(t1, T)] = x.mean()
    return x.mean(), y.mean(), 1.0


@pytest.mark.parametrize("norm", NORMS)
def test_reference_masks_touch_only_what_they_cover(batch, norm):
    for m, n in LFR:
        Tl = -(-TMAX // n)
        plain, _ = batch.run(norm, m, n, Tl, torch.float32)
        got, got_len = batch.run(norm, m, n, Tl, torch.float32, masks=MASKS)
        got16, len16 = batch.run(norm, m, n, Tl, torch.bfloat16, masks=MASKS)
        assert same_bits(got16, got.cpu().to(torch.bfloat16)) and torch.equal(len16, got_len)
        assert got_len.tolist() == [-(-T // n) for T in FRAMES]
        g, p = got.cpu().numpy().view(np.int32), plain.cpu().numpy().view(np.int32)
        assert np.array_equal(g[0], p[0])                      # the empty utterance and the empty mask
        for b in (1, 2, 3):
            T, rows = FRAMES[b], -(-FRAMES[b] // n)
            t0, t1, f0, f1 = MASKS[b]
            t1 = min(t1, T)
            src = np.minimum(np.arange(rows)[:, None] * n + np.arange(m)[None, :], T - 1)      # (rows, m): the frame of every stacked slot
            in_t = np.broadcast_to(((src >= t0) & (src < t1))[:, :, None], (rows, m, F))
            in_f = np.broadcast_to(((np.arange(F) >= f0) & (np.arange(F) < f1))[None, None, :], (rows, m, F))
            gb, pb = g[b, :rows].reshape(rows, m, F), p[b, :rows].reshape(rows, m, F)
            assert np.array_equal(g[b, rows:], p[b, rows:]) and not g[b, rows:].any()
            assert np.array_equal(gb[~in_t & ~in_f], pb[~in_t & ~in_f]), (b, m, n)             # outside: the bits of the unmasked call
            mel, tim = gb[in_f], gb[in_t & ~in_f]
            assert mel.size and tim.size and (in_t & in_f).any()
            assert np.all(mel == mel[0]) and np.all(tim == tim[0]), (b, m, n)                  # one value each; mel wins where they cross
            if norm == "global" and b != 1:                    # (utterance 1 is one frame, all of it masked: the two fills coincide)
                assert mel[0] != tim[0]
            fill_f, fill_t = float(mel[:1].view(np.float32)[0]), float(tim[:1].view(np.float32)[0])
            want_t, want_f, scale = fills_of_the_definition(batch, norm, b)
            e_t = abs(fill_t - want_t) / (scale or abs(want_t))
            e_f = abs(fill_f - want_f) / (scale or abs(want_f))
            print(f"{norm} LFR {m}/{n} utterance {b}: time fill {fill_t:.6g} (definition {want_t:.6g}, error {e_t:.3g}), "
                  f"mel fill {fill_f:.6g} (definition {want_f:.6g}, error {e_f:.3g})")
            assert e_t <= 1e-5 and e_f <= 1e-5, (b, m, n)


# ---- the tiled grid's second trip: 1100 x 7 x 160 = 1 232 000 elements per utterance > the 256 x 4096 of one pass of the largest grid
BIG_FRAMES, BIG_F, BIG_M, BIG_N = [1100, 733], 160, 7, 1


@pytest.fixture(scope="module")
def big(K):
    from asr_chinese_e2e_amd.data_handler import build_LFR_features
    b = Batch.random(K, BIG_FRAMES, [160 * (T - 1) + 1 for T in BIG_FRAMES], BIG_F, seed=9)
    b.x = [CR.normalise(b.feat_np[i, :T], b.mean_np, b.istd_np) for i, T in enumerate(BIG_FRAMES)]      # exact: one subtraction, one multiplication
    want = np.zeros((b.B, b.Tmax, BIG_M * BIG_F), dtype=np.float32)
    for i, T in enumerate(BIG_FRAMES):
        want[i, :T] = build_LFR_features(b.x[i], BIG_M, BIG_N)
    b.want = torch.from_numpy(want)
    assert b.Tmax * BIG_M * BIG_F > 256 * 4096
    return b


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
def test_tiled_grid_past_its_first_pass(big, dtype):
    Tl = big.Tmax
    tiled, tiled_len = big.run("global", BIG_M, BIG_N, Tl, dtype)
    one, one_len = big.run("global", BIG_M, BIG_N, Tl, dtype, masks=[[0, 0, 0, 0]] * big.B)      # one workgroup per utterance
    zero, zero_len = big.policy("global", [[0] * 21] * big.B, (3, 2, 3), BIG_M, BIG_N, Tl, dtype)
    assert tiled_len.tolist() == BIG_FRAMES and one_len.tolist() == BIG_FRAMES and zero_len.tolist() == BIG_FRAMES
    assert same_bits(tiled, big.want.to(dtype))
    assert same_bits(one, tiled.cpu()) and same_bits(zero, tiled.cpu())


def test_tiled_policy_past_its_first_pass(big):
    T, counts = BIG_FRAMES[0], (2, 1, 1)
    row = [400, 520, 100, 160, 1050, 1100, 30, 47, 600, 640, 90]      # warp, two time masks (one to the last frame), a mel mask, a substitution
    one = Batch(big.K, big.feat_np[:1], [160 * (T - 1) + 1], big.mean_np, big.istd_np)
    y = SR.apply(big.x[0], row, *counts)
    want, want_len = SR.stack(y, BIG_M, BIG_N, T)
    assert not np.array_equal(want, big.want[0].numpy())
    for dtype in DTYPES:
        got, got_len = one.policy("global", [row], counts, BIG_M, BIG_N, T, dtype)
        assert got_len.tolist() == [want_len] and same_bits(got, torch.from_numpy(want)[None].to(dtype)), dtype


def test_utterance_entries_refuse_what_the_global_ones_refuse(K, batch):
    """Tlfr_max * m * n_mels past INT32_MAX, and B = 65536 (utterances are indexed by blockIdx.y on every path): ASR_EINVAL before a launch."""
    from asr_chinese_e2e_amd import _lib
    p = lambda t: t.data_ptr()
    rg = torch.zeros(batch.B, 21, dtype=torch.int32, device=DEV)
    for dtype in DTYPES:
        out = torch.full((batch.B, 4, F), -1e30, dtype=dtype, device=DEV)
        out_len = torch.full((batch.B,), -7, dtype=torch.int32, device=DEV)
        untouched, dt = out.clone(), K._dt(out)
        head = (p(batch.feat), p(batch.wl))

        def calls(B, m, Tl):
            tail = (p(out), p(out_len), B, TMAX, F, m, 1, Tl, dt, None)
            return (_lib.fast.asr_utt_norm_lfr_fwd(*head, *tail), _lib.fast.asr_utt_norm_augment_lfr_fwd(*head, None, *tail),
                    _lib.fast.asr_utt_norm_specaug_lfr_fwd(*head, p(rg), 21, 3, 2, 3, *tail))

        assert (2 ** 20) * 64 * F > 2 ** 31 - 1
        assert calls(batch.B, 64, 2 ** 20) == (-1, -1, -1)
        assert calls(65536, 1, 4) == (-1, -1, -1)
        torch.cuda.synchronize()
        assert torch.equal(out, untouched) and bool((out_len == -7).all())      # nothing ran
        assert calls(batch.B, 1, 4) == (0, 0, 0)                                # the same calls in range do
        torch.cuda.synchronize()
        assert out_len.tolist() == [0, 1, 4, 4] and not bool((out[1:] == untouched[1:]).any())
