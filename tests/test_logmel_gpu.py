"""logmel_kernel against the float64 front end (tests/logmel_emul.py, oracle/logmel_ref.py) where it can go wrong: its dynamic range
below a frame's peak, silence, the first and last frame of short and tile-filling utterances, padding rows and tiles, every mel
width's lane layout, tile independence, a length past the row - and utt_norm_lfr at the same edges.  Every output buffer starts
full of NaN, so a row nobody writes shows.  The streaming kernel shares the tile body and is tied to this one bit for bit
(tests/test_cmvn_gpu.py), so what holds here holds for both.

Hard gate, every frame and bin: |exp(got) - (mel64 + 1e-20)| <= bound, the bound from fp32 arithmetic alone (logmel_emul.bound).
Cells with nothing but the floor under the log (an all-zero frame or filterbank column) hold exactly logf(1e-20f).
Tighter gate: the kernel's largest err / bound per signal is at most 4 times that of the float32 numpy restatement (the margin
covers the MFMA's accumulation order and sincospif against numpy start values)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import logmel_ref as LM  # noqa: E402
from tests import logmel_emul as E  # noqa: E402

DEV = "cuda"
GARBAGE = 1e3            # what lies in a row past its utterance


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


_tables = {}


def tables(n_mels):
    if n_mels not in _tables:
        _tables[n_mels] = (torch.from_numpy(LM.hann_periodic().astype(np.float32)).to(DEV),
                           torch.from_numpy(LM.mel_filterbank(n_mels).astype(np.float32)).to(DEV))
    return _tables[n_mels]


def logmel(K, wav, lens, n_mels, Tmax):
    """wav (B, S) float32 numpy, lens -> (B, Tmax, n_mels) float32 numpy, the kernel writing into a buffer full of NaN."""
    window, fb = tables(n_mels)
    feat = torch.full((wav.shape[0], Tmax, n_mels), float("nan"), dtype=torch.float32, device=DEV)
    out = K.logmel(torch.from_numpy(np.ascontiguousarray(wav)).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), window, fb, Tmax, feat=feat)
    assert out.data_ptr() == feat.data_ptr()
    return feat.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


_floor = []


def is_floor(K, x):
    """x holds logf(1e-20f) and nothing else, bit for bit: the one value every cell of a silent utterance holds.  The compiler's
    logf is not correctly rounded, so the value cannot be named from the host; what can be said from the formats is that it lies
    within 2 ulp of logmel_emul.LOG_FLOOR32, the float32 nearest to log(1e-20): logf is the hardware's log2 (1 ulp of
    log2(1e-20) = -66.4, a binade whose ulp times ln 2 is 1.39 ulp at -46.05) times ln 2, then one rounding (0.5 ulp).
    Measured on an MI355X: 2 ulp (1.67 ulp from the real number)."""
    if not _floor:
        got = bits(logmel(K, np.zeros((1, 3000), dtype=np.float32), [3000], 80, LM.num_frames(3000)))
        assert np.all(got == got.flat[0]), "silent cells differ among themselves"
        assert abs(int(got.flat[0]) - int(bits(np.array([E.LOG_FLOOR32]))[0])) <= 2, got.flat[0]
        _floor.append(got.flat[0])
    return bool(np.all(bits(x) == _floor[0]))


def ragged(lens, Smax, seed):
    """(B, Smax) float32: noise of amplitude 0.1 in [0, len), GARBAGE behind it."""
    rng = np.random.RandomState(seed)
    wav = np.full((len(lens), Smax), GARBAGE, dtype=np.float32)
    for b, l in enumerate(lens):
        wav[b, :l] = 0.1 * rng.randn(l)
    return wav


def check_row(K, got, wav, n_mels, what):
    """One batch row (Tmax, n_mels) against the utterance wav (len,): hard gate and exact floor cells on its frames (as many as
    Tmax leaves), exact zeros behind them, no NaN.  -> the largest err / bound."""
    assert not np.isnan(got).any(), f"{what}: {int(np.isnan(got).sum())} cells never written"
    T = min(LM.num_frames(len(wav)), got.shape[0]) if len(wav) else 0
    assert np.array_equal(bits(got[T:]), np.zeros_like(bits(got[T:]))), f"{what}: rows past frame {T} are not zero"
    if T == 0:
        return 0.0
    floor = E.floor_cells(wav, n_mels)[:T]
    assert is_floor(K, got[:T][floor]), f"{what}: floor cells"
    ratio, at = E.error_ratio(got[:T], wav, n_mels)
    assert ratio <= 1.0, f"{what}: err / bound {ratio:.3e} at (frame, bin) {at}"
    return ratio


# ------------------------------------------------------------------------------------ accuracy against float64
@pytest.mark.parametrize("n_mels", [40, 80])
def test_accuracy_and_dynamic_range(K, n_mels):
    """Measured on an MI355X (err / bound, kernel | float32 emulation), n_mels 40 and 80: see DESIGN.md, "Log-mel accuracy"."""
    sig = E.signals()
    names = list(sig)
    got = logmel(K, np.stack([sig[k] for k in names]), [E.N_SIG] * len(names), n_mels, LM.num_frames(E.N_SIG))
    failed = []
    for b, name in enumerate(names):
        emul, _ = E.error_ratio(E.emulate32(sig[name], n_mels), sig[name], n_mels)
        assert not np.isnan(got[b]).any(), name
        kern, at = E.error_ratio(got[b], sig[name], n_mels)
        print(f"n_mels {n_mels:3d}  {name:24s} err/bound kernel {kern:.3e} at {at}  emulation {emul:.3e}  kernel/emulation {kern / emul:.2f}")
        floor = E.floor_cells(sig[name], n_mels)
        if not is_floor(K, got[b][floor]):
            failed.append(f"{name}: floor cells are not logf(1e-20f)")
        if not kern <= 1.0:
            failed.append(f"{name}: hard gate, err / bound {kern:.3e} at {at}")
        if not kern <= 4.0 * emul:
            failed.append(f"{name}: kernel {kern:.3e} > 4 x emulation {emul:.3e}")
    assert not failed, failed


def test_silence(K):
    """Every cell of an all-zero utterance holds logf(1e-20f): one value, at most 2 ulp from the nearest float32 (is_floor), and the
    same in a batch beside a loud row."""
    assert LM.num_frames(3000) == 19
    assert is_floor(K, logmel(K, np.zeros((1, 3000), dtype=np.float32), [3000], 80, 19))
    wav = ragged([3000, 3000], 3000, seed=2)
    wav[1] = 0.0
    assert is_floor(K, logmel(K, wav, [3000, 3000], 80, 19)[1])


# ------------------------------------------------------------------------------------ frame count, tile and padding edges
EDGE_LENS = [0, 1, 150, 159, 160, 200, 201, 4959, 4960, 5119, 5120, 10240]
EDGE_SMAX = 10240 + 7


@pytest.fixture(scope="module")
def edge_wav():
    return ragged(EDGE_LENS, EDGE_SMAX, seed=11)


@pytest.fixture(scope="module")
def edge_run65(K, edge_wav):
    return logmel(K, edge_wav, EDGE_LENS, 80, 65)


@pytest.mark.parametrize("Tmax", [65, 70])
def test_ragged_lengths_and_padding(K, edge_wav, edge_run65, Tmax):
    """Tmax = 70 puts padding rows behind every utterance, the tile 64..69 of the longest being padding throughout."""
    assert [LM.num_frames(l) for l in EDGE_LENS[1:]] == [1, 1, 1, 2, 2, 2, 31, 32, 32, 33, 65]
    got = edge_run65 if Tmax == 65 else logmel(K, edge_wav, EDGE_LENS, 80, Tmax)
    for b, l in enumerate(EDGE_LENS):
        ratio = check_row(K, got[b], edge_wav[b, :l], 80, f"len {l}, Tmax {Tmax}")
        print(f"len {l:6d}  Tmax {Tmax}  err/bound {ratio:.3e}")
    if Tmax != 65:
        assert np.array_equal(bits(got[:, :65]), bits(edge_run65))


def test_truncating_tmax(K, edge_wav, edge_run65):
    got = logmel(K, edge_wav, EDGE_LENS, 80, 20)
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(edge_run65[:, :20]))      # zeros behind the short utterances included
    assert np.all(got[EDGE_LENS.index(4959)] != 0.0)                # and 20 frames of the long ones


# ------------------------------------------------------------------------------------ mel width
@pytest.mark.parametrize("n_mels", [23, 40, 80, 128, 160])
def test_mel_width(K, n_mels):
    """160: two mel tiles per wave; 23 and 40: lanes without a column; 128 and 160 have all-zero filterbank columns."""
    wav = ragged([5000], 5000, seed=n_mels)
    got = logmel(K, wav, [5000], n_mels, 33)         # one row of padding behind 32 frames
    zero_cols = ~LM.mel_filterbank(n_mels).any(axis=0)
    assert zero_cols.any() == (n_mels >= 128)
    ratio = check_row(K, got[0], wav[0], n_mels, f"n_mels {n_mels}")
    print(f"n_mels {n_mels:3d}  err/bound {ratio:.3e}  all-zero columns {int(zero_cols.sum())}")
    assert is_floor(K, got[0, :32][:, zero_cols])
    assert np.all(got[0, :32][:, ~zero_cols] > E.LOG_FLOOR32 + 10.0)


# ------------------------------------------------------------------------------------ tile independence
def test_tile_independence(K):
    lens = [9000, 100, 6000]
    wav = ragged(lens, 9000, seed=5)
    batch = logmel(K, wav, lens, 80, 57)
    alone = logmel(K, wav[2:3, :6000], [6000], 80, 38)
    assert LM.num_frames(6000) == 38 and not np.isnan(alone).any()
    assert np.array_equal(bits(batch[2, :38]), bits(alone[0]))


# ------------------------------------------------------------------------------------ a length past the row
def test_length_past_the_row_is_clamped(K):
    """Row 0 claims more samples than a row holds (the overrun would stay inside the tensor: it would read row 1), and a negative
    length is an empty row."""
    Smax = 4000
    wav = ragged([Smax, Smax], Smax, seed=9)
    Tmax = LM.num_frames(Smax + 500)
    want = logmel(K, wav, [Smax, Smax], 80, Tmax)
    got = logmel(K, wav, [Smax + 500, Smax], 80, Tmax)
    assert not np.isnan(got).any() and np.array_equal(bits(got), bits(want))
    assert not want[0, LM.num_frames(Smax):].any() and want[0, :LM.num_frames(Smax)].all()
    got = logmel(K, wav, [-3, Smax], 80, Tmax)
    assert not got[0].any() and np.array_equal(bits(got[1]), bits(want[1]))


# ------------------------------------------------------------------------------------ utt_norm_lfr at the same edges
LFR_FRAMES = [1, 2, 3, 33]
LFR_LENS = [100, 160 + 5, 320 + 17, 32 * 160 + 3]


@pytest.fixture(scope="module")
def lfr_feat(K):
    assert [LM.num_frames(l) for l in LFR_LENS] == LFR_FRAMES
    window, fb = tables(80)
    wav = torch.from_numpy(ragged(LFR_LENS, max(LFR_LENS), seed=21)).to(DEV)
    wl = torch.tensor(LFR_LENS, dtype=torch.int32, device=DEV)
    feat = K.logmel(wav, wl, window, fb, 33, feat=torch.full((len(LFR_LENS), 33, 80), float("nan"), dtype=torch.float32, device=DEV))
    return feat, wl, feat.cpu().double().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,n", [(4, 3), (7, 6), (1, 1)])
def test_utt_norm_lfr_edges(K, lfr_feat, m, n, dtype):
    """One to 33 frames (a one-frame utterance still has n_mels > 1 values, so its deviation is defined), m past the utterance's
    end (every stacked slot repeats the last frame), and a Tlfr_max that clamps out_len.  Tolerances: those of test_logmel_lfr."""
    feat, wl, feat_np = lfr_feat
    rtol, atol = (1e-4, 1e-4) if dtype == torch.float32 else (1e-2, 2e-2)
    full = -(-33 // n)
    for Tl in (full, max(1, full // 2)):
        got, got_len = K.utt_norm_lfr(feat, wl, m, n, Tl, dtype)
        got = got.float().cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any()
        for b, T in enumerate(LFR_FRAMES):
            ref = LM.build_lfr(LM.utt_normalize(feat_np[b, :T]), m, n)
            rows = min(ref.shape[0], Tl)
            assert ref.shape[0] == -(-T // n) and int(got_len[b]) == rows
            err = np.abs(got[b, :rows] - ref[:rows])
            assert np.all(err <= atol + rtol * np.abs(ref[:rows])), (T, Tl, float(err.max()))
            assert not got[b, rows:].any()
            if T == 1:
                assert np.array_equal(got[b, 0].reshape(m, 80), np.repeat(got[b, 0, :80][None], m, axis=0))
