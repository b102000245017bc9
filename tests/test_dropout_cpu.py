"""The host restatement of the dropout masks (tests/dropout_ref.py) and the oracle's dropout sites (oracle/ref_model.py `drop`).

No GPU: the restatement is checked against a second, scalar restatement in plain Python integers and for the statistics a dropout mask
must have; the device generators are compared with it bit for bit in tests/test_dropout_gpu.py.
"""
import numpy as np
import pytest
import torch

from oracle import ref_model as R
from tests import dropout_ref as D


def _hash_scalar(pair, seed):
    """drop_hash in Python integers (asr_common.h), independent of the numpy code."""
    h = (pair ^ seed) & 0xFFFFFFFF
    h ^= h >> 15
    h = ((h & 0xFFFFFF) * 0x2C1B3D) & 0xFFFFFFFF
    h ^= h >> 13
    h = ((h & 0xFFFFFF) * 0x297A2D) & 0xFFFFFFFF
    return h ^ (h >> 16)


def test_vectorised_hash_matches_scalar_restatement():
    rng = np.random.default_rng(0)
    pairs = np.concatenate([np.arange(64), rng.integers(0, 2 ** 32, 2000), [2 ** 31 - 1, 2 ** 32 - 1]]).astype(np.uint64)
    for seed in (0, 1, 0x165667B1, 0xFFFFFFFF):
        got = D.drop_hash(pairs.astype(np.uint32), seed)
        want = np.array([_hash_scalar(int(x), seed) for x in pairs], dtype=np.uint32)
        assert np.array_equal(got, want), seed
    # __umul24 keeps the LOW 32 bits of the 48-bit product (the products here overflow 32 bits)
    assert int(D.umul24(np.uint32(0xFFFFFF), 0x2C1B3D)) == (0xFFFFFF * 0x2C1B3D) & 0xFFFFFFFF


def test_threshold_and_scale():
    assert D.drop_thr16(0.0) == 0 and D.drop_thr16(-1.0) == 0
    assert D.drop_thr16(0.1) == 6554 and D.drop_thr16(0.5) == 32768 and D.drop_thr16(0.3) == 19661
    m = D.ln_mask(4, 6, 0.25, 3)
    assert set(np.unique(m)) <= {0.0, 1.0 / 0.75}       # 1 / (1 - p), not 1 / (1 - thr16 / 65536)


def test_p_zero_keeps_everything():
    assert np.array_equal(D.ln_mask(7, 10, 0.0, 5), np.ones((7, 10)))
    assert np.array_equal(D.sdpa_mask(2, 3, 5, 7, 0.0, 9), np.ones((2, 3, 5, 7)))


def test_element_counters():
    """ln: row * d + c; sdpa: ((b*H+h)*Tq+q) * ((Tk+1) & ~1) + k - at even and odd column counts."""
    p, seed = 0.3, 77
    thr = D.drop_thr16(p)
    for rows, d in ((5, 8), (3, 7)):
        keep = D.ln_mask(rows, d, p, seed) > 0
        for r in range(rows):
            for c in range(d):
                e = r * d + c
                h = _hash_scalar(e >> 1, seed)
                assert keep[r, c] == (((h >> (16 * (e & 1))) & 0xFFFF) >= thr)
    for B, H, Tq, Tk in ((2, 3, 4, 6), (2, 2, 3, 7), (1, 1, 5, 1)):
        keep = D.sdpa_mask(B, H, Tq, Tk, p, seed) > 0
        tkp = (Tk + 1) & ~1
        for b in range(B):
            for h in range(H):
                for q in range(Tq):
                    for k in range(Tk):
                        e = ((b * H + h) * Tq + q) * tkp + k
                        hs = _hash_scalar(e >> 1, seed)
                        assert keep[b, h, q, k] == (((hs >> (16 * (e & 1))) & 0xFFFF) >= thr)
    # an odd key count: the unpadded stride gives a different mask (the negative control of the GPU tests relies on it)
    assert not np.array_equal(D.sdpa_mask(1, 2, 40, 131, p, seed), D.sdpa_mask(1, 2, 40, 131, p, seed, stride=131))


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_keep_rate_within_binomial_bounds(p):
    keep = D.keep_bits(1024, 1024, p, 1234)
    for half in (keep[:, 0::2], keep[:, 1::2], keep):
        n = half.size
        rate = float(half.mean())
        sigma = (p * (1 - p) / n) ** 0.5
        assert abs(rate - (1 - p)) < 5 * sigma, (p, rate)


def _corr(a, b):
    a = a.astype(np.float64).ravel()
    b = b.astype(np.float64).ravel()
    a -= a.mean()
    b -= b.mean()
    return float((a @ b) / np.sqrt((a @ a) * (b @ b)))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_bits_are_uncorrelated(p):
    """|correlation| between the halves of the pair hash, at lags 1 / Tk / d, and between the seeds the engine gives neighbouring sites
    and neighbouring steps.  2^20 samples: one standard deviation of an estimate is ~1e-3; bound 5e-3."""
    n = 1 << 20
    flat = D.keep_bits(1, n + 1024, p, 4242)[0]
    lo, hi = flat[0:n:2], flat[1:n:2]
    assert abs(_corr(lo, hi)) < 5e-3
    for lag in (1, 131, 250, 512):      # 1: neighbours; 131 / 250: key counts; 512: d_model
        assert abs(_corr(flat[:n], flat[lag:n + lag])) < 5e-3, lag
    seeds = [D.engine_site_seed(s, site) for s in (1, 2) for site in (1, 2, 10, 11, 12, 14, 100, 101, 102, 103, 104, 108)]
    assert len(set(seeds)) == len(seeds)
    masks = [D.keep_bits(1, 1 << 18, p, s)[0] for s in seeds[:6] + seeds[12:14]]
    for i in range(len(masks)):
        for j in range(i + 1, len(masks)):
            assert abs(_corr(masks[i], masks[j])) < 1e-2, (i, j)


def test_swap_pair_halves():
    m = np.arange(2 * 7).reshape(2, 7)
    s = D.swap_pair_halves(m)
    assert s[0].tolist() == [1, 0, 3, 2, 5, 4, 6] and s[1].tolist() == [8, 7, 10, 9, 12, 11, 13]


# ----------------------------------------------------------------------------------------- oracle dropout sites
def _oracle_case(**over):
    cfg = R.default_cfg(**{**dict(n_mels=6, lfr_m=1, d_model=16, hidden_size=4, num_head=4, ff_size=24, layer_num=2, ctc_weight=0.3), **over})
    V = 13
    sd = R.init_state_dict(cfg, V, seed=3)
    g = torch.Generator().manual_seed(4)
    B, T = 3, 11
    wave_len = torch.tensor([11, 8, 5])
    tgt_len = torch.tensor([4, 2, 3])
    tgt = torch.zeros(B, 4, dtype=torch.long)
    for b in range(B):
        tgt[b, :tgt_len[b]] = torch.randint(4, V, (int(tgt_len[b]),), generator=g)
    batch = dict(wave=torch.randn(B, T, 6, generator=g), wave_len=wave_len, tgt_for_input=tgt, tgt_len=tgt_len)
    return cfg, sd, batch


def _site_shapes(cfg, batch):
    B, T = batch["wave"].shape[:2]
    To = int(batch["tgt_len"].max()) + 1
    H, d = cfg.num_head, cfg.d_model
    shapes = {}
    for s in R.dropout_sites(cfg):
        enc = s.startswith("encoder")
        Tq = T if enc else To
        if s.endswith(".attn"):
            shapes[s] = (B, H, Tq, T if (enc or "enc_attn" in s) else To)
        else:
            shapes[s] = (B, Tq, d)
    return shapes


class _Recording(dict):
    def __init__(self, *a):
        super().__init__(*a)
        self.read = []

    def __getitem__(self, k):
        self.read.append(k)
        return super().__getitem__(k)


@pytest.mark.parametrize("over", [dict(), dict(cross_mask="wave_len"), dict(use_decoder=False, ctc_weight=1.0)])
def test_all_ones_masks_equal_no_dropout(over):
    cfg, sd, batch = _oracle_case(**over)
    ref = R.RefTrainer(sd, cfg, warmup=10)
    out0, g0 = ref.loss_and_grads(batch)
    ones = _Recording({s: torch.ones(sh) for s, sh in _site_shapes(cfg, batch).items()})
    out1, g1 = ref.loss_and_grads(batch, drop=ones)
    assert torch.equal(out0["loss"], out1["loss"])
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert ones.read == R.dropout_sites(cfg)      # every site read once, in forward order


def test_masks_act_where_the_reference_applies_them():
    """A real mask changes the step; zeroing a whole site does what the reference's nn.Dropout would do there."""
    cfg, sd, batch = _oracle_case()
    shapes = _site_shapes(cfg, batch)
    ones = {s: torch.ones(sh) for s, sh in shapes.items()}
    base = R.forward_losses(sd, cfg, batch, drop=ones)
    for s in R.dropout_sites(cfg):
        m = dict(ones)
        m[s] = torch.from_numpy(D.keep_bits(int(np.prod(shapes[s][:-1])), shapes[s][-1], 0.5, 1).reshape(shapes[s]) * 2.0).float()
        out = R.forward_losses(sd, cfg, batch, drop=m)
        assert float(out["loss"]) != float(base["loss"]), s
    # attention probabilities all dropped: the context is 0, the block is LayerNorm(fc.bias + x)
    m = dict(ones)
    m["decoder.layer_stack.1.enc_attn.attn"] = torch.zeros(shapes["decoder.layer_stack.1.enc_attn.attn"])
    m2 = dict(ones)
    m2["decoder.layer_stack.1.enc_attn.attn"] = torch.zeros(shapes["decoder.layer_stack.1.enc_attn.attn"])
    sd2 = dict(sd)
    sd2["decoder.layer_stack.1.enc_attn.w_vs.weight"] = torch.randn_like(sd["decoder.layer_stack.1.enc_attn.w_vs.weight"])
    assert torch.equal(R.forward_losses(sd, cfg, batch, drop=m)["loss"], R.forward_losses(sd2, cfg, batch, drop=m2)["loss"])


def test_missing_or_misshapen_site_raises():
    cfg, sd, batch = _oracle_case()
    shapes = _site_shapes(cfg, batch)
    for s in ("encoder.input", "decoder.layer_stack.1.pos_ffn.w_2", "decoder.layer_stack.0.enc_attn.attn"):
        m = {k: torch.ones(sh) for k, sh in shapes.items() if k != s}
        with pytest.raises(KeyError, match=s.replace(".", r"\.")):
            R.RefTrainer(sd, cfg, warmup=10).iterate(batch, drop=m)
    m = {k: torch.ones(sh) for k, sh in shapes.items()}
    m["encoder.layer_stack.0.slf_attn.attn"] = torch.ones(shapes["encoder.layer_stack.0.slf_attn.attn"][:-1] + (5,))
    with pytest.raises(ValueError):
        R.forward_losses(sd, cfg, batch, drop=m)


def test_oracle_does_not_import_the_package():
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(R))
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    names += [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert not any(n.startswith("asr_chinese_e2e_amd") or n.startswith("tests") for n in names), names
