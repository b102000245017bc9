"""Dropout on the GPU against the oracle: the device mask generators against the host restatement (tests/dropout_ref.py), every dropout
dispatch of asr_sdpa_fwd / asr_sdpa_bwd against the fp64 dense reference masked by the HOST mask, and whole training steps with dropout
against oracle.ref_model.RefTrainer given the masks of the seeds the engine used.  Needs a real MI355X: run with `-m gpu`.

Every gate here is shown to be able to fail: each case also builds the reference with wrong masks (the next seed, the two halves of every
hash pair swapped, the unpadded row stride at odd key counts; for whole steps the next step's masks) and requires the kernel to be at
least ten times closer to the right one.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_model as R  # noqa: E402
from tests import dropout_ref as D  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _record(name, row):
    """Print the measured errors and negative-control ratios as one JSON line (shown by `pytest -rP`); the figures quoted below come
    from these lines."""
    print("dropout_parity " + json.dumps({"test": name, **row}))


# ------------------------------------------------------------------------------------------------ device mask generators
@pytest.mark.parametrize("p", [0.1, 0.3])
def test_device_masks_equal_host_restatement(K, p):
    seed = 0x165667B1 + int(p * 10)
    for rows, cols in ((37, 512), (5, 48), (3, 2)):
        got = K.dropout_mask(rows, cols, p, seed).cpu().numpy().astype(bool)
        assert np.array_equal(got, D.keep_bits(rows, cols, p, seed)), (rows, cols)
    for B, H, Tq, Tk in ((2, 3, 21, 21), (1, 2, 17, 45), (2, 2, 40, 131), (1, 1, 7, 1), (2, 8, 24, 500), (1, 2, 97, 513)):
        got = K.sdpa_dropout_mask(B, H, Tq, Tk, p, seed).cpu().numpy().astype(bool)
        assert np.array_equal(got, D.sdpa_mask(B, H, Tq, Tk, p, seed) > 0), (B, H, Tq, Tk)
    with pytest.raises(Exception):      # the LayerNorm / embedding sites hash pairs of one row: odd widths are refused
        K.dropout_mask(4, 7, p, seed)


# ------------------------------------------------------------------------------------------------ attention dropout kernel matrix
def _attn_ref(q, k, v, do, klen, causal, window, scale, mask):
    """fp64 dense attention with the multiplicative probability mask `mask` (B, H, Tq, Tk) after the softmax (attention.py:82-84).
    q (B, Tq, H, dk) etc.  Returns o, lse, (dq, dk, dv), dead (B, Tq)."""
    B, Tq, H, dk = q.shape
    Tk = k.shape[1]
    qr, kr, vr = (x.clone().requires_grad_(True) for x in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qr, kr) * scale
    qi = torch.arange(Tq).view(1, 1, Tq, 1)
    kj = torch.arange(Tk).view(1, 1, 1, Tk)
    vis = kj < klen.view(B, 1, 1, 1)
    if causal:
        vis = vis & (kj <= qi)
    if window >= 0:
        vis = vis & ((kj - qi).abs() <= window)
    dead = ~vis.any(-1, keepdim=True)
    s = s.masked_fill(~vis & ~dead, float("-inf"))
    p = torch.softmax(s, -1) * (~dead).to(s.dtype) * torch.as_tensor(mask, dtype=s.dtype)
    o = torch.einsum("bhqk,bkhd->bqhd", p, vr)
    lse = torch.logsumexp(s, -1).masked_fill(dead.squeeze(-1), float("-inf"))
    grads = torch.autograd.grad((o * do).sum(), (qr, kr, vr))
    return o.detach(), lse.detach(), grads, dead.expand(B, 1, Tq, 1)[:, 0, :, 0]


def _rel(a, r, sel):
    """Relative Frobenius error of a against r over the rows sel (a bool (B, T) mask of dims 0, 1)."""
    a, r = a.double()[sel], r.double()[sel]
    return float((a - r).norm() / r.norm().clamp_min(1e-300))


def _close(a, b, rtol, atol, what):
    a, b = a.double(), b.double()
    bad = (a - b).abs() > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float((a - b).abs().max()):.3e}"


BF16, F32 = torch.bfloat16, torch.float32
# dtype, B, H, Tq, Tk, dk, causal, window, klens, o_lo; what it runs.  Measured on an MI355X, the larger of p = 0.1 and 0.3: relative
# Frobenius error of o and of the worst of dQ / dK / dV against the right mask, and the largest ratio of a tensor's error against the right
# mask to its error against a wrong one (gate 0.1).
ATTN_DROP_CASES = [
    (BF16, 2, 2, 300, 300, 64, False, 50, [300, 100], False),    # fused fwd/bwd, non-causal window; queries >= 151 of row 1 see no key; measured o 2.3e-03, grads 3.6e-03, ratio 0.008
    (BF16, 3, 8, 21, 21, 64, True, -1, [21, 13, 1], False),      # fused causal Tk <= 64, odd: the decoder's self-attention with dropout; measured o 2.4e-03, grads 3.9e-03, ratio 0.010
    (BF16, 2, 4, 63, 63, 64, True, -1, [63, 40], False),         # fused causal, 63 keys: the last pair of a row is half outside; measured o 2.3e-03, grads 3.8e-03, ratio 0.008
    (BF16, 2, 2, 131, 131, 64, False, -1, [131, 70], False),     # fused, odd Tk self-attention: lane-pair hash and its key clamp; measured o 2.3e-03, grads 3.7e-03, ratio 0.008
    (BF16, 2, 2, 17, 45, 64, False, -1, [45, 30], False),        # fused, odd Tk cross-attention 17 x 45; measured o 2.3e-03, grads 3.6e-03, ratio 0.007
    (BF16, 1, 2, 97, 513, 64, False, -1, [513], False),          # tiled fwd + dQ / dK-dV pair <true>, without o_lo; measured o 2.3e-03, grads 2.4e-03, ratio 0.006
    (BF16, 2, 2, 40, 601, 64, False, -1, [601, 333], True),      # tiled fwd + pair, cross, odd Tk, with o_lo; measured o 2.3e-03, grads 2.4e-03, ratio 0.006
    (BF16, 1, 1, 40, 700, 64, False, 60, [650], True),           # pair path with a band, with o_lo; dead rows; measured o 2.3e-03, grads 2.4e-03, ratio 0.006
    (BF16, 2, 2, 1100, 1100, 64, False, 50, [1100, 700], True),  # band backward <true,true,true> + halo kernel; dead rows; measured o 2.3e-03, grads 3.5e-03, ratio 0.008
    (BF16, 1, 2, 513, 513, 64, False, 7, [513], True),           # band backward, odd Tk, narrow band; measured o 2.3e-03, grads 3.6e-03, ratio 0.008
    (BF16, 1, 1, 2000, 2000, 64, False, 50, [2000], True),       # the long-form head (T = 2000, +-50 band); measured o 2.3e-03, grads 3.6e-03, ratio 0.008
    (BF16, 2, 2, 21, 21, 16, True, -1, [21, 9], False),          # generic bf16 kernels (dk = 16), causal, odd Tk; measured o 1.7e-03, grads 3.1e-03, ratio 0.006
    (F32, 2, 3, 19, 19, 16, True, -1, [19, 7], False),           # fp32 generic, causal; measured o 1.0e-07, grads 2.4e-07, ratio 0.000
    (F32, 2, 2, 71, 71, 32, False, 10, [71, 30], False),         # fp32 generic, window, odd Tk, dead rows; measured o 1.5e-07, grads 2.6e-07, ratio 0.000
]
BOUND = {BF16: (1.5e-2, 3e-2), F32: (1e-5, 1e-4)}      # relative Frobenius error of o, of the gradients


@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("dtype,B,H,Tq,Tk,dk,causal,window,klens,with_lo", ATTN_DROP_CASES)
def test_sdpa_dropout_matches_host_masked_reference(K, dtype, B, H, Tq, Tk, dk, causal, window, klens, with_lo, p):
    g = torch.Generator().manual_seed(Tq * 31 + Tk + int(p * 100))
    seed = 1000 + Tq + 7 * Tk
    d = H * dk
    self_attn = Tq == Tk
    if self_attn:      # the engine's fused Q|K|V rows
        qkv = torch.randn(B * Tq, 3 * d, generator=g).to(dtype)
        q2, k2, v2 = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    else:
        q2 = torch.randn(B * Tq, d, generator=g).to(dtype)
        kv = torch.randn(B * Tk, 2 * d, generator=g).to(dtype)
        k2, v2 = kv[:, :d], kv[:, d:]
    do = torch.randn(B * Tq, d, generator=g).to(dtype)
    klen = torch.tensor(klens, dtype=torch.int32)
    scale = dk ** -0.5
    shp = lambda x, T: x.double().reshape(B, T, H, dk)
    args = (shp(q2, Tq), shp(k2, Tk), shp(v2, Tk), shp(do, Tq), klen, causal, window, scale)

    # the kernel, outputs NaN-filled first: every element it owes must be written
    if self_attn:
        gd = qkv.to(DEV)
        q, k, v = gd[:, :d], gd[:, d:2 * d], gd[:, 2 * d:]
        dg = torch.full_like(gd, float("nan"))
        dq, dk_, dv = dg[:, :d], dg[:, d:2 * d], dg[:, 2 * d:]
    else:
        q = q2.to(DEV)
        gd = kv.to(DEV)
        k, v = gd[:, :d], gd[:, d:]
        dq = torch.full_like(q, float("nan"))
        dg = torch.full_like(gd, float("nan"))
        dk_, dv = dg[:, :d], dg[:, d:]
    o = torch.full((B * Tq, d), float("nan"), dtype=dtype, device=DEV)
    o_lo = torch.full_like(o, float("nan")) if with_lo else None
    kl = klen.to(DEV)
    o, lse = K.sdpa_fwd(q, k, v, kl, B, H, Tq, Tk, dk, causal, window, scale, o=o, drop_p=p, drop_seed=seed, o_lo=o_lo)
    K.sdpa_bwd(q, k, v, o, do.to(DEV), lse, kl, B, H, Tq, Tk, dk, dq, dk_, dv, causal, window, scale, drop_p=p, drop_seed=seed, o_lo=o_lo)
    torch.cuda.synchronize()
    got = [t.cpu().double().reshape(B, T, H, dk) for t, T in ((o, Tq), (dq, Tq), (dk_, Tk), (dv, Tk))]

    mask = D.sdpa_mask(B, H, Tq, Tk, p, seed)
    o_r, lse_r, (gq, gk, gv), dead = _attn_ref(*args, mask)
    want = [o_r, gq, gk, gv]
    alive = ~dead
    kvalid = torch.arange(Tk).view(1, Tk) < klen.view(B, 1)
    sel = [alive, alive, kvalid, kvalid]
    names = ("o", "dq", "dk", "dv")

    # exact zeros: o and dQ of a query that sees no key, dK and dV of keys past the utterance's end
    assert torch.equal(got[0][dead], torch.zeros_like(got[0][dead])), "o on dead rows"
    assert torch.equal(got[1][dead], torch.zeros_like(got[1][dead])), "dq on dead rows"
    assert torch.equal(got[2][~kvalid], torch.zeros_like(got[2][~kvalid])), "dk past klen"
    assert torch.equal(got[3][~kvalid], torch.zeros_like(got[3][~kvalid])), "dv past klen"
    for t, n in zip(got, names):
        assert torch.isfinite(t).all(), n

    # the elementwise gates of test_sdpa_dropout (tests/test_kernels_gpu.py)
    ft = dict(rtol=2e-5, atol=2e-5) if dtype == F32 else dict(rtol=2e-2, atol=2e-2)
    gt = dict(rtol=2e-4, atol=2e-4) if dtype == F32 else dict(rtol=3e-2, atol=5e-2)
    _close(got[0], o_r, **ft, what="o")
    for t, r, n in zip(got[1:], want[1:], names[1:]):
        _close(t, r, **gt, what=n)
    lv = alive.view(B, 1, Tq).expand(B, H, Tq)
    _close(lse.cpu()[lv], lse_r[lv], rtol=1e-4, atol=2e-3 if dtype == BF16 else 1e-4, what="lse")

    # relative Frobenius error against the right mask
    err = {n: _rel(t, r, s) for t, r, s, n in zip(got, want, sel, names)}
    bo, bg = BOUND[dtype]
    assert err["o"] <= bo and max(err["dq"], err["dk"], err["dv"]) <= bg, err

    # negative controls: the same gates against wrong masks
    wrong = {"seed+1": D.sdpa_mask(B, H, Tq, Tk, p, seed + 1), "pair halves swapped": D.swap_pair_halves(mask)}
    if Tk & 1:
        wrong["unpadded stride"] = D.sdpa_mask(B, H, Tq, Tk, p, seed, stride=Tk)
    ratio = {}
    for wn, wm in wrong.items():
        wo, _, (wq, wk, wv), _ = _attn_ref(*args, wm)
        for t, r, s, n in zip(got, (wo, wq, wk, wv), sel, names):
            ratio[(wn, n)] = err[n] / max(_rel(t, r, s), 1e-300)
    worst = max(ratio, key=ratio.get)
    _record(f"sdpa_dropout[{dtype}-{B}x{H}x{Tq}x{Tk}-dk{dk}-c{int(causal)}-w{window}-lo{int(with_lo)}-p{p}]",
            dict(err=err, worst_ratio=ratio[worst], worst_control=list(worst)))
    assert ratio[worst] <= 0.1, (worst, ratio[worst], err)


# ------------------------------------------------------------------------------------------------ whole training steps with dropout
# engine site ids (asr_chinese_e2e_amd/engine.py: Engine._drop's callers) of the oracle's named sites (oracle.ref_model.dropout_sites)
def _engine_site(name):
    if name == "encoder.input":
        return 1
    if name == "decoder.input":
        return 2
    part = name.split(".")
    i = int(part[2])
    if part[0] == "encoder":
        return {"slf_attn.attn": 10, "slf_attn.fc": 11, "pos_ffn.w_2": 12}[part[3] + "." + part[4]] + 4 * i
    return {"slf_attn.attn": 100, "slf_attn.fc": 101, "enc_attn.attn": 102, "enc_attn.fc": 103, "pos_ffn.w_2": 104}[part[3] + "." + part[4]] + 8 * i


def _recording_kernels(monkeypatch):
    """Wrap the three launchers that take a dropout seed; returns the list of (launcher, arguments) of every call with p > 0."""
    import inspect
    from asr_chinese_e2e_amd import kernels
    calls = []
    for fn in ("sdpa_fwd", "add_ln_fwd", "embed_pe_fwd"):
        orig = getattr(kernels, fn)
        sig = inspect.signature(orig)

        def wrap(*a, _orig=orig, _sig=sig, _fn=fn, **kw):
            ba = _sig.bind(*a, **kw)
            ba.apply_defaults()
            if ba.arguments["drop_p"] > 0:
                calls.append((_fn, ba.arguments))
            return _orig(*a, **kw)
        monkeypatch.setattr(kernels, fn, wrap)
    return calls


def _engine_step(cfg, sd, batch, V, dtype, dec_exec, monkeypatch, p):
    from tests.test_model_gpu import build, to_pack
    monkeypatch.setenv("ASR_DEC_EXEC", dec_exec)
    calls = _recording_kernels(monkeypatch)
    model = build(cfg, V, "TransformerCTC" if not cfg.use_decoder else "TransformerOffical", dtype=dtype, dropout=p).cuda()
    model.load_state_dict(sd)
    model.train()
    eng = model._ensure_engine(DEV)
    assert eng.dec_exec == (dec_exec == "1") and eng.drop_p == p
    model.zero_flat_grads()
    loss, _ = model.train_step(to_pack(batch))
    torch.cuda.synchronize()
    monkeypatch.undo()
    return model, eng, loss.detach().cpu().double(), calls


def _site_calls(cfg, eng, calls):
    """Assert the recorded seeds are Engine._drop's for the documented site ids, that every site the engine launches in Python was reached
    exactly once and that all seeds differ; returns {site name: (launcher, arguments)}."""
    sites = R.dropout_sites(cfg)
    by_seed = {}
    for fn, a in calls:
        assert a["drop_seed"] not in by_seed, "two launches share a dropout seed"
        by_seed[a["drop_seed"]] = (fn, a)
    out = {}
    for s in sites:
        sid = _engine_site(s)
        seed = eng._drop(sid)[1]
        assert seed == D.engine_site_seed(eng.step_seed, sid), s
        if seed in by_seed:
            out[s] = by_seed.pop(seed)
    assert not by_seed, f"launches with seeds of no documented site: {list(by_seed)}"
    want_fn = lambda s: "sdpa_fwd" if s.endswith(".attn") else ("embed_pe_fwd" if s == "decoder.input" else "add_ln_fwd")
    for s, (fn, a) in out.items():
        assert fn == want_fn(s), (s, fn)
        if s == "encoder.input":
            assert a["drop_mode"] == 2
        elif fn == "add_ln_fwd":
            assert a["drop_mode"] == 1
    return out


def _oracle_masks(cfg, batch, step_seed, p, key_rows):
    """{site: mask} in the oracle's layout from the host restatement, for the engine's seeds of step `step_seed`.  key_rows[site]: the key
    count of an attention site's launch (Tk < T for the compact cross-attention rows of ref_compat: the mask is generated over Tk keys and
    padded to T; the padded columns carry P = 0)."""
    B, T = batch["wave"].shape[:2]
    To = int(batch["tgt_len"].max()) + 1
    H, d = cfg.num_head, cfg.d_model
    masks = {}
    for s in R.dropout_sites(cfg):
        seed = D.engine_site_seed(step_seed, _engine_site(s))
        Tq = T if s.startswith("encoder") else To
        if s.endswith(".attn"):
            Tk = key_rows[s]
            full = T if (s.startswith("encoder") or "enc_attn" in s) else To
            m = np.zeros((B, H, Tq, full))
            m[..., :Tk] = D.sdpa_mask(B, H, Tq, Tk, p, seed)
        else:
            m = D.ln_mask(B * Tq, d, p, seed).reshape(B, Tq, d)
        masks[s] = torch.from_numpy(m)
    return masks


def _grad_cosines(model, ref_grads):
    from tests.test_model_gpu import cos
    gmax = max(float(g.abs().max()) for g in ref_grads.values())
    return {n: cos(p.grad, ref_grads[n]) for n, p in model.named_parameters()
            if float(ref_grads[n].abs().max()) >= 1e-6 * gmax and not n.endswith("w_ks.bias")}


def _dropout_step_case(monkeypatch, cfg, sd, batch, V, dtype, dec_exec, p=0.1, oracle64=False, bf16_weights=False):
    """One training step of the engine with dropout p; the oracle's loss and gradients for the same masks and for the next step's masks."""
    model, eng, loss, calls = _engine_step(cfg, sd, batch, V, dtype, "0", monkeypatch, p)
    sites = _site_calls(cfg, eng, calls)
    assert set(sites) == set(R.dropout_sites(cfg)), set(R.dropout_sites(cfg)) - set(sites)
    key_rows = {s: a["Tk"] for s, (fn, a) in sites.items() if fn == "sdpa_fwd"}
    step = eng.step_seed
    if dec_exec == "1":      # the sequencer launches the decoder's kernels natively: same step seed, same site ids (engine._dec_exec_fwd)
        model, eng, loss, calls = _engine_step(cfg, sd, batch, V, dtype, "1", monkeypatch, p)
        assert eng.step_seed == step and bool(eng._dec_cache)
        _site_calls(cfg, eng, calls)
    osd, ob = sd, batch
    if bf16_weights:      # the numbers the MFMA path multiplies by
        osd = {k: (v.bfloat16().float() if v.dim() == 2 else v) for k, v in sd.items()}
    if oracle64:
        osd = {k: v.double() for k, v in osd.items()}
        ob = dict(batch, wave=batch["wave"].double())
    res = {}
    for which, s in (("right", step), ("next step", step + 1)):
        out, grads = R.RefTrainer(osd, cfg, warmup=25).loss_and_grads(ob, drop=_oracle_masks(cfg, batch, s, p, key_rows))
        res[which] = (dict(out, loss=out["loss"].detach()), {k: v.float() for k, v in grads.items()})
    return model, loss, res


def _neg_control_misses(model, loss, ref_out, ref_grads, loss_bound):
    """The gate fed the next step's masks must miss by a wide margin: loss error > 10 x its bound or some gradient cosine < 0.99."""
    rel = abs(float(loss[0]) - float(ref_out["loss"])) / abs(float(ref_out["loss"]))
    worst = min(_grad_cosines(model, ref_grads).values())
    assert rel > 10 * loss_bound or worst < 0.99, (rel, worst)
    return rel, worst


@pytest.mark.parametrize("mode", ["joint", "ctc_only", "ce_wave_len"])
def test_fp32_dropout_step_matches_oracle(mode, monkeypatch):
    """fp32, d_model 32 / 4 heads x 8 (generic attention kernels), p = 0.1: the gates of test_fp32_ctc_paths_match_oracle - loss 1e-4
    relative, every gradient rtol 3e-4.  Measured: loss 0 / 1.1e-7 / 0 (joint / ctc_only / ce_wave_len), every gradient cosine 1 - 1e-11;
    the next step's masks: loss 2.0e-2 / 5.0e-2 / 1.4e-3, lowest gradient cosine 0.052 / 0.74 / 0.059."""
    from tests.test_model_gpu import oracle_case
    over = dict(d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=2)
    if mode == "joint":
        over.update(ctc_weight=0.3)
    elif mode == "ctc_only":
        over.update(use_decoder=False, ctc_weight=1.0)
    else:
        over.update(cross_mask="wave_len")
    cfg, sd, batch = oracle_case(4, 30, 16, 40, 6, over)
    model, loss, res = _dropout_step_case(monkeypatch, cfg, sd, batch, 40, "fp32", "0")
    out, grads = res["right"]
    rel = abs(float(loss[0]) - float(out["loss"])) / abs(float(out["loss"]))
    assert rel < 1e-4, (float(loss[0]), float(out["loss"]))
    gmax = max(float(g.abs().max()) for g in grads.values())
    for n, p in model.named_parameters():
        assert np.allclose(p.grad.cpu().numpy(), grads[n].numpy(), rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), n
    neg = _neg_control_misses(model, loss, *res["next step"], 1e-4)
    _record(f"fp32_dropout_step[{mode}]", dict(loss_rel=rel, worst_cos=min(_grad_cosines(model, grads).values()), next_step=neg))


@pytest.mark.parametrize("dec_exec", ["1", "0"])
def test_bf16_dropout_step_matches_oracle(dec_exec, monkeypatch):
    """bf16, d_model 512 / 8 x 64 (MFMA kernels), joint, ref_compat cross mask (compact key rows, Tk < T), To = 13 (odd), p = 0.1, on the
    decoder's launch sequencer (ASR_DEC_EXEC=1) and the per-kernel path (=0): the gates of bf16_gradient_gate (loss 1e-3, cosine >= 0.999).
    Measured (both paths): loss 1.9e-4, worst cosine 0.99947 (relaxed class 0.99793); the next step's masks: loss 8.2e-3, lowest cosine 0.026."""
    from tests.test_model_gpu import BF16_LOSS_RTOL, bf16_gradient_gate, oracle_case
    over = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=2, ctc_weight=0.3)
    cfg, sd, batch = oracle_case(4, 136, 80, 56, 12, over, seed=9)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
    sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    assert (int(batch["tgt_len"].max()) + 1) % 2 == 1
    model, loss, res = _dropout_step_case(monkeypatch, cfg, sd, batch, 56, "bf16", dec_exec)
    out, grads = res["right"]
    rel = abs(float(loss[0]) - float(out["loss"])) / abs(float(out["loss"]))
    worst, worst_name, ratio = bf16_gradient_gate(model, dict(grads=grads), "dropout_bf16")
    assert rel < BF16_LOSS_RTOL, (float(loss[0]), float(out["loss"]))
    neg = _neg_control_misses(model, loss, *res["next step"], BF16_LOSS_RTOL)
    _record(f"bf16_dropout_step[dec_exec={dec_exec}]", dict(loss_rel=rel, worst_cos=worst, worst_tensor=worst_name, norm_ratio=ratio, next_step=neg))


def test_bf16_dropout_step_wave_len_long_keys(monkeypatch):
    """bf16, cross_mask = "wave_len" at T = 600: the encoder's self-attention and the decoder's cross-attention over 600 keys run the
    tiled forward and the dQ + dK/dV pair with dropout and o_lo.  Oracle in fp64 on the bf16-rounded weight matrices (as in
    test_wave_len_cross_attention_over_long_keys_matches_oracle); gates of bf16_gradient_gate.  Measured: loss 1.1e-4, worst cosine
    0.99972 (relaxed class 0.99850); the next step's masks: loss 5.2e-3, lowest cosine 0.048."""
    from tests.test_model_gpu import BF16_LOSS_RTOL, bf16_gradient_gate, oracle_case
    over = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=2, ctc_weight=0.3, cross_mask="wave_len")
    cfg, sd, batch = oracle_case(2, 600, 80, 56, 12, over, seed=21)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
    sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    model, loss, res = _dropout_step_case(monkeypatch, cfg, sd, batch, 56, "bf16", "1", oracle64=True, bf16_weights=True)
    out, grads = res["right"]
    rel = abs(float(loss[0]) - float(out["loss"])) / abs(float(out["loss"]))
    worst, worst_name, ratio = bf16_gradient_gate(model, dict(grads=grads), "dropout_wave_len_600")
    assert rel < BF16_LOSS_RTOL, (float(loss[0]), float(out["loss"]))
    neg = _neg_control_misses(model, loss, *res["next step"], BF16_LOSS_RTOL)
    _record("bf16_dropout_step_wave_len_600", dict(loss_rel=rel, worst_cos=worst, worst_tensor=worst_name, norm_ratio=ratio, next_step=neg))


def test_bf16_dropout_step_long_form_band(monkeypatch):
    """bf16 long-form configuration, attn_window = 50 at T = 1100 (wave_len 1100 / 837): the encoder's backward takes the band kernel
    with dropout.  Oracle in fp64 (as in test_long_form_window_matches_oracle) on the bf16-rounded weight matrices; loss 2e-3 (the
    long-form bound of that test), gradients by bf16_gradient_gate.  Measured: loss 2.7e-4, worst cosine 0.99966 (relaxed class 0.99905);
    the next step's masks: loss 3.0e-3, lowest cosine -0.010."""
    from tests.test_model_gpu import BF16_LOSS_RTOL, bf16_gradient_gate, oracle_case
    over = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=2, ctc_weight=0.3, attn_window=50)
    cfg, sd, batch = oracle_case(2, 1100, 80, 56, 20, over, seed=13)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
    sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    model, loss, res = _dropout_step_case(monkeypatch, cfg, sd, batch, 56, "bf16", "1", oracle64=True, bf16_weights=True)
    out, grads = res["right"]
    rel = abs(float(loss[0]) - float(out["loss"])) / abs(float(out["loss"]))
    worst, worst_name, ratio = bf16_gradient_gate(model, dict(grads=grads), "dropout_long_form")
    assert rel < 2 * BF16_LOSS_RTOL, (float(loss[0]), float(out["loss"]))
    neg = _neg_control_misses(model, loss, *res["next step"], 2 * BF16_LOSS_RTOL)
    _record("bf16_dropout_step_long_form_1100", dict(loss_rel=rel, worst_cos=worst, worst_tensor=worst_name, norm_ratio=ratio, next_step=neg))
