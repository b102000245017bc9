"""Compact key rows of the decoder's encoder-decoder attention (Engine.cross_rows).

Under the reference's cross mask (cross_mask = "ref_compat": key lengths are the TEXT lengths, transformer_official.py:78) a query sees only
encoder frames t < tgt_len[b] <= W, the padded target width.  The K|V projections, their weight gradient and the encoder-output gradient
then run on the first Tk = round_up(W, 16) frames of each utterance only.  These tests pin that the cut is exact: frames past Tk
influence nothing and receive nothing, the masked rows inside Tk get exact zero gradients, and both decoder paths still match the oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_model as R  # noqa: E402
from tests.test_model_gpu import BF16_COS, BF16_COS_EXEMPT, BF16_LOSS_RTOL, DEV, build, cos, oracle_case, to_pack  # noqa: E402

D512 = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=2, ctc_weight=0.3, dropout=0.0)


def _model(cfg, sd, V, dtype):
    m = build(cfg, V, "TransformerOffical", dtype=dtype).cuda()
    m.load_state_dict({k: v for k, v in sd.items()})
    m.train()
    return m, m._ensure_engine(DEV)


@pytest.mark.parametrize("L", [9, 17])
def test_masked_key_rows_get_exact_zero_gradients(L):
    """g_kv_all filled with NaN before a step: the attention backward writes every row of it, exact zeros at klen <= t < Tk, and every
    gradient of the step is finite (no NaN from an unwritten row reaches d_enc or the K|V weight gradient)."""
    B, T, V = 8, 200, 56
    cfg, sd, batch = oracle_case(B, T, 80, V, L, D512, seed=41)
    pack = to_pack(batch)
    W = batch["tgt_for_input"].shape[1]
    Tk = (W + 15) // 16 * 16
    model, eng = _model(cfg, sd, V, "bf16")
    model.zero_flat_grads()
    model.train_step(pack)
    torch.cuda.synchronize()
    (bufs,) = [v for k, v in eng._dec_cache.items() if k[:4] == (B, W + 1, T, Tk)]
    bufs["g_kv_all"].fill_(float("nan"))
    model.zero_flat_grads()
    loss, _ = model.train_step(pack)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
    g = bufs["g_kv_all"].view(B, Tk, -1).float().cpu()
    for b, n in enumerate(batch["tgt_len"].tolist()):
        assert n < Tk
        assert bool(torch.isfinite(g[b, :n]).all()), b
        assert bool((g[b, n:] == 0).all()), (b, n)
    assert bool(torch.isfinite(model._flat.g).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_frames_past_key_rows_change_nothing(dtype):
    """Encoder-output rows t >= Tk perturbed: the decoder's logits are bit-identical, and its backward pass adds nothing to those rows of
    d_enc (bf16: the native sequencer; fp32: the per-kernel path)."""
    B, T, V = 6, 160, 56
    cfg, sd, batch = oracle_case(B, T, 80, V, 9, D512, seed=43)
    pack = to_pack(batch)
    model, eng = _model(cfg, sd, V, dtype)
    model.zero_flat_grads()
    eng.refresh_transposes()
    ev, x, wave_len, prep = model._prepare(pack, training=True)
    enc, _ = eng.encoder_fwd(x, wave_len)
    cross_len, Tk = model._cross(eng, pack, wave_len, T)
    assert Tk == 16 < T
    pred0, _ = eng.decoder_fwd(prep, enc, cross_len, B, T, Tk)
    pred0 = pred0.clone()
    enc2 = enc.clone()
    enc2.view(B, T, -1)[:, Tk:] += torch.randn_like(enc2.view(B, T, -1)[:, Tk:].float()).to(enc2.dtype)
    pred1, cache = eng.decoder_fwd(prep, enc2, cross_len, B, T, Tk)
    assert torch.equal(pred0, pred1)
    d_enc = torch.zeros_like(enc2)
    eng.decoder_bwd(cache, torch.randn_like(pred1), d_enc)
    eng.join_side()
    torch.cuda.synchronize()
    eng._release_kept(joined=True)
    d3 = d_enc.view(B, T, -1)
    assert bool((d3[:, Tk:] == 0).all())
    assert float(d3[:, :Tk].float().abs().sum()) > 0


def test_kv_buffers_hold_only_the_key_rows():
    """The persistent K|V activation and gradient buffers of the sequencer are (B*Tk, L 2 H dk), not (B*T, ...)."""
    B, T, V = 8, 300, 56
    cfg, sd, batch = oracle_case(B, T, 80, V, 22, D512, seed=45)
    model, eng = _model(cfg, sd, V, "bf16")
    model.zero_flat_grads()
    model.train_step(to_pack(batch))
    torch.cuda.synchronize()
    W = batch["tgt_for_input"].shape[1]
    Tk = eng.cross_rows(W, T, True)
    assert Tk == (W + 15) // 16 * 16
    (bufs,) = eng._dec_cache.values()
    n = B * Tk * cfg.layer_num * 2 * cfg.num_head * cfg.hidden_size
    assert bufs["kv_all"].numel() == n and bufs["g_kv_all"].numel() == n
    assert bufs["enc_x"].shape == (B * Tk, cfg.d_model)
    assert eng.cross_rows(W, T, False) == T and eng.cross_rows(W, 20, True) == 20 and eng.cross_rows(0, T, True) == 16


def test_text_length_past_the_target_width_is_refused():
    """A host-resident tgt_len longer than the padded target width would let queries see frames that were never projected: refused."""
    B, T, V = 2, 64, 40
    cfg, sd, batch = oracle_case(B, T, 16, V, 5, dict(d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=1, ctc_weight=0.3), seed=47)
    model, _ = _model(cfg, sd, V, "bf16")
    pack = to_pack(batch)
    pack["tgt_len"] = torch.tensor([batch["tgt_for_input"].shape[1] + 1, 1], dtype=torch.int64)
    with pytest.raises(ValueError, match="tgt_len"):
        model.train_step(pack)


@pytest.mark.parametrize("mode", ["1", "0"])
def test_compact_rows_match_oracle_both_decoder_paths(mode, monkeypatch):
    """A ragged ref_compat batch in bf16 through the native sequencer (ASR_DEC_EXEC=1) and the per-kernel path (=0), against the fp32
    oracle, with the gates of test_model_gpu.py::test_full_size_step_matches_oracle: loss to 1e-3, cosine >= 0.999 for every significant
    gradient tensor, 0.97 for the insignificant ones."""
    monkeypatch.setenv("ASR_DEC_EXEC", mode)
    B, T, V = 6, 120, 56
    cfg, sd, batch = oracle_case(B, T, 80, V, 9, D512, seed=49)
    sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
    sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    ref = R.RefTrainer({k: v.clone() for k, v in sd.items()}, cfg, warmup=25).iterate(batch)
    model, eng = _model(cfg, sd, V, "bf16")
    model.zero_flat_grads()
    loss, _ = model.train_step(to_pack(batch))
    torch.cuda.synchronize()
    assert bool(eng._dec_cache) == (mode == "1")
    want = float(ref["loss"])
    assert abs(float(loss[0]) - want) < BF16_LOSS_RTOL * abs(want), (float(loss[0]), want)
    gmax = max(float(g.abs().max()) for g in ref["grads"].values())
    for n, p in model.named_parameters():
        g = ref["grads"][n]
        assert bool(torch.isfinite(p.grad).all()), n
        if n.endswith(BF16_COS_EXEMPT) or float(g.abs().max()) < 1e-9 * gmax:
            continue
        c = cos(p.grad, g)
        assert c > (BF16_COS if float(g.abs().max()) >= 1e-5 * gmax else 0.97), (n, c)
