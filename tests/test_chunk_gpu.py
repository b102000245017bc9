"""Chunk-masked encoder attention on the GPU: the kernels of every dispatch path against fp64 dense attention with the mask
(tests/chunk_ref.py), the training step under a static chunk against the chunk-masked oracle, the streaming encoder against the
offline model under the same decoding mask, and a static-chunk captured step against the eager one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import chunk_ref as CR  # noqa: E402
from tests import dropout_ref as DR  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs() - atol - rtol * b.abs()
    assert torch.isfinite(a).all(), what + ": non-finite"
    assert float(err.max()) <= 0, f"{what}: max excess {float(err.max()):.3g}, max abs diff {float((a - b).abs().max()):.3g}"


def _klens(B, T, C):
    """ragged: full, not a multiple of C, shorter than one chunk, zero"""
    base = [T, T - C // 2 - 3, max(1, C // 2), 0, T - 2 * C - 1, 3 * C + 1]
    return [max(0, min(T, x)) for x in base[:B]]


CASES = [
    # dtype, B, H, T, dk    (T = 500: fused paths; T = 2000: tiled forward, dQ + dK/dV pair; fp32 / dk = 16: generic)
    (torch.bfloat16, 4, 3, 500, 64),
    (torch.bfloat16, 4, 1, 2000, 64),
    (torch.float32, 4, 2, 150, 16),
]


def _run(K, dtype, B, H, T, dk, C, left, klens, drop_p=0.0, seed=0):
    torch.manual_seed(T * 31 + C * 7 + left)
    d = H * dk
    qkv = torch.randn(B * T, 3 * d).to(dtype)
    do = torch.randn(B * T, d).to(dtype)
    klen = torch.tensor(klens, dtype=torch.int32)
    scale = dk ** -0.5
    qr, kr, vr = (qkv[:, i * d:(i + 1) * d].double().reshape(B, T, H, dk).clone().requires_grad_(True) for i in range(3))
    if drop_p > 0:      # the kernels' keep mask (tests/dropout_ref.py), applied to the probabilities as the oracle does
        keep = torch.from_numpy(DR.sdpa_mask(B, H, T, T, drop_p, seed))
        o_ref, lse_ref, vis = CR.sdpa_chunk_ref(qr, kr, vr, klen, C, left, scale)
        s = torch.einsum("bqhd,bkhd->bhqk", qr, kr) * scale
        dead = ~vis.any(-1, keepdim=True)
        p = torch.softmax(s.masked_fill(~vis & ~dead, float("-inf")), -1) * (~dead).double() * keep
        o_ref = torch.einsum("bhqk,bkhd->bqhd", p, vr)
    else:
        o_ref, lse_ref, vis = CR.sdpa_chunk_ref(qr, kr, vr, klen, C, left, scale)
    (o_ref * do.double().reshape(B, T, H, dk)).sum().backward()
    g = qkv.to(DEV)
    q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
    dg = torch.full_like(g, float("nan"))
    o_lo = torch.empty(B * T, d, dtype=dtype, device=DEV) if (dtype == torch.bfloat16 and T > 512) else None
    o, lse = K.sdpa_fwd(q, k, v, klen.to(DEV), B, H, T, T, dk, scale=scale, drop_p=drop_p, drop_seed=seed, o_lo=o_lo, chunk=C, left_chunks=left)
    K.sdpa_bwd(q, k, v, o, do.to(DEV), lse, klen.to(DEV), B, H, T, T, dk, dg[:, :d], dg[:, d:2 * d], dg[:, 2 * d:], scale=scale,
               drop_p=drop_p, drop_seed=seed, o_lo=o_lo, chunk=C, left_chunks=left)
    return o, lse, dg, o_ref, lse_ref, qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize("case", CASES, ids=["bf16_fused_T500", "bf16_tiled_T2000", "fp32_generic"])
@pytest.mark.parametrize("C,left", [(1, -1), (5, 0), (16, -1), (16, 2), (64, 0), (64, 2), (5, 2), (10000, -1), (10000, 2)])
def test_chunk_kernels_match_dense_reference(K, case, C, left):
    dtype, B, H, T, dk = case
    klens = _klens(B, T, C if C < T else 7)
    o, lse, dg, o_ref, lse_ref, gq, gk, gv = _run(K, dtype, B, H, T, dk, C, left, klens)
    d = H * dk
    ft = dict(rtol=2e-5, atol=2e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=1.5e-2)
    close(o.reshape(B, T, H, dk), o_ref, **ft, what="o")
    assert torch.isfinite(lse).all()
    close(lse, lse_ref, rtol=1e-4, atol=2e-3 if dtype == torch.bfloat16 else 1e-4, what="lse")
    _grad_gate(dtype, dg, d, (B, T, H, dk), gq, gk, gv)


def _tile_gate(got, ref, what, rel=2e-2):
    """bf16 gradients: relative error per (utterance, head, 32-row block) - a query tile for dQ, a key block for dK / dV - so that an
    error confined to one tile or one chunk edge of one head shows; blocks whose reference is ~0 (padded keys, dead queries) are held
    to a floor of 1e-3 of the tensor's typical block norm."""
    B, T, H, dk = ref.shape
    nb = (T + 31) // 32
    pad = nb * 32 - T
    a, r = (torch.nn.functional.pad(x.detach().double().cpu(), (0, 0, 0, 0, 0, pad)).reshape(B, nb, 32, H, dk) for x in (got, ref))
    assert torch.isfinite(a).all(), what + ": non-finite"
    err = (a - r).pow(2).sum((2, 4)).sqrt()          # (B, nb, H)
    rn = r.pow(2).sum((2, 4)).sqrt()
    floor = 1e-3 * float(rn.pow(2).mean().sqrt())
    bad = err > rel * rn + floor
    assert not bad.any(), f"{what}: {int(bad.sum())} blocks over the gate, first (b, block, h) = {tuple(torch.nonzero(bad)[0].tolist())}, " \
                          f"worst error {float(err[bad].max()):.3g}"


def _grad_gate(dtype, dg, d, shape, gq, gk, gv):
    """fp32: element-wise, as test_kernels_gpu's sdpa cases; bf16: per 32-row block of each head (_tile_gate) - element-wise gates
    fail on the few elements where a sum of up to T bf16-rounded products cancels."""
    for i, (g, what) in enumerate(((gq, "dq"), (gk, "dk"), (gv, "dv"))):
        got = dg[:, i * d:(i + 1) * d].reshape(shape)
        if dtype == torch.float32:
            close(got, g, rtol=2e-4, atol=2e-4, what=what)
        else:
            _tile_gate(got, g, what)


@pytest.mark.parametrize("case", CASES, ids=["bf16_fused_T500", "bf16_tiled_T2000", "fp32_generic"])
@pytest.mark.parametrize("C,left", [(16, -1), (5, 2)])
def test_chunk_kernels_with_dropout(K, case, C, left):
    dtype, B, H, T, dk = case
    o, lse, dg, o_ref, lse_ref, gq, gk, gv = _run(K, dtype, B, H, T, dk, C, left, _klens(B, T, C), drop_p=0.1, seed=1234)
    d = H * dk
    ft = dict(rtol=2e-5, atol=2e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    close(o.reshape(B, T, H, dk), o_ref, **ft, what="o")
    _grad_gate(dtype, dg, d, (B, T, H, dk), gq, gk, gv)


def test_full_chunk_is_full_attention(K):
    """chunk >= T with unlimited left context is full attention: the unmasked call's output and lse."""
    B, H, T, dk = 3, 4, 300, 64
    d = H * dk
    g = torch.randn(B * T, 3 * d, device=DEV).bfloat16()
    klen = torch.tensor([300, 211, 17], dtype=torch.int32, device=DEV)
    q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
    o0, l0 = K.sdpa_fwd(q, k, v, klen, B, H, T, T, dk)
    o1, l1 = K.sdpa_fwd(q, k, v, klen, B, H, T, T, dk, chunk=T, left_chunks=-1)
    close(o1, o0, rtol=1e-2, atol=1e-3, what="o")
    close(l1, l0, rtol=1e-5, atol=1e-5, what="lse")


# ----------------------------------------------------------------------------------------------- model
def _build(cfg, V, cls_name, **over):
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    M = getattr(Models, cls_name)
    mc = M.get_default_config()()
    d = dict(vars(cfg))
    d.pop("use_decoder", None)
    d.update(over)
    mc.fn_build(d)
    return M(mc, Vocab.synthetic(V))


def _pack(batch):
    from asr_chinese_e2e_amd.Utils import Pack
    p = Pack()
    p.add(**{k: v.to(DEV) for k, v in batch.items()})
    p.add(tgt_for_metric=p.tgt_for_input.clone())
    return p


def _case(B, T, F, V, L, over, seed=5):
    from oracle import ref_model as R
    from asr_chinese_e2e_amd.data_handler import synthetic_pack
    cfg = R.default_cfg(n_mels=F, lfr_m=1, **over)
    sd = R.init_state_dict(cfg, V, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:
        if "layer_norm" in k and k.endswith("weight"):
            sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g)
        elif "layer_norm" in k and k.endswith("bias"):
            sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=g)
    if "decoder.tgt_word_emb.weight" in sd:
        sd["decoder.tgt_word_emb.weight"] = sd["decoder.tgt_word_emb.weight"] * 0.05
        sd["decoder.tgt_word_prj.weight"] = sd["decoder.tgt_word_emb.weight"]
    pack = synthetic_pack(B, T, F, V, seed=seed + 2, ragged=True, Lmin=max(1, L - 4), Lmax=L)
    return cfg, sd, {k: pack[k] for k in ("wave", "wave_len", "tgt_for_input", "tgt_len")}


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["joint", "ctc_only"])
@pytest.mark.parametrize("left", [-1, 2])
def test_training_step_under_chunk_mask_matches_oracle(dtype, mode, left):
    if dtype == "fp32":
        over = dict(d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=2)
        B, T, F, V, L = 4, 70, 16, 40, 6
    else:
        over = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=2)
        B, T, F, V, L = 4, 136, 80, 56, 12
    over.update(dict(ctc_weight=0.3) if mode == "joint" else dict(use_decoder=False, ctc_weight=1.0))
    cfg, sd, batch = _case(B, T, F, V, L, over)
    sd64 = {k: v.double() for k, v in sd.items()}      # the oracle in fp64: what is left is the GPU's rounding
    b64 = dict(batch, wave=batch["wave"].double())
    out, grads = CR.loss_and_grads(sd64, cfg, b64, 16, left)
    full_out, _ = CR.loss_and_grads(sd64, cfg, b64, 0, -1)
    assert abs(float(out["loss"].detach()) - float(full_out["loss"].detach())) > 1e-4 * abs(float(full_out["loss"].detach()))      # the mask matters here
    model = _build(cfg, V, "TransformerCTC" if mode == "ctc_only" else "TransformerOffical", dtype=dtype, chunk_size=16,
                   left_chunks=left).cuda()
    model.load_state_dict(sd)
    model._ensure_engine(DEV)
    model.zero_flat_grads()
    loss, _ = model.train_step(_pack(batch))
    want = float(out["loss"])
    gmax = max(float(g.abs().max()) for g in grads.values())
    if dtype == "fp32":
        assert abs(float(loss[0]) - want) < 1e-5 * abs(want), (float(loss[0]), want)
        for n, p in model.named_parameters():
            got, ref = p.grad.double().cpu(), grads[n]
            excess = float(((got - ref).abs() - 3e-4 * ref.abs() - 3e-6 * max(gmax, 1.0)).max())
            assert excess <= 0, (n, excess, float((got - ref).abs().max()))
    else:
        assert abs(float(loss[0]) - want) < 1e-3 * abs(want), (float(loss[0]), want)
        for n, p in model.named_parameters():
            g = grads[n]
            if float(g.abs().max()) < 1e-6 * gmax or n.endswith("w_ks.bias"):
                continue
            relaxed = n.startswith("decoder.") and "pos_ffn.w_1." in n      # as test_model_gpu's bf16 gate
            assert _cos(p.grad, g) > (0.997 if relaxed else 0.999), (n, _cos(p.grad, g))


def test_chunk_at_least_T_reproduces_full_attention(deterministic_mode):
    over = dict(d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=2, ctc_weight=0.3)
    cfg, sd, batch = _case(4, 40, 16, 40, 6, over)
    res = []
    for chunk in (0, 64):
        model = _build(cfg, 40, "TransformerOffical", dtype="fp32", chunk_size=chunk).cuda()
        model.load_state_dict(sd)
        model._ensure_engine(DEV)
        model.zero_flat_grads()
        loss, _ = model.train_step(_pack(batch))
        res.append((float(loss[0]), {n: p.grad.clone() for n, p in model.named_parameters()}))
    assert res[0][0] == res[1][0]
    for n, g in res[0][1].items():
        assert torch.equal(g, res[1][1][n]), n


# ----------------------------------------------------------------------------------------------- streaming
def _stream_model(dtype, left, cls_name="TransformerOffical", C=8, dk=16, ctc_weight=None):
    if ctc_weight is None:
        ctc_weight = 0.5 if cls_name == "TransformerOffical" else 1.0
    over = dict(d_model=4 * dk, hidden_size=dk, num_head=4, ff_size=8 * dk, layer_num=2, ctc_weight=ctc_weight)
    if cls_name == "TransformerCTC":
        over["use_decoder"] = False
    cfg, sd, _ = _case(1, 8, 16, 30, 4, over, seed=11)
    model = _build(cfg, 30, cls_name, dtype=dtype, chunk_size=C, left_chunks=left, cross_mask="wave_len").cuda().eval()
    model.load_state_dict(sd)
    return model


def _stream_all(model, feats, lens, C):
    B, T, _ = feats.shape
    st = model.stream(B)
    parts = [[] for _ in range(B)]
    for c0 in range(0, T, C):
        nv = [max(0, min(C, int(l) - c0)) for l in lens]
        for b, ids in enumerate(st.push(feats[:, c0:c0 + C].contiguous(), nv)):
            parts[b] += ids
    return st, parts


@pytest.mark.parametrize("left", [-1, 0, 2])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_streaming_equals_offline(dtype, left):
    from asr_chinese_e2e_amd.Utils import Pack
    C = 8
    model = _stream_model(dtype, left, C=C)
    torch.manual_seed(3)
    B, T = 4, 8 * C
    lens = [T, T - 3, 2 * C + 5, C - 2]          # one ends several chunks before the others, one inside its first chunk
    feats = torch.randn(B, T, 16, device=DEV).to(torch.float32 if dtype == "fp32" else torch.bfloat16)
    wl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        ref = model.forward(Pack(wave=feats, wave_len=wl)).encoder_out
    st, parts = _stream_all(model, feats, lens, C)
    enc, got_lens = st.encoder_output()
    assert got_lens.tolist() == lens
    for b, l in enumerate(lens):
        a, r = enc[b, :l].float(), ref[b, :l].float()
        if dtype == "fp32":
            assert float((a - r).abs().max()) <= 1e-4, (b, float((a - r).abs().max()))
        else:
            assert _cos(a, r) >= 0.999, (b, _cos(a, r))
    if dtype == "fp32":
        assert parts == model.ctc_greedy_search(Pack(wave=feats, wave_len=wl))
        for w8 in (0.0, 0.5):      # the attention beam alone (its cross-attention reads the streamed output), and rescored by CTC
            want = model.transcribe(Pack(wave=feats, wave_len=wl), beam_size=3, ctc_weight=w8)
            got = st.finish(beam_size=3, ctc_weight=w8)
            assert [g["ids"] for g in got] == [w["ids"] for w in want]
            assert any(g["ids"] for g in got) or w8 > 0
            scores = [(g["score"], w["score"]) for g, w in zip(got, want)]
            assert all(a == b or abs(a - b) <= 1e-3 * max(1.0, abs(b)) for a, b in scores), scores


@pytest.mark.parametrize("left", [-1, 3])
def test_streaming_equals_offline_mfma_heads(left):
    """The production head shape (bf16, dk = 64): the chunks stream through the MFMA key-length kernels - the fused one with C = 16
    queries over the cache, and the tiled one once the unlimited-left cache grows past 512 rows - and the offline model through the
    chunk-masked ones (T = 640 > 512: the tiled forward)."""
    from asr_chinese_e2e_amd.Utils import Pack
    C = 16
    model = _stream_model("bf16", left, C=C, dk=64)
    torch.manual_seed(5)
    B, T = 3, 40 * C
    lens = [T, T - 37, 5 * C + 3]
    feats = torch.randn(B, T, 16, device=DEV).bfloat16()
    wl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        ref = model.forward(Pack(wave=feats, wave_len=wl)).encoder_out
    st, _ = _stream_all(model, feats, lens, C)
    if left < 0:
        assert st.cap > 512
    enc, _ = st.encoder_output()
    for b, l in enumerate(lens):
        for c0 in range(0, l, 8 * C):      # every stretch of the utterance, not only the whole
            a, r = enc[b, c0:min(l, c0 + 8 * C)].float(), ref[b, c0:min(l, c0 + 8 * C)].float()
            assert _cos(a, r) >= 0.999, (b, c0, _cos(a, r))


def test_streaming_ctc_model_finish_matches_transcribe():
    from asr_chinese_e2e_amd.Utils import Pack
    C = 8
    model = _stream_model("fp32", 1, "TransformerCTC", C=C)
    torch.manual_seed(4)
    B, T = 3, 5 * C
    lens = [T, 3 * C, 11]
    feats = torch.randn(B, T, 16, device=DEV)
    wl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    st, parts = _stream_all(model, feats, lens, C)
    assert parts == model.ctc_greedy_search(Pack(wave=feats, wave_len=wl))
    assert [g["ids"] for g in st.finish(beam_size=4)] == [w["ids"] for w in model.transcribe(Pack(wave=feats, wave_len=wl), beam_size=4)]


def test_streaming_past_the_positional_table_raises():
    model = _stream_model("fp32", -1, "TransformerCTC", C=8)
    st = model.stream(1)
    eng = model._ensure_engine(DEV)
    st.core.frames[0] = eng.pe.shape[0] - 4      # the frame counter of slot 0 of the sessions under the lock-step view
    with pytest.raises(ValueError, match="positional-encoding"):
        st.push(torch.zeros(1, 8, 16, device=DEV), [8])


def test_attention_only_model_streams_and_finishes_with_the_attention_beam():
    """A model without the CTC head (ctc_weight = 0): the tick ends once the encoder rows are stored, push has no ids to return, and
    finish runs the attention beam over the streamed rows.  model.sessions keeps refusing such a model."""
    from asr_chinese_e2e_amd.Utils import Pack
    C = 8
    model = _stream_model("fp32", 1, C=C, ctc_weight=0.0)
    assert not model.use_ctc
    torch.manual_seed(6)
    lens = [3 * C, C + 3]
    feats = torch.randn(2, 3 * C, 16, device=DEV)
    wl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    st = model.stream(2)
    for c0 in range(0, 3 * C, C):
        assert st.push(feats[:, c0:c0 + C].contiguous(), [max(0, min(C, l - c0)) for l in lens]) == [[], []]
    enc, got_lens = st.encoder_output()
    assert got_lens.tolist() == lens
    with torch.no_grad():
        ref = model.forward(Pack(wave=feats, wave_len=wl)).encoder_out
    for b, l in enumerate(lens):
        err = float((enc[b, :l] - ref[b, :l]).abs().max())
        assert err <= 1e-4, (b, err)
    # timestamps come from the CTC head: without one, transcribe - and so finish - gives results only with timestamps=False
    want = model.transcribe(Pack(wave=feats, wave_len=wl), beam_size=3, ctc_weight=0.0, timestamps=False)
    got = st.finish(beam_size=3, ctc_weight=0.0, timestamps=False)
    assert [g["ids"] for g in got] == [w["ids"] for w in want]
    with pytest.raises(ValueError, match="timestamps come from the CTC head"):
        st.finish(beam_size=3, ctc_weight=0.0)
    with pytest.raises(RuntimeError, match="CTC head"):
        model.sessions(2)
    for kw in (dict(timed=True), dict(beam_times=True, search="prefix_beam")):
        with pytest.raises(ValueError, match="CTC head"):
            model.stream(2, **kw)
    with pytest.raises(RuntimeError, match="CTC head"):
        model.stream(2, search="prefix_beam")


def test_finish_does_not_consume_the_stream():
    """finish() reads: the hypotheses, the encoder rows and a second finish are what they were.  The last utterance ends without a
    frame: the empty result, the single empty hypothesis, and zero rows like every row past an utterance's length."""
    C = 8
    model = _stream_model("fp32", -1, C=C)
    torch.manual_seed(8)
    lens = [2 * C + 5, C - 2, 0]
    feats = torch.randn(3, 3 * C, 16, device=DEV)
    st = model.stream(3, search="prefix_beam", beam_size=4, frame_topk=6)
    for c0 in range(0, 3 * C, C):
        st.push(feats[:, c0:c0 + C].contiguous(), [max(0, min(C, l - c0)) for l in lens])
    assert st.ended == [True, True, True] and st.valid == lens and st.offset == 3 * C
    before = st.nbest()
    first = st.finish(joint="ctc_rescore")
    assert st.nbest() == before
    assert st.finish(joint="ctc_rescore") == first
    assert first[2] == {"text": "", "ids": [], "score": float("-inf"), "tokens": []} and before[2] == [{"yseq": [], "score": 0.0}]
    assert any(r["ids"] for r in first)
    enc, got_lens = st.encoder_output()
    assert got_lens.tolist() == lens and enc.shape[1] == 3 * C
    for b, l in enumerate(lens):
        assert not enc[b, l:].any() and (l == 0 or enc[b, :l].any()), b


def test_sessions_results_is_finish_without_the_freeing():
    C = 8
    model = _stream_model("fp32", -1, C=C)
    torch.manual_seed(9)
    feats = torch.zeros(2, 2 * C, 16, device=DEV)
    feats[0] = torch.randn(2 * C, 16, device=DEV)
    ss = model.sessions(2)
    ss.open(0)
    ss.push(feats[:, :C].contiguous(), [C, 0], [False, False])
    ss.push(feats[:, C:].contiguous(), [C, 0], [True, False])
    assert ss.status(0)["state"] == "ended"
    res = ss.results([0])
    assert ss.status(0)["state"] == "ended" and ss.status(0)["frames"] == 2 * C
    assert res == ss.finish([0]) and set(res[0]) >= {"text", "ids", "score", "tokens"}
    assert ss.status(0)["state"] == "free"


def test_static_chunk_graphed_step_replays_the_eager_step(deterministic_mode):
    from asr_chinese_e2e_amd.graph import GraphedStep
    from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
    over = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=1, ctc_weight=0.3)
    cfg, sd, batch = _case(4, 96, 80, 60, 8, over)
    losses = []
    for graphed in (False, True):
        model = _build(cfg, 60, "TransformerOffical", dtype="bf16", chunk_size=16, left_chunks=2, dropout=0.0).cuda()
        model.load_state_dict(sd)
        opt = NoamOpt(512, 1, 25, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
        pack = _pack(batch)
        if graphed:
            step = GraphedStep(model, opt, pack)
            m = [float(step(pack)[0].loss) for _ in range(2)]      # a replay's metrics live in the graph's static buffers
        else:
            m = [float(model.iterate(pack, optimizer=opt, is_train=True)[0].loss) for _ in range(2)]
        torch.cuda.synchronize()
        losses.append((m, model._flat.p.clone()))
    assert losses[0][0] == losses[1][0]
    assert torch.equal(losses[0][1], losses[1][1])
