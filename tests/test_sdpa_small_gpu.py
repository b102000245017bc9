"""The one-wave attention kernels for heads of at most 64 queries and 64 keys (sdpa_fwd_small_bf16_kernel / sdpa_bwd_small_bf16_kernel,
tuning option "sdpa_small", on by default) against an fp64 reference, and against the one-workgroup kernels they stand in front of.

Tolerance.  Both kernel families compute in fp32 and round to bf16 once at each output, so the yardstick is the OLD kernels' own error
against the same fp64 reference on the same inputs (option off): max |x - ref| / max |ref| per output tensor, and the new kernels are
allowed twice that - a different fp32 summation order, nothing worse.  Two floors keep the rule meaningful where the old error is (nearly)
zero: 2^-20 max |ref| for o and lse (sixteen fp32 roundings: below that two fp32 orders cannot be told apart), and for the gradients
2^-24 dk max|dO| max|V| max(max|Q|, max|K|) scale - the rounding of ONE fp32 dk-term sum dP = dO . V carried through dS = p (dP - delta)
into a product with a row of K or Q; it decides only where the true gradient is exactly zero (a head whose queries see one key).
tools/sdpa_small_parity.py prints the same figures as a table (profiles/sdpa_small_parity.txt)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, H, DK, L_KV = 3, 8, 64, 6
SHAPES = [(1, 1), (8, 8), (17, 17), (23, 23), (23, 32), (32, 32), (33, 33), (40, 64), (64, 64)]
CASES = [(tq, tk, causal, layout) for tq, tk in SHAPES for causal in (False, True) for layout in ("self", "cross") if layout == "cross" or tq == tk]


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def key_lengths(Tk):
    """ragged, with 1 and Tk among them"""
    return torch.tensor([1, Tk, max(1, Tk // 2 + 1)], dtype=torch.int32)


def make_inputs(Tq, Tk, layout, seed, gain=1.0):
    """Rows as the decoder passes them: "self" = Q | K | V side by side in one (B*T, 3 H dk) buffer; "cross" = Q dense, K | V the columns
    of layer 2 in the (B*Tk, L 2 H dk) buffer of all layers.  Returns views (q, k, v, do) and the same-layout gradient views (dq, dk, dv)."""
    g = torch.Generator().manual_seed(seed)
    hd = H * DK
    rnd = lambda *s: (torch.randn(*s, generator=g) * gain).bfloat16().to(DEV)
    if layout == "self":
        assert Tq == Tk
        buf, gbuf = rnd(B * Tq, 3 * hd), torch.full((B * Tq, 3 * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
        q, k, v = (buf[:, i * hd:(i + 1) * hd] for i in range(3))
        dq, dk, dv = (gbuf[:, i * hd:(i + 1) * hd] for i in range(3))
    else:
        q, kv = rnd(B * Tq, hd), rnd(B * Tk, L_KV * 2 * hd)
        gkv = torch.full((B * Tk, L_KV * 2 * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
        k, v = kv[:, 4 * hd:5 * hd], kv[:, 5 * hd:6 * hd]
        dq, dk, dv = torch.full((B * Tq, hd), float("nan"), dtype=torch.bfloat16, device=DEV), gkv[:, 4 * hd:5 * hd], gkv[:, 5 * hd:6 * hd]
    return (q, k, v, rnd(B * Tq, hd)), (dq, dk, dv)


def reference(q, k, v, do, klen, Tq, Tk, causal, keep=None, drop_p=0.0):
    """fp64: o, lse, dq, dk, dv as (B, H, T, dk) / (B, H, Tq).  keep: (B, H, Tq, Tk) dropout keep mask or None."""
    f = lambda t, T: t.double().cpu().reshape(B, T, H, DK).transpose(1, 2)
    q, k, v, do = f(q, Tq), f(k, Tk), f(v, Tk), f(do, Tq)
    scale = DK ** -0.5
    s = q @ k.transpose(-1, -2) * scale
    vis = (torch.arange(Tk)[None, :] < klen.cpu()[:, None])[:, None, None, :].expand(B, H, Tq, Tk).clone()
    if causal:
        vis &= torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None]
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    m = torch.ones_like(p) if keep is None else keep.double().cpu() / (1.0 - drop_p)
    pd = p * m
    o = pd @ v
    dp = (do @ v.transpose(-1, -2)) * m
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    return dict(o=o, lse=lse, dq=ds @ k * scale, dk=ds.transpose(-1, -2) @ q * scale, dv=pd.transpose(-1, -2) @ do)


def run(K, mode, ins, grads, klen, Tq, Tk, causal, drop_p=0.0, seed=0):
    q, k, v, do = ins
    dq, dk, dv = grads
    prev = K.set_option("sdpa_small", mode)
    try:
        o, lse = K.sdpa_fwd(q, k, v, klen, B, H, Tq, Tk, DK, causal, -1, drop_p=drop_p, drop_seed=seed)
        for t in grads:
            t.fill_(float("nan"))
        K.sdpa_bwd(q, k, v, o, do, lse, klen, B, H, Tq, Tk, DK, dq, dk, dv, causal, -1, drop_p=drop_p, drop_seed=seed)
        torch.cuda.synchronize()
    finally:
        K.set_option("sdpa_small", prev)
    f = lambda t, T: t.double().cpu().reshape(B, T, H, DK).transpose(1, 2).clone()
    return dict(o=f(o, Tq), lse=lse.double().cpu().clone(), dq=f(dq, Tq), dk=f(dk, Tk), dv=f(dv, Tk))


def errors(got, ref):
    """max |x - ref| per output, and the scale max |ref| it is taken relative to (1 where the reference is identically zero)"""
    out = {}
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n]).all()), n
        den = float(ref[n].abs().max())
        out[n] = (float((got[n] - ref[n]).abs().max()), den if den > 0 else 1.0)
    return out


def floors(ins, ref):
    q, k, v, do = (float(t.float().abs().max()) for t in ins)
    g = 2.0 ** -24 * DK * do * v * max(q, k) * DK ** -0.5
    return dict(o=2.0 ** -20 * float(ref["o"].abs().max()), lse=2.0 ** -20 * float(ref["lse"].abs().max()), dq=g, dk=g, dv=g)


def measure(K, Tq, Tk, causal, layout, drop_p=0.0, seed=0, keep=None, gain=1.0, ins_grads=None):
    ins, grads = ins_grads or make_inputs(Tq, Tk, layout, 1000 * Tq + 10 * Tk + causal, gain)
    klen = key_lengths(Tk).to(DEV)
    ref = reference(*ins, klen, Tq, Tk, causal, keep, drop_p)
    old = errors(run(K, 0, ins, grads, klen, Tq, Tk, causal, drop_p, seed), ref)
    new = errors(run(K, 1, ins, grads, klen, Tq, Tk, causal, drop_p, seed), ref)
    return old, new, floors(ins, ref)


def check(old, new, floor, what):
    lines, bad = [], []
    for n in ("o", "lse", "dq", "dk", "dv"):
        (eo, den), (en, _) = old[n], new[n]
        bound = max(2.0 * eo, floor[n])
        lines.append(f"{what} {n:3s} old {eo / den:.3e} new {en / den:.3e} (relative to max |ref| = {den:.3e}; bound {bound / den:.3e})")
        if en > bound:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, bad


@pytest.mark.parametrize("Tq,Tk,causal,layout", CASES)
def test_small_kernels_match_fp64_within_twice_the_old_kernels_error(K, Tq, Tk, causal, layout):
    old, new, floor = measure(K, Tq, Tk, causal, layout)
    check(old, new, floor, f"Tq={Tq} Tk={Tk} causal={int(causal)} {layout}")


def test_padded_key_rows_get_zero_gradients_and_nan_free_outputs(K):
    """Rows of K and V past k_len hold NaN: nothing of them reaches an output, and their dK / dV rows are exact zeros (as the old kernels leave them)."""
    Tq, Tk = 23, 32
    ins, grads = make_inputs(Tq, Tk, "cross", 77)
    klen = key_lengths(Tk)
    for b, n in enumerate(klen.tolist()):
        ins[1][b * Tk + n:(b + 1) * Tk] = float("nan")
        ins[2][b * Tk + n:(b + 1) * Tk] = float("nan")
    got = run(K, 1, ins, grads, klen.to(DEV), Tq, Tk, False)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n]).all()), n
    for b, n in enumerate(klen.tolist()):
        assert bool((got["dk"][b, :, n:] == 0).all()) and bool((got["dv"][b, :, n:] == 0).all())


@pytest.mark.parametrize("Tq,Tk,causal", [(17, 17, True), (23, 32, False), (40, 64, False), (64, 64, True), (33, 33, True)])
def test_dropout_masks_equal_the_old_path_element_for_element(K, Tq, Tk, causal):
    """drop_p = 0.1.  V = one-hot rows (row j = e_j) makes o[q, j] = p_qj keep_qj / 0.9: its zero pattern inside the visible region IS the
    forward's keep mask.  dO = one-hot rows makes dV[j, q] = p_qj keep_qj / 0.9: the backward's (key-on-the-lane) mask.  Both must equal the
    old path's element for element; the backward's other (query-on-the-lane) use of the mask is pinned numerically, against the fp64
    reference under that mask, with the rule of the module docstring."""
    drop_p, seed = 0.1, 0x5EED + Tq
    ins, grads = make_inputs(Tq, Tk, "cross", 500 + Tq, gain=0.25)      # small scores: no probability rounds to zero in bf16
    q, k, v, do = ins
    eye_k = torch.eye(Tk, DK, device=DEV).bfloat16()[None, :, None, :].expand(B, Tk, H, DK).reshape(B * Tk, H * DK)
    eye_q = torch.eye(Tq, DK, device=DEV).bfloat16()[None, :, None, :].expand(B, Tq, H, DK).reshape(B * Tq, H * DK)
    v.copy_(eye_k)
    do.copy_(eye_q)
    klen = key_lengths(Tk).to(DEV)
    out = {m: run(K, m, ins, grads, klen, Tq, Tk, causal, drop_p, seed) for m in (0, 1)}
    keep = {m: out[m]["o"][..., :Tk] != 0 for m in (0, 1)}                                   # (B, H, Tq, Tk)
    keep_b = {m: out[m]["dv"][..., :Tq].transpose(-1, -2) != 0 for m in (0, 1)}              # (B, H, Tq, Tk)
    vis = (torch.arange(Tk)[None, :] < klen.cpu()[:, None])[:, None, None, :].expand(B, H, Tq, Tk).clone()
    if causal:
        vis &= torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None]
    assert torch.equal(keep[0], keep[1]) and torch.equal(keep_b[0], keep_b[1]) and torch.equal(keep[1], keep_b[1])
    assert not bool(keep[1][~vis].any())
    rate = 1.0 - float(keep[1][vis].double().mean())
    assert 0.05 < rate < 0.15, rate
    # every use of the mask, numerically: random V and dO, the reference under the mask just read
    ins2, grads2 = make_inputs(Tq, Tk, "cross", 900 + Tq)
    _, _, v0, do0 = ins2
    v.copy_(v0)
    do.copy_(do0)
    old, new, floor = measure(K, Tq, Tk, causal, "cross", drop_p, seed, keep[1] | ~vis, ins_grads=(ins, grads))
    check(old, new, floor, f"dropout Tq={Tq} Tk={Tk} causal={int(causal)}")


def test_backward_takes_the_armed_completion_event(K):
    """The cross-attention backward is the launch that hands dK | dV to the auxiliary stream by its own completion event
    (decoder_exec.hip): the one-wave kernel must take an arm as the one-workgroup kernel does, and a copy queued on the other stream
    right after the launch sees the finished dQ (the dense one of the three outputs: the copy kernel wants contiguous rows)."""
    Tq, Tk = 23, 32
    ins, grads = make_inputs(Tq, Tk, "cross", 5)
    q, k, v, do = ins
    dq, dk, dv = grads
    klen = key_lengths(Tk).to(DEV)
    o, lse = K.sdpa_fwd(q, k, v, klen, B, H, Tq, Tk, DK, False, -1)
    K.sdpa_bwd(q, k, v, o, do, lse, klen, B, H, Tq, Tk, DK, dq, dk, dv, False, -1)
    torch.cuda.synchronize()
    want = dq.clone()
    side = torch.cuda.Stream()
    for it in range(4):
        dq.fill_(float("nan"))
        copy = torch.zeros(B * Tq, H * DK, dtype=torch.bfloat16, device=DEV)
        torch.cuda.synchronize()
        K.stream_arm(side.cuda_stream)
        K.sdpa_bwd(q, k, v, o, do, lse, klen, B, H, Tq, Tk, DK, dq, dk, dv, False, -1)
        assert not K.stream_arm_pending()      # the launch took the arm
        K.STREAM_OVERRIDE = side.cuda_stream
        try:
            K.cast(dq, copy)
        finally:
            K.STREAM_OVERRIDE = None
        torch.cuda.synchronize()
        assert torch.equal(copy, want), it


def test_decoder_layer_backward_still_releases_the_auxiliary_stream(monkeypatch):
    """One decoder layer, forward and backward through the native sequencer, with the auxiliary stream (d_enc += dK|dV W_kv runs there,
    released by the attention backward's completion event) and on one stream: the same d_enc to two bf16 steps of its largest element (the
    GEMM beside the chain is sized for fewer CUs, so its fp32 sums may run in another order).  The dK | dV buffer holds NaN before the
    backward pass: a GEMM released too early would carry them into d_enc."""
    from tests.test_model_gpu import build, oracle_case, to_pack
    D512 = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=1, ctc_weight=0.3, dropout=0.0)
    Bm, T, V = 6, 160, 56
    cfg, sd, batch = oracle_case(Bm, T, 80, V, 9, D512, seed=43)
    pack = to_pack(batch)
    got = {}
    for overlap in ("1", "0"):
        monkeypatch.setenv("ASR_WGRAD_OVERLAP", overlap)
        model = build(cfg, V, "TransformerOffical", dtype="bf16").cuda()
        model.load_state_dict({k: v for k, v in sd.items()})
        model.train()
        eng = model._ensure_engine(torch.device("cuda", 0))
        assert eng._aux_active() == (overlap == "1")
        model.zero_flat_grads()
        eng.refresh_transposes()
        ev, x, wave_len, prep = model._prepare(pack, training=True)
        enc, _ = eng.encoder_fwd(x, wave_len)
        cross_len, Tk = model._cross(eng, pack, wave_len, T)
        assert Tk == 16 and prep[0].shape[1] <= 64
        pred, cache = eng.decoder_fwd(prep, enc, cross_len, Bm, T, Tk)
        assert eng._dec_cache      # the sequencer ran
        for bufs in eng._dec_cache.values():
            bufs["g_kv_all"].fill_(float("nan"))      # a d_enc GEMM that started early would read these
        dpred = torch.randn(pred.shape, generator=torch.Generator().manual_seed(3)).to(pred.dtype).to(DEV)
        d_enc = torch.zeros_like(enc)
        eng.decoder_bwd(cache, dpred, d_enc)
        eng.join_side()
        torch.cuda.synchronize()
        eng._release_kept(joined=True)
        got[overlap] = d_enc.float().cpu()
    assert bool(torch.isfinite(got["1"]).all()) and float(got["1"].abs().sum()) > 0
    assert float((got["1"] - got["0"]).abs().max()) <= 2.0 ** -6 * float(got["0"].abs().max())
