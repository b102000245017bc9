"""Kernel-level parity: every C-ABI entry point (through asr_chinese_e2e_amd.kernels) against the
CPU oracle on the same seeded inputs.  Needs a real MI355X: run with `-m gpu`.

Tolerances (stated per test): f32 storage -> fp32 round-off (1e-5 rel fwd, 1e-4 rel grads);
bf16 storage -> inputs are rounded to bf16 FIRST and the oracle computes in fp32/fp64 on the
rounded values, so the remaining error is the output rounding (2^-9 rel) plus, for the MFMA
attention, the bf16 rounding of the probabilities.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ctc_ref, logmel_ref, ref_model as R  # noqa: E402
from tests.helpers import ROOT, golden_model_case, load_npz  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def ws(K):
    return K.Workspace(DEV)


def close(a, b, rtol, atol, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})"


TOL = {torch.float32: dict(rtol=2e-5, atol=2e-5), torch.bfloat16: dict(rtol=1.6e-2, atol=1e-2)}


# ------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("d,use_res,use_pe,use_len", [(512, True, False, True), (512, False, True, False), (48, True, False, True),
                                                     (32, False, True, False), (1024, True, True, True), (200, True, False, True)])
def test_add_ln(K, ws, dtype, d, use_res, use_pe, use_len):
    torch.manual_seed(d)
    B, T = 3, 37
    x = torch.randn(B * T, d).to(dtype)
    res = torch.randn(B * T, d).to(dtype) if use_res else None
    gamma, beta = 1 + 0.2 * torch.randn(d), 0.1 * torch.randn(d)
    pe = R.positional_encoding(64, d) if use_pe else None
    lens = torch.tensor([37, 20, 1], dtype=torch.int32) if use_len else None
    dy = torch.randn(B * T, d).to(dtype)
    dy2 = torch.randn(B * T, d).to(dtype)
    # oracle in fp64 on the (rounded) inputs
    xr = x.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if use_res else None
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = xr + (rr if use_res else 0)
    yr = F.layer_norm(z, (d,), g64, b64, 1e-5)
    if use_pe:
        yr = yr + pe[:T].double().repeat(B, 1)
    mask = torch.ones(B * T, 1, dtype=torch.float64)
    if use_len:
        mask = (torch.arange(T).unsqueeze(0) < lens.view(-1, 1)).reshape(-1, 1).double()
    yr = yr * mask
    (yr * (dy.double() + dy2.double())).sum().backward()

    to = lambda t: None if t is None else t.to(DEV)
    y, xhat, rstd = K.add_ln_fwd(to(x), to(res), to(gamma), to(beta), to(pe), to(lens), B, T)
    close(y, yr, **TOL[dtype], what="ln fwd")
    dgamma, dbeta, dbias = (torch.zeros(d, device=DEV) for _ in range(3))
    dgamma += 1.0  # accumulate semantics
    dz, dxg = K.add_ln_bwd(to(dy), to(dy2), xhat, rstd, to(gamma), to(lens), dgamma, dbeta, dbias, B, T, ws)
    assert dxg is dz
    gt = dict(rtol=2e-4, atol=2e-4) if dtype == torch.float32 else dict(rtol=3e-2, atol=6e-2)
    close(dz, xr.grad, **gt, what="ln dz")
    close(dgamma - 1.0, g64.grad, rtol=gt["rtol"], atol=gt["atol"] * 4, what="ln dgamma")
    close(dbeta, b64.grad, rtol=gt["rtol"], atol=gt["atol"] * 4, what="ln dbeta")
    close(dbias, xr.grad.sum(0), rtol=gt["rtol"], atol=gt["atol"] * 4, what="ln dbias")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_add_ln_bwd_batched_reduce(K, ws, dtype):
    """Parameter gradients of several LayerNorm sites reduced by ONE asr_add_ln_bwd_reduce_batched launch ==
    the per-site reduction inside asr_add_ln_bwd: a small site (20 partial rows), a site at the cap of ln_grid() (5600 rows ->
    512 partial rows), one without a bias gradient, accumulate semantics.  Every site takes the one-workgroup-per-column-group
    path with plain adds: the split + atomic-add branches of both reductions ask for >= 1024 partial rows, which ln_grid()'s cap
    of 512 never yields.  Both routes are compared with each other only; tests/test_rowwise_states_gpu.py holds the sums to fp64."""
    d = 512
    sites = [(2, 40, True), (8, 700, True), (3, 37, False)]
    items, want = [], []
    for i, (B, T, with_bias) in enumerate(sites):
        g = torch.Generator().manual_seed(100 + i)
        x = torch.randn(B * T, d, generator=g).to(dtype).to(DEV)
        res = torch.randn(B * T, d, generator=g).to(dtype).to(DEV)
        gamma, beta = (1 + 0.2 * torch.randn(d, generator=g)).to(DEV), (0.1 * torch.randn(d, generator=g)).to(DEV)
        dy = torch.randn(B * T, d, generator=g).to(dtype).to(DEV)
        y, xhat, rstd = K.add_ln_fwd(x, res, gamma, beta, None, None, B, T)
        ref = [torch.full((d,), 0.5, device=DEV) for _ in range(3)]
        K.add_ln_bwd(dy, None, xhat, rstd, gamma, None, ref[0], ref[1], ref[2] if with_bias else None, B, T, ws)
        got = [torch.full((d,), 0.5, device=DEV) for _ in range(3)]
        part = torch.empty(K.add_ln_bwd_workspace_bytes(B * T, d), dtype=torch.uint8, device=DEV)
        dz, _ = K.add_ln_bwd(dy, None, xhat, rstd, gamma, None, got[0], got[1], got[2] if with_bias else None, B, T, ws, partials=part)
        assert all(float((t - 0.5).abs().max()) == 0.0 for t in got)       # nothing reduced yet
        items.append((part, got[0], got[1], got[2] if with_bias else None, B * T))
        want.append((ref, got, with_bias))
    K.add_ln_bwd_reduce_batched(items, d)
    for ref, got, with_bias in want:
        for k in range(3 if with_bias else 2):
            close(got[k], ref[k], rtol=1e-5, atol=1e-4, what=f"batched LN reduce, vector {k}")
        if not with_bias:
            assert float((got[2] - 0.5).abs().max()) == 0.0


# ------------------------------------------------------------------------------------ attention
def sdpa_ref(q, k, v, klen, causal, window, scale):
    """q (B,Tq,H,dk) etc., fp64 dense reference with autograd."""
    B, Tq, H, dk = q.shape
    Tk = k.shape[1]
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    qi = torch.arange(Tq).view(1, 1, Tq, 1)
    kj = torch.arange(Tk).view(1, 1, 1, Tk)
    vis = kj < klen.view(B, 1, 1, 1)
    if causal:
        vis = vis & (kj <= qi)
    if window >= 0:
        vis = vis & ((kj - qi).abs() <= window)
    dead = ~vis.any(-1, keepdim=True)          # a query with no admissible key (padded frame beyond the band): output 0, lse -inf
    s = s.masked_fill(~vis & ~dead, float("-inf"))
    p = torch.softmax(s, -1) * (~dead).to(s.dtype)
    lse = torch.logsumexp(s, -1).masked_fill(dead.squeeze(-1), float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", p, v), lse


SDPA_CASES = [
    # dtype, B, H, Tq, Tk, dk, causal, window, klens
    (torch.float32, 2, 4, 9, 11, 8, False, -1, [11, 5]),
    (torch.float32, 3, 2, 7, 7, 16, True, -1, [7, 4, 1]),
    (torch.float32, 2, 2, 70, 70, 64, False, 10, [70, 33]),
    (torch.bfloat16, 2, 3, 200, 200, 64, False, -1, [200, 77]),
    (torch.bfloat16, 2, 2, 130, 130, 64, True, -1, [130, 65]),
    (torch.bfloat16, 2, 2, 16, 500, 64, False, -1, [12, 7]),      # decoder cross-attention shape (text-length quirk)
    (torch.bfloat16, 1, 8, 500, 500, 64, False, -1, [500]),
    (torch.bfloat16, 2, 2, 300, 300, 64, False, 50, [300, 150]),  # +-50 frame band (long-form config)
    (torch.bfloat16, 2, 2, 20, 20, 16, True, -1, [20, 9]),        # bf16 storage, generic path
    (torch.bfloat16, 2, 2, 500, 500, 64, False, -1, [500, 333]),  # config-2 head shape, ragged: single-pass backward (all keys in one workgroup)
    (torch.bfloat16, 1, 2, 512, 512, 64, False, -1, [512]),       # exactly the 512 keys the single-pass backward holds
    (torch.bfloat16, 1, 2, 97, 513, 64, False, -1, [513]),        # one key more: the dQ + dK/dV kernel pair
    (torch.bfloat16, 2, 2, 300, 300, 64, False, 50, [300, 100]),  # band + short utterance: queries >= 151 of row 1 see NO key (lse -inf, zero gradients)
    (torch.bfloat16, 2, 2, 24, 24, 64, True, -1, [24, 11]),       # decoder self-attention shape (causal, To ~ 20)
    (torch.bfloat16, 1, 1, 40, 700, 64, False, 60, [650]),        # band on the kernel-pair path, dead rows included
    (torch.bfloat16, 2, 4, 48, 48, 64, False, 5, [48, 31]),       # a band over <= 64 keys: the short heads' own-delta pass with a window, two query tiles
    (torch.bfloat16, 3, 2, 64, 64, 64, True, -1, [64, 33, 1]),    # causal, exactly the 64 keys one wave holds; an utterance of one key
    # the long-form configuration's shape (BASELINE configs[4]: T = 2000 frames, +-50-frame band): single-pass band backward, one
    # workgroup per 512-key block, dQ of the tiles on a block boundary summed from two fp32 partials
    (torch.bfloat16, 1, 8, 2000, 2000, 64, False, 50, [2000]),
    (torch.bfloat16, 2, 2, 1100, 1100, 64, False, 50, [1100, 700]),   # ragged: the second utterance ends inside a key block; dead rows behind it
    (torch.bfloat16, 1, 2, 513, 513, 64, False, 7, [513]),            # one key past a block, narrow band
    (torch.bfloat16, 1, 1, 1024, 1024, 64, False, 240, [1000]),       # the widest band the kernel takes (2 w + 32 <= 512), block-aligned length
]


@pytest.mark.parametrize("dtype,B,H,Tq,Tk,dk,causal,window,klens", SDPA_CASES)
def test_sdpa(K, dtype, B, H, Tq, Tk, dk, causal, window, klens):
    torch.manual_seed(Tq * 7 + Tk)
    self_attn = Tq == Tk
    d = H * dk
    # fused QKV buffer (rows, 3*d) as the engine lays it out; cross attention: separate q and kv
    if self_attn:
        qkv = torch.randn(B * Tq, 3 * d).to(dtype)
        q2, k2, v2 = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    else:
        q2 = torch.randn(B * Tq, d).to(dtype)
        kv = torch.randn(B * Tk, 2 * d).to(dtype)
        k2, v2 = kv[:, :d], kv[:, d:]
    do = torch.randn(B * Tq, d).to(dtype)
    klen = torch.tensor(klens, dtype=torch.int32)
    scale = dk ** -0.5
    qr = q2.double().reshape(B, Tq, H, dk).clone().requires_grad_(True)
    kr = k2.double().reshape(B, Tk, H, dk).clone().requires_grad_(True)
    vr = v2.double().reshape(B, Tk, H, dk).clone().requires_grad_(True)
    o_ref, lse_ref = sdpa_ref(qr, kr, vr, klen, causal, window, scale)
    (o_ref * do.double().reshape(B, Tq, H, dk)).sum().backward()

    if self_attn:
        g = qkv.to(DEV)
        q, k, v = g[:, :d], g[:, d:2 * d], g[:, 2 * d:]
        dg = torch.full_like(g, float("nan"))
        dq, dk_, dv = dg[:, :d], dg[:, d:2 * d], dg[:, 2 * d:]
    else:
        q = q2.to(DEV)
        g = kv.to(DEV)
        k, v = g[:, :d], g[:, d:]
        dq = torch.full_like(q, float("nan"))
        dg = torch.full_like(g, float("nan"))
        dk_, dv = dg[:, :d], dg[:, d:]
    o, lse = K.sdpa_fwd(q, k, v, klen.to(DEV), B, H, Tq, Tk, dk, causal, window, scale)
    ft = dict(rtol=2e-5, atol=2e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=1.5e-2)
    close(o.reshape(B, Tq, H, dk), o_ref, **ft, what="sdpa o")
    close(lse, lse_ref, rtol=1e-4, atol=2e-3 if dtype == torch.bfloat16 else 1e-4, what="sdpa lse")
    K.sdpa_bwd(q, k, v, o, do.to(DEV), lse, klen.to(DEV), B, H, Tq, Tk, dk, dq, dk_, dv, causal, window, scale)
    gt = dict(rtol=2e-4, atol=2e-4) if dtype == torch.float32 else dict(rtol=3e-2, atol=4e-2)
    close(dq.reshape(B, Tq, H, dk), qr.grad, **gt, what="sdpa dq")
    close(dk_.reshape(B, Tk, H, dk), kr.grad, **gt, what="sdpa dk")
    close(dv.reshape(B, Tk, H, dk), vr.grad, **gt, what="sdpa dv")


@pytest.mark.parametrize("T,ragged", [(17, False), (12, True), (64, False), (40, True)])
def test_sdpa_bwd_short_causal_heads_reach_the_rounding_floor(K, T, ragged):
    """The decoder's self-attention backward (causal, every key of a head in one wave) takes delta = sum p dP / sum p from its own p and
    dP - the softmax backward the reference's autograd runs (/root/reference/Predictor/Models/attention.py:76-84) - instead of
    rowsum(dO o O) from the bf16-rounded O.  Where the rows of V are close to one another dP - delta cancels: the flash form
    measured 1 - cos(dQ) = 4.9e-4 here (T = 17), the floor set by rounding Q, K, V, dO to bf16 is 1.5e-4, this form 1.65e-4
    (tools/sdpa_delta_ab.py, tools/sdpa_delta_forms.py).  The gate sits between the two."""
    B, H, dk = 8, 8, 64
    d = H * dk
    g = torch.Generator().manual_seed(T)
    q, k, do = (torch.randn(B * T, d, generator=g, dtype=torch.float64) for _ in range(3))
    v = torch.randn(1, d, generator=g, dtype=torch.float64) + 0.1 * torch.randn(B * T, d, generator=g, dtype=torch.float64)
    klen = torch.tensor([T - (3 * b) % 5 if ragged else T for b in range(B)], dtype=torch.int32)
    qr, kr, vr = (x.reshape(B, T, H, dk).clone().requires_grad_(True) for x in (q, k, v))
    o_ref, _ = sdpa_ref(qr, kr, vr, klen, True, -1, dk ** -0.5)
    (o_ref * do.reshape(B, T, H, dk)).sum().backward()
    qb, kb, vb, dob = (x.bfloat16().to(DEV) for x in (q, k, v, do))
    o, lse = K.sdpa_fwd(qb, kb, vb, klen.to(DEV), B, H, T, T, dk, True, -1)
    dq, dk_, dv = (torch.full_like(qb, float("nan")) for _ in range(3))
    K.sdpa_bwd(qb, kb, vb, o, dob, lse, klen.to(DEV), B, H, T, T, dk, dq, dk_, dv, True, -1)
    valid = (torch.arange(T)[None, :] < klen[:, None]).reshape(B * T).to(DEV)      # rows past an utterance's end: zero gradients of keys nobody sees
    def one_minus_cos(a, r):
        a, r = a.double()[valid].flatten(), r.reshape(B * T, d).to(DEV)[valid].flatten()
        return 1.0 - float(torch.nn.functional.cosine_similarity(a, r, dim=0))
    assert torch.isfinite(dq).all() and torch.isfinite(dk_).all() and torch.isfinite(dv).all()
    assert one_minus_cos(dq, qr.grad) < 2.6e-4, one_minus_cos(dq, qr.grad)
    assert one_minus_cos(dk_, kr.grad) < 2.6e-4, one_minus_cos(dk_, kr.grad)
    assert one_minus_cos(dv, vr.grad) < 2e-5, one_minus_cos(dv, vr.grad)


@pytest.mark.parametrize("T,window", [(500, -1), (700, 60)])
def test_sdpa_bwd_delta_from_both_pieces_of_the_output(K, T, window):
    """Where the rows of K and of V share a component (here: one common vector of twice the noise's size - a bias behind a LayerNorm does it
    in the model) the bf16 rounding of O enters dQ through delta = rowsum(dO o O) multiplied by the MEAN key, and dK multiplied by the mean
    query - terms the true gradients do not contain (every query's dS sums to zero over its keys): at full size the top encoder layer's
    Q / K projection gradients measured 0.989 against the oracle.  Two remedies, both here:
    T = 500, the fused single-pass backward: the kernel centres the keys and takes the mean over the keys out of dK - 1 - cos(dQ) 5e-3 ->
    4e-5 with or without the low-order piece, and the rows of dK sum to zero over a head's keys;
    T = 700 with a band, the tiled forward and the dQ + dK/dV kernel pair: asr_sdpa_fwd's o_lo (ABI 10), delta from both pieces of O.
    (tools/sdpa_delta_forms_500.py and tools/sdpa_dk_mean.py emulate the forms in fp64.)"""
    B, H, dk = 2, 4, 64
    d = H * dk
    g = torch.Generator().manual_seed(T)
    q, do = (torch.randn(B * T, d, generator=g, dtype=torch.float64) for _ in range(2))
    k = torch.randn(B * T, d, generator=g, dtype=torch.float64) + 2.0 * torch.randn(1, d, generator=g, dtype=torch.float64)
    v = torch.randn(B * T, d, generator=g, dtype=torch.float64) + 2.0 * torch.randn(1, d, generator=g, dtype=torch.float64)
    klen = torch.tensor([T, T - 37], dtype=torch.int32)
    qr, kr, vr = (x.reshape(B, T, H, dk).clone().requires_grad_(True) for x in (q, k, v))
    o_ref, _ = sdpa_ref(qr, kr, vr, klen, False, window, dk ** -0.5)
    (o_ref * do.reshape(B, T, H, dk)).sum().backward()
    qb, kb, vb, dob = (x.bfloat16().to(DEV) for x in (q, k, v, do))
    valid = (torch.arange(T)[None, :] < klen[:, None]).reshape(B * T).to(DEV)
    err = {}
    for lo in (False, True):
        o_lo = torch.full_like(qb, float("nan")) if lo else None
        o, lse = K.sdpa_fwd(qb, kb, vb, klen.to(DEV), B, H, T, T, dk, False, window, o_lo=o_lo)
        if lo and T <= 512:      # the backward pass of these shapes does not read the piece: the forward pass clears the buffer
            assert not o_lo.any()
        elif lo:      # the two pieces together are the kernel's fp32 output to ~2^-17: against the fp64 output of the SAME rounded inputs the pair is
            # several times closer than o alone (what is left is the bf16 rounding of the probabilities in the P V product)
            with torch.no_grad():
                o_rb, _ = sdpa_ref(*(x.double().cpu().reshape(B, T, H, dk) for x in (qb, kb, vb)), klen, False, window, dk ** -0.5)
            o_rb = o_rb.reshape(B * T, d).to(DEV)[valid]
            e_pair, e_hi = float(((o.double() + o_lo.double())[valid] - o_rb).abs().max()), float((o.double()[valid] - o_rb).abs().max())
            assert e_pair < 0.35 * e_hi, (e_pair, e_hi)
            assert float(o_lo[valid].abs().max()) <= float(o[valid].abs().max()) * 2.0 ** -8
        dq, dk_, dv = (torch.full_like(qb, float("nan")) for _ in range(3))
        K.sdpa_bwd(qb, kb, vb, o, dob, lse, klen.to(DEV), B, H, T, T, dk, dq, dk_, dv, False, window, o_lo=o_lo)
        a, r = dq.double()[valid].flatten(), qr.grad.reshape(B * T, d).to(DEV)[valid].flatten()
        err[lo] = 1.0 - float(torch.nn.functional.cosine_similarity(a, r, dim=0))
        assert torch.isfinite(dk_).all() and torch.isfinite(dv).all()
        if T <= 512:      # single-pass kernel: sum_j dK_j = 0 per head (it would be ~ eps * T * mean query otherwise: ~2e-2 of the rows' total size here)
            dkh = dk_.double().reshape(B, T, H, dk) * (torch.arange(T, device=DEV)[None, :, None, None] < klen.to(DEV)[:, None, None, None])
            assert float(dkh.sum(1).norm(dim=-1).max()) < 2e-3 * float(dkh.norm(dim=-1).sum(1).max()), float(dkh.sum(1).norm(dim=-1).max())
    if T <= 512:
        assert err[False] < 2e-4 and err[True] < 2e-4, err
    else:
        assert err[True] < 2e-4 and err[True] < 0.2 * err[False], err


def test_sdpa_bf16_integer_exact(K):
    """Layout check with exact small-integer data (guide section 3: asymmetric operands): with
    one visible key per query the output must equal that key's V row exactly."""
    B, H, T, dk = 1, 2, 96, 64
    d = H * dk
    q = torch.zeros(B * T, d)
    k = torch.zeros(B * T, d)
    v = (torch.arange(B * T * d).reshape(B * T, d) % 251 - 125).float()
    q[:, :] = 1.0
    o, lse = K.sdpa_fwd(q.bfloat16().to(DEV), k.bfloat16().to(DEV), v.bfloat16().to(DEV),
                        torch.tensor([T], dtype=torch.int32, device=DEV), B, H, T, T, dk, True, 0, 1.0)
    # causal + window 0 -> each query sees exactly key i
    assert torch.equal(o.float().cpu(), v.bfloat16().float())


# ------------------------------------------------------------------------------------ CTC
def ctc_case(seed, B, T, V, Lmax, repeat=False, dtype=torch.float32):
    rng = np.random.RandomState(seed)
    logits = (rng.randn(B, T, V) * 2).astype(np.float32)
    in_len = rng.randint(max(T // 2, 1), T + 1, size=B)
    in_len[0] = T
    lab_len = rng.randint(0, Lmax + 1, size=B)
    lab_len[B - 1] = Lmax
    if B > 2:
        lab_len[1] = 0
    labels = rng.randint(1, V, size=(B, Lmax))
    if repeat:
        labels[:, 1::2] = labels[:, 0::2][:, : labels[:, 1::2].shape[1]]
    labels = np.where(np.arange(Lmax)[None] < lab_len[:, None], labels, 0)
    lt = torch.from_numpy(logits).to(dtype)
    return lt, in_len, labels, lab_len


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("seed,B,T,V,Lmax,repeat", [(0, 4, 20, 12, 5, False), (1, 3, 33, 50, 7, True), (2, 2, 100, 4232, 22, False),
                                                    (3, 5, 64, 31, 40, True), (4, 2, 12, 9, 3, False),
                                                    # bf16 row-in-registers kernels (V % 8 == 0): repeated labels, 2 and 4 registers per lane
                                                    (5, 3, 40, 64, 9, True), (6, 2, 160, 1024, 70, True), (7, 2, 300, 512, 130, True),
                                                    # long-form (BASELINE configs[4]): 2000 frames through the rescaled fp64 lattice
                                                    (8, 2, 2000, 64, 60, True)])
def test_ctc(K, ws, dtype, seed, B, T, V, Lmax, repeat):
    lt, in_len, labels, lab_len = ctc_case(seed, B, T, V, Lmax, repeat, dtype)
    # oracle: numpy float64 alpha/beta on the (rounded) logits + torch F.ctc_loss as second opinion
    nll_ref, g_ref = ctc_ref.ctc_batch(lt.double().numpy(), in_len, labels, lab_len, zero_infinity=True)
    x = lt.double().requires_grad_(True)
    tn = F.ctc_loss(F.log_softmax(x, -1).transpose(0, 1), torch.from_numpy(labels), torch.from_numpy(in_len), torch.from_numpy(lab_len),
                    blank=0, reduction="none", zero_infinity=True)
    tn.sum().backward()
    assert np.allclose(nll_ref, tn.detach().numpy(), rtol=1e-9, atol=1e-9)
    nll, dl = K.ctc_fwd_bwd(lt.to(DEV), torch.from_numpy(in_len).int().to(DEV), torch.from_numpy(labels).int().to(DEV),
                            torch.from_numpy(lab_len).int().to(DEV), ws, zero_infinity=True, grad_scale=0.5)
    # north_star: CTC loss within 1e-4 relative of the reference
    close(nll, torch.from_numpy(nll_ref), rtol=1e-4, atol=1e-4, what="ctc nll")
    gt = dict(rtol=1e-3, atol=2e-5) if dtype == torch.float32 else dict(rtol=1e-2, atol=4e-3)
    close(dl, 0.5 * torch.from_numpy(g_ref), **gt, what="ctc dlogits")
    close(dl, 0.5 * x.grad, **gt, what="ctc dlogits vs torch")


def test_ctc_infeasible_and_inplace(K, ws):
    # 'aa' over 2 frames is infeasible -> +inf (or 0 with zero_infinity), gradient 0; in-place grad
    logits = torch.zeros(2, 3, 4)
    labels = torch.tensor([[1, 1], [2, 3]], dtype=torch.int32)
    in_len = torch.tensor([2, 3], dtype=torch.int32)
    lab_len = torch.tensor([2, 2], dtype=torch.int32)
    x = logits.to(DEV)
    nll, dl = K.ctc_fwd_bwd(x, in_len.to(DEV), labels.to(DEV), lab_len.to(DEV), ws, zero_infinity=False, dlogits=x)
    assert dl.data_ptr() == x.data_ptr()
    assert math.isinf(float(nll[0])) and float(nll[0]) > 0
    assert float(dl[0].abs().max()) == 0.0
    ref, gref = ctc_ref.ctc_batch(logits.double().numpy(), [2, 3], labels.numpy(), [2, 2], zero_infinity=True)
    assert abs(float(nll[1]) - ref[1]) < 1e-5
    close(dl[1], torch.from_numpy(gref[1]), rtol=1e-4, atol=1e-6, what="inplace grad")
    nll0, _ = K.ctc_fwd_bwd(logits.to(DEV), in_len.to(DEV), labels.to(DEV), lab_len.to(DEV), ws, zero_infinity=True)
    assert float(nll0[0]) == 0.0


def test_ctc_rows_kernel_inplace_and_padding(K, ws):
    """bf16, V % 8 == 0: dlogits aliasing logits, padded frames zeroed, an infeasible utterance zeroed."""
    lt, in_len, labels, lab_len = ctc_case(11, 4, 24, 256, 6, True, torch.bfloat16)
    in_len[2] = 2
    lab_len[2] = 6      # infeasible: 6 labels in 2 frames
    nll_ref, g_ref = ctc_ref.ctc_batch(lt.double().numpy(), in_len, labels, lab_len, zero_infinity=True)
    x = lt.to(DEV).clone()
    nll, dl = K.ctc_fwd_bwd(x, torch.from_numpy(in_len).int().to(DEV), torch.from_numpy(labels).int().to(DEV),
                            torch.from_numpy(lab_len).int().to(DEV), ws, zero_infinity=True, dlogits=x)
    assert dl.data_ptr() == x.data_ptr()
    close(nll, torch.from_numpy(nll_ref), rtol=1e-4, atol=1e-4, what="ctc nll (in place)")
    close(dl, torch.from_numpy(g_ref), rtol=1e-2, atol=4e-3, what="ctc dlogits (in place)")
    assert float(dl[2].abs().max()) == 0.0
    for b in range(4):
        assert float(dl[b, in_len[b]:].abs().max() if in_len[b] < 24 else 0.0) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,V", [(3, 37, 11), (4, 130, 64), (2, 500, 4232)])
def test_ctc_greedy_decode(K, dtype, B, T, V):
    from oracle import ref_model as R
    rng = np.random.RandomState(B * T + V)
    # peaked logits along a random path with repeats and blanks, plus noise and a few exact ties
    path = rng.randint(0, min(V, 6), size=(B, T))
    path[:, 1::3] = path[:, 0:-1:3][:, : path[:, 1::3].shape[1]]
    x = rng.randn(B, T, V).astype(np.float32)
    np.put_along_axis(x, path[..., None], 6.0, axis=-1)
    x[0, 2, :] = 0.0                  # all-equal frame: first index (= blank) wins
    x[1, 3, 1] = x[1, 3, 4] = 9.0      # two-way tie: id 1 wins
    lens = rng.randint(T // 2, T + 1, size=B)
    lens[0] = T
    lt = torch.from_numpy(x).to(dtype)
    want = R.ctc_greedy_decode(lt.float().numpy(), lens)
    ids, n = K.ctc_greedy_decode(lt.to(DEV), torch.from_numpy(lens).int().to(DEV))
    ids, n = ids.cpu(), n.cpu()
    for b in range(B):
        assert ids[b, : int(n[b])].tolist() == want[b]
        assert int(ids[b, int(n[b]):].abs().sum()) == 0


@pytest.mark.parametrize("dtype,B,T,V,ld", [(torch.bfloat16, 3, 40, 4232, 4288), (torch.bfloat16, 4, 130, 64, 64), (torch.bfloat16, 2, 24, 256, 320),
                                            (torch.bfloat16, 2, 20, 50, 56), (torch.float32, 3, 37, 11, 11), (torch.bfloat16, 2, 30, 1024, 1024)])
@pytest.mark.parametrize("inplace", [False, True])
def test_ctc_best_path_from_the_loss_kernels(K, ws, dtype, B, T, V, ld, inplace):
    """asr_ctc_fwd_bwd's best_path (ABI 9): the frame-wise argmax taken by the kernel that holds the row (first index on ties, blank past
    in_len), also when the gradient overwrites the logits in place; collapsed by asr_ctc_collapse it is asr_ctc_greedy_decode's result and
    the oracle's (oracle.ref_model.ctc_greedy_decode).  Loss and gradient are the same bits with and without the extra output."""
    from oracle import ref_model as R
    lt, in_len, labels, lab_len = ctc_case(41, B, T, V, 6, True, dtype)
    lt[0, 2, :] = 0.0                      # all-equal frame: index 0 (blank) wins
    lt[1, 3, 1] = lt[1, 3, V - 1] = 30.0   # two-way tie at the two ends of the row: id 1 wins
    lt[B - 1, 5, V - 1] = 31.0             # the row's last element
    in_len[0] = T
    dev = lambda a: torch.from_numpy(a).int().to(DEV)
    buf = torch.full((B * T, ld), 40.0, dtype=dtype, device=DEV)      # the padding columns hold a LARGER value: they must not be looked at
    frames = buf.view(B, T, ld)[:, :, :V]
    frames.copy_(lt.to(DEV))
    ids0, n0 = K.ctc_greedy_decode(frames, dev(in_len))
    nll0, dl0 = K.ctc_fwd_bwd(frames.clone(), dev(in_len), dev(labels), dev(lab_len), ws, grad_scale=0.5)
    path = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    nll1, dl1 = K.ctc_fwd_bwd(frames, dev(in_len), dev(labels), dev(lab_len), ws, grad_scale=0.5, dlogits=frames if inplace else None, best_path=path)
    assert torch.equal(nll0, nll1) and torch.equal(dl0.contiguous(), dl1.contiguous())
    want = lt.float().argmax(-1)
    for b in range(B):
        assert path[b, : in_len[b]].cpu().tolist() == want[b, : in_len[b]].tolist(), b
        assert int(path[b, in_len[b]:].abs().sum()) == 0
    ids1, n1 = K.ctc_collapse(path, dev(in_len))
    assert ids1.data_ptr() == path.data_ptr()
    assert torch.equal(ids0, ids1) and torch.equal(n0, n1)
    hyp = R.ctc_greedy_decode(lt.float().numpy(), in_len)
    for b in range(B):
        assert ids1[b, : int(n1[b])].cpu().tolist() == hyp[b]
    # forward only (no gradient): the path is available too
    path2 = torch.empty(B, T, dtype=torch.int32, device=DEV)
    buf2 = torch.zeros(B * T, ld, dtype=dtype, device=DEV)
    fr2 = buf2.view(B, T, ld)[:, :, :V]
    fr2.copy_(lt.to(DEV))
    K.ctc_fwd_bwd(fr2, dev(in_len), dev(labels), dev(lab_len), ws, want_grad=False, best_path=path2)
    assert torch.equal(K.ctc_collapse(path2, dev(in_len))[0], ids0)


@pytest.mark.parametrize("dtype,B,T,V,ld", [(torch.bfloat16, 3, 40, 4232, 4288), (torch.bfloat16, 2, 24, 256, 320), (torch.float32, 2, 20, 12, 16),
                                            (torch.bfloat16, 2, 20, 50, 56)])
def test_ctc_padded_rows(K, ws, dtype, B, T, V, ld):
    """Rows `ld` > V elements apart (the training engine pads the CTC head's rows to whole 128-byte lines): loss, gradient and greedy
    path are bit-identical to the dense layout's, in place too, and the padding columns are never written."""
    lt, in_len, labels, lab_len = ctc_case(21, B, T, V, 6, True, dtype)
    dev = lambda a: torch.from_numpy(a).int().to(DEV)
    nll0, dl0 = K.ctc_fwd_bwd(lt.to(DEV), dev(in_len), dev(labels), dev(lab_len), ws, grad_scale=0.25)
    buf = torch.full((B * T, ld), 7.0, dtype=dtype, device=DEV)
    frames = buf.view(B, T, ld)[:, :, :V]
    frames.copy_(lt.to(DEV))
    ids0, n0 = K.ctc_greedy_decode(lt.to(DEV), dev(in_len))
    ids1, n1 = K.ctc_greedy_decode(frames, dev(in_len))
    assert torch.equal(ids0, ids1) and torch.equal(n0, n1)
    nll1, dl1 = K.ctc_fwd_bwd(frames, dev(in_len), dev(labels), dev(lab_len), ws, grad_scale=0.25, dlogits=frames)
    assert dl1.data_ptr() == buf.data_ptr() and dl1.stride() == frames.stride()
    assert torch.equal(nll0, nll1) and torch.equal(dl0, dl1.contiguous())
    assert float((buf[:, V:] - 7.0).abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="row stride"):
        K.ctc_fwd_bwd(torch.zeros(B * T, V + 3, dtype=dtype, device=DEV).view(B, T, V + 3)[:, :, :V], dev(in_len), dev(labels), dev(lab_len), ws)


def test_transposed_copies_with_own_offset_and_stride(K):
    """asr_transpose_batched_bf16 (ABI 6): every copy at its own offset and row stride."""
    torch.manual_seed(3)
    src = torch.randn(100 * 70 + 200 * 64, device=DEV).bfloat16()
    a, b = src[:7000].view(100, 70), src[7000:].view(200, 64)
    dst = torch.zeros(70 * 128 + 64 * 200 + 64, dtype=torch.bfloat16, device=DEV)
    tiles = [[0, 100, 70, (r << 16) | c, 64, 128] for r in range(2) for c in range(2)]
    tiles += [[7000, 200, 64, (r << 16) | 0, 64 + 70 * 128, 200] for r in range(4)]
    K.transpose_batched(src, dst, torch.tensor(tiles, dtype=torch.int32, device=DEV))
    assert torch.equal(dst[64:64 + 70 * 128].view(70, 128)[:, :100], a.t())
    assert float(dst[64:64 + 70 * 128].view(70, 128)[:, 100:].abs().max()) == 0.0 and float(dst[:64].abs().max()) == 0.0
    assert torch.equal(dst[64 + 70 * 128:].view(64, 200), b.t())


def test_ctc_full_size_properties(K, ws):
    """BASELINE size (B=32, T=500, V=4232): size-independent properties - every gradient row of a
    valid frame sums to 0 (softmax minus a distribution), padded frames are exactly 0, and the
    loss agrees with torch's own CTC on the same logits."""
    B, T, V, Lmax = 32, 500, 4232, 22
    lt, in_len, labels, lab_len = ctc_case(9, B, T, V, Lmax)
    lab_len = np.maximum(lab_len, 1)
    dev = lambda a: torch.from_numpy(a).int().to(DEV)
    nll, dl = K.ctc_fwd_bwd(lt.to(DEV), dev(in_len), dev(labels), dev(lab_len), ws)
    rows = dl.double().sum(-1).cpu()
    valid = torch.arange(T).unsqueeze(0) < torch.from_numpy(in_len).unsqueeze(1)
    assert float(rows[valid].abs().max()) < 1e-4
    assert float(dl.cpu()[~valid].abs().max()) == 0.0
    tn = F.ctc_loss(F.log_softmax(lt.double(), -1).transpose(0, 1), torch.from_numpy(labels), torch.from_numpy(in_len),
                    torch.from_numpy(lab_len), blank=0, reduction="none")
    close(nll, tn, rtol=1e-4, atol=1e-4, what="ctc nll full size")


# ------------------------------------------------------------------------------------ xent
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,V,smoothing", [(12, 17, 0.0), (12, 17, 0.1), (64, 4232, 0.0), (9, 33, 0.0)])
def test_xent(K, dtype, M, V, smoothing):
    torch.manual_seed(M + V)
    logits = (torch.randn(M, V) * 3).to(dtype)
    gold = torch.randint(1, V, (M,))
    gold[::3] = 0
    x = logits.double().requires_grad_(True)
    ref = R.ce_loss(x.unsqueeze(0), gold.unsqueeze(0), smoothing)
    ref.backward()
    n_valid = torch.tensor([float((gold != 0).sum())], device=DEV)
    row, dl = K.xent_fwd_bwd(logits.to(DEV), gold.int().to(DEV), n_valid, smoothing=smoothing, grad_scale=0.7)
    loss = row.sum() / n_valid
    assert abs(float(loss) - float(ref)) < (2e-5 if dtype == torch.float32 else 2e-5) * abs(float(ref)) + 1e-6
    gt = dict(rtol=1e-4, atol=1e-7) if dtype == torch.float32 else dict(rtol=1e-2, atol=2e-4)
    close(dl, 0.7 * x.grad, **gt, what="xent grad")
    # greedy ids from the same pass (ABI 9), in place too: every row - ignored ones included - first index on ties (torch.argmax)
    lt = logits.clone()
    lt[1, 5] = lt[1, V - 1] = 50.0      # a two-way tie at a valid row: the lower index wins
    lt[0] = 0.0                         # an ignored row (gold 0) whose logits are all equal: index 0
    buf = lt.to(DEV)
    ids = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    row2, dl2 = K.xent_fwd_bwd(buf, gold.int().to(DEV), n_valid, smoothing=smoothing, grad_scale=0.7, dlogits=buf, argmax=ids)
    assert dl2.data_ptr() == buf.data_ptr()
    assert torch.equal(ids.cpu().long(), lt.float().argmax(-1)), (ids.cpu(), lt.float().argmax(-1))
    row3, dl3 = K.xent_fwd_bwd(lt.to(DEV), gold.int().to(DEV), n_valid, smoothing=smoothing, grad_scale=0.7)
    assert torch.equal(row2, row3) and torch.equal(dl2, dl3)      # the extra output changes nothing else


def test_xent_golden(K):
    z = load_npz("ops.npz")
    pred, gold = torch.from_numpy(z["loss/pred"]), torch.from_numpy(z["loss/gold"])
    n_valid = torch.tensor([float((gold != 0).sum())], device=DEV)
    for sm, key in ((0.0, "loss/ce"), (0.1, "loss/ce_smooth01")):
        row, _ = K.xent_fwd_bwd(pred.to(DEV), gold.int().to(DEV), n_valid, smoothing=sm, want_grad=False)
        assert abs(float(row.sum() / n_valid) - float(z[key])) < 1e-5


@pytest.mark.parametrize("B,H,Tq,Tk,ragged", [(4, 8, 500, 500, True), (3, 2, 17, 500, False), (2, 8, 333, 470, True), (2, 4, 600, 200, True)])
def test_sdpa_fwd_pair_kernel_matches_two_pass_kernel(K, B, H, Tq, Tk, ragged):
    """Tuning option "sdpa_pair": both 32-query blocks of a wave in one pass over the key tiles - the same arithmetic per element in the same
    order as the two-pass kernel: outputs and log-sum-exp are bit-identical (partial last query block, more than 512 queries, ragged key lengths)."""
    torch.manual_seed(B + Tq)
    d = H * 64
    q, k, v = (torch.randn(B * T_, d, device=DEV).bfloat16() for T_ in (Tq, Tk, Tk))
    klen = torch.randint(max(1, Tk // 3), Tk + 1, (B,), dtype=torch.int32, device=DEV) if ragged else torch.full((B,), Tk, dtype=torch.int32, device=DEV)
    out = {}
    for mode in (0, 1):
        prev = K.set_option("sdpa_pair", mode)
        try:
            out[mode] = K.sdpa_fwd(q, k, v, klen, B, H, Tq, Tk, 64, False, -1)
        finally:
            K.set_option("sdpa_pair", prev)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------ decoder glue
def test_dec_preprocess_and_embed(K):
    for case in ("model_small_ragged.npz", "model_small_full.npz"):
        cfg, sd, batch, z = golden_model_case(case)
        tgt = batch["tgt_for_input"]
        ys_in, ys_out, lab, dec_len, lab_len, n_valid = K.dec_preprocess(tgt.to(DEV))
        assert np.array_equal(ys_in.cpu().numpy(), z["fwd/ys_in"])
        assert np.array_equal(ys_out.cpu().numpy(), z["fwd/ys_out"])
        assert np.array_equal(lab_len.cpu().numpy(), batch["tgt_len"].numpy())
        assert np.array_equal(dec_len.cpu().numpy(), batch["tgt_len"].numpy() + 1)
        assert float(n_valid) == float((torch.from_numpy(z["fwd/ys_out"]) != 0).sum())
    # interior zeros are stripped like y[y != 0] (transformer_official.py:264)
    t = torch.tensor([[5, 0, 6, 0], [0, 0, 0, 7]])
    ys_in, ys_out, lab, dec_len, lab_len, _ = K.dec_preprocess(t.to(DEV))
    ri, ro = R.decoder_preprocess(t)
    assert np.array_equal(ys_in.cpu().numpy()[:, : ri.shape[1]], ri.numpy())
    assert np.array_equal(ys_out.cpu().numpy()[:, : ro.shape[1]], ro.numpy())
    assert lab.cpu().tolist() == [[5, 6, 0, 0], [7, 0, 0, 0]]
    # embedding
    torch.manual_seed(0)
    V, d, B, To = 30, 48, 3, 5
    emb = torch.randn(V, d)
    ids = torch.randint(0, V, (B, To), dtype=torch.int32)
    pe = R.positional_encoding(16, d)
    for dtype in (torch.float32, torch.bfloat16):
        y = K.embed_pe_fwd(ids.to(DEV).reshape(-1), emb.to(DEV), pe.to(DEV), d ** -0.5, B, To, dtype)
        ref = emb[ids.long()] * d ** -0.5 + pe[:To].unsqueeze(0)
        close(y.reshape(B, To, d), ref, **TOL[dtype], what="embed fwd")
        dy = torch.randn(B * To, d).to(dtype)
        demb = torch.zeros(V, d, device=DEV)
        K.embed_bwd(ids.to(DEV).reshape(-1), dy.to(DEV), demb, d ** -0.5)
        refg = torch.zeros(V, d).index_add_(0, ids.long().reshape(-1), dy.float() * d ** -0.5)
        close(demb, refg, rtol=1e-5, atol=1e-5, what="embed bwd")
        dy2 = torch.randn(B * To, d).to(dtype)      # the gradient as a (projection path, residual path) pair, added in fp32 inside the kernel
        demb.zero_()
        K.embed_bwd(ids.to(DEV).reshape(-1), dy.to(DEV), demb, d ** -0.5, dy2=dy2.to(DEV))
        refg = torch.zeros(V, d).index_add_(0, ids.long().reshape(-1), (dy.float() + dy2.float()) * d ** -0.5)
        close(demb, refg, rtol=1e-5, atol=1e-5, what="embed bwd of a gradient pair")


# ------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_relu_colsum_cast(K, ws, dtype):
    torch.manual_seed(1)
    for rows, cols in ((37, 1024), (500, 48), (129, 4232), (5, 7)):
        a = torch.randn(rows, cols).to(dtype)
        da = torch.randn(rows, cols).to(dtype)
        r = K.relu_(a.clone().to(DEV))
        assert torch.equal(r.cpu(), torch.relu(a))
        dbias = torch.ones(cols, device=DEV)
        out = K.relu_bwd_(da.clone().to(DEV), torch.relu(a).to(DEV), dbias, ws)
        ref = da * (a > 0)
        assert torch.equal(out.cpu(), ref.to(dtype))
        close(dbias - 1, ref.double().sum(0), rtol=1e-5, atol=1e-4 if dtype == torch.float32 else 2e-2, what="relu_bwd dbias")
        big = torch.randn(rows, cols + 8).to(dtype).to(DEV)
        view = big[:, 3:3 + cols] if dtype == torch.float32 else big[:, 4:4 + cols]
        cs = torch.zeros(cols, device=DEV)
        K.colsum(view, cs, ws, accumulate=False)
        close(cs, view.double().sum(0), rtol=1e-5, atol=1e-4, what="colsum strided")
    x = torch.randn(1003)
    y = K.cast(x.to(DEV), torch.empty(1003, dtype=torch.bfloat16, device=DEV))
    assert torch.equal(y.cpu(), x.bfloat16())
    z = K.cast(y, torch.empty(1003, dtype=torch.float32, device=DEV))
    assert torch.equal(z.cpu(), x.bfloat16().float())


# ------------------------------------------------------------------------------------ optimizer
def test_optimizer(K, ws):
    torch.manual_seed(3)
    n = 100003
    p, g = torch.randn(n), torch.randn(n) * 3
    m, v = torch.zeros(n), torch.zeros(n)
    P, G, M_, V_ = (t.clone().to(DEV) for t in (p, g, m, v))
    lp = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    hyper = torch.zeros(4, device=DEV)
    sumsq = torch.zeros(1, device=DEV)
    z = load_npz("ops.npz")
    for it in range(1, 4):
        K.grad_sumsq(G, sumsq, ws)
        assert abs(float(sumsq) - float((g.double() ** 2).sum())) < 1e-5 * float((g.double() ** 2).sum())
        K.noam_hyper(step, hyper, 512, 4000, 1.0, 0.0, 0.9, 0.98)
        lr = R.noam_rate(it, 512, 4000)
        assert abs(float(hyper[0]) - lr) < 1e-6 * lr and int(step) == it
        K.adam_step(P, G, M_, V_, lp, hyper, sumsq, 5.0, 0.9, 0.98, 1e-9)
        total, (gc,) = R.clip_grad_norm([g])
        p, m, v = R.adam_update(p, gc, m, v, it, lr)
        close(G, gc, rtol=1e-5, atol=1e-7, what="clipped grad written back")
        close(P, p, rtol=1e-5, atol=1e-6, what=f"adam p step {it}")
        close(M_, m, rtol=1e-5, atol=1e-7, what="adam m")
        close(V_, v, rtol=1e-5, atol=1e-9, what="adam v")
        assert torch.equal(lp.cpu(), P.cpu().bfloat16())
        g = torch.randn(n) * (0.1 if it == 1 else 3)   # second step: no clipping active
        G.copy_(g)
    # Noam rates from the reference (golden)
    step.zero_()
    for s, want in zip(z["noam/steps"], z["noam/rate_512_4000"]):
        step.fill_(int(s) - 1)
        K.noam_hyper(step, hyper, 512, 4000, 1.0, 0.0, 0.9, 0.98)
        assert abs(float(hyper[0]) - want) < 2e-6 * want
    row = torch.rand(10, device=DEV)
    nll = torch.rand(4, device=DEV)
    nv = torch.tensor([7.0], device=DEV)
    out = K.loss_combine(row, nv, nll, 0.7, 0.3)
    ce, ctc = float(row.sum()) / 7.0, float(nll.sum()) / 4.0
    assert abs(float(out[0]) - (0.7 * ce + 0.3 * ctc)) < 1e-6 and abs(float(out[1]) - ce) < 1e-6 and abs(float(out[2]) - ctc) < 1e-6


# ------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K_,act,use_bias,use_res", [(256, 128, 64, 0, True, False), (1000, 512, 80, 0, True, False),
                                                          (333, 1536, 512, 0, True, False), (512, 4232, 512, 0, False, False),
                                                          (640, 1024, 512, 1, True, False), (384, 512, 1024, 0, True, True),
                                                          (130, 40, 24, 1, True, True),
                                                          # reduction length a multiple of 8 but not of 64 (the CTC head's input gradient reduces
                                                          # over V = 4232): the persistent kernel pads its last k-step from a zero page
                                                          (1000, 512, 4232, 0, False, False), (300, 256, 136, 0, True, False), (512, 640, 200, 0, True, False),
                                                          (16000, 512, 80, 0, True, False)])      # linear_in (F = 80): two k-steps, the second with 16 columns
def test_gemm_nt(K, M, N, K_, act, use_bias, use_res):
    torch.manual_seed(M + N)
    a = torch.randn(M, K_).bfloat16()
    w = (torch.randn(N, K_) * 0.1).bfloat16()
    bias = torch.randn(N) if use_bias else None
    res = torch.randn(M, N).bfloat16() if use_res else None
    ref = a.double() @ w.double().t()
    if use_bias:
        ref = ref + bias.double()
    if act:
        ref = torch.relu(ref)
    if use_res:
        ref = ref + res.double()
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.gemm_nt(a.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV), out, act, None if res is None else res.to(DEV))
    close(out, ref, rtol=1e-2, atol=1e-2, what="gemm_nt")


@pytest.mark.parametrize("M,N,K_,mode", [(16000, 512, 512, "none"), (16000, 1536, 512, "none"), (16000, 1024, 512, "relu"), (16000, 1024, 512, "mask"),
                                            (16000, 512, 1024, "res"), (1000, 512, 4232, "none"), (777, 520, 192, "none"), (300, 4232, 512, "relu"),
                                            (16000, 512, 80, "none")])
def test_gemm_nt_full_size_store_tails(K, M, N, K_, mode):
    """The persistent loader / consumer NT GEMM (gemm_nt_spec_kernel: four waves only issue the LDS-DMA, four only compute) at the sizes of
    the training step, every store-tail variant (bias, ReLU, ReLU mask, residual add), the ragged last k-step, edge tiles - against the
    fp32 product of the same bf16 operands.  (Rounds 2 - 3 compared it bit for bit with the all-in-one kernel it replaced; that kernel
    is in the git history.)"""
    from asr_chinese_e2e_amd._lib import ACT_RELU_MASK
    torch.manual_seed(M + N + K_)
    a = torch.randn(M, K_, device=DEV).bfloat16()
    w = (torch.randn(N, K_, device=DEV) * 0.1).bfloat16()
    bias = torch.randn(N, device=DEV) if mode in ("none", "relu") and K_ % 64 == 0 else None
    res = torch.relu(torch.randn(M, N, device=DEV)).bfloat16() if mode in ("mask", "res") else None
    act = {"none": 0, "relu": 1, "mask": ACT_RELU_MASK, "res": 0}[mode]
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.gemm_nt(a, w, bias, out, act, res)
    ref = a.float() @ w.float().t()
    if bias is not None:
        ref = ref + bias
    if mode == "relu":
        ref = torch.relu(ref)
    if mode == "mask":
        ref = torch.where(res.float() > 0, ref, torch.zeros_like(ref))
    if mode == "res":
        ref = ref + res.float()
    assert not bool(torch.isnan(out.float()).any())
    close(out, ref, rtol=1e-2, atol=1e-2 * max(1.0, (K_ / 512) ** 0.5), what=f"gemm_nt {mode}")
    if mode == "mask":      # masked elements are exact zeros
        assert bool((out[res.float() <= 0] == 0).all())


def test_armed_hand_over_orders_the_other_stream(K):
    """asr_stream_arm: the next armed-capable launch (here the NT GEMM) carries its own completion event and the other stream waits for
    it - no event record behind the kernel.  A copy of the GEMM's output queued on the other stream right after the launch sees the
    finished output, every time; an arm that no launch takes is reported as pending (the caller then forks)."""
    torch.manual_seed(5)
    side = torch.cuda.Stream()
    a = torch.randn(16000, 512, device=DEV).bfloat16()
    w = (torch.randn(1536, 512, device=DEV) * 0.1).bfloat16()
    ref = K.gemm_nt(a, w, None, torch.empty(16000, 1536, dtype=torch.bfloat16, device=DEV))
    torch.cuda.synchronize()
    for it in range(6):
        out = torch.zeros(16000, 1536, dtype=torch.bfloat16, device=DEV)
        copy = torch.full_like(out, 3.0)
        torch.cuda.synchronize()
        K.stream_arm(side.cuda_stream)
        K.gemm_nt(a, w, None, out)
        assert not K.stream_arm_pending()      # the launch took the arm
        K.STREAM_OVERRIDE = side.cuda_stream
        try:
            K.cast(out, copy)                  # bf16 -> bf16 copy on the other stream
        finally:
            K.STREAM_OVERRIDE = None
        torch.cuda.synchronize()
        assert torch.equal(copy, ref), it
    K.stream_arm(side.cuda_stream)
    K.cast(ref, torch.empty_like(ref))         # not an armed-capable entry point
    assert K.stream_arm_pending() and not K.stream_arm_pending()
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K_,ta,tb,act,acc,bias", [
    (420, 512, 80, False, True, 0, False, True),       # forward x W^T + b (linear_in of the d_model 512 golden case)
    (420, 1024, 512, False, True, 1, False, True),     # forward with ReLU (w_1)
    (420, 512, 1536, False, False, 0, False, False),   # input gradient dy W (qkv)
    (420, 1024, 512, False, False, 2, False, False),   # input gradient through the ReLU mask (w_2)
    (1536, 512, 420, True, False, 0, True, False),     # weight gradient dW += dy^T x
    (96, 32, 20, False, True, 0, False, True),         # toy widths of the small goldens
    (28, 30, 32, False, True, 0, False, False),        # tied output projection, V = 30
    (28, 32, 30, False, False, 0, True, False),        # its input gradient: reduction over V = 30 (not a multiple of 4), accumulate
    (21, 48, 36, True, False, 0, True, False),         # odd everything
    (70, 50, 66, True, True, 0, False, True),          # both operands transposed
    (1, 1, 1, False, True, 0, False, True),
])
def test_gemm_f32(K, M, N, K_, ta, tb, act, acc, bias):
    """asr_gemm_f32 (fp32 on the matrix cores: every projection of the parity mode) against the fp64 product: all four operand
    layouts, bias, ReLU, ReLU-mask store tail, accumulation into C, shapes with nothing a multiple of 4, strided views; and the
    same call twice gives the same bits (the reduction is never split)."""
    torch.manual_seed(M * 7 + N * 3 + K_)
    a = torch.randn((K_, M) if ta else (M, K_), device=DEV)
    b = torch.randn((N, K_) if tb else (K_, N), device=DEV) * 0.3
    bv = torch.randn(N, device=DEV) if bias else None
    c0 = torch.randn(M, N, device=DEV)
    mask = torch.relu(torch.randn(M, N, device=DEV)) if act == 2 else None
    if mask is not None:
        mask[::3, ::2] = -0.0
    ref = (a.double().t() if ta else a.double()) @ (b.double().t() if tb else b.double())
    if bias:
        ref = ref + bv.double()
    if act == 1:
        ref = torch.relu(ref)
    if act == 2:
        ref = ref * (mask.double() > 0)
    if acc:
        ref = ref + c0.double()
    scale = float(ref.abs().max()) + 1e-30
    outs = []
    for _ in range(2):
        out = c0.clone() if acc else torch.full((M, N), float("nan"), device=DEV)
        K.gemm_f32(a, b, out, bias=bv, trans_a=ta, trans_b=tb, act=act, mask=mask, accumulate=acc)
        outs.append(out)
    close(outs[0], ref, rtol=1e-5, atol=2e-6 * scale, what="gemm_f32")
    assert torch.equal(outs[0], outs[1])
    if act == 2:
        assert bool((outs[0][mask <= 0] == (c0[mask <= 0] if acc else 0)).all())
    # column-slice views of wider buffers (the fused Q|K|V buffer): leading dimensions larger than the rows
    if not ta and not tb and N >= 8 and K_ >= 8:
        wide_a = torch.randn(M, K_ + 24, device=DEV)
        wide_c = torch.full((M, N + 8), float("nan"), device=DEV)
        K.gemm_f32(wide_a[:, 8:8 + K_], b, wide_c[:, 4:4 + N])
        close(wide_c[:, 4:4 + N], wide_a[:, 8:8 + K_].double() @ b.double(), rtol=1e-5, atol=2e-6 * scale, what="gemm_f32 views")
        assert bool(torch.isnan(wide_c[:, :4]).all()) and bool(torch.isnan(wide_c[:, 4 + N:]).all())


@pytest.mark.parametrize("M,N,K_,trans_b,act", [(544, 512, 512, False, 0), (544, 1536, 512, False, 0), (544, 1024, 512, False, 1), (544, 512, 1024, False, 0),
                                                 (544, 512, 1536, True, 0), (544, 1024, 512, True, 0), (544, 512, 1024, True, 2), (37, 40, 24, False, 0),
                                                 (70, 264, 136, True, 2), (1000, 4232, 512, False, 0),
                                                 (544, 512, 4232, True, 0)])      # input gradient of the tied output projection: reduction over V
def test_gemm_small(K, M, N, K_, trans_b, act):
    """Small-M projections of the decoder: forward (x W^T + bias, ReLU) and input gradient (dy W from the weight as stored, ReLU mask in
    the store tail) against the fp64 product of the bf16-rounded operands."""
    torch.manual_seed(M + N + K_)
    a = torch.randn(M, K_).bfloat16()
    bm = (torch.randn(K_, N) if trans_b else torch.randn(N, K_)).bfloat16() * 0.25
    bias = torch.randn(N) if act != 2 else None
    ref = a.double() @ (bm.double() if trans_b else bm.double().t())
    if bias is not None:
        ref = ref + bias.double()
    mask = None
    if act == 1:
        ref = ref.clamp_min(0)
    elif act == 2:
        mask = torch.randn(M, N).bfloat16()
        ref = torch.where(mask.double() > 0, ref, torch.zeros_like(ref))
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.gemm_small(a.to(DEV), bm.to(DEV), bias.to(DEV) if bias is not None else None, out, trans_b=trans_b, act=act, mask=mask.to(DEV) if mask is not None else None)
    close(out, ref, rtol=1e-2, atol=2e-2 * math.sqrt(K_ / 64), what=f"gemm_small {M}x{N}x{K_} trans_b={trans_b} act={act}")
    with pytest.raises(RuntimeError):
        K.gemm_small(a.to(DEV)[:, :12], bm.to(DEV)[:12] if trans_b else bm.to(DEV)[:, :12], None, out, trans_b=trans_b)      # K not a multiple of 8


@pytest.mark.parametrize("M,N,K_", [(16000, 1024, 512), (777, 264, 128), (4100, 512, 1536)])
def test_gemm_nt_relu_mask_epilogue(K, M, N, K_):
    """ACT_RELU_MASK: C = (A W^T) where the mask tensor is > 0, else exactly 0 (the ReLU backward folded into the
    input-gradient GEMM's store tail); masks with +0, -0, negative and positive entries."""
    from asr_chinese_e2e_amd._lib import ACT_RELU_MASK
    torch.manual_seed(M + N)
    a = torch.randn(M, K_, device=DEV).bfloat16()
    w = (torch.randn(N, K_, device=DEV) * 0.05).bfloat16()
    h = torch.relu(torch.randn(M, N, device=DEV)).bfloat16()
    h[::7, ::5] = -0.0
    h[1::9, 1::3] = -1.5            # never produced by a ReLU; must be masked all the same
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.gemm_nt(a, w, None, out, ACT_RELU_MASK, h)
    ref = (a.float() @ w.float().t()) * (h.float() > 0)
    close(out, ref, rtol=1e-2, atol=1e-2, what="relu-mask epilogue")
    assert bool((out[h.float() <= 0] == 0).all())


def test_gemm_nt_integer_exact(K):
    """A = I (padded), asymmetric integer W: output must be W^T exactly (catches row/col swaps)."""
    M = N = 128
    Kd = 128
    a = torch.eye(M, Kd).bfloat16()
    w = ((torch.arange(N * Kd).reshape(N, Kd) * 7) % 201 - 100).float().bfloat16()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    K.gemm_nt(a.to(DEV), w.to(DEV), None, out)
    assert torch.equal(out.cpu().float(), w.float().t())


@pytest.mark.parametrize("N,K_", [(1536, 512), (4232, 512), (512, 1024)])
def test_gemm_full_size_persistent_paths(K, N, K_):
    """BASELINE-size GEMMs (M = 16000): every workgroup of the persistent NT kernel walks several
    tiles (ring and vmcnt accounting across tile boundaries, interior and edge tiles), the wgrad
    kernel takes both its ring-4 and its two-per-CU ring-2 form.  Reference: fp32 GEMM on the GPU."""
    M = 16000
    torch.manual_seed(N)
    a = torch.randn(M, K_, device=DEV).bfloat16()
    w = (torch.randn(N, K_, device=DEV) * 0.05).bfloat16()
    b = torch.randn(N, device=DEV)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    for _ in range(2):          # second launch: same result with warm caches / different arrival order
        K.gemm_nt(a, w, b, out, 1)
        ref = torch.relu(a.float() @ w.float().t() + b)
        close(out, ref, rtol=1e-2, atol=1e-2, what="persistent gemm_nt")
    dy = (torch.randn(M, N, device=DEV) * 0.5 + 0.1).bfloat16()
    dw = torch.zeros(N, K_, device=DEV)
    db = torch.ones(N, device=DEV)
    K.gemm_tn(dy, a, dw, accumulate=True, dbias=db)
    ref = dy.float().t() @ a.float()
    close(dw, ref, rtol=2e-3, atol=2e-3 * math.sqrt(M), what="dma gemm_tn")
    close(db - 1, dy.float().sum(0), rtol=1e-4, atol=1e-3 * math.sqrt(M), what="fused bias gradient")


@pytest.mark.parametrize("M,N,K_", [(256, 128, 128), (1000, 512, 80), (4000, 1536, 512), (513, 4232, 64), (70, 40, 24), (8197, 512, 512)])
def test_gemm_tn(K, M, N, K_):
    torch.manual_seed(M + K_)
    dy = (torch.randn(M, N) * 0.5).bfloat16()
    x = torch.randn(M, K_).bfloat16()
    ref = dy.double().t() @ x.double()
    dw = torch.ones(N, K_, device=DEV)
    K.gemm_tn(dy.to(DEV), x.to(DEV), dw, accumulate=True)
    close(dw - 1, ref, rtol=2e-3, atol=2e-3 * math.sqrt(M), what="gemm_tn accumulate")
    dw2 = torch.full((N, K_), float("nan"), device=DEV)
    K.gemm_tn(dy.to(DEV), x.to(DEV), dw2, accumulate=False)
    close(dw2, ref, rtol=2e-3, atol=2e-3 * math.sqrt(M), what="gemm_tn overwrite")
    db = torch.full((N,), 2.0, device=DEV)        # bias gradient from the same kernel (ragged M, clamped edge columns)
    K.gemm_tn(dy.to(DEV), x.to(DEV), dw2, accumulate=True, dbias=db)
    close(db - 2, dy.double().sum(0), rtol=1e-4, atol=1e-3 * math.sqrt(M), what="gemm_tn bias gradient")


@pytest.mark.parametrize("M,N,K_", [(16000, 512, 512), (16000, 4232, 512), (1000, 1536, 512), (8197, 264, 72)])
def test_gemm_tn_deterministic_mode(K, ws, deterministic_mode, M, N, K_):
    """ASR_DETERMINISTIC / asr_set_deterministic: partial tiles of the M-splits go to slabs that a second pass adds in split
    order - two launches on the same inputs give IDENTICAL bits (the default path adds them with fp32 atomics in arrival
    order), the values equal the fp32 product, and the bias gradient comes out of the same pass."""
    assert K.deterministic()
    torch.manual_seed(M + N)
    dy = (torch.randn(M, N) * 0.5).bfloat16().to(DEV)
    x = torch.randn(M, K_).bfloat16().to(DEV)
    ref = dy.double().cpu().t() @ x.double().cpu()
    outs = []
    for rep in range(3):
        dw = torch.ones(N, K_, device=DEV)
        db = torch.full((N,), 2.0, device=DEV)
        K.gemm_tn(dy, x, dw, accumulate=True, dbias=db, ws=ws)
        outs.append((dw.clone(), db.clone()))
    close(outs[0][0] - 1, ref, rtol=2e-3, atol=2e-3 * math.sqrt(M), what="deterministic gemm_tn")
    close(outs[0][1] - 2, dy.double().sum(0), rtol=1e-4, atol=1e-3 * math.sqrt(M), what="deterministic bias gradient")
    for dw, db in outs[1:]:
        assert torch.equal(dw, outs[0][0]) and torch.equal(db, outs[0][1])
    dw2 = torch.full((N, K_), float("nan"), device=DEV)
    K.gemm_tn(dy, x, dw2, accumulate=False, ws=ws)
    close(dw2, ref, rtol=2e-3, atol=2e-3 * math.sqrt(M), what="deterministic gemm_tn overwrite")
    with pytest.raises(RuntimeError):          # the grouped kernel only has the atomic form
        K.gemm_tn_grouped([(dy, x, dw2, None)])


def test_deterministic_mode_small_reductions(K, ws, deterministic_mode):
    """Embedding scatter with repeated ids, column sums and the batched LayerNorm reduce: bit-identical across launches."""
    torch.manual_seed(3)
    ids = torch.randint(0, 7, (512,), dtype=torch.int32, device=DEV)          # many repeats per id
    dy = torch.randn(512, 64, device=DEV)
    outs = []
    for _ in range(3):
        demb = torch.zeros(7, 64, device=DEV)
        K.embed_bwd(ids, dy, demb, 0.125)
        outs.append(demb)
    ref = torch.zeros(7, 64, dtype=torch.float64)
    ref.index_add_(0, ids.cpu().long(), dy.double().cpu() * 0.125)
    close(outs[0], ref, rtol=1e-5, atol=1e-5, what="serial embedding scatter")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    x = torch.randn(16000, 512, device=DEV).bfloat16()
    sums = []
    for _ in range(3):
        out = torch.zeros(512, device=DEV)
        K.colsum(x, out, ws, accumulate=True)
        sums.append(out)
    close(sums[0], x.double().sum(0), rtol=1e-4, atol=0.05, what="column sums")
    assert torch.equal(sums[0], sums[1]) and torch.equal(sums[0], sums[2])


def _tn_problem(M, N, K_, with_bias, seed, strided=False):
    g = torch.Generator().manual_seed(seed)
    dy = (torch.randn(M, N, generator=g) * 0.5 + 0.1).bfloat16().to(DEV)
    x = torch.randn(M, K_, generator=g).bfloat16().to(DEV)
    if strided:                                     # a column slice of a wider tensor (the K|V part of a Q|K|V gradient)
        wide = torch.zeros(M, N + 64, dtype=torch.bfloat16, device=DEV)
        wide[:, 64:] = dy
        dy = wide[:, 64:]
    dw = torch.full((N, K_), 1.0, device=DEV)
    db = torch.full((N,), 2.0, device=DEV) if with_bias else None
    return dy, x, dw, db


@pytest.mark.parametrize("shapes", [
    [(16000, 1536, 512, True), (16000, 512, 512, False), (16000, 1024, 512, True), (16000, 512, 1024, False)],   # one encoder layer of config 2
    [(16000, 512, 1024, False), (16000, 1024, 512, True)],                                                       # a feed-forward block's pair (w_2, w_1): 64 tiles of 128 x 128 x 4 splits
    [(16000, 512, 512, False), (16000, 1536, 512, True)],                                                        # an attention block's pair (out-projection, Q|K|V)
    [(4100, 264, 136, True), (4100, 520, 72, False)],                                                            # same rows, ragged: last stage partial, clamped edge columns
    [(16000, 4232, 512, True)],                                                                                # one problem: the CTC output layer
    [(1000, 1536, 512, True), (16000, 1024, 512, True), (1000, 512, 512, False), (1037, 1024, 512, True), (1037, 512, 1024, False)],  # decoder-like: different M per problem
    [(70, 40, 24, True), (513, 264, 136, True), (8197, 512, 80, False), (300, 128, 128, True), (64, 8, 8, True),
     (129, 256, 128, False), (4000, 520, 72, True), (999, 2048, 8, True), (77, 16, 512, False)],                 # ragged rows, clamped edge columns, > 8 problems (two launches)
])
def test_gemm_tn_grouped(K, shapes):
    """All weight gradients of a layer in one launch == the fp32 GEMM of each, bias gradients included."""
    probs = [_tn_problem(M, N, K_, wb, 31 * i + M, strided=(i % 2 == 1)) for i, (M, N, K_, wb) in enumerate(shapes)]
    if K.deterministic():      # ASR_DETERMINISTIC=1 for the whole run: the grouped kernel (fp32 atomics only) must refuse
        with pytest.raises(RuntimeError):
            K.gemm_tn_grouped(probs, accumulate=True)
        return
    for rep in range(2):                            # second launch accumulates on top of the first
        K.gemm_tn_grouped(probs, accumulate=True)
    for (M, N, K_, wb), (dy, x, dw, db) in zip(shapes, probs):
        ref = dy.float().t() @ x.float()
        close(dw - 1, 2 * ref, rtol=2e-3, atol=4e-3 * math.sqrt(M), what=f"grouped gemm_tn {M}x{N}x{K_}")
        if wb:
            close(db - 2, 2 * dy.float().sum(0), rtol=1e-4, atol=2e-3 * math.sqrt(M), what=f"grouped bias gradient {M}x{N}")
    for dy, x, dw, db in probs:
        dw.fill_(float("nan"))
    K.gemm_tn_grouped([(dy, x, dw, None) for dy, x, dw, db in probs], accumulate=False)
    for (M, N, K_, wb), (dy, x, dw, db) in zip(shapes, probs):
        close(dw, dy.float().t() @ x.float(), rtol=2e-3, atol=2e-3 * math.sqrt(M), what=f"grouped gemm_tn overwrite {M}x{N}x{K_}")


def test_gemm_tn_grouped_same_rows_takes_the_single_launch_tile_code(K):
    """Problems over the same >= 4096 rows run on the 128 x 128-tile code of the single launches (gemm_tn_multi_kernel; option "tn_multi" = 0 keeps
    the 256 x 128-tile grouped kernel): both give the fp32 product, and the single launches per problem give the same values."""
    if K.deterministic():
        pytest.skip("grouped launches are refused in deterministic mode")
    shapes = [(16000, 512, 1024, False), (16000, 1024, 512, True)]
    outs = {}
    for mode in (1, 0, "single"):
        probs = [_tn_problem(M, N, K_, wb, 7 * i + 3) for i, (M, N, K_, wb) in enumerate(shapes)]
        if mode == "single":
            for dy, x, dw, db in probs:
                K.gemm_tn(dy, x, dw, accumulate=True, dbias=db)
        else:
            prev = K.set_option("tn_multi", mode)
            try:
                K.gemm_tn_grouped(probs, accumulate=True)
            finally:
                K.set_option("tn_multi", prev)
        outs[mode] = probs
    for i, (M, N, K_, wb) in enumerate(shapes):
        dy, x = outs[1][i][0], outs[1][i][1]
        ref = dy.float().t() @ x.float()
        for mode in outs:
            close(outs[mode][i][2] - 1, ref, rtol=2e-3, atol=2e-3 * math.sqrt(M), what=f"tn_multi={mode} {M}x{N}x{K_}")
            if wb:
                close(outs[mode][i][3] - 2, dy.float().sum(0), rtol=1e-4, atol=1e-3 * math.sqrt(M), what=f"tn_multi={mode} bias gradient")
        close(outs[1][i][2], outs["single"][i][2], rtol=1e-5, atol=1e-3, what="multi vs single launches")      # same tile code, other split boundaries: fp32 summation order only


def test_gemm_tn_grouped_rejects_bad_arguments(K):
    dy, x, dw, db = _tn_problem(64, 16, 16, True, 0)
    with pytest.raises(RuntimeError):
        K.gemm_tn_grouped([(dy, x[:, :12], dw[:, :12], db)])          # K not a multiple of 8
    with pytest.raises(RuntimeError):
        K.gemm_tn_grouped([(dy[:, 1:9], x, dw[:8], None)])            # misaligned dY


# ------------------------------------------------------------------------------------ CER on the device
def test_cer_kernel_against_reference_golden(K):
    """asr_cer against the REFERENCE's own values, no host function in between: tests/golden/ops.npz cer/* are outputs of the reference's
    calculate_cer(convert_id2str(hyp), convert_id2str(ref)) (Utils/score.py:4-13 over vocab.py:75-79, written by oracle/gen_golden.py with
    the 12-token synthetic vocabulary)."""
    from asr_chinese_e2e_amd.data_handler import Vocab
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "ops.npz"))
    v = Vocab.synthetic(12)
    table = K.token_table(v._id2token, DEV)
    hyp = torch.from_numpy(z["cer/hyp"]).int().to(DEV)
    ref = torch.from_numpy(z["cer/ref"]).int().to(DEV)
    got = K.cer(hyp, ref, table, v._token2id[v.PAD]).cpu().numpy()
    assert np.allclose(got, z["cer/vals"], rtol=1e-6, atol=0), (got, z["cer/vals"])


def test_cer_matches_host_convention(K):
    """asr_cer == calculate_cer(convert_id2str(hyp), convert_id2str(ref)) (score.py:4-13 over vocab.py:75-79
    strings): pads dropped anywhere in the row, multi-character tokens, empty strings, rows longer than one
    64-lane chunk, explicit lengths."""
    from asr_chinese_e2e_amd.Utils import calculate_cer
    from asr_chinese_e2e_amd.data_handler import Vocab
    v = Vocab.synthetic(60)
    for tok in ("<unk>", "ab", "a", "b", "abc", " x"):          # multi-character tokens, one even containing a space
        v._token2id[tok] = len(v._token2id)
    v._id2token = list(v._token2id)
    V = len(v._id2token)
    table = K.token_table(v._id2token, DEV)
    rng = np.random.RandomState(5)
    B, Lh, Lr = 24, 150, 140
    hyp = rng.randint(0, V, size=(B, Lh)).astype(np.int32)
    ref = rng.randint(0, V, size=(B, Lr)).astype(np.int32)
    hyp[rng.rand(B, Lh) < 0.2] = 0                               # pads anywhere (argmax rows of the reference contain them)
    ref[rng.rand(B, Lr) < 0.2] = 0
    for b in range(0, B, 3):                                     # related strings: small distances
        n = min(Lh, Lr)
        hyp[b, :n] = ref[b, :n]
        hyp[b, rng.randint(0, n, 7)] = rng.randint(1, V, 7)
    hl = rng.randint(0, Lh + 1, B).astype(np.int32)
    rl = rng.randint(1, Lr + 1, B).astype(np.int32)
    hl[0], hl[1], rl[1] = 0, 0, 1
    hyp[2], ref[3] = 0, 0                                         # all pad: empty strings ("".split(" ") has one word)
    ref[1, 0] = 0
    hd, rd = torch.from_numpy(hyp).to(DEV), torch.from_numpy(ref).to(DEV)

    def host(h, r):
        return calculate_cer(v.convert_id2str(h.tolist()), v.convert_id2str(r.tolist()))

    got = K.cer(hd, rd, table, 0).cpu().numpy()
    want = np.array([host(hyp[b], ref[b]) for b in range(B)])
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)
    got = K.cer(hd, rd, table, 0, hyp_len=torch.from_numpy(hl).to(DEV), ref_len=torch.from_numpy(rl).to(DEV)).cpu().numpy()
    want = np.array([host(hyp[b, :hl[b]], ref[b, :rl[b]]) for b in range(B)])
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)
    with pytest.raises(RuntimeError):                            # strings that cannot fit the LDS are refused, not truncated
        K.cer(torch.zeros(1, 9000, dtype=torch.int32, device=DEV), torch.zeros(1, 9000, dtype=torch.int32, device=DEV), table, 0)


# ------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("m,n", [(1, 1), (4, 3)])
def test_spec_augment_in_front_end(K, m, n):
    """Normalise -> SpecAugment -> frame stacking on the device == oracle (whose augment step is pinned
    by the reference's own time_mask / freq_mask outputs), masks drawn with the reference's RNG calls."""
    import random
    from asr_chinese_e2e_amd.data_handler.processor import sample_spec_augment
    rng = np.random.RandomState(3)
    B, Tmax, n_mels = 5, 260, 80
    lens = [160 * (Tmax - 1), 160 * 199 + 11, 160 * 64, 160 * 45, 160 * 120 + 159]
    feat = torch.from_numpy(rng.randn(B, Tmax, n_mels).astype(np.float32) * 3 - 5).to(DEV)
    pyrng = random.Random(11)
    frames = [1 + l // 160 for l in lens]
    masks = [sample_spec_augment(n_mels, fr, pyrng) for fr in frames]
    assert any(mk[1] > mk[0] for mk in masks) and any(mk[3] > mk[2] for mk in masks)
    wl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    Tl = (Tmax + n - 1) // n
    out, out_len = K.utt_norm_lfr(feat, wl, m, n, Tl, torch.float32, masks=torch.tensor(masks, dtype=torch.int32, device=DEV))
    for i, fr in enumerate(frames):
        x = logmel_ref.utt_normalize(feat[i, :fr].cpu().double().numpy())          # (T, n_mels)
        y = logmel_ref.spec_augment(x.T, masks[i]).T                                 # augment works on (n_mels, T)
        ref = logmel_ref.build_lfr(y, m, n)
        got = out[i, : ref.shape[0]].cpu().numpy()
        assert int(out_len[i]) == ref.shape[0]
        assert np.allclose(got, ref, rtol=1e-4, atol=2e-5), i
        assert float(out[i, ref.shape[0]:].abs().max() if ref.shape[0] < Tl else 0.0) == 0.0


def test_logmel_lfr(K):
    rng = np.random.RandomState(0)
    lens = [16000 * 2 + 37, 16000, 4001]
    Smax = max(lens)
    wav = np.zeros((3, Smax), dtype=np.float32)
    for i, l in enumerate(lens):
        wav[i, :l] = rng.randn(l) * 0.1
    n_mels = 80
    Tmax = 1 + Smax // 160
    window = torch.from_numpy(logmel_ref.hann_periodic().astype(np.float32)).to(DEV)
    fb = torch.from_numpy(logmel_ref.mel_filterbank(n_mels).astype(np.float32)).to(DEV)
    wl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    feat = K.logmel(torch.from_numpy(wav).to(DEV), wl, window, fb, Tmax)
    for i, l in enumerate(lens):
        ref = logmel_ref.log_mel(wav[i, :l].astype(np.float64), n_mels)
        got = feat[i, : ref.shape[0]].cpu().numpy()
        # power spectrum in fp32: compare in the log domain with an absolute tolerance
        assert np.abs(got - ref).max() < 2e-3, np.abs(got - ref).max()
        assert float(feat[i, ref.shape[0]:].abs().max()) == 0.0 if ref.shape[0] < Tmax else True
    for dtype in (torch.float32, torch.bfloat16):
        Tl = (Tmax + 2) // 3
        out, out_len = K.utt_norm_lfr(feat, wl, 4, 3, Tl, dtype)
        for i, l in enumerate(lens):
            ref = logmel_ref.build_lfr(logmel_ref.utt_normalize(feat[i, : 1 + l // 160].cpu().double().numpy()), 4, 3)
            assert int(out_len[i]) == ref.shape[0]
            close(out[i, : ref.shape[0]], torch.from_numpy(ref), rtol=1e-4 if dtype == torch.float32 else 1e-2,
                  atol=1e-4 if dtype == torch.float32 else 2e-2, what="lfr")
            if ref.shape[0] < Tl:
                assert float(out[i, ref.shape[0]:].float().abs().max()) == 0.0
    # LFR index rule against the reference's own build_LFR_features (golden)
    z = load_npz("ops.npz")
    x9 = z["lfr/x9"]
    assert np.array_equal(logmel_ref.build_lfr(x9, 3, 1), z["lfr/x9_m3n1"])


# ------------------------------------------------------------------------------------ dropout
def test_dropout_mask_statistics(K):
    for p in (0.1, 0.5):
        m = K.dropout_mask(512, 1024, p, 1234).float()
        assert abs(float(m.mean()) - (1 - p)) < 3e-3
        assert abs(float(m[:, 0::2].mean()) - float(m[:, 1::2].mean())) < 5e-3          # both halves of the pair hash
        m2 = K.dropout_mask(512, 1024, p, 1235).float()
        assert 0.3 * p < float((m != m2).float().mean()) < 2.2 * p * (1 - p) + 0.05       # seeds decorrelate
    assert float(K.dropout_mask(8, 64, 0.0, 7).float().mean()) == 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode,d", [(1, 512), (2, 512), (1, 48)])
def test_add_ln_dropout(K, ws, dtype, mode, d):
    """Forward/backward with the kernel's own (regenerated) mask fed explicitly to the oracle."""
    torch.manual_seed(d + mode)
    B, T, p, seed = 2, 19, 0.3, 4242
    x = torch.randn(B * T, d).to(dtype)
    res = torch.randn(B * T, d).to(dtype)
    gamma, beta = 1 + 0.2 * torch.randn(d), 0.1 * torch.randn(d)
    pe = R.positional_encoding(32, d) if mode == 2 else None
    lens = torch.tensor([19, 11], dtype=torch.int32)
    dy = torch.randn(B * T, d).to(dtype)
    mask = K.dropout_mask(B * T, d, p, seed).cpu().double() / (1 - p)
    xr, rr = x.double().requires_grad_(True), res.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = (xr * mask if mode == 1 else xr) + rr
    yr = F.layer_norm(z, (d,), g64, b64, 1e-5)
    if mode == 2:
        yr = (yr + pe[:T].double().repeat(B, 1)) * mask
    keep = (torch.arange(T).unsqueeze(0) < lens.view(-1, 1)).reshape(-1, 1).double()
    yr = yr * keep
    (yr * dy.double()).sum().backward()
    to = lambda t: None if t is None else t.to(DEV)
    y, xhat, rstd = K.add_ln_fwd(to(x), to(res), to(gamma), to(beta), to(pe), to(lens), B, T, drop_p=p, drop_seed=seed, drop_mode=mode)
    close(y, yr, **TOL[dtype], what="ln dropout fwd")
    dgamma, dbeta, dbias = (torch.zeros(d, device=DEV) for _ in range(3))
    dz, dxg = K.add_ln_bwd(to(dy), None, xhat, rstd, to(gamma), to(lens), dgamma, dbeta, dbias, B, T, ws, drop_p=p, drop_seed=seed, drop_mode=mode)
    gt = dict(rtol=2e-4, atol=2e-4) if dtype == torch.float32 else dict(rtol=3e-2, atol=6e-2)
    close(dz, rr.grad, **gt, what="ln dropout dres")
    close(dxg, xr.grad, **gt, what="ln dropout dx")
    close(dbias, xr.grad.sum(0), rtol=gt["rtol"], atol=gt["atol"] * 4, what="ln dropout dbias")
    close(dgamma, g64.grad, rtol=gt["rtol"], atol=gt["atol"] * 4, what="ln dropout dgamma")


@pytest.mark.parametrize("dtype,B,H,Tq,Tk,dk,causal", [(torch.float32, 2, 2, 9, 12, 16, False), (torch.bfloat16, 2, 2, 130, 130, 64, False),
                                                     (torch.bfloat16, 1, 2, 70, 200, 64, False), (torch.bfloat16, 2, 2, 96, 96, 64, True)])
def test_sdpa_dropout(K, dtype, B, H, Tq, Tk, dk, causal):
    torch.manual_seed(Tq + Tk)
    p, seed, d = 0.2, 99, H * dk
    q = torch.randn(B * Tq, d).to(dtype)
    kv = torch.randn(B * Tk, 2 * d).to(dtype)
    do = torch.randn(B * Tq, d).to(dtype)
    klen = torch.tensor([Tk, max(Tk // 2, 1)][:B], dtype=torch.int32)
    scale = dk ** -0.5
    mask = K.sdpa_dropout_mask(B, H, Tq, Tk, p, seed).cpu().double() / (1 - p)
    qr = q.double().reshape(B, Tq, H, dk).clone().requires_grad_(True)
    kr = kv[:, :d].double().reshape(B, Tk, H, dk).clone().requires_grad_(True)
    vr = kv[:, d:].double().reshape(B, Tk, H, dk).clone().requires_grad_(True)
    s = torch.einsum("bqhd,bkhd->bhqk", qr, kr) * scale
    vis = torch.arange(Tk).view(1, 1, 1, Tk) < klen.view(B, 1, 1, 1)
    if causal:
        vis = vis & (torch.arange(Tk).view(1, 1, 1, Tk) <= torch.arange(Tq).view(1, 1, Tq, 1))
    pr = torch.softmax(s.masked_fill(~vis, float("-inf")), -1) * mask           # attention.py:82-83
    o_ref = torch.einsum("bhqk,bkhd->bqhd", pr, vr)
    (o_ref * do.double().reshape(B, Tq, H, dk)).sum().backward()
    g = kv.to(DEV)
    qd = q.to(DEV)
    o, lse = K.sdpa_fwd(qd, g[:, :d], g[:, d:], klen.to(DEV), B, H, Tq, Tk, dk, causal, -1, scale, drop_p=p, drop_seed=seed)
    ft = dict(rtol=2e-5, atol=2e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    close(o.reshape(B, Tq, H, dk), o_ref, **ft, what="sdpa dropout o")
    dq = torch.empty_like(qd)
    dg = torch.empty_like(g)
    K.sdpa_bwd(qd, g[:, :d], g[:, d:], o, do.to(DEV), lse, klen.to(DEV), B, H, Tq, Tk, dk, dq, dg[:, :d], dg[:, d:], causal, -1, scale,
               drop_p=p, drop_seed=seed)
    gt = dict(rtol=2e-4, atol=2e-4) if dtype == torch.float32 else dict(rtol=3e-2, atol=5e-2)
    close(dq.reshape(B, Tq, H, dk), qr.grad, **gt, what="sdpa dropout dq")
    close(dg[:, :d].reshape(B, Tk, H, dk), kr.grad, **gt, what="sdpa dropout dk")
    close(dg[:, d:].reshape(B, Tk, H, dk), vr.grad, **gt, what="sdpa dropout dv")


def test_embed_dropout(K):
    torch.manual_seed(0)
    V, d, B, To, p, seed = 30, 48, 3, 6, 0.25, 5
    emb = torch.randn(V, d)
    ids = torch.randint(0, V, (B, To), dtype=torch.int32)
    pe = R.positional_encoding(16, d)
    mask = K.dropout_mask(B * To, d, p, seed).cpu().float() / (1 - p)
    y = K.embed_pe_fwd(ids.to(DEV).reshape(-1), emb.to(DEV), pe.to(DEV), d ** -0.5, B, To, torch.float32, drop_p=p, drop_seed=seed)
    ref = (emb[ids.long()] * d ** -0.5 + pe[:To].unsqueeze(0)).reshape(B * To, d) * mask
    close(y, ref, rtol=1e-6, atol=1e-6, what="embed dropout fwd")
    dy = torch.randn(B * To, d)
    demb = torch.zeros(V, d, device=DEV)
    K.embed_bwd(ids.to(DEV).reshape(-1), dy.to(DEV), demb, d ** -0.5, drop_p=p, drop_seed=seed)
    refg = torch.zeros(V, d).index_add_(0, ids.long().reshape(-1), dy * mask * d ** -0.5)
    close(demb, refg, rtol=1e-5, atol=1e-5, what="embed dropout bwd")


@pytest.mark.parametrize("B,T,V,k,beam,nbest,peak", [(3, 60, 12, 6, 5, 5, 3.0), (2, 200, 50, 10, 5, 3, 1.0), (4, 37, 9, 8, 7, 7, 0.3), (1, 500, 40, 3, 16, 4, 2.0)])
def test_ctc_prefix_beam_kernel_matches_host_restatement(K, B, T, V, k, beam, nbest, peak):
    """asr_ctc_prefix_beam against oracle/decode_ref.ctc_prefix_beam_search (fp64 dictionaries of prefixes) fed with the same
    per-frame candidates: same n-best prefixes in the same order, scores to 1e-5 relative.  Ragged lengths, peaky and flat
    posteriors (flat ones keep many near-equal prefixes alive: the merge of an extension into an existing beam entry and the
    repeated-symbol rule are exercised on every frame), beam up to the kernel's maximum."""
    from oracle import decode_ref as D
    g = torch.Generator().manual_seed(B * 1000 + T)
    logits = torch.randn(B, T, V, generator=g) * peak
    lens = torch.randint(max(1, T // 2), T + 1, (B,), generator=g).to(torch.int32)
    lens[0] = T
    vals, ids, blank_lp = K.ctc_frame_topk(logits.reshape(B * T, V).to(DEV), k, 0)
    tok, ln, sc = K.ctc_prefix_beam(vals, ids, blank_lp, lens.to(DEV), B, T, beam, nbest, 0)
    tok, ln, sc = tok.cpu(), ln.cpu(), sc.cpu()
    logp = torch.log_softmax(logits.double(), -1).numpy()
    ids_h = ids.view(B, T, k).cpu().numpy()
    for b in range(B):
        Tb = int(lens[b])
        want = D.ctc_prefix_beam_search(logp[b, :Tb], beam, candidates=[list(ids_h[b, t]) for t in range(Tb)])[:nbest]
        want = [(p, s_) for p, s_ in want if s_ > -1e300]
        got = [(tuple(tok[b, r, : int(ln[b, r])].tolist()), float(sc[b, r])) for r in range(nbest) if int(ln[b, r]) >= 0]
        assert [p for p, _ in got] == [p for p, _ in want], (b, got, want)
        for (_, a), (_, w) in zip(got, want):
            assert abs(a - w) < 1e-5 * max(1.0, abs(w)), (a, w)


def test_ctc_prefix_beam_refuses_what_one_wave_cannot_rank(K):
    from asr_chinese_e2e_amd._lib import AsrHipError
    vals = torch.zeros(4, 10, device=DEV); ids = torch.zeros(4, 10, dtype=torch.int32, device=DEV); bl = torch.zeros(4, device=DEV)
    with pytest.raises(AsrHipError):
        K.ctc_prefix_beam(vals, ids, bl, None, 1, 4, 8, 1, 0)      # 8 * 11 > 64


@pytest.mark.parametrize("M,N,Kd,ldb_extra,inplace", [(1000, 512, 1024, 512, True), (700, 384, 128, 0, False), (16000, 512, 1024, 512, True)])
def test_gemm_nt_residual_add_store_tail(K, M, N, Kd, ldb_extra, inplace):
    """asr_gemm_nt_bf16 with a residual operand on the persistent kernel: C = A W^T + bias + res in the store tail, also in place
    (res = C: the accumulating cross-attention K|V input gradient d_enc += dKV W_kv, where W is a column slice of a wider
    transposed weight copy - row stride > K)."""
    torch.manual_seed(M + N)
    a = torch.randn(M, Kd).bfloat16()
    wfull = (torch.randn(N, Kd + ldb_extra) * 0.05).bfloat16()
    w = wfull[:, ldb_extra:]                       # (N, Kd) view, row stride Kd + ldb_extra
    bias = None if inplace else torch.randn(N)
    res = torch.randn(M, N).bfloat16()
    prod = a.double() @ w.double().t() + (0 if bias is None else bias.double())
    want = prod + res.double()
    ad, wd, rd = a.to(DEV), wfull.to(DEV)[:, ldb_extra:], res.to(DEV)
    out = rd.clone() if inplace else torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    K.gemm_nt(ad, wd, None if bias is None else bias.to(DEV), out, res=out if inplace else rd)
    got = out.double().cpu()
    # two bf16 roundings: the product (+ bias) when it crosses the LDS transpose of the store tail, then the sum - each within half an
    # ulp (2^-9 relative) of its own magnitude, so the bound is elementwise in |product| and |sum| (they differ where res cancels)
    err = (got - want).abs()
    tol = 2.0 ** -8 * (prod.abs() + want.abs()) + 1e-3
    assert bool((err <= tol).all()), f"{int((err > tol).sum())}/{err.numel()} off, max err {float(err.max()):.3e}"
