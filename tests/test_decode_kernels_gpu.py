"""The search and row-compaction entry points against plain restatements written here: asr_decode_attn (fp64 dense softmax
attention), asr_logsoftmax_topk / asr_ctc_frame_topk (fp64 log_softmax + stable descending sort), asr_beam_step
(tests/beam_ref.py, exact), asr_cache_gather / asr_rows_gather / asr_rows_scatter_add (index arithmetic, exact) and
asr_grad_sumsq_noam (asr_grad_sumsq + asr_noam_hyper).  The whole beam searches of test_model_gpu.py reach these kernels only
through argmax / top-k decisions on small golden cases; here each runs at the shapes and edges where it could go wrong.

bf16 inputs are rounded to bf16 first and the restatement computes on the rounded values (as in test_kernels_gpu.py).
Needs a real MI355X: run with `-m gpu`.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import beam_ref as BR  # noqa: E402

DEV = "cuda"
U32 = 2.0 ** -24          # unit round-off of fp32
U16 = 2.0 ** -8           # unit round-off of bf16 (8-bit significand)


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def AsrHipError():
    from asr_chinese_e2e_amd._lib import AsrHipError
    return AsrHipError


def bits(t):
    """Integer view of a tensor's storage: bit-for-bit comparison, NaN / -0.0 included."""
    t = t.detach().contiguous().cpu()
    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(t.dtype, t.dtype))


# ------------------------------------------------------------------------------------ decode_attn
def _attn_ref(q, kc, vc, n_of_row, grp_of_row, H, dk, Tk_cap, scale):
    """fp64 single-query softmax attention: row r, head h sees keys t < n_of_row[r] of kv group grp_of_row[r]."""
    R = q.shape[0]
    out = np.zeros((R, H * dk))
    for r in range(R):
        n = n_of_row[r]
        if n <= 0:
            continue
        g = grp_of_row[r]
        for h in range(H):
            cs = slice(h * dk, (h + 1) * dk)
            k = kc[g * Tk_cap:g * Tk_cap + n, cs]
            v = vc[g * Tk_cap:g * Tk_cap + n, cs]
            s = (k @ q[r, cs]) * scale
            p = np.exp(s - s.max())
            out[r, cs] = (p / p.sum()) @ v
    return out


def _attn_case(K, dtype, dk, H, Tk_cap, form, lens, seed):
    """One asr_decode_attn call (through K.decode_attn) with q / k / v / o as strided column views, every cache row past its
    length NaN; returns (o, o's padded buffer, reference, effective lengths)."""
    B, beam = 2, 3
    R, hd = B * beam, H * dk
    kv_div = beam if form in ("cross", "uniform_kvdiv") else 1
    len_div = beam if form == "cross" else 1
    G = R // kv_div
    g = torch.Generator().manual_seed(seed)
    qbuf = (2.0 * torch.randn(R, hd + 24, generator=g)).to(dtype)                  # q = columns [8, 8 + hd): ldq = hd + 24
    kv = torch.randn(G * Tk_cap, 2 * hd, generator=g).to(dtype)                    # k | v fused, as the decoder's caches
    if form.startswith("uniform"):
        n_row = [min(lens, Tk_cap)] * R
        k_len, k_len_uniform = None, lens
    else:
        per = R // len_div
        lv = [lens[i % len(lens)] for i in range(per)]
        n_row = [min(lv[r // len_div], Tk_cap) for r in range(R)]
        k_len, k_len_uniform = torch.tensor(lv, dtype=torch.int32, device=DEV), 0
    grp = [r // kv_div for r in range(R)]
    for r in range(R):                                   # keys / values the kernel must not read
        kv[grp[r] * Tk_cap + max(n_row[r], 0):(grp[r] + 1) * Tk_cap] = float("nan")
    q64, kv64 = qbuf[:, 8:8 + hd].double().numpy(), kv.double().numpy()
    scale = dk ** -0.5
    ref = _attn_ref(q64, kv64[:, :hd], kv64[:, hd:], n_row, grp, H, dk, Tk_cap, scale)
    qd, kvd = qbuf.to(DEV), kv.to(DEV)
    obuf = torch.full((R, hd + 16), 7.0, dtype=dtype, device=DEV)                  # o = columns [16, 16 + hd): the rest must stay 7
    o = K.decode_attn(qd[:, 8:8 + hd], kvd[:, :hd], kvd[:, hd:], H, dk, Tk_cap, kv_div=kv_div, k_len=k_len, k_len_uniform=k_len_uniform,
                      len_div=len_div, o=obuf[:, 16:16 + hd])
    torch.cuda.synchronize()
    return o, obuf, ref, n_row, kv64[:, hd:]


# lengths per form: 0 (exact zero output), 1, a partial wave, Tk_cap and past it (clamped to Tk_cap)
@pytest.mark.parametrize("Tk_cap", [1, 63, 64, 65, 600, 2000])
@pytest.mark.parametrize("dk,H", [(64, 1), (64, 4), (48, 1), (48, 4), (128, 1), (128, 4)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_decode_attn_matches_fp64_softmax_attention(K, dtype, dk, H, Tk_cap):
    """Tolerance: the kernel accumulates in fp32 (scores over dk products, the softmax sum and the weighted values over n keys, one
    lane per key / per output dimension, sequentially).  Error of such sums of round-to-nearest terms grows like sqrt(terms) u
    for these random inputs, and 16 sqrt(n + dk) u max|v| leaves 16x room for it, while one key missed or read twice moves the
    output by ~ max|v| / n (5e-4 of max|v| at n = 2000 against a bound of 4.3e-5 of it).  bf16 output: plus
    the rounding of the stored value, 2^-8 |o|.  Rows of length 0 give exactly 0; NaN past every length must never surface."""
    mid = max(1, Tk_cap // 2 + 1)
    cases = [("uniform", 0), ("uniform", 1), ("uniform", mid), ("uniform", Tk_cap + 3), ("uniform_kvdiv", Tk_cap),
             ("self", [0, 1, mid, Tk_cap, Tk_cap + 5, 2]), ("cross", [Tk_cap + 1, mid]), ("cross", [0, Tk_cap])]
    for i, (form, lens) in enumerate(cases):
        o, obuf, ref, n_row, v64 = _attn_case(K, dtype, dk, H, Tk_cap, form, lens, seed=1000 * dk + 10 * Tk_cap + i)
        got = o.double().cpu().numpy()
        what = f"{form} lens={lens}"
        assert np.isfinite(got).all(), what
        pad = obuf.cpu()
        assert (pad[:, :16] == 7).all() and (pad[:, 16 + H * dk:] == 7).all(), what + ": wrote outside its columns"
        fin = v64[np.isfinite(v64)]                      # every value NaN when every length is 0
        vmax = float(np.abs(fin).max()) if fin.size else 0.0
        for r, n in enumerate(n_row):
            if n <= 0:
                assert (bits(o[r]) == 0).all(), what + f": row {r} of length 0 is not exactly 0"
        tol = 16 * math.sqrt(max(n_row) + dk) * U32 * vmax + 2 * U32 * np.abs(ref)
        if dtype == torch.bfloat16:
            tol = 2 * tol + 1.01 * U16 * np.abs(ref)
        err = np.abs(got - ref)
        assert (err <= tol).all(), f"{what}: max err {err.max():.3e} (bound {tol.flat[err.argmax()]:.3e})"


def test_decode_attn_refuses_a_score_buffer_past_the_lds(K, AsrHipError):
    """Four waves keep Tk_cap fp32 scores each in the LDS: up to 160 KB (Tk_cap = 10240) runs, one more key is refused before any
    launch.  The buffers hold Tk_cap rows either way, so even a wrong launch stays inside them."""
    H, dk = 1, 64
    for Tk_cap, ok in ((10240, True), (10241, False)):
        g = torch.Generator().manual_seed(Tk_cap)
        q = torch.randn(4, dk, generator=g)
        kv = torch.randn(Tk_cap, 2 * dk, generator=g)
        o = torch.full((4, dk), 5.0, device=DEV)
        qd, kvd = q.to(DEV), kv.to(DEV)
        if ok:
            K.decode_attn(qd, kvd[:, :dk], kvd[:, dk:], H, dk, Tk_cap, kv_div=4, k_len_uniform=Tk_cap, o=o)
            ref = _attn_ref(q.double().numpy(), kv.double().numpy()[:, :dk], kv.double().numpy()[:, dk:], [Tk_cap] * 4, [0] * 4, H, dk,
                            Tk_cap, dk ** -0.5)
            tol = 16 * math.sqrt(Tk_cap + dk) * U32 * float(kv[:, dk:].abs().max()) + 2 * U32 * np.abs(ref)
            assert (np.abs(o.double().cpu().numpy() - ref) <= tol).all()
        else:
            with pytest.raises(AsrHipError, match="LDS"):
                K.decode_attn(qd, kvd[:, :dk], kvd[:, dk:], H, dk, Tk_cap, kv_div=4, k_len_uniform=Tk_cap, o=o)
            torch.cuda.synchronize()
            assert (o.cpu() == 5.0).all()


# ------------------------------------------------------------------------------------ logsoftmax_topk / ctc_frame_topk
def _topk_rows(V, dtype, seed):
    """Rows of V logits: plain normal, exact ties (small integers), many bf16 collisions, and mostly -inf (fewer finite entries
    than any beam > 2)."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randn(V, generator=g) * 3,
            torch.randint(0, 3, (V,), generator=g).float(),
            (3.0 + 0.01 * torch.randn(V, generator=g)).to(dtype).float(),       # in bf16 these collapse onto a few values
            torch.full((V,), float("-inf"))]
    rows[3][torch.randperm(V, generator=g)[:min(2, V)]] = torch.randn(min(2, V), generator=g)
    rows.append(torch.where(torch.rand(V, generator=g) < 0.5, torch.randn(V, generator=g), torch.tensor(float("-inf"))))
    rows[4][V // 2] = 1.0                                                       # at least one finite entry per row
    return torch.stack(rows).to(dtype)


def _topk_ref(x, k):
    """fp64 log_softmax of each row, the k largest entries by a stable descending sort (ties: ascending index)."""
    x = x.double().numpy()
    m = x.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    lp = x - lse
    ids = np.argsort(-x, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(lp, ids, axis=1), ids, lp, lse[:, 0], x


def _lp_tol(x_sel, lse, V):
    """fp32 bound of x - (m + log sum exp(x - m)): the sum of V positive terms carries <= (V + 2) u relative error (expf within
    an ulp or two per term), log adds an ulp of lse, the subtraction rounds once."""
    return 4 * U32 * (1 + np.abs(x_sel) + np.abs(lse)[:, None]) + (V + 4) * U32


@pytest.mark.parametrize("V", [1, 5, 63, 64, 65, 4232])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_logsoftmax_topk_matches_stable_sort(K, dtype, V):
    """ids exact; vals within the fp32 bound of _lp_tol; -inf entries stay -inf.  The rows sit ld = V + 3 apart with huge finite
    values in the padding columns, which would win every pick (and wreck the normaliser) if they were read."""
    x = _topk_rows(V, dtype, seed=V)
    ld = V + 3
    buf = torch.full((x.shape[0], ld), 3.0e38).to(dtype)
    buf[:, :V] = x
    xd = buf.to(DEV)[:, :V]
    for beam in sorted({1, min(4, V), min(V, 8)}):
        vals, ids = K.logsoftmax_topk(xd, beam)
        vr, ir, lp, lse, x64 = _topk_ref(x, beam)
        assert np.array_equal(ids.cpu().numpy(), ir), f"beam {beam}: ids {ids.cpu().numpy()} vs {ir}"
        got = vals.double().cpu().numpy()
        inf = np.isneginf(vr)
        assert np.array_equal(np.isneginf(got), inf), f"beam {beam}: -inf entries differ"
        tol = _lp_tol(np.take_along_axis(x64, ir, axis=1), lse, V)
        err = np.abs(got[~inf] - vr[~inf])
        assert (err <= tol[~inf]).all(), f"beam {beam}: max err {err.max():.3e}"


@pytest.mark.parametrize("V", [1, 5, 64, 65, 4232])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ctc_frame_topk_matches_stable_sort_and_blank(K, dtype, V):
    """The CTC form of the same kernel: top-k as above plus log_softmax of the blank class, at blank = 0 and V - 1."""
    x = _topk_rows(V, dtype, seed=V + 7)
    ld = V + 5
    buf = torch.full((x.shape[0], ld), 3.0e38).to(dtype)
    buf[:, :V] = x
    xd = buf.to(DEV)[:, :V]
    k = min(V, 8)
    for blank in sorted({0, V - 1}):
        vals, ids, blp = K.ctc_frame_topk(xd, k, blank)
        vr, ir, lp, lse, x64 = _topk_ref(x, k)
        assert np.array_equal(ids.cpu().numpy(), ir)
        got = vals.double().cpu().numpy()
        inf = np.isneginf(vr)
        assert np.array_equal(np.isneginf(got), inf)
        assert (np.abs(got[~inf] - vr[~inf]) <= _lp_tol(np.take_along_axis(x64, ir, axis=1), lse, V)[~inf]).all()
        b_got, b_ref = blp.double().cpu().numpy(), lp[:, blank]
        binf = np.isneginf(b_ref)
        assert np.array_equal(np.isneginf(b_got), binf), (b_got, b_ref)
        assert (np.abs(b_got[~binf] - b_ref[~binf]) <= _lp_tol(x64[:, blank:blank + 1], lse, V)[~binf, 0]).all(), (b_got, b_ref)


# ------------------------------------------------------------------------------------ beam_step
def _beam_inputs(rng, B, beam, scenario, step):
    V = 11
    eos = V - 1
    if scenario == "ties":
        vals = -rng.integers(0, 3, size=(B, beam, beam)).astype(np.float32)          # exact ties within and across hypotheses
    else:
        vals = np.log(rng.dirichlet(np.ones(V), size=(B, beam)))[..., :beam].astype(np.float32)
        vals[rng.random((B, beam, beam)) < 0.1] = -np.inf
    vals = -np.sort(-vals, axis=2)                                                    # as logsoftmax_topk delivers them
    ids = rng.integers(0, V, size=(B, beam, beam)).astype(np.int32)
    ids[rng.random((B, beam, beam)) < 0.25] = eos
    return vals, ids, eos


@pytest.mark.parametrize("scenario", ["random", "ties"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("beam", [1, 2, 5, 8])
def test_beam_step_matches_restatement(K, beam, B, scenario):
    """Nine consecutive steps from [sos] (only slot 0 alive at step 0), the kernel's state and the restatement's carried separately
    and compared exactly after every step: scores, alive flags, last tokens, parents, the records (dead slots -inf) and the survivor
    count added onto the caller's value.  Per-utterance maxlen 3 / 5 / 9: forced ends at step 2 and 4, then an utterance with no
    candidates.  beam 8 fills all 64 lanes."""
    rng = np.random.default_rng(100 * beam + 10 * B + (scenario == "ties"))
    steps = 9
    maxlen = np.array([3, 9, 5], np.int32) if B > 1 else np.array([5], np.int32)
    st = dict(score=np.zeros((B, beam), np.float32), alive=np.zeros((B, beam), np.int32), last_tok=np.full((B, beam), 1, np.int32))
    st["alive"][:, 0] = 1
    d = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in st.items()}
    d["parent"] = torch.full((B, beam), -3, dtype=torch.int32, device=DEV)
    rec = {k: torch.full((steps, B, beam), -5, dtype=torch.int32, device=DEV) for k in ("rec_tok", "rec_par", "rec_end")}
    rec["rec_score"] = torch.full((steps, B, beam), 123.0, device=DEV)
    maxlen_d = torch.from_numpy(maxlen).to(DEV)
    for step in range(steps):
        vals, ids, eos = _beam_inputs(rng, B, beam, scenario, step)
        total = torch.tensor([11], dtype=torch.int32, device=DEV)
        K.beam_step(torch.from_numpy(vals).to(DEV), torch.from_numpy(ids).to(DEV), d["score"], d["alive"], d["last_tok"], d["parent"],
                    rec["rec_tok"], rec["rec_par"], rec["rec_end"], rec["rec_score"], maxlen_d, total, B, beam, step, eos)
        want = BR.beam_step(vals, ids, st["score"], st["alive"], st["last_tok"], maxlen, step, eos)
        for k in ("score", "alive", "last_tok", "parent"):
            assert np.array_equal(bits(d[k]).numpy(), torch.from_numpy(want[k]).view(bits(d[k]).dtype).numpy()), (step, k, d[k], want[k])
        for k in ("rec_tok", "rec_par", "rec_end", "rec_score"):
            got = rec[k][step]
            assert np.array_equal(bits(got).numpy(), torch.from_numpy(want[k]).view(bits(got).dtype).numpy()), (step, k, got, want[k])
        later = rec["rec_score"][step + 1:]
        assert bool((later == 123.0).all()), f"step {step} wrote records of later steps"
        assert int(total) == 11 + want["n_alive"], (step, int(total), want["n_alive"])
        st = {k: want[k] for k in ("score", "alive", "last_tok")}
    assert int(d["alive"].sum()) == 0          # every utterance was forced to end (maxlen <= 9 steps)


# ------------------------------------------------------------------------------------ cache_gather
@pytest.mark.parametrize("dtype,row_elems", [(torch.bfloat16, 16), (torch.bfloat16, 256), (torch.float32, 12), (torch.float32, 4)])
@pytest.mark.parametrize("L", [1, 6])
def test_cache_gather_matches_index_arithmetic(K, dtype, row_elems, L):
    """dst[l, r, t] = src[l, (r // beam) * beam + parent[r], t] bit for bit for t < n_pos; positions t >= n_pos keep the sentinel.
    Row bytes 32 / 512 / 48 / 16: one to 32 16-byte pieces."""
    B, beam, Lcap = 3, 4, 9
    R = B * beam
    g = torch.Generator().manual_seed(L * row_elems)
    src = torch.randn(L, R, Lcap, row_elems, generator=g).to(dtype).to(DEV)
    row_bytes = row_elems * src.element_size()
    parents = [torch.arange(beam).repeat(B), torch.zeros(R, dtype=torch.long), torch.randint(0, beam, (R,), generator=g),
               torch.tensor([3, 3, 0, 1] * B)]
    for par in parents:
        par = par.to(torch.int32)
        for n_pos in (0, 1, Lcap):
            dst = torch.full_like(src, -2.5)
            K.cache_gather(src, dst, par.to(DEV), L, R, beam, Lcap, n_pos, row_bytes)
            src_rows = (torch.arange(R) // beam) * beam + par.long()
            want = torch.full_like(src, -2.5).cpu()
            want[:, :, :n_pos] = src.cpu()[:, src_rows, :n_pos]
            assert torch.equal(bits(dst), bits(want)), (par.tolist(), n_pos)


def test_cache_gather_refusals(K, AsrHipError):
    """Rows not a multiple of 16 bytes, a misaligned pointer, n_pos > Lcap, R not a multiple of beam: refused, nothing written.
    The buffers hold 64 spare elements, so even a wrong launch stays inside them."""
    L, R, beam, Lcap, row = 2, 8, 4, 5, 16
    flat = torch.randn(L * R * Lcap * row + 64, device=DEV)
    dst_flat = torch.full_like(flat, 9.0)
    par = torch.zeros(R, dtype=torch.int32, device=DEV)
    src, dst = flat[:L * R * Lcap * row], dst_flat[:L * R * Lcap * row]
    bad = [(src, dst, L, R, beam, Lcap, 2, 24, "bad shape"),                     # 24-byte rows
           (flat[1:1 + src.numel()], dst, L, R, beam, Lcap, 2, 64, "misaligned"),
           (src, dst_flat[2:2 + src.numel()], L, R, beam, Lcap, 2, 64, "misaligned"),
           (src, dst, L, R, beam, Lcap, Lcap + 1, 64, "bad shape"),
           (src, dst, L, 6, beam, Lcap, 2, 64, "bad shape")]                      # R = 6, beam = 4
    for s, d_, L_, R_, beam_, Lcap_, n_pos, rb, msg in bad:
        with pytest.raises(AsrHipError, match=msg):
            K.cache_gather(s, d_, par, L_, R_, beam_, Lcap_, n_pos, rb)
    torch.cuda.synchronize()
    assert (dst_flat == 9.0).all()


# ------------------------------------------------------------------------------------ rows_gather / rows_scatter_add
def _rows(shape, dtype, offset, seed, fill=None):
    """A contiguous (rows, d) tensor; offset = 1 puts it one element past an aligned allocation (the kernels' scalar path)."""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n + offset, generator=g) if fill is None else torch.full((n + offset,), float(fill))
    return base.to(dtype).to(DEV)[offset:].view(*shape)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("d", [512, 6, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_gather_and_scatter_add_match_index_arithmetic(K, dtype, d, offset):
    """gather: out[b Tk + t] = src[b T + t] for t < Tk, exact.  scatter-add: rows t < Tk of dst become the dtype's rounding of
    float(dst) + float(src) (one fp32 add, one rounding: computed once here and compared exactly), rows t >= Tk bit-identical.
    d = 512 / 4 aligned take the 4-wide path; d = 6 and every offset-1 view the scalar one."""
    T = 37
    for B in (0, 1, 7):
        for Tk in sorted({0, 1, 16, T}):
            seed = 1000 * B + Tk + d
            src = _rows((B * T, d), dtype, offset, seed)
            out = _rows((B * Tk, d), dtype, offset, seed + 1, fill=-7.0)
            K.rows_gather(src, B, T, Tk, out=out)
            want = src.cpu().view(B, T, d)[:, :Tk].reshape(B * Tk, d)
            assert torch.equal(bits(out), bits(want)), (B, Tk)
            g_c = _rows((B * Tk, d), dtype, offset, seed + 2)
            dst = _rows((B * T, d), dtype, offset, seed + 3)
            before = dst.cpu()
            want = before.clone().view(B, T, d)
            want[:, :Tk] = (want[:, :Tk].float() + g_c.cpu().float().view(B, Tk, d)).to(dtype)
            K.rows_scatter_add(g_c, dst, B, T, Tk)
            assert torch.equal(bits(dst), bits(want.reshape(B * T, d))), (B, Tk)


def test_rows_compact_refuses_more_key_rows_than_frames(K, AsrHipError):
    """T < Tk is refused by the C entry points (and by the wrappers' asserts): nothing is launched or written.  The buffers hold Tk
    rows per utterance, so even a wrong launch stays inside them."""
    from asr_chinese_e2e_amd import _lib
    B, T, Tk, d = 2, 5, 8, 4
    src = torch.randn(B * Tk, d, device=DEV)
    dst = torch.full((B * Tk, d), 3.0, device=DEV)
    for fn in (_lib.lib.asr_rows_gather, _lib.lib.asr_rows_scatter_add):
        rc = fn(src.data_ptr(), dst.data_ptr(), B, T, Tk, d, _lib.ASR_F32, None)
        assert rc == -1 and "bad shape" in _lib.last_error(), (rc, _lib.last_error())
    with pytest.raises(AssertionError):
        K.rows_gather(src[:B * T], B, T, Tk)
    with pytest.raises(AssertionError):
        K.rows_scatter_add(src, dst[:B * T], B, T, Tk)
    torch.cuda.synchronize()
    assert (dst == 3.0).all()


# ------------------------------------------------------------------------------------ grad_sumsq_noam
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4 * 2 ** 20 + 3])
@pytest.mark.parametrize("sched", ["noam", "const"])
def test_grad_sumsq_noam_matches_the_two_kernel_route(K, n, sched):
    """asr_grad_sumsq_noam = asr_grad_sumsq then asr_noam_hyper: three steps on each route from the same state (crossing the end of
    the warmup for the Noam schedule; warmup = 0 is the constant rate lr_const).  sumsq: within the fp32 summation bound of the fp64
    sum - each of the <= 1024 x 256 threads adds ceil(n / 262144) vectors of 4 squares, then two 256-wide tree sums and a 1024-long
    one: (4 ceil(n / 262144) + 40) u relative - and bit-identical to the unfused route (same partial and finalizer order).  step and
    hyper: bit-identical, advanced once per call."""
    from asr_chinese_e2e_amd.kernels import Workspace
    ws1, ws2 = Workspace(DEV), Workspace(DEV)
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.5
    gd = g.to(DEV)
    want = float((g.double() ** 2).sum())
    tol = (4 * math.ceil(n / 262144) + 40) * U32 * want
    warmup, lr_const = (4000.0, 0.0) if sched == "noam" else (0.0, 3e-4)
    step0 = 3998 if sched == "noam" else 6
    s1, s2 = (torch.tensor([step0], dtype=torch.int32, device=DEV) for _ in range(2))
    h1, h2 = (torch.full((4,), -1.0, device=DEV) for _ in range(2))
    o1, o2 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    for it in range(1, 4):
        K.grad_sumsq_noam(gd, o1, ws1, s1, h1, 512, warmup, 1.0, lr_const, 0.9, 0.98)
        K.grad_sumsq(gd, o2, ws2)
        K.noam_hyper(s2, h2, 512, warmup, 1.0, lr_const, 0.9, 0.98)
        assert abs(float(o1) - want) <= tol, (float(o1), want, tol)
        assert torch.equal(bits(o1), bits(o2))
        assert int(s1) == step0 + it and torch.equal(s1, s2)
        assert torch.equal(bits(h1), bits(h2)), (h1, h2)
        s = step0 + it
        lr = (512 ** -0.5) * min(s ** -0.5, s * warmup ** -1.5) if warmup > 0 else lr_const
        assert abs(float(h1[0]) - lr) <= 1e-6 * lr and float(h1[3]) == s
