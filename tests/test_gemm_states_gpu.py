"""The bf16 NT GEMM (gemm_nt_spec_kernel, gemm_nt_kernel) and the weight-gradient GEMMs (gemm_tn_dma_kernel<2|3>, gemm_tn_multi_kernel,
gemm_tn_grouped_kernel, tn_slab_reduce_kernel) at the ring, split and edge states listed in tests/gemm_cases.py, on integer operands whose
results are exact: every output must equal the int64 product bit for bit, and every element around the output must keep its sentinel.
Operands are views into buffers whose surroundings hold NaN, so one read past K, N or M shows.  tests/test_gemm_states_cpu.py proves
which state each case reaches (the state lists assume the 256 CUs of an MI355X for cu_limit = 0) and that the checker sees a defect.

One random-data case per kernel route goes against the fp64 product of the bf16-rounded operands with the tolerances of
tests/test_kernels_gpu.py::test_gemm_nt and ::test_gemm_tn; the integer data has no rounding in the accumulate path to exercise."""
import math

import pytest
import torch

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def ws(K):
    return K.Workspace(DEV)


@pytest.fixture(scope="module")
def nt_data():
    return G.NtData(DEV)


@pytest.fixture(scope="module")
def tn_data():
    return G.TnData(DEV)


class cu_limit:
    """The process-wide option "cu_limit" for the duration of a block; always back to 0 (the whole device)"""

    def __init__(self, K, n):
        self.K, self.n = K, n

    def __enter__(self):
        self.K.set_cu_limit(self.n)

    def __exit__(self, *exc):
        self.K.set_cu_limit(0)


def _describe(c):
    tail = ("mask" if c.act == G.ACT_RELU_MASK else ("relu " if c.act else "") + ("bias " if c.bias else "") + (c.res or "")).strip() or "plain"
    return f"gemm_nt [{c.table}] {c.M}x{c.N}x{c.K} {tail} cu_limit={c.limit} ldc={c.ldc} c_off={c.c_off}"


def _run_nt_cases(K, data, cases):
    for c in cases:
        a, w, bias, res, out, (cbuf, init, off) = data.operands(c)
        ref = data.reference(c)
        with cu_limit(K, c.limit):
            K.gemm_nt(a, w, bias, out, c.act, res)
        G.check_exact(cbuf, init, ref, c.M, c.N, off, what=_describe(c))


# ------------------------------------------------------------------------------------------------------------------ NT
@pytest.mark.parametrize("limit", G.NT_RING_LIMITS)
def test_nt_ring_across_tile_boundaries(K, nt_data, limit):
    """1 .. 3 tiles per workgroup x 2, 3, 4, 5, 7 k-steps and a ragged last one: every phase of the 3-slot ring at a tile boundary, the
    mask / residual prefetch step on a second and third tile, XCD shares of zero and of 3,3,3,3,2,2,2,2, grids of 8, 9 and 16"""
    _run_nt_cases(K, nt_data, [c for c in G.nt_ring_cases() if c.limit == limit])


def test_nt_edges(K, nt_data):
    """M = 1, 8, 255, 256, 257 x N = 8, 120, 128, 136, 264, every store tail, padded lda / ldb / ldc: clamped rows, the bias prologue at
    N = 8, a last tile of 8 columns, the unpredicated and the predicated store tail"""
    _run_nt_cases(K, nt_data, G.nt_edge_cases())


def test_nt_dispatch_ladder(K, nt_data):
    """One exact case per branch of asr_gemm_nt_bf16, the all-in-one kernel for each of its reasons (its scalar store tail included)"""
    _run_nt_cases(K, nt_data, G.nt_ladder_cases())


def _close(got, ref, rtol, atol, what):
    err = (got.double().cpu() - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})"


@pytest.mark.parametrize("mode,K_,limit", [("bias", 192, 8), ("relu_bias", 256, 8), ("mask", 128, 16), ("res", 320, 8), ("bias", 200, 16),
                                            ("relu_bias_res", 200, 0)])
def test_nt_random_data_per_route(K, mode, K_, limit):
    """Random normal operands (rounding in the accumulate path) on each route - persistent plain, ReLU, mask, residual, ragged, and the
    all-in-one kernel - against the fp64 product of the bf16-rounded operands; tolerance of test_gemm_nt.  Nine tiles per column on 8 or
    16 CUs, two tile columns, the second of 8."""
    M, N = 256 * 9 - 37, 136
    c = G._nt("random", M, N, K_, mode, limit)
    g = torch.Generator().manual_seed(K_ + limit)
    a = torch.randn(M, K_, generator=g).bfloat16()
    w = (torch.randn(N, K_, generator=g) * 0.1).bfloat16()
    bias = torch.randn(N, generator=g) if c.bias else None
    res = torch.randn(M, N, generator=g).bfloat16() if c.res else None
    ref = a.double() @ w.double().t()
    if c.act == G.ACT_RELU_MASK:
        ref = torch.where(res.double() > 0, ref, torch.zeros_like(ref))
    else:
        if c.bias:
            ref = ref + bias.double()
        if c.act == G.ACT_RELU:
            ref = torch.relu(ref)
        if c.res:
            ref = ref + res.double()
    nan = float("nan")
    abuf = torch.full((M + 1, K_ + G.PAD), nan, dtype=torch.bfloat16, device=DEV)
    wbuf = torch.full((N + 1, K_ + G.PAD), nan, dtype=torch.bfloat16, device=DEV)
    abuf[:M, :K_], wbuf[:N, :K_] = a.to(DEV), w.to(DEV)
    cbuf = torch.full((M + 1, N + G.PAD), G.SENTINEL_BF16, dtype=torch.bfloat16, device=DEV)
    init = cbuf.clone()
    rbuf = None
    if c.res:
        rbuf = torch.full((M + 1, N + G.PAD), nan, dtype=torch.bfloat16, device=DEV)
        rbuf[:M, :N] = res.to(DEV)
    with cu_limit(K, limit):
        K.gemm_nt(abuf[:M, :K_], wbuf[:N, :K_], None if bias is None else bias.to(DEV), cbuf[:M, :N], c.act, None if rbuf is None else rbuf[:M, :N])
    _close(cbuf[:M, :N], ref, rtol=1e-2, atol=1e-2, what=_describe(c))
    assert torch.equal(cbuf[M:].view(torch.int16), init[M:].view(torch.int16)) and torch.equal(cbuf[:M, N:].contiguous().view(torch.int16), init[:M, N:].contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------ TN
def _run_tn(K, data, M, N, K_, accumulate, with_dbias, ws=None):
    """One launch on fresh poisoned buffers; returns the whole dW and dbias buffers after checking them against the int64 reference"""
    dy, x, dw, dbias, wbuf, winit, bbuf, binit = data.operands(M, N, K_, accumulate, with_dbias)
    ref_w, ref_b = data.reference(M, N, K_, accumulate)
    K.gemm_tn(dy, x, dw, accumulate=accumulate, dbias=dbias, ws=ws)
    what = f"gemm_tn {M}x{N}x{K_} accumulate={accumulate} dbias={with_dbias} deterministic={K.deterministic()}"
    G.check_exact(wbuf, winit, ref_w, N, K_, what=what)
    if with_dbias:
        G.check_exact(bbuf, binit, ref_b.unsqueeze(0), 1, N, what=what + " (bias gradient)")
    return wbuf, bbuf


@pytest.mark.parametrize("limit", G.TN_LIMITS)
def test_tn_stages_splits_and_tails(K, ws, tn_data, limit):
    """Stages within one split (a prologue shorter than, as long as and longer than the ring, both ring depths), two and more splits,
    staggered or declined, a last split shorter than one stage, N / K of one 8-group and one 8-group past a tile; padded ldy / ldx / ldw,
    with and without the bias gradient, accumulating and overwriting: dW and dbias equal the int64 product, nothing around them is written"""
    with cu_limit(K, limit):
        for M, N, K_ in G.tn_shapes():
            for accumulate in (True, False):
                for with_dbias in (True, False):
                    _run_tn(K, tn_data, M, N, K_, accumulate, with_dbias, ws)


@pytest.mark.parametrize("limit", G.TN_LIMITS)
def test_tn_deterministic_mode_equals_atomic_mode(K, ws, tn_data, deterministic_mode, limit):
    """The same table through the slab mode (tn_slab_reduce_kernel): equal to the int64 product, hence to the atomic mode - compared
    directly as well, buffer against buffer"""
    assert K.deterministic()
    with cu_limit(K, limit):
        for M, N, K_ in G.tn_shapes():
            for accumulate, with_dbias in ((True, True), (True, False), (False, True), (False, False)):
                det = _run_tn(K, tn_data, M, N, K_, accumulate, with_dbias, ws)
                K.set_deterministic(False)
                try:
                    atomic = _run_tn(K, tn_data, M, N, K_, accumulate, with_dbias, ws)
                finally:
                    K.set_deterministic(True)
                for d, a in zip(det, atomic):
                    assert (d is None and a is None) or torch.equal(d.view(torch.int32), a.view(torch.int32)), f"{M}x{N}x{K_}: slab and atomic mode differ"


def _group(data, group, accumulate):
    probs, checks = [], []
    for M, N, K_, with_dbias in group:
        dy, x, dw, dbias, wbuf, winit, bbuf, binit = data.operands(M, N, K_, accumulate, with_dbias)
        probs.append((dy, x, dw, dbias))
        checks.append((M, N, K_, wbuf, winit, bbuf, binit))
    return probs, checks


@pytest.mark.parametrize("limit", G.TN_LIMITS)
@pytest.mark.parametrize("name", sorted(G.TN_GROUPS))
def test_tn_grouped_and_multi_launch(K, tn_data, name, limit):
    """Groups that qualify for the multi launch (same M >= 4096; with the option "tn_multi" off they take the grouped kernel) and one
    that does not: every dW and dbias equals the int64 product - so the two kernels agree bit for bit - and nothing else is written"""
    group = G.TN_GROUPS[name]
    if K.deterministic():      # deterministic for the whole run: the grouped entry point (fp32 atomics only) must refuse
        with pytest.raises(RuntimeError):
            K.gemm_tn_grouped(_group(tn_data, group, True)[0], accumulate=True)
        return
    for multi in (1, 0):
        for accumulate in (True, False):
            probs, checks = _group(tn_data, group, accumulate)
            prev = K.set_option("tn_multi", multi)
            try:
                with cu_limit(K, limit):
                    K.gemm_tn_grouped(probs, accumulate=accumulate)
            finally:
                K.set_option("tn_multi", prev)
            for M, N, K_, wbuf, winit, bbuf, binit in checks:
                what = f"gemm_tn_grouped [{name}] {M}x{N}x{K_} accumulate={accumulate} tn_multi={multi} cu_limit={limit}"
                ref_w, ref_b = tn_data.reference(M, N, K_, accumulate)
                G.check_exact(wbuf, winit, ref_w, N, K_, what=what)
                if bbuf is not None:
                    G.check_exact(bbuf, binit, ref_b.unsqueeze(0), 1, N, what=what + " (bias gradient)")


def _tn_random(M, N, K_, seed):
    g = torch.Generator().manual_seed(seed)
    dy = (torch.randn(M, N, generator=g) * 0.5).bfloat16()
    x = torch.randn(M, K_, generator=g).bfloat16()
    nan = float("nan")
    ybuf = torch.full((M + 1, N + G.PAD), nan, dtype=torch.bfloat16, device=DEV)
    xbuf = torch.full((M + 1, K_ + G.PAD), nan, dtype=torch.bfloat16, device=DEV)
    ybuf[:M, :N], xbuf[:M, :K_] = dy.to(DEV), x.to(DEV)
    wbuf = torch.full((N + 1, K_ + G.PAD), G.SENTINEL_F32, device=DEV)
    wbuf[:N, :K_] = 1.0
    db = torch.full((N,), 2.0, device=DEV)
    return ybuf[:M, :N], xbuf[:M, :K_], wbuf, db, dy.double().t() @ x.double(), dy.double().sum(0)


def _tn_random_check(M, N, K_, wbuf, db, ref, ref_b, what):
    _close(wbuf[:N, :K_] - 1, ref, rtol=2e-3, atol=2e-3 * math.sqrt(M), what=what)
    _close(db - 2, ref_b, rtol=1e-4, atol=1e-3 * math.sqrt(M), what=what + " bias gradient")
    assert bool((wbuf[N:] == G.SENTINEL_F32).all()) and bool((wbuf[:, K_:] == G.SENTINEL_F32).all()), what + ": wrote outside dW"


@pytest.mark.parametrize("route,M,N,K_,limit", [("ring 3, staggered splits", 1600, 256, 128, 8), ("ring 2", 1400, 384, 128, 8),
                                                 ("ring 3, 13 splits", 3100, 136, 72, 0), ("slabs", 1600, 256, 128, 8)])
def test_tn_random_data_per_route(K, ws, route, M, N, K_, limit):
    """Random normal operands on each route of the single-problem launch against the fp64 product of the bf16-rounded operands;
    tolerances of test_gemm_tn"""
    dy, x, wbuf, db, ref, ref_b = _tn_random(M, N, K_, M + K_)
    old = K.set_deterministic(True) if route == "slabs" else None
    try:
        with cu_limit(K, limit):
            K.gemm_tn(dy, x, wbuf[:N, :K_], accumulate=True, dbias=db, ws=ws)
    finally:
        if old is not None:
            K.set_deterministic(old)
    _tn_random_check(M, N, K_, wbuf, db, ref, ref_b, f"gemm_tn {route} {M}x{N}x{K_}")


@pytest.mark.parametrize("name,limit", [("multi", 0), ("multi_staggered", 8), ("grouped", 0)])
def test_tn_grouped_random_data_per_route(K, name, limit):
    """The multi launch and the grouped kernel on random normal operands; tolerances of test_gemm_tn"""
    built = [_tn_random(M, N, K_, 7 * i + M) for i, (M, N, K_, _) in enumerate(G.TN_GROUPS[name])]
    if K.deterministic():      # deterministic for the whole run: the grouped entry point must refuse
        with pytest.raises(RuntimeError):
            K.gemm_tn_grouped([(b[0], b[1], b[2][:N, :K_], b[3]) for b, (M, N, K_, _) in zip(built, G.TN_GROUPS[name])], accumulate=True)
        return
    with cu_limit(K, limit):
        K.gemm_tn_grouped([(dy, x, wbuf[:N, :K_], db) for (dy, x, wbuf, db, _, _), (M, N, K_, _) in zip(built, G.TN_GROUPS[name])], accumulate=True)
    for (dy, x, wbuf, db, ref, ref_b), (M, N, K_, _) in zip(built, G.TN_GROUPS[name]):
        _tn_random_check(M, N, K_, wbuf, db, ref, ref_b, f"gemm_tn_grouped [{name}] {M}x{N}x{K_}")
