"""The row-wise kernels past their single-trip states: csrc/ln.hip (add_ln_fwd / add_ln_bwd and their reductions) and csrc/misc.hip (column
sums, ReLU backward, ReLU, cast, Adam, the embedding pair, dropout_mask) at the sizes where their hand tuning engages - grid caps with
grid-stride loops, two rows in flight per wave, the four-row unrolled column sums, vector bodies with scalar tails - each against an fp64
reference on the CPU computed from the operands after they were rounded to the storage type (tests/test_kernels_gpu.py's header).
Needs a real MI355X: run with `-m gpu`.

tests/rowwise_ref.py holds the references, the kernels' launch arithmetic restated (so each docstring below can say which loop state its
shape reaches; tests/test_rowwise_ref_cpu.py asserts that arithmetic) and the summation bounds: a column sum over fp32 terms is held to

    gamma(A + c) * sum_rows |term|,   gamma(n) = n u / (1 - n u),  u = 2^-24,

A = the adds on the longest path from a term to the result, counted from the kernel code (rowwise_ref.ln_bwd_sum_adds, colsum_adds), c = the
fp32 roundings that formed the term, sum|term| from the fp64 reference.  No bound here was fitted to what the GPU returns; the negative
controls of tests/test_rowwise_ref_cpu.py show that a row taken from its neighbour, a dropped last row and a clipped gradient written back
leave these gates by factors of 13 to 1.8e5.  Measured on an MI355X (largest error / tolerance over all cases of a gate; every test prints
its own figures, `pytest -rP`): LayerNorm y / xhat 0.21, dz / dx 0.10, rstd 0.007, dbeta 0.035, dgamma 0.056, dbias 0.15; column sums and ReLU
backward's dbias 0.011; large-mean rows xhat 0.070 (fp32, the emulation's own figure) / 0.19 (bf16), rstd 0.004; embedding forward 0.15,
backward 0.997 (one addend: a single correctly rounded product may use all of u |addend|); no kernel defect was found.

Three branches of the reductions cannot be reached by any call, because ln_grid() caps the partial count at 512 and cs_row_slots() at 256;
nothing here (or anywhere) covers them, and this file leaves them as they are:
  * colsum_finalize_kernel's `gridDim.y > 1` / atomicAdd branch: asr_add_ln_bwd asks for P >= 1024 partial rows, colsum_impl for
    slots >= 1024;
  * ln_reduce_batched_kernel's `ns > 1` split (P >= 1024) and its atomicAdd.
Noted and left alone as well: the dropout counters `(uint32_t)row * (uint32_t)d` wrap at 2^32 elements, far past any size the model reaches.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_model as R  # noqa: E402
from tests import dropout_ref as D  # noqa: E402
from tests import rowwise_ref as W  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: dict(rtol=2e-5, atol=2e-5), BF16: dict(rtol=1.6e-2, atol=1e-2)}      # test_add_ln: forward outputs
GT = {F32: dict(rtol=2e-4, atol=2e-4), BF16: dict(rtol=3e-2, atol=6e-2)}         # test_add_ln: per-element gradients


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def ws(K):
    return K.Workspace(DEV)


def _record(name, **row):
    """The measured figures as one JSON line (shown by `pytest -rP`), printed before the assertion they belong to."""
    print("rowwise_states " + json.dumps({"test": name, **row}))


def close(a, b, rtol, atol, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    _record(what, max_err=float(err.max()), max_err_over_tol=float((err / tol).max()))
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})"


def within(got, ref, tol, what):
    """|got - ref| <= tol element-wise, tol a tensor derived on the reference side (0 where the result must be exact)."""
    err = (got.detach().double().cpu() - ref).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    ratio = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    _record(what, max_err=float(err.max()), max_err_over_tol=float(ratio.max()))
    bad = err > tol
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} outside the bound, worst err / tol {float(ratio.max()):.3e}"


def bits(t):
    """Integer view of a tensor's storage: bit-for-bit comparison, NaN / -0.0 included."""
    t = t.detach().contiguous().cpu()
    return t.view({F32: torch.int32, BF16: torch.int16}.get(t.dtype, t.dtype))


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


SENT = 64


def guarded(data, sentinel):
    """data (flat or 2-D, CPU) copied to the front of a device allocation with SENT sentinel elements behind it: (view shaped like data,
    whole buffer)."""
    flat = data.reshape(-1)
    buf = torch.full((flat.numel() + SENT,), sentinel, dtype=data.dtype)
    buf[:flat.numel()] = flat
    buf = buf.to(DEV)
    return buf[:flat.numel()].view(data.shape), buf


def untouched(buf, n, sentinel):
    tail = buf[n:].cpu()
    return tail.numel() == SENT and same_bits(tail, torch.full((SENT,), sentinel, dtype=buf.dtype))


# ------------------------------------------------------------------------------------------------ 1. LayerNorm, several rows per wave
def _ln_inputs(seed, rows, d, T, dtype, use_res, use_pe, use_dy2):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(rows, d).to(dtype)
    res = rn(rows, d).to(dtype) if use_res else None
    gamma, beta = 1 + 0.2 * rn(d), 0.1 * rn(d)
    dy = rn(rows, d).to(dtype)
    dy2 = rn(rows, d).to(dtype) if use_dy2 else None
    pe = R.positional_encoding(T, d) if use_pe else None
    return dict(x=x, res=res, gamma_=gamma, beta=beta, pe=pe, dy=dy, dy2=dy2)


def _dev(t):
    return None if t is None else t.to(DEV)


def _ln_run(K, ws, inp, lens, B, T, mode=0, p=0.0, seed=0):
    """Forward and backward on the GPU -> dict of outputs (parameter gradients accumulated onto zeros) and the device operands."""
    dv = {k: _dev(v) for k, v in inp.items()}
    dv["lens"] = _dev(lens)
    d = inp["x"].shape[1]
    y, xhat, rstd = K.add_ln_fwd(dv["x"], dv["res"], dv["gamma_"], dv["beta"], dv["pe"], dv["lens"], B, T, drop_p=p, drop_seed=seed, drop_mode=mode)
    dgamma, dbeta, dbias = (torch.zeros(d, device=DEV) for _ in range(3))
    dz, dx = K.add_ln_bwd(dv["dy"], dv["dy2"], xhat, rstd, dv["gamma_"], dv["lens"], dgamma, dbeta, dbias, B, T, ws, drop_p=p, drop_seed=seed, drop_mode=mode)
    return dict(y=y, xhat=xhat, rstd=rstd, dz=dz, dx=dx, dgamma=dgamma, dbeta=dbeta, dbias=dbias), dv


def _ln_compare(out, ref, rows, dtype, mode, tag):
    """The gates of section 1.  Per element: y, xhat (test_add_ln's forward tolerance), rstd (fp32 whatever the storage: 2e-5 relative),
    dz and dx (test_add_ln's gradient tolerance).  Column sums over the live rows, A = ln_bwd_sum_adds(rows):
      dbeta   gamma(A + 2) sum|gy|            terms dy + dy2 (* dropout scale): two roundings
      dgamma  gamma(A + 3) sum|gy xhat|       against the fp64 sum over the xhat the kernel STORED (its operand, rounded to the storage type);
              against the autograd sum the same bound plus sum|gy| * (the per-element tolerance of xhat), which is what the xhat gate implies
      dbias   gamma(A + 40) sum(pieces of dx) (+ test_add_ln's per-element gradient tolerance, once, in bf16); rowwise_ref.ln_param_tolerances"""
    close(out["y"], ref["y"], **TOL[dtype], what=f"{tag} y")
    close(out["xhat"], ref["xhat"], **TOL[dtype], what=f"{tag} xhat")
    close(out["rstd"], ref["rstd"], rtol=2e-5, atol=0.0, what=f"{tag} rstd")
    close(out["dz"], ref["dz"], **GT[dtype], what=f"{tag} dz")
    if mode == 1:
        close(out["dx"], ref["dx"], **GT[dtype], what=f"{tag} dx")
    else:
        assert out["dx"] is out["dz"]
    tol = W.ln_param_tolerances(ref, rows, None if dtype == F32 else (GT[dtype]["rtol"], GT[dtype]["atol"]))
    within(out["dbeta"], ref["dbeta"], tol["dbeta"], f"{tag} dbeta")
    xs = out["xhat"].double().cpu()
    within(out["dgamma"], (ref["gy"] * xs).sum(0), W.gamma(W.ln_bwd_sum_adds(rows) + W.LN_TERM_GAMMA) * (ref["gy"] * xs).abs().sum(0), f"{tag} dgamma (stored xhat)")
    implied = (ref["gy"].abs() * (TOL[dtype]["rtol"] * ref["xhat"].abs() + TOL[dtype]["atol"])).sum(0)
    within(out["dgamma"], ref["dgamma"], tol["dgamma"] + implied, f"{tag} dgamma (autograd)")
    within(out["dbias"], ref["dbias"], tol["dbias"], f"{tag} dbias")


def _ln_row_locality(K, ws, out, dv, lens, B, T):
    """Every output row depends on its own input row only: y, xhat, rstd, dz of the big launch equal, bit for bit, the same rows computed by
    launches of one utterance slice of at most 2048 rows each (one row per wave and trip there: ln_states(1370, 512) has no live second
    row and one trip), with the slice's own length and its own rows of the positional table."""
    d = dv["x"].shape[1]
    nsl = W.ceil_div(T, 2048)
    chunk = W.ceil_div(T, nsl)
    for b in range(B):
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            assert n <= 2048
            r0 = b * T + t0
            sl = lambda t: None if t is None else t[r0:r0 + n]
            ls = None if lens is None else torch.tensor([min(max(int(lens[b]) - t0, 0), n)], dtype=torch.int32, device=DEV)
            pe = None if dv["pe"] is None else dv["pe"][t0:t0 + n]
            y, xhat, rstd = K.add_ln_fwd(sl(dv["x"]), sl(dv["res"]), dv["gamma_"], dv["beta"], pe, ls, 1, n)
            for name, got in (("y", y), ("xhat", xhat), ("rstd", rstd)):
                assert same_bits(got, out[name][r0:r0 + n]), f"row locality: {name} of utterance {b}, rows {t0}..{t0 + n}"
            g3 = [torch.zeros(d, device=DEV) for _ in range(3)]
            dz, _ = K.add_ln_bwd(sl(dv["dy"]), sl(dv["dy2"]), sl(out["xhat"]), sl(out["rstd"]), dv["gamma_"], ls, g3[0], g3[1], g3[2], 1, n, ws)
            assert same_bits(dz, out["dz"][r0:r0 + n]), f"row locality: dz of utterance {b}, rows {t0}..{t0 + n}"


def _ln_garbage_in_padded_rows(K, ws, out, dv, lens, B, T):
    """NaN in every padded row (t >= lens[b]) of dy, dy2, xhat and rstd: dz of those rows is exactly +0, every live row and the three
    parameter gradients keep their bits (the backward kernel loads row 0 in place of a padded row - itself NaN when lens[0] = 0 - and must
    use nothing of it)."""
    d = dv["x"].shape[1]
    pad = (W.keep_rows(lens, B, T).reshape(-1) == 0).to(DEV)
    assert int(pad.sum()) > 0
    nan = float("nan")
    poison = lambda t: None if t is None else torch.where(pad.view(-1, *([1] * (t.dim() - 1))), torch.full_like(t, nan), t)
    g3 = [torch.zeros(d, device=DEV) for _ in range(3)]
    dz, _ = K.add_ln_bwd(poison(dv["dy"]), poison(dv["dy2"]), poison(out["xhat"]), poison(out["rstd"]), dv["gamma_"], dv["lens"], g3[0], g3[1], g3[2], B, T, ws)
    assert int(bits(dz[pad]).abs().max()) == 0, "dz of a padded row is not +0"
    assert same_bits(dz[~pad], out["dz"][~pad]), "garbage in padded rows reached a live row of dz"
    for got, name in zip(g3, ("dgamma", "dbeta", "dbias")):
        assert same_bits(got, out[name]), f"garbage in padded rows reached {name}"


BIG_B, BIG_T, BIG_D = 3, 2740, 512
BIG_VARIANTS = {
    # name: (use_res, use_pe, use_dy2, lens)
    "res_pe_dy2": (True, True, True, [2740, 1371, 0]),
    "plain": (False, False, False, [2740, 1371, 0]),
    "row0_padded": (True, False, True, [0, 2740, 1371]),
}


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("variant", list(BIG_VARIANTS))
def test_add_ln_two_rows_per_wave_and_a_second_trip(K, ws, dtype, variant):
    """B = 3, T = 2740, d = 512: 8220 rows.  Forward: ln_grid_fwd = min(2055, 1024) workgroups of 4 waves, stride 4096, two rows per wave and
    trip -> trip 1 takes rows 0..8191 (row0 < 4096 and row0 + 4096: all 4096 second rows live), trip 2 rows 8192..8219, whose 28 second-row
    slots lie past the end and re-read row 8219.  Backward: ln_grid = 512, stride 2048 -> trips at row0 in [0, 2048), [4096, 6144),
    [8192, 8220), the last with 28 dead second rows that load row 0.  lens = [2740, 1371, 0]: an utterance that ends inside a trip (row 4111)
    and an empty one; "row0_padded" puts the empty utterance first, so that row 0, which stands in for every padded row, is padded itself.
    4111 live rows; a wave accumulator receives at most 5 rows: A = 5 + 3 + 16 + 32 + 1 = 57 (see _ln_compare for the bounds).
    Then the row-locality and the padded-row checks on the same launch (_ln_row_locality, _ln_garbage_in_padded_rows)."""
    use_res, use_pe, use_dy2, lens = BIG_VARIANTS[variant]
    lens = torch.tensor(lens, dtype=torch.int32)
    inp = _ln_inputs(11, BIG_B * BIG_T, BIG_D, BIG_T, dtype, use_res, use_pe, use_dy2)
    ref = W.ln_reference(lens=lens, B=BIG_B, T=BIG_T, **inp)
    out, dv = _ln_run(K, ws, inp, lens, BIG_B, BIG_T)
    _ln_compare(out, ref, BIG_B * BIG_T, dtype, 0, f"ln 8220x512 {variant}")
    _ln_row_locality(K, ws, out, dv, lens, BIG_B, BIG_T)
    _ln_garbage_in_padded_rows(K, ws, out, dv, lens, BIG_B, BIG_T)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("d", [1024, 1536, 2048])
def test_add_ln_wide_rows_past_the_grid_cap(K, ws, dtype, d):
    """B = 2, T = 2050: 4100 rows, lens = [2050, 1021].  d = 1024 (16 values per lane, two rows per trip): forward stride 4096, one trip with 4
    live and 4092 dead second rows; backward stride 2048, two trips, 2048 live and 4 dead second rows.  d = 1536 and d = 2048 (24 / 32 values
    per lane, the only one-row-per-trip kernels): a second forward trip (rows 4096..4099) and a third backward trip.
    A = ceil(4100 / 2048) + 3 + 16 + 32 + 1 = 55."""
    B, T = 2, 2050
    lens = torch.tensor([2050, 1021], dtype=torch.int32)
    inp = _ln_inputs(d, B * T, d, T, dtype, True, True, True)
    ref = W.ln_reference(lens=lens, B=B, T=T, **inp)
    out, dv = _ln_run(K, ws, inp, lens, B, T)
    _ln_compare(out, ref, B * T, dtype, 0, f"ln 4100x{d}")
    _ln_garbage_in_padded_rows(K, ws, out, dv, lens, B, T)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("d,mode", [(100, 0), (100, 1), (320, 0), (320, 2), (1000, 0), (1000, 1), (1100, 0), (1100, 2), (2047, 0)])
def test_add_ln_scalar_instantiations(K, ws, dtype, d, mode):
    """3 x 37 rows as in test_add_ln at the widths whose scalar (64 columns per step) instantiations nothing ran: d = 100 -> 2 values per
    lane, 320 -> 8, 1000 -> 16, 1100 and 2047 -> 32 (ceil(d / 64) rounded up to 1, 2, 4, 8, 16, 32); every one with masked lanes in its last
    step, 2047 odd (no dropout there: the pair hash needs an even width).  With dropout (p = 0.3) the mask comes from K.dropout_mask, itself
    held to the host restatement.  111 rows: A = 1 + 3 + 1 + 32 + 1 = 38."""
    B, T, p, seed = 3, 37, 0.3, 77
    lens = torch.tensor([37, 20, 1], dtype=torch.int32)
    inp = _ln_inputs(d + mode, B * T, d, T, dtype, True, mode != 1 and d % 2 == 0, True)      # the positional table needs an even width
    mask = None
    if mode:
        keep = K.dropout_mask(B * T, d, p, seed).cpu().numpy().astype(bool)
        assert np.array_equal(keep, D.keep_bits(B * T, d, p, seed))
        mask = torch.from_numpy(keep).double() * W.dropout_scale_f32(p)
    ref = W.ln_reference(lens=lens, B=B, T=T, mask=mask, mode=mode, **inp)
    out, _ = _ln_run(K, ws, inp, lens, B, T, mode, p if mode else 0.0, seed)
    _ln_compare(out, ref, B * T, dtype, mode, f"ln 111x{d} mode {mode}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("mode", [1, 2])
def test_add_ln_dropout_at_size(K, ws, dtype, mode):
    """drop_mode 1 (on x, before the residual add) and 2 (on the output), p = 0.3, at 8220 x 512 - the loop states of
    test_add_ln_two_rows_per_wave_and_a_second_trip with the mask regenerated per (row, column) from the element counter row * 512 + column.
    The oracle mask is K.dropout_mask(8220, 512), asserted equal to tests/dropout_ref.keep_bits: 4 208 640 mask bytes on a grid capped at
    2048 x 256 threads are 9 trips of dropout_mask_kernel's loop, its first multi-trip comparison with the host restatement."""
    p, seed = 0.3, 90210 + mode
    rows = BIG_B * BIG_T
    lens = torch.tensor([2740, 1371, 0], dtype=torch.int32)
    keep = K.dropout_mask(rows, BIG_D, p, seed).cpu().numpy().astype(bool)
    assert np.array_equal(keep, D.keep_bits(rows, BIG_D, p, seed))
    mask = torch.from_numpy(keep).double() * W.dropout_scale_f32(p)
    inp = _ln_inputs(20 + mode, rows, BIG_D, BIG_T, dtype, True, mode == 2, mode == 2)
    ref = W.ln_reference(lens=lens, B=BIG_B, T=BIG_T, mask=mask, mode=mode, **inp)
    out, _ = _ln_run(K, ws, inp, lens, BIG_B, BIG_T, mode, p, seed)
    _ln_compare(out, ref, BIG_B * BIG_T, dtype, mode, f"ln 8220x512 dropout mode {mode}")


# ------------------------------------------------------------------------------------------------ 2. LayerNorm of rows with a large mean
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_add_ln_rows_with_a_large_mean(K, dtype):
    """x = 1000 + randn, 48 rows, d = 512: the kernel subtracts the mean before it squares.  The bounds and the offset come from
    tests/test_rowwise_ref_cpu.py::test_large_mean_offset_separates_the_two_variance_forms, where a one-pass E[x^2] - mean^2 variance in the
    kernel's own summation order misses the xhat bound by 352x in fp32 and the rstd bound by 5.5e3x (fp32 storage) / 1.5e3x (bf16 storage):
        |xhat - ref| <= test_add_ln's tolerance + 14 u mean|z| rstd;    |rstd / ref - 1| <= 2e-5 + (14 u mean|z| rstd)^2 / 2."""
    x = W.large_mean_rows(dtype)
    rows, d = x.shape
    xhat_ref, rstd_ref, xb, rb = W.large_mean_bounds(x, TOL[dtype]["rtol"], TOL[dtype]["atol"])
    gamma, beta = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    y, xhat, rstd = K.add_ln_fwd(x.to(DEV), None, gamma, beta, None, None, 1, rows)
    within(xhat, xhat_ref, xb, f"large mean xhat {dtype}")
    within(rstd.double().cpu() / rstd_ref - 1, torch.zeros(rows, dtype=torch.float64), rb, f"large mean rstd {dtype}")
    within(y, xhat_ref, xb, f"large mean y {dtype}")               # gamma = 1, beta = 0: y is xhat again


# ------------------------------------------------------------------------------------------------ 3. column sums, ReLU backward
CS_SHAPES = [(4100, 512), (1500, 4232), (4100, 50)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,cols", CS_SHAPES)
def test_colsum_in_the_unrolled_loop(K, ws, dtype, rows, cols):
    """asr_colsum where the four-rows-in-flight loop runs (rowwise_ref.cs_states):
      (4100, 512)   2 column tiles -> row_slots = min(1024, 1025, 256) = 256, row stride 1024: every wave one unrolled round (4 rows), rows
                    4096..4099 in the tail loop; 5 rows per accumulator.
      (1500, 4232)  17 tiles -> row_slots = 2048 / 17 = 120, stride 480: waves r < 60 one unrolled round, the others 3 tail iterations; the
                    last tile has 136 columns = 34 lanes of a wave.
      (4100, 50)    ld = 50: the scalar path, 5 rows per wave, lane 12 with two live columns.
    Views: contiguous; ld = cols + 3 (ld % 4 != 0: the scalar path over many rows); ld = cols + 8 (the vector path with padding, except at
    cols = 50 where 58 is no multiple of 4 - there ld = 60 as well: lanes 0..11 vector, lane 12 scalar).  accumulate=True onto a non-zero out
    and accumulate=False onto NaN.  Bound: gamma(A) (sum|x| + |out before|), A = ceil(rows / (4 row_slots)) + 3 + ceil(row_slots / 32) + 32 + 1
    = 49 / 44 / 49; the terms are stored values, exact in fp32.  The reference side's kernel-order emulation uses under 1 % of it."""
    g = torch.Generator().manual_seed(rows + cols)
    views = [(0, cols), (1, cols + 3), (4, cols + 8)] + ([(4, 60)] if cols == 50 else [])
    for off, ld in views:
        big = torch.randn(rows, ld, generator=g).to(dtype).to(DEV)
        view = big[:, off:off + cols] if ld != cols else big
        assert view.stride(0) == ld
        x64 = view.double().cpu()
        init = torch.randn(cols, generator=g)
        out = init.clone().to(DEV)
        K.colsum(view, out, ws, accumulate=True)
        within(out, x64.sum(0) + init.double(), W.colsum_tolerance(x64, rows, cols, init), f"colsum ({rows},{cols}) ld {ld} accumulate")
        out = torch.full((cols,), float("nan"), device=DEV)
        K.colsum(view, out, ws, accumulate=False)
        within(out, x64.sum(0), W.colsum_tolerance(x64, rows, cols), f"colsum ({rows},{cols}) ld {ld} overwrite")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("rows,cols", CS_SHAPES)
def test_relu_bwd_in_the_unrolled_loop(K, ws, dtype, rows, cols):
    """asr_relu_bwd (the same kernel body, ld = cols) at the shapes of test_colsum_in_the_unrolled_loop; a holds +0, -0, negatives and
    positives.  da afterwards is da * (a > 0): kept elements bit for bit, masked ones zero (the kernel selects +0; the product in torch
    would give -0 under a negative da, so zeros are compared by value).  dbias (+= onto ones) is within gamma(A) (sum|da (a > 0)| + 1) of the fp64
    column sum.  With dbias=None da is masked the same and nothing else is written: a, and the 64 sentinels behind da, keep their bits."""
    g = torch.Generator().manual_seed(rows * 3 + cols)
    a = torch.randn(rows, cols, generator=g)
    z = torch.rand(rows, cols, generator=g)
    a[z < 0.05] = 0.0
    a[z > 0.95] = -0.0
    a = a.to(dtype)
    assert int((bits(a) == 0).sum()) > 0 and int(((a == 0) & (bits(a) != 0)).sum()) > 0
    da = torch.randn(rows, cols, generator=g).to(dtype)
    live = a > 0
    want = torch.where(live, da, torch.zeros_like(da))
    ad = a.to(DEV)
    for with_bias in (True, False):
        dad, buf = guarded(da, -3.0)
        dbias = torch.ones(cols, device=DEV) if with_bias else None
        got = K.relu_bwd_(dad, ad, dbias, ws)
        assert got is dad
        got = got.cpu()
        assert torch.equal(got, want), "relu_bwd_ mask"
        assert torch.equal(bits(got)[live], bits(da)[live]), "relu_bwd_ changed a kept element"
        assert untouched(buf, rows * cols, -3.0) and same_bits(ad, a)
        if with_bias:
            w64 = want.double()
            within(dbias, w64.sum(0) + 1.0, W.colsum_tolerance(w64, rows, cols, torch.ones(cols)), f"relu_bwd dbias ({rows},{cols})")


# ------------------------------------------------------------------------------------------------ 4. ReLU and cast past the grid cap
EW_N = [4194304 + 8 * 300 + 5, 1, 7, 8, 9]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("n", EW_N)
def test_relu_past_the_grid_cap(K, dtype, n):
    """n = 4 194 304 + 8 * 300 + 5: 524 588 vectors of 8 on a grid capped at 2048 x 256 threads = 524 288 -> a second trip of 300 vectors, then
    5 tail elements (workgroup 0, one per thread).  n = 1, 7: tail only (n8 = 0); 8: body only; 9: both.  Exact against torch.relu.  The input
    holds -0.0: IEEE 754 maxNum (fmaxf) may return either zero for (-0, +0), so those elements - and only those - are compared by value.
    64 sentinels (negative, so a stray ReLU would show) lie behind the buffer and stay."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x[torch.rand(n, generator=g) < 0.1] = -0.0
    x[0] = -0.0
    x = x.to(dtype)
    xd, buf = guarded(x, -7.0)
    got = K.relu_(xd).cpu()
    want = torch.relu(x)
    negzero = (x == 0) & (bits(x) != 0)
    assert torch.equal(got, want)
    assert torch.equal(bits(got)[~negzero], bits(want)[~negzero])
    assert untouched(buf, n, -7.0)


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)])
@pytest.mark.parametrize("n", EW_N)
def test_cast_past_the_grid_cap(K, src, dst, n):
    """All four dtype pairs of asr_cast (f32 -> f32 and bf16 -> bf16 had no caller in the suite) at the sizes of test_relu_past_the_grid_cap;
    bit-exact against torch's round-to-nearest-even conversion, sentinels behind source and destination untouched."""
    g = torch.Generator().manual_seed(n + 1)
    x = (torch.randn(n, generator=g) * 3).to(src)
    xd, xbuf = guarded(x, 5.0)
    yd, ybuf = guarded(torch.zeros(n, dtype=dst), 9.0)
    got = K.cast(xd, yd)
    assert same_bits(got, x.to(dst))
    assert untouched(ybuf, n, 9.0) and untouched(xbuf, n, 5.0) and same_bits(xd, x)


# ------------------------------------------------------------------------------------------------ 5. Adam
def _adam_state(n, seed, gscale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g) * gscale, torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.1)


def _adam_reference(p, g, m, v, step, lr, max_norm):
    """fp64 Adam step of the oracle (R.clip_grad_norm, R.adam_update) on the fp32 operands -> (clipped g, p, m, v, coef).  b1 and b2 are the C
    floats the kernel receives: with m and v non-zero, 0.9 m + 0.1 g cancels, and 1.f - 0.9f = 0.10000002 against 0.1 would use up the 1e-7 on m."""
    gc = g.double()
    coef = 1.0
    if max_norm > 0:
        total, (gc,) = R.clip_grad_norm([g.double()], max_norm)
        coef = float(torch.clamp(max_norm / (total + 1e-6), max=1.0))
    p2, m2, v2 = R.adam_update(p.double(), gc, m.double(), v.double(), step, lr, b1=float(np.float32(0.9)), b2=float(np.float32(0.98)))
    return gc, p2, m2, v2, coef


def _adam_close(P, M_, V_, p, m, v, tag):
    close(P, p, rtol=1e-5, atol=1e-6, what=f"{tag} p")
    close(M_, m, rtol=1e-5, atol=1e-7, what=f"{tag} m")
    close(V_, v, rtol=1e-5, atol=1e-9, what=f"{tag} v")


def test_adam_past_the_grid_cap(K, ws):
    """n = 2 097 152 + 4 * 77 + 3: 524 365 vectors of 4 on 2048 x 256 threads -> a second trip of 77 vectors, then 3 tail elements.  Three steps
    (clipping active in the first and third, the norm below max_norm in the second) against R.adam_update / R.clip_grad_norm in fp64 at
    test_optimizer's tolerances; the Noam schedule runs with warmup = 25, so that a step moves p by ~4e-4, far above the tolerance on p
    (1e-5 |p| + 1e-6) - with warmup = 4000 a step is 2e-7 and a missing update would pass.  Sentinels behind p, g, m, v, lp."""
    n = 2097152 + 4 * 77 + 3
    p, g, m, v = _adam_state(n, 3)
    m.zero_()
    v.zero_()
    (P, Pb), (G, Gb), (M_, Mb), (V_, Vb) = (guarded(t, s) for t, s in ((p, 11.0), (g, 12.0), (m, 13.0), (v, 14.0)))
    lp, lpb = guarded(torch.zeros(n, dtype=BF16), 15.0)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    hyper = torch.zeros(4, device=DEV)
    sumsq = torch.zeros(1, device=DEV)
    for it in range(1, 4):
        K.grad_sumsq(G, sumsq, ws)
        K.noam_hyper(step, hyper, 512, 25, 1.0, 0.0, 0.9, 0.98)
        lr = R.noam_rate(it, 512, 25)
        assert abs(float(hyper[0]) - lr) < 1e-6 * lr
        p_before = P.clone()
        K.adam_step(P, G, M_, V_, lp, hyper, sumsq, 5.0, 0.9, 0.98, 1e-9)
        gc, p, m, v, coef = _adam_reference(p, g, m, v, it, lr, 5.0)
        assert (coef < 1.0) == (it != 2)
        close(G, gc, rtol=1e-5, atol=1e-7, what=f"adam step {it} clipped g")
        if it == 2:
            assert same_bits(G, g), "nothing clipped: g keeps its bits"
        _adam_close(P, M_, V_, p, m, v, f"adam step {it}")
        assert float((P - p_before).abs().double().mean()) > 1e-5       # the step is visible at the tolerance
        assert torch.equal(lp.cpu(), P.cpu().bfloat16())
        p, m, v = P.cpu().clone(), M_.cpu().clone(), V_.cpu().clone()  # the next step's operands are what the kernel stored
        g = torch.randn(n, generator=torch.Generator().manual_seed(40 + it)) * (0.001 if it == 1 else 3)
        G.copy_(g)
    for buf, s in ((Pb, 11.0), (Gb, 12.0), (Mb, 13.0), (Vb, 14.0), (lpb, 15.0)):
        assert untouched(buf, n, s)


@pytest.mark.parametrize("n", [100003, 1, 2, 3])
def test_adam_unvisited_arguments(K, ws, n):
    """The argument combinations nothing called: p_lp=None; max_norm = 0 with sumsq=None (Trainer/optimizer.py's per-tensor path);
    write_clipped=False while clipping is active; a norm below max_norm.  n = 100 003 (one trip, tail of 3) and n = 1, 2, 3 (n4 = 0: the tail
    alone).  hyper is set by hand (lr = 1e-2, step 3), so every step moves p by ~1e-2.  g keeps its bits wherever the kernel must not write
    it (rowwise_ref_cpu: a written-back clipped gradient changes > 99.9 % of the elements); p, m, v follow the clipped gradient at
    test_optimizer's tolerances.  Sentinels behind every buffer."""
    b1, b2, t, lr = 0.9, 0.98, 3, 1e-2
    hyper = torch.tensor([lr, 1 - b1 ** t, (1 - b2 ** t) ** 0.5, t], dtype=torch.float32, device=DEV)
    sumsq = torch.zeros(1, device=DEV)
    p0, g0, m0, v0 = _adam_state(n, n)
    norm = float(torch.sqrt((g0.double() ** 2).sum()))
    cases = [
        # name, p_lp, max_norm, pass sumsq, write_clipped, clipping active
        ("no shadow", False, 0.25 * norm, True, True, True),
        ("no clipping, no sumsq", False, 0.0, False, False, False),
        ("no clipping, write_clipped left on", True, 0.0, False, True, False),
        ("clipped, not written back", True, 0.25 * norm, True, False, True),
        ("norm below max_norm", True, 4.0 * norm, True, True, False),
    ]
    for name, with_lp, max_norm, with_sumsq, write_clipped, active in cases:
        (P, Pb), (G, Gb), (M_, Mb), (V_, Vb) = (guarded(x, s) for x, s in ((p0, 11.0), (g0, 12.0), (m0, 13.0), (v0, 14.0)))
        lp, lpb = guarded(torch.zeros(n, dtype=BF16), 15.0)
        if with_sumsq:
            K.grad_sumsq(G, sumsq, ws)
        K.adam_step(P, G, M_, V_, lp if with_lp else None, hyper, sumsq if with_sumsq else None, max_norm, b1, b2, 1e-9, write_clipped=write_clipped)
        gc, p, m, v, coef = _adam_reference(p0, g0, m0, v0, t, lr, max_norm)
        assert (coef < 1.0) == active, name
        _adam_close(P, M_, V_, p, m, v, f"adam n={n} {name}")
        if active and write_clipped:
            close(G, gc, rtol=1e-5, atol=1e-7, what=f"adam n={n} {name} clipped g")
            assert not same_bits(G, g0)
        else:
            assert same_bits(G, g0), f"{name}: g was written"
        if with_lp:
            assert torch.equal(lp.cpu(), P.cpu().bfloat16())
        else:
            assert float(lp.float().abs().max()) == 0.0
        for buf, s in ((Pb, 11.0), (Gb, 12.0), (Mb, 13.0), (Vb, 14.0), (lpb, 15.0)):
            assert untouched(buf, n, s), name


# ------------------------------------------------------------------------------------------------ 6. embedding at model width
EMB_V, EMB_D, EMB_B, EMB_TO = 4232, 512, 8, 25


def _embed_ids(kind):
    g = torch.Generator().manual_seed(6)
    rows = EMB_B * EMB_TO
    if kind == "random":           # a few repeats, and the out-of-range ids -1 and V
        ids = torch.randint(0, EMB_V, (rows,), generator=g, dtype=torch.int32)
        ids[3], ids[77], ids[150], ids[199] = -1, EMB_V, -1, EMB_V
        ids[10:20] = ids[5]
    elif kind == "same":           # 200 atomics contend on each of 512 addresses
        ids = torch.full((rows,), 1234, dtype=torch.int32)
    else:                          # all distinct: one addend per element
        ids = torch.randperm(EMB_V, generator=g)[:rows].to(torch.int32)
    return ids


def _embed_case(K, dtype, kind):
    """d = 512 (the kernels' `c += blockDim.x` loops run twice; the suite had d = 48), V = 4232, B * To = 8 * 25, fp32 and bf16 activations,
    without dropout and with p = 0.1 (mask from K.dropout_mask, held to the host restatement).  Forward: ids -1 and V clamp to rows 0 and
    V - 1 of the table.  Backward: the same ids contribute nothing; every element of demb is within gamma(n + c - 1) sum|addend| of the fp64
    index_add_ reference, n = its number of addends (200 when every token is the same id, 1 when all differ, 0 -> exact), c = 1 rounding for
    dy * scale, 2 with the dropout scale (rowwise_ref.embed_bwd_reference): n u sum|addend| without dropout.  The order of the adds is free."""
    rows = EMB_B * EMB_TO
    g = torch.Generator().manual_seed(8)
    emb = torch.randn(EMB_V, EMB_D, generator=g)
    pe = R.positional_encoding(EMB_TO, EMB_D)
    dy = torch.randn(rows, EMB_D, generator=g).to(dtype)
    ids = _embed_ids(kind)
    scale = EMB_D ** -0.5
    for p, seed in ((0.0, 0), (0.1, 31337)):
        mask = None
        if p:
            keep = K.dropout_mask(rows, EMB_D, p, seed).cpu().numpy().astype(bool)
            assert np.array_equal(keep, D.keep_bits(rows, EMB_D, p, seed))
            mask = torch.from_numpy(keep).double() * W.dropout_scale_f32(p)
        y = K.embed_pe_fwd(ids.to(DEV), emb.to(DEV), pe.to(DEV), scale, EMB_B, EMB_TO, dtype, drop_p=p, drop_seed=seed)
        close(y, W.embed_reference(ids, emb, pe, scale, EMB_TO, mask), **TOL[dtype], what=f"embed fwd {kind} p={p}")
        demb = torch.zeros(EMB_V, EMB_D, device=DEV)
        K.embed_bwd(ids.to(DEV), dy.to(DEV), demb, scale, drop_p=p, drop_seed=seed)
        ref, tol = W.embed_bwd_reference(ids, dy, scale, EMB_V, mask, term_roundings=2 if p else 1)
        within(demb, ref, tol, f"embed bwd {kind} p={p}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("kind", ["random", "same", "distinct"])
def test_embedding_at_model_width(K, dtype, kind):
    """_embed_case with the atomic backward kernel (one workgroup per token)."""
    assert not K.deterministic()
    _embed_case(K, dtype, kind)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("kind", ["random", "same", "distinct"])
def test_embedding_at_model_width_serial_kernel(K, deterministic_mode, dtype, kind):
    """_embed_case with embed_bwd_serial_kernel (deterministic mode: a thread per column, tokens in order; two column blocks at d = 512)."""
    assert K.deterministic()
    _embed_case(K, dtype, kind)
