"""tests/rowwise_ref.py without a GPU: the restated launch arithmetic proves that every shape of tests/test_rowwise_states_gpu.py reaches
the loop state it is named after, the fp64 references agree with torch's own, the summation bounds hold a correct fp32 implementation and
reject plausible defects (negative controls on the reference side), and the offset of the large-mean LayerNorm rows is chosen here."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import rowwise_ref as W

TOL = {torch.float32: (2e-5, 2e-5), torch.bfloat16: (1.6e-2, 1e-2)}          # test_add_ln: (rtol, atol) of y, here also of xhat
GT = {torch.float32: (2e-4, 2e-4), torch.bfloat16: (3e-2, 6e-2)}             # test_add_ln: per-element gradients


# ------------------------------------------------------------------------------------------------ the shapes reach their states
def test_layernorm_shapes_reach_the_named_states():
    """The instantiations: d -> (values per lane, vector path).  Then, per shape, stride / trips / second-row slots."""
    assert [W.ln_instance(d) for d in (32, 48, 100, 200, 320, 1000, 1100, 2047)] == \
        [(1, False), (1, False), (2, False), (4, False), (8, False), (16, False), (32, False), (32, False)]
    assert [W.ln_instance(d) for d in (512, 1024, 1536, 2048)] == [(8, True), (16, True), (24, True), (32, True)]
    assert [W.ln_rows_per_trip(d) for d in (512, 1024, 1536, 2048, 1000, 1100)] == [2, 2, 1, 1, 2, 1]
    # what the suite had: every loop once, no live second row
    for rows in (111, 38):
        for bwd in (False, True):
            s = W.ln_states(rows, 512, bwd)
            assert s["trips"] == 1 and s["live2"] == 0
    # 8220 x 512 forward: 1024 workgroups, stride 4096; trip 1 = rows 0..8191 (4096 live second rows), trip 2 = rows 8192..8219 whose 28
    # second-row slots lie past the end (the clamped re-read of row 8219)
    assert W.ln_states(8220, 512, False) == dict(stride=4096, trips=2, live2=4096, dead2=28)
    # backward: 512 workgroups, stride 2048; trips at row0 in [0, 2048), [4096, 6144), [8192, 8220): 4096 live second rows, 28 dead ones
    assert W.ln_states(8220, 512, True) == dict(stride=2048, trips=3, live2=4096, dead2=28)
    # the one-utterance slices of the row-locality check (1370 rows): one row per wave, one trip
    for bwd in (False, True):
        s = W.ln_states(1370, 512, bwd)
        assert s["trips"] == 1 and s["live2"] == 0 and s["dead2"] == 1370
    # 4100 x 1024 (N = 16, two rows per trip): forward 4 live + 4092 dead second rows in one trip; backward two trips
    assert W.ln_states(4100, 1024, False) == dict(stride=4096, trips=1, live2=4, dead2=4092)
    assert W.ln_states(4100, 1024, True) == dict(stride=2048, trips=2, live2=2048, dead2=4)
    # 4100 x 1536 / 2048 (one row per trip): a second forward trip, a third backward trip
    for d in (1536, 2048):
        assert W.ln_states(4100, d, False)["trips"] == 2 and W.ln_states(4100, d, True)["trips"] == 3
    # adds on the longest path of a parameter-gradient sum: 8220 rows -> 5 + 3 + 16 + 32 + 1
    assert W.ln_bwd_sum_adds(8220) == 57 and W.ln_bwd_sum_adds(4100) == 3 + 3 + 16 + 32 + 1 and W.ln_bwd_sum_adds(111) == 1 + 3 + 1 + 32 + 1


def test_colsum_shapes_reach_the_unrolled_loop():
    # what the suite had: 4 * row_slots >= rows, the four-row loop never entered
    for rows, cols in ((37, 1024), (500, 48), (129, 4232), (5, 7)):
        assert W.cs_states(rows, cols, cols)["unrolled"] == 0
    # (4100, 512): 2 column tiles, 256 row slots, row stride 1024: one unrolled round (rows r .. r + 3072), then rows 4096..4099 in the tail
    assert W.cs_states(4100, 512, 512) == dict(slots=256, ctiles=2, vector=True, unrolled=1, tail=1, adds=5)
    # (1500, 4232): 17 tiles, 120 slots, stride 480: waves r < 60 run one unrolled round, the others three tail iterations;
    # the last tile holds 4232 - 4096 = 136 columns = 34 lanes of a wave
    assert W.cs_states(1500, 4232, 4232) == dict(slots=120, ctiles=17, vector=True, unrolled=1, tail=3, adds=4)
    assert (4232 - 16 * 256) // 4 == 34
    # (4100, 50): ld = 50 is no multiple of 4 -> the scalar path over 5 rows per wave; lane 12 holds columns 48, 49 only
    assert W.cs_states(4100, 50, 50) == dict(slots=256, ctiles=1, vector=False, unrolled=0, tail=5, adds=5)
    # views: ld % 4 != 0 (scalar path over many rows) and ld = cols + 8 (vector path with padding; cols = 50 needs ld = 60 for that)
    for cols in (512, 4232, 50):
        assert not W.cs_states(1500, cols, cols + 3)["vector"]
    assert W.cs_states(4100, 512, 520)["unrolled"] == 1 and W.cs_states(1500, 4232, 4240)["unrolled"] == 1
    assert not W.cs_states(4100, 50, 58)["vector"] and W.cs_states(4100, 50, 60) == dict(slots=256, ctiles=1, vector=True, unrolled=1, tail=1, adds=5)
    assert W.colsum_adds(4100, 512) == 5 + 3 + 8 + 32 + 1 and W.colsum_adds(1500, 4232) == 4 + 3 + 4 + 32 + 1


def test_elementwise_sizes_pass_the_grid_cap():
    n = 4194304 + 8 * 300 + 5
    assert W.ew_states(n, 8) == dict(nvec=524588, grid=2048, trips=2, tail=5)          # 300 vectors in the second trip, 5 tail elements
    assert W.ew_states(545928, 8)["trips"] == 1                                         # the largest n the suite had
    assert [W.ew_states(k, 8)["nvec"] for k in (1, 7, 8, 9)] == [0, 0, 1, 1] and [W.ew_states(k, 8)["tail"] for k in (1, 7, 8, 9)] == [1, 7, 0, 1]
    n = 2097152 + 4 * 77 + 3
    assert W.ew_states(n, 4) == dict(nvec=524365, grid=2048, trips=2, tail=3)          # adam: 77 vectors in the second trip, 3 tail elements
    assert W.ew_states(100003, 4)["trips"] == 1 and [W.ew_states(k, 4)["nvec"] for k in (1, 2, 3)] == [0, 0, 0]
    assert W.mask_trips(37 * 512) == 1 and W.mask_trips(512 * 1024) == 1 and W.mask_trips(8220 * 512) == 9


# ------------------------------------------------------------------------------------------------ the references
def _ln_case(rows_bt=(3, 37), d=64, dtype=torch.float32, seed=0, mode=0):
    B, T = rows_bt
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, res, dy, dy2 = (rn(B * T, d).to(dtype) for _ in range(4))
    gamma, beta = 1 + 0.2 * rn(d), 0.1 * rn(d)
    pe = rn(T, d)
    lens = torch.tensor([T, T // 2, 0][:B], dtype=torch.int32)
    mask = (torch.rand(B * T, d, generator=g) > 0.3).double() / 0.7 if mode else None
    return dict(x=x, res=res, gamma_=gamma, beta=beta, pe=pe, lens=lens, B=B, T=T, dy=dy, dy2=dy2, mask=mask, mode=mode)


def test_ln_reference_equals_torch_layer_norm_autograd():
    for mode in (0, 1, 2):
        c = _ln_case(mode=mode)
        ref = W.ln_reference(**c)
        xr, rr = c["x"].double().requires_grad_(True), c["res"].double().requires_grad_(True)
        g64, b64 = c["gamma_"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
        z = (xr * c["mask"] if mode == 1 else xr) + rr
        y = F.layer_norm(z, (64,), g64, b64, 1e-5) + c["pe"].double().repeat(3, 1)
        if mode == 2:
            y = y * c["mask"]
        y = y * W.keep_rows(c["lens"], 3, 37)
        (y * (c["dy"].double() + c["dy2"].double())).sum().backward()
        for got, want in ((ref["y"], y.detach()), (ref["dz"], rr.grad), (ref["dx"], xr.grad), (ref["dgamma"], g64.grad), (ref["dbeta"], b64.grad),
                          (ref["dbias"], xr.grad.sum(0))):
            assert float((got - want).abs().max()) < 1e-12
        assert float((ref["abs_bias"] - ref["dx"].abs().sum(0)).min()) >= 0          # the pieces dominate the rows they cancel to
        z64 = z.detach()
        assert float((ref["rstd"] - (z64.var(1, unbiased=False) + 1e-5) ** -0.5).abs().max()) < 1e-12


def test_fp32_column_sum_in_kernel_order_sits_inside_the_bound():
    """A correct fp32 implementation (the kernel's order, emulated) uses a small part of the worst-case bound: measured 0.3 % of it at
    (4100, 512), 0.9 % at (1500, 4232)."""
    for rows, cols in ((4100, 512), (1500, 4232)):
        x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows))
        got = W.colsum_emulate_f32(x.numpy(), rows, cols)
        err = np.abs(got.astype(np.float64) - x.double().sum(0).numpy())
        tol = W.colsum_tolerance(x.double(), rows, cols).numpy()
        print("colsum emulation, largest err / tol", float((err / tol).max()))
        assert (err <= tol).all() and float((err / tol).max()) < 0.05


# ------------------------------------------------------------------------------------------------ the gates can fail (negative controls)
def test_a_row_taken_from_its_neighbour_leaves_the_per_element_gate():
    """Defect: one output row of LayerNorm computed from the next input row (a wrong row index in the second slot of a trip).  Measured on the
    reference side with y, xhat, dz of row r replaced by row r + 1: the largest |error| / tolerance is 1.8e5 / 1.1e5 / 1.6e4 (fp32) and
    3.5e2 / 2.0e2 / 56 (bf16) for y / xhat / dz; a single such row among 111 fails the gate by these factors."""
    for dtype in (torch.float32, torch.bfloat16):
        ref = W.ln_reference(**_ln_case(dtype=dtype, d=512, seed=3))
        for key, (rtol, atol) in (("y", TOL[dtype]), ("xhat", TOL[dtype]), ("dz", GT[dtype])):
            want = ref[key]
            bad = want.clone()
            bad[5] = want[6]
            over = float(((bad - want).abs() / (atol + rtol * want.abs())).max())
            print("neighbour row", dtype, key, over)
            assert over > 50


def test_a_dropped_last_row_leaves_the_summation_gates():
    """Defect: the last (partial) row of a column sum dropped - the tail loop of colsum_partial_kernel one iteration short, or the last trip
    of add_ln_bwd skipped.  Measured: the dropped row's largest |term| / tolerance is 4.5e2 at (4100, 512) and 1.1e3 at (1500, 4232) for
    asr_colsum; for the LayerNorm sums over 8220 rows (4111 live) 3.8e2 (dbeta), 6.9e2 (dgamma) and 99 (dbias) in fp32, and with the bf16
    per-element allowance on dbias 13."""
    for rows, cols in ((4100, 512), (1500, 4232)):
        x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(cols)).double()
        over = float((x[-1].abs() / W.colsum_tolerance(x, rows, cols)).max())
        print("dropped row, colsum", rows, cols, over)
        assert over > 100
    B, T, d = 3, 2740, 512
    for dtype in (torch.float32, torch.bfloat16):
        c = _ln_case(rows_bt=(B, T), d=d, dtype=dtype, seed=9)
        c["lens"] = torch.tensor([2740, 1371, 0], dtype=torch.int32)
        ref = W.ln_reference(**c)
        tol = W.ln_param_tolerances(ref, B * T, None if dtype == torch.float32 else GT[dtype])
        last = T + 1370                                                     # the last live row
        terms = dict(dbeta=ref["gy"][last], dgamma=ref["gy"][last] * ref["xhat"][last], dbias=ref["dx"][last])
        for k, t in terms.items():
            over = float((t.abs() / tol[k]).max())
            print("dropped row, ln", dtype, k, over)
            assert over > 10


def test_a_clipped_gradient_written_back_changes_its_bits():
    """Defect: adam_kernel writes g * coef although write_clipped is off (or although nothing is clipped and coef is taken as something
    other than 1).  The gate on g is bit equality; with coef = 0.25 * norm / (norm + 1e-6) every non-zero element changes."""
    g = torch.randn(100003, generator=torch.Generator().manual_seed(1)) * 3
    norm = torch.sqrt((g.double() ** 2).sum()).float()
    coef = torch.clamp(0.25 * norm / (norm + 1e-6), max=1.0)
    changed = float(((g * coef).view(torch.int32) != g.view(torch.int32)).float().mean())
    assert changed > 0.999


# ------------------------------------------------------------------------------------------------ rows with a large mean
def test_large_mean_offset_separates_the_two_variance_forms():
    """x = offset + randn, d = 512, 48 rows, both forms emulated in fp32 with the kernel's summation order (8 values per lane, 64-lane tree).

    Measured at offset = 1000 (largest error / bound over the 48 x 512 elements, resp. 48 rows):
                               xhat, two-pass   xhat, one-pass   rstd, two-pass   rstd, one-pass
        fp32 storage               0.070             352             0.0055         5.5e3
        bf16 storage               0.19              1.7             0.0033         1.5e3
    fp32: the one-pass form leaves the xhat bound by 352x.  bf16 storage: x is rounded to multiples of 4 there and the xhat bound carries the
    bf16 output tolerance (1e-2 + 1.6e-2 |xhat|), which a 4 % error of rstd exceeds by 1.7x only; no offset does better (a row of bf16 values
    cannot have mean / std much above 2^8 without becoming constant).  The kernel writes rstd in fp32 whatever the storage type, so the
    separation for bf16 storage is shown, and the kernel held to it, on rstd: 1.5e3x.  The two-pass form stays inside every bound."""
    for dtype in (torch.float32, torch.bfloat16):
        x = W.large_mean_rows(dtype)
        xhat, rstd, xb, rb = W.large_mean_bounds(x, *TOL[dtype])
        rnd = (lambda a: torch.from_numpy(a).to(dtype).double())            # the kernel stores xhat in the storage type
        over = {}
        for one_pass in (False, True):
            xe, re = W.ln_emulate_f32(x.float().numpy(), one_pass)
            over[one_pass] = (float(((rnd(xe) - xhat).abs() / xb).max()), float(((torch.from_numpy(re).double() / rstd - 1).abs() / rb).max()))
        print("large mean", dtype, "two-pass (xhat, rstd)", over[False], "one-pass", over[True])
        assert over[False][0] < 1 and over[False][1] < 1
        assert over[True][1] > 10
        if dtype == torch.float32:
            assert over[True][0] > 10
    # a smaller offset would not do in fp32 either way round: at 100 the one-pass form is only 18x outside
    x = W.large_mean_rows(torch.float32, offset=100.0)
    xhat, _, xb, _ = W.large_mean_bounds(x, *TOL[torch.float32])
    xe, _ = W.ln_emulate_f32(x.numpy(), True)
    assert 10 < float(((torch.from_numpy(xe).double() - xhat).abs() / xb).max()) < 352


# ------------------------------------------------------------------------------------------------ embedding
def test_embed_references():
    g = torch.Generator().manual_seed(0)
    V, d, To = 11, 8, 5
    emb, pe, dy = torch.randn(V, d, generator=g), torch.randn(To, d, generator=g), torch.randn(10, d, generator=g)
    ids = torch.tensor([3, -1, V, 3, 0, 10, 3, 7, 7, 2], dtype=torch.int32)
    y = W.embed_reference(ids, emb, pe, 0.5, To)
    assert torch.equal(y[1], emb[0].double() * 0.5 + pe[1].double()) and torch.equal(y[2], emb[V - 1].double() * 0.5 + pe[2].double())
    ref, tol = W.embed_bwd_reference(ids, dy, 0.5, V)
    want = torch.zeros(V, d, dtype=torch.float64)
    for r, i in enumerate(ids.tolist()):
        if 0 <= i < V:
            want[i] += dy[r].double() * 0.5
    assert float((ref - want).abs().max()) < 1e-15
    assert float(tol[1].max()) == 0.0 and float(tol[4].max()) == 0.0              # no addend: exact
    assert torch.allclose(tol[3], 3 * W.U32 * (dy[[0, 3, 6]].double().abs() * 0.5).sum(0), rtol=1e-6)      # n u sum|addend|
    assert abs(W.dropout_scale_f32(0.1) - 1 / 0.9) < 1e-7
