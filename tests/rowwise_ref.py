"""Host references for the row-wise kernels (csrc/ln.hip; csrc/misc.hip: column sums, ReLU, cast, Adam, embedding), numpy / torch on the CPU.

Three things live here, all shared by tests/test_rowwise_states_gpu.py (which holds the kernels to them) and tests/test_rowwise_ref_cpu.py
(which checks the helpers themselves and the choice of inputs without a GPU):

  * the launch arithmetic of the kernels restated (ln_grid_fwd, ln_grid, cs_row_slots, ew_grid and the per-instantiation constants), so that a
    test can prove that a shape reaches the loop state it is named after (a second trip, a live second row of a trip, the unrolled loop);
  * fp64 references, computed from the operands after they were rounded to the storage type (tests/test_kernels_gpu.py's header);
  * fp32 summation bounds derived on the reference side.  For a sum of terms t_i in fp32, whatever the order, the first-order error is at
    most A * u * sum|t_i| with u = 2^-24 and A the number of roundings on the longest path from a term to the result (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2); gamma(A) = A u / (1 - A u) makes it exact.  A is counted from the kernels' code:

        serial adds per accumulator + adds that combine the accumulators (LDS, finalize pass) + roundings that formed the term.
"""
import numpy as np
import torch

U32 = 2.0 ** -24          # unit round-off of fp32


def ceil_div(a, b):
    return -(-a // b)


def gamma(n):
    """Higham's gamma_n for fp32: n roundings in sequence perturb a sum by at most gamma(n) * sum|terms|."""
    return n * U32 / (1.0 - n * U32)


# ------------------------------------------------------------------------------------------------ launch arithmetic, restated
LN_WAVES = 4


def ln_instance(d):
    """(N values per lane, vector path?) of the add_ln kernels for width d (launch_ln_fwd / launch_ln_bwd)."""
    if d % 512 == 0 and d <= 2048:
        return d // 64, True
    nk = ceil_div(d, 64)
    for n in (1, 2, 4, 8, 16):
        if nk <= n:
            return n, False
    return 32, False


def ln_rows_per_trip(d):
    """LN_U: rows a wave loads together in one trip (2 up to N = 16, then 1)."""
    return 2 if ln_instance(d)[0] <= 16 else 1


def ln_grid_fwd(rows):
    return min(ceil_div(rows, LN_WAVES), 1024)


def ln_grid(rows):
    return min(ceil_div(rows, LN_WAVES), 512)


def ln_states(rows, d, bwd):
    """Loop states of one add_ln launch: dict(stride, trips, live2, dead2).
    trips: iterations of the busiest wave's row loop; live2 / dead2: second-row slots of a trip that hold a row / lie past the end (the
    forward kernel re-reads the last row there, the backward kernel row 0)."""
    stride = (ln_grid(rows) if bwd else ln_grid_fwd(rows)) * LN_WAVES
    u = ln_rows_per_trip(d)
    r = np.arange(rows)
    row0 = r[(r // stride) % u == 0]               # the rows that are a wave's first row of a trip
    second = row0 + stride
    live2 = int((second < rows).sum()) if u == 2 else 0
    dead2 = int((second >= rows).sum()) if u == 2 else 0
    return dict(stride=stride, trips=ceil_div(rows, u * stride), live2=live2, dead2=dead2)


def ln_bwd_sum_adds(rows):
    """Adds on the longest path of a parameter-gradient column sum of add_ln_bwd: rows per wave accumulator (acc += term, one wave takes
    every (4 * grid)-th row) + 3 (the four waves of a workgroup, s0 + s1 + s2 + s3 through LDS) + ceil(P / 32) (colsum_finalize_kernel: a
    thread adds every 32nd of the P = grid partial rows) + 32 (its 32 partial groups, added in series) + 1 (out[c] + t)."""
    g = ln_grid(rows)
    return ceil_div(rows, LN_WAVES * g) + 3 + ceil_div(g, 32) + 32 + 1


CS_WAVES = 4


def cs_row_slots(rows, cols):
    want = 2048 // ceil_div(cols, 256)
    return max(1, min(want, ceil_div(rows, CS_WAVES), 256))


def cs_states(rows, cols, ld):
    """Loop states of colsum_partial_kernel: dict(slots, ctiles, vector, unrolled, tail, adds).
    vector: lanes whose four columns are all live take 16-byte loads (needs ld % 4 == 0); unrolled / tail: the largest number of
    four-row rounds / single-row iterations that any wave runs; adds: the most rows any accumulator receives."""
    slots = cs_row_slots(rows, cols)
    rs = slots * CS_WAVES
    vector = ld % 4 == 0 and cols >= 4
    unrolled = tail = adds = 0
    for r0 in range(min(rs, rows)):
        r, k = r0, 0
        while vector and r + 3 * rs < rows:
            r += 4 * rs
            k += 1
        t = ceil_div(rows - r, rs) if r < rows else 0
        unrolled, tail, adds = max(unrolled, k), max(tail, t), max(adds, 4 * k + t)
    return dict(slots=slots, ctiles=ceil_div(cols, 256), vector=vector, unrolled=unrolled, tail=tail, adds=adds)


def colsum_adds(rows, cols):
    """As ln_bwd_sum_adds for asr_colsum / asr_relu_bwd: rows per accumulator + 3 (LDS) + ceil(slots / 32) + 32 (finalize) + 1 (out[c] + t)."""
    s = cs_row_slots(rows, cols)
    return ceil_div(rows, CS_WAVES * s) + 3 + ceil_div(s, 32) + 32 + 1


EW_BLOCK = 256


def ew_grid(nvec):
    return max(1, min(ceil_div(nvec, EW_BLOCK), 2048))


def ew_states(n, vec):
    """relu / cast (vec = 8) and adam (vec = 4): dict(nvec, grid, trips, tail) - trips of the busiest thread's grid-stride loop, tail
    elements handled one per thread by workgroup 0."""
    nvec = n // vec
    g = ew_grid(nvec)
    return dict(nvec=nvec, grid=g, trips=ceil_div(nvec, g * EW_BLOCK), tail=n - nvec * vec)


def mask_trips(n):
    """dropout_mask_kernel: iterations of the busiest thread over n mask bytes (grid capped at 2048 x 256 threads)."""
    return ceil_div(n, min(ceil_div(n, 256), 2048) * 256)


# ------------------------------------------------------------------------------------------------ LayerNorm in fp64
def keep_rows(lens, B, T):
    """(B*T, 1) float64: 1 for rows t < lens[b] (all ones without lens)."""
    if lens is None:
        return torch.ones(B * T, 1, dtype=torch.float64)
    return (torch.arange(T).unsqueeze(0) < lens.view(-1, 1)).reshape(-1, 1).double()


def ln_reference(x, res, gamma_, beta, pe, lens, B, T, dy, dy2=None, mask=None, mode=0):
    """fp64 autograd reference of asr_add_ln_fwd / asr_add_ln_bwd on the (already rounded) operands, as in test_add_ln, with the
    normalisation written out so that xhat and rstd can be compared too:
        z = (x * mask if mode == 1 else x) + res;  xhat = (z - mean) * rstd;  rstd = (var + 1e-5)^-1/2
        y = (xhat * gamma + beta + pe[t]) * (mask if mode == 2) * (t < lens[b])
    mask is the SCALED keep mask (keep / (1 - p)).  Returns a dict of detached fp64 tensors: y, xhat, rstd, dz (gradient at z), dx (at x),
    dgamma, dbeta, dbias (= column sums of dx) and, for the summation bounds, the column sums of the terms' magnitudes: abs_beta
    (sum |gy|), abs_gamma (sum |gy xhat|), abs_bias (sum of the un-cancelled pieces of a dx row, see ln_param_tolerances), and gy itself
    (the upstream gradient that reaches the normalisation's output: (dy + dy2) * mask(mode 2) * keep)."""
    xr = x.double().requires_grad_(True)
    g64, b64 = gamma_.double().requires_grad_(True), beta.double().requires_grad_(True)
    m = None if mask is None else torch.as_tensor(mask, dtype=torch.float64)
    z = xr * m if mode == 1 else xr * 1.0
    if res is not None:
        z = z + res.double()
    z.retain_grad()
    mean = z.mean(1, keepdim=True)
    var = ((z - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + 1e-5) ** -0.5
    xhat = (z - mean) * rstd
    y = xhat * g64 + b64
    if pe is not None:
        y = y + pe[:T].double().repeat(B, 1)
    if mode == 2:
        y = y * m
    keep = keep_rows(lens, B, T)
    y = y * keep
    up = dy.double() + (dy2.double() if dy2 is not None else 0.0)
    (y * up).sum().backward()
    gy = up * keep * (m if mode == 2 else 1.0)
    xh, rs, g = xhat.detach(), rstd.detach(), g64.detach()
    gg = gy * g
    pieces = rs * (gg.abs() + gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True))
    if mode == 1:
        pieces = pieces * m
    return dict(y=y.detach(), xhat=xh, rstd=rs.reshape(-1), dz=z.grad, dx=xr.grad, dgamma=g64.grad, dbeta=b64.grad, dbias=xr.grad.sum(0),
                gy=gy, abs_beta=gy.abs().sum(0), abs_gamma=(gy * xh).abs().sum(0), abs_bias=pieces.sum(0))


# term roundings in fp32 between the stored operands and the value an accumulator receives
LN_TERM_BETA = 2      # dy + dy2, * dropout scale
LN_TERM_GAMMA = 3     # ... * xhat
LN_TERM_BIAS = 40     # a dz element: gy * gamma (2, with the one above) + a row mean (8 serial + 6 tree + 1 scale = 15) under each of s1 and s2 + two
#                       products and two subtractions (4) = 36, + 4 for the fp32 error that the stored xhat and rstd carry themselves


def ln_param_tolerances(ref, rows, elem_tol=None):
    """Per-column tolerances of dgamma / dbeta / dbias of one add_ln_bwd launch over `rows` rows against ln_reference's sums:
        gamma(A + c) * sum_rows |term|,   A = ln_bwd_sum_adds(rows), c = the roundings that formed the term (LN_TERM_*).
    dbias sums rows of dx whose pieces cancel (gy g - s1 - xhat s2), so its magnitude is the sum of the pieces, rstd (|gy g| + mean|gy g| +
    |xhat| mean|gy g xhat|) >= |dx|.  elem_tol = (rtol, atol): the per-element gradient tolerance of the storage type, added once to dbias
    (bf16: the kernel normalises with the bf16 xhat it stored, the reference with the exact one)."""
    a = ln_bwd_sum_adds(rows)
    tol = dict(dbeta=gamma(a + LN_TERM_BETA) * ref["abs_beta"], dgamma=gamma(a + LN_TERM_GAMMA) * ref["abs_gamma"],
               dbias=gamma(a + LN_TERM_BIAS) * ref["abs_bias"])
    if elem_tol is not None:
        tol["dbias"] = tol["dbias"] + elem_tol[0] * ref["dbias"].abs() + elem_tol[1]
    return tol


def colsum_tolerance(x64, rows, cols, init=None):
    """Per-column tolerance of asr_colsum / asr_relu_bwd's dbias over the fp64 terms x64 (rows, cols): gamma(colsum_adds) * (sum|x| + |init|);
    the terms are stored values (exact in fp32), so nothing is added for forming them."""
    mag = x64.abs().sum(0)
    if init is not None:
        mag = mag + init.double().abs()
    return gamma(colsum_adds(rows, cols)) * mag


def colsum_emulate_f32(x, rows, cols):
    """asr_colsum of a contiguous fp32 (rows, cols) array in the kernel's order, in numpy fp32 (the lanes' accumulators, the four waves
    through LDS, the finalize pass); out starts at 0.  Only there to show that a correct fp32 implementation sits inside colsum_tolerance."""
    x = np.asarray(x, dtype=np.float32)
    slots = cs_row_slots(rows, cols)
    rs = slots * CS_WAVES
    acc = np.zeros((rs, cols), np.float32)
    for k in range(ceil_div(rows, rs)):
        blk = x[k * rs:(k + 1) * rs]
        acc[:blk.shape[0]] = acc[:blk.shape[0]] + blk
    a = acc.reshape(slots, CS_WAVES, cols)
    part = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
    s = np.zeros((32, cols), np.float32)
    for p0 in range(0, slots, 32):
        blk = part[p0:p0 + 32]
        s[:blk.shape[0]] = s[:blk.shape[0]] + blk
    t = np.zeros(cols, np.float32)
    for i in range(32):
        t = t + s[i]
    return t


# ------------------------------------------------------------------------------------------------ rows with a large mean
LARGE_MEAN_OFFSET = 1000.0      # chosen by tests/test_rowwise_ref_cpu.py::test_large_mean_offset_separates_the_two_variance_forms
LARGE_MEAN_ROWS = 48


def large_mean_rows(dtype, offset=LARGE_MEAN_OFFSET, rows=LARGE_MEAN_ROWS, d=512, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (offset + torch.randn(rows, d, generator=g)).to(dtype)


def _tree64(v):
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def _wave_row_sum(z):
    """(R, 512) fp32 -> (R,): a lane adds its 8 consecutive values in series, then the 64 lanes in a tree (wave_sum)."""
    zz = z.reshape(z.shape[0], 64, 8)
    s = np.zeros(zz.shape[:2], np.float32)
    for j in range(8):
        s = (s + zz[..., j]).astype(np.float32)
    return _tree64(s)


def ln_emulate_f32(x, one_pass):
    """xhat, rstd of add_ln_fwd_kernel<T, 8, true> (d = 512, no residual) in numpy fp32 with the kernel's summation order.
    one_pass = False: the kernel's form, the mean subtracted before squaring.  True: var = E[x^2] - mean^2, the form the kernel avoids."""
    f32 = np.float32
    z = np.asarray(x, dtype=f32)
    assert z.shape[1] == 512
    inv = f32(1.0) / f32(512.0)
    mean = (_wave_row_sum(z) * inv).astype(f32)
    c = (z - mean[:, None]).astype(f32)
    if one_pass:
        ex2 = (_wave_row_sum((z * z).astype(f32)) * inv).astype(f32)
        var = (ex2 - (mean * mean).astype(f32)).astype(f32)
    else:
        var = (_wave_row_sum((c * c).astype(f32)) * inv).astype(f32)
    with np.errstate(invalid="ignore"):
        rstd = (f32(1.0) / np.sqrt((var + f32(1e-5)).astype(f32))).astype(f32)
    return (c * rstd[:, None]).astype(f32), rstd


def large_mean_bounds(x, base_rtol, base_atol):
    """fp64 xhat, rstd of the rows x and the bounds the kernel is held to:
        |xhat - ref| <= base_atol + base_rtol |ref| + (8 + 6) u mean|z| rstd     (the fp32 error of the mean: 8 serial adds + 6 tree levels)
        |rstd / ref - 1| <= 2e-5 + ((8 + 6) u mean|z| rstd)^2 / 2                (a mean off by e adds e^2 to the variance, no more:
                                                                                  the deviations from the true mean sum to zero)"""
    x64 = x.double()
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + 1e-5) ** -0.5
    xhat = (x64 - mean) * rstd
    e = 14 * U32 * x64.abs().mean(1, keepdim=True) * rstd
    return xhat, rstd.reshape(-1), base_atol + base_rtol * xhat.abs() + e, (2e-5 + e * e / 2).reshape(-1)


# ------------------------------------------------------------------------------------------------ embedding
def embed_reference(ids, emb, pe, scale, To, mask=None):
    """fp64 embed_pe_fwd: out-of-range ids clamp to rows 0 / V - 1; scale as the C float the kernel receives."""
    V = emb.shape[0]
    idc = ids.long().clamp(0, V - 1)
    y = emb.double()[idc] * float(np.float32(scale)) + pe[:To].double().repeat(ids.numel() // To, 1)
    return y if mask is None else y * torch.as_tensor(mask, dtype=torch.float64)


def embed_bwd_reference(ids, dy, scale, V, mask=None, term_roundings=1):
    """fp64 index_add_ reference of embed_bwd and its per-element tolerance.  Out-of-range ids contribute nothing.
    An element of demb receives n addends g = dy * scale (* dropout scale): one rounding per product, then n - 1 adds in any order (atomics)
    or in token order (serial kernel): at most n + term_roundings - 1 roundings on a path, so
        |demb - ref| <= gamma(n + term_roundings - 1) * sum|addend|      (n * u * sum|addend| for term_roundings = 1, no dropout)
    and an element without addends keeps its value exactly."""
    ok = (ids >= 0) & (ids < V)
    idx = ids.long()[ok]
    g = dy.double()[ok] * float(np.float32(scale))
    if mask is not None:
        g = g * torch.as_tensor(mask, dtype=torch.float64)[ok]
    d = dy.shape[-1]
    ref = torch.zeros(V, d, dtype=torch.float64).index_add_(0, idx, g)
    mag = torch.zeros(V, d, dtype=torch.float64).index_add_(0, idx, g.abs())
    n = torch.zeros(V, dtype=torch.float64).index_add_(0, idx, torch.ones(idx.numel(), dtype=torch.float64))
    a = (n + term_roundings - 1).clamp(min=0).unsqueeze(1)
    return ref, a * U32 / (1 - a * U32) * mag


def dropout_scale_f32(p):
    """1.f / (1.f - p) as the kernels compute it (C floats), for references that must not count its rounding as an error."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
