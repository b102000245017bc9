"""Case tables, exact operand builders, int64 references and host-arithmetic restatements for the bf16 NT GEMM (asr_gemm_nt_bf16) and the
weight-gradient GEMMs (asr_gemm_tn_bias_bf16, asr_gemm_tn_grouped_bf16): shared by tests/test_gemm_states_cpu.py (which proves which
state of the kernels every case reaches, and that the checker would see a defect) and tests/test_gemm_states_gpu.py (which runs them).

Exact operands.  NT: A in {-1, 0, 1} with at most 32 non-zeros per row, W in {-2 .. 2}, integer bias and residual: every product,
product + bias and (+ res) is an integer of magnitude <= 256, so it is a bf16 value, every fp32 partial sum is exact and neither the
order nor the number of roundings inside a kernel can matter - the output must equal the integer product bit for bit.  TN: dY and X in
{-4 .. 4}, dW / dbias start from integers, every partial sum stays below 2^24: fp32 addition is exact and order-independent, so the
atomic mode, the deterministic slab mode, the multi launch and the grouped kernel must all equal the integer product.
(The products are formed in fp64, where they are exact - every value is an integer far below 2^53 - and held as int64.)

Poisoned surroundings.  Every operand is a view into a larger buffer whose columns behind K (A, W, X), behind N (dY, res, mask, bias)
and rows behind M hold NaN; output buffers carry a sentinel outside [:M, :N] (NT) / [:N, :K] (TN) that must survive bit for bit.

The restatements (nt_branch, nt_walk, tn_plan, tn_stagger, tn_ranges, tn_multi_plan, tn_grouped_plan) mirror the host code of
csrc/gemm.hip with the CU count as a parameter.  Their only job is to prove which state a case reaches; no expected value of a GPU test
comes from them."""
import collections

import torch

ACT_NONE, ACT_RELU, ACT_RELU_MASK = 0, 1, 2
DEVICE_CUS = 256      # MI355X; also what cu_count() falls back to without a device
PAD = 8               # every leading dimension is larger than its row by this much unless a case says otherwise
TM = 64               # reduction rows per stage of the weight-gradient kernels


def ceil_div(a, b):
    return (a + b - 1) // b


def cu_count(limit, device=DEVICE_CUS):
    """gemm.hip cu_count(): option "cu_limit" (> 0, below the device's count, floor 8), else the device's CUs"""
    return max(limit, 8) if 0 < limit < device else device


# ======================================================================================================= NT: restatements
def nt_branch(M, N, K, ldc, act, bias, res, c_off_bytes=0):
    """The dispatch ladder of asr_gemm_nt_bf16 (buffers here are 16-byte aligned, so only C's offset can break the alignment)."""
    rows16 = N % 8 == 0 and ldc % 8 == 0 and c_off_bytes % 16 == 0
    if act == ACT_RELU_MASK:
        return "persistent:mask" if (res and K % 64 == 0 and K >= 128 and rows16 and not bias) else "refused"
    if res and act == ACT_NONE and not bias and K % 64 == 0 and K >= 128 and rows16:
        return "persistent:res"
    if K % 64 != 0 and K > 64 and not res and act == ACT_NONE and rows16:
        return "persistent:ragged"
    if K % 64 == 0 and K >= 128 and not res and rows16:
        return "persistent:relu" if act == ACT_RELU else "persistent:plain"
    return "all_in_one"


NtWalk = collections.namedtuple("NtWalk", "ntiles grid nk shares my_tiles trem full_tiles partial_tiles")


def nt_walk(M, N, K, cus):
    """launch_nt_spec + the tile-list arithmetic at the top of gemm_nt_spec_kernel: tiles per XCD (shares), tiles per workgroup (my_tiles)."""
    t_n, t_m = ceil_div(N, 128), ceil_div(M, 256)
    ntiles = t_n * t_m
    grid = min(ntiles, cus)
    nk = ceil_div(K, 64)
    tq, trem = ntiles >> 3, ntiles & 7
    shares = [tq + (1 if x < trem else 0) for x in range(8)]
    my_tiles = []
    for b in range(grid):
        xcd, idx = b & 7, b >> 3
        nb_x = (grid - xcd + 7) >> 3
        lo = xcd * tq + min(xcd, trem)
        hi = lo + shares[xcd]
        first = lo + idx
        my_tiles.append(0 if first >= hi else (hi - first + nb_x - 1) // nb_x)
    full = sum(1 for tm in range(t_m) for tn in range(t_n) if tm * 256 + 256 <= M and tn * 128 + 128 <= N)
    return NtWalk(ntiles, grid, nk, shares, my_tiles, trem, full, ntiles - full)


# ======================================================================================================= NT: case tables
# act, bias, res ("res": its own buffer, "inplace": res is out); ldc / c_off: None = N + PAD / 0
NtCase = collections.namedtuple("NtCase", "table M N K act bias res limit ldc c_off branch")


def _nt(table, M, N, K, mode, limit, ldc=None, c_off=0, branch=None):
    act, bias, res = {"plain": (ACT_NONE, False, None), "bias": (ACT_NONE, True, None), "relu": (ACT_RELU, False, None),
                      "relu_bias": (ACT_RELU, True, None), "mask": (ACT_RELU_MASK, False, "res"), "res": (ACT_NONE, False, "res"),
                      "res_inplace": (ACT_NONE, False, "inplace"), "bias_res": (ACT_NONE, True, "res"),
                      "relu_bias_res": (ACT_RELU, True, "res")}[mode]
    return NtCase(table, M, N, K, act, bias, res, limit, ldc, c_off, branch)


NT_RING_T = [1, 3, 8, 9, 17, 20]
NT_RING_K = [128, 192, 256, 320, 448]      # nk = 2, 3, 4, 5, 7
NT_RAGGED_K = [72, 136, 200]               # nk = 2, 3, 4, the last k-step of 8 columns
NT_RING_LIMITS = [8, 16]
NT_TAILS = ["relu_bias", "mask", "res", "res_inplace"]


def nt_ring_cases():
    """The 3-slot ring across tile boundaries: N = 128, M = 256 t - 37 (t tiles, the last one partial), under cu_limit 8 and 16"""
    out = []
    for limit in NT_RING_LIMITS:
        for t in NT_RING_T:
            for K in NT_RING_K + NT_RAGGED_K:
                out.append(_nt("ring", 256 * t - 37, 128, K, "bias", limit))
        for t in (3, 9, 20):
            for K in (128, 192, 256):
                for mode in NT_TAILS:
                    out.append(_nt("ring", 256 * t - 37, 128, K, mode, limit))
        for mode in ("bias", "mask"):      # two tile columns
            out.append(_nt("ring", 256 * 9 - 37, 256, 320, mode, limit))
    return out


def nt_edge_cases():
    """One row, one row short of / past a tile; one 8-column group, a last tile of 8 columns; every store tail; the whole device"""
    return [_nt("edge", M, N, K, mode, 0) for M in (1, 8, 255, 256, 257) for N in (8, 120, 128, 136, 264) for K in (128, 192)
            for mode in ["bias"] + NT_TAILS]


def nt_ladder_cases():
    """One case per branch of asr_gemm_nt_bf16; `branch` is what nt_branch must return (tests/test_gemm_states_cpu.py asserts it)."""
    return [
        # act == ASR_ACT_RELU_MASK: the mask in res, K % 64 == 0, K >= 128, 16-byte rows
        _nt("ladder", 300, 136, 128, "mask", 0, branch="persistent:mask"),
        # res && act == NONE && !bias && K % 64 == 0 && K >= 128 && rows16
        _nt("ladder", 300, 136, 192, "res", 0, branch="persistent:res"),
        # K % 64 != 0 && K > 64 && !res && act == NONE && rows16: ragged last k-step, with and without a bias
        _nt("ladder", 300, 136, 200, "bias", 0, branch="persistent:ragged"),
        _nt("ladder", 300, 136, 72, "plain", 0, branch="persistent:ragged"),
        # K % 64 == 0 && K >= 128 && !res && rows16: plain and ReLU
        _nt("ladder", 300, 136, 128, "plain", 0, branch="persistent:plain"),
        _nt("ladder", 300, 136, 128, "relu", 0, branch="persistent:relu"),
        # the all-in-one kernel, reason: K < 128 (one k-step)
        _nt("ladder", 300, 136, 64, "relu_bias", 0, branch="all_in_one"),
        # the all-in-one kernel, reason: ragged K with ReLU
        _nt("ladder", 300, 136, 200, "relu_bias", 0, branch="all_in_one"),
        _nt("ladder", 300, 136, 200, "relu", 0, branch="all_in_one"),
        # the all-in-one kernel, reason: ragged K with a residual
        _nt("ladder", 300, 136, 200, "res", 0, branch="all_in_one"),
        # the all-in-one kernel, reason: bias together with res
        _nt("ladder", 300, 136, 128, "bias_res", 0, branch="all_in_one"),
        _nt("ladder", 300, 136, 128, "relu_bias_res", 0, branch="all_in_one"),
        # the all-in-one kernel, reason: N (and ldc) not a multiple of 8 - the scalar store tail (n + 3 >= N) of 1, 2 and 3 columns
        _nt("ladder", 130, 129, 128, "relu_bias_res", 0, ldc=132, branch="all_in_one"),
        _nt("ladder", 130, 130, 128, "bias", 0, ldc=132, branch="all_in_one"),
        _nt("ladder", 130, 131, 128, "bias_res", 0, ldc=132, branch="all_in_one"),
        # the all-in-one kernel, reason: C starts 8 bytes off a 16-byte boundary
        _nt("ladder", 300, 136, 128, "bias", 0, c_off=8, branch="all_in_one"),
    ]


def nt_cases():
    return nt_ring_cases() + nt_edge_cases() + nt_ladder_cases()


def nt_ldc(c):
    """Row stride of C (and res): N + PAD unless the case sets it; a C that starts c_off bytes into its row keeps rows of a multiple of 8"""
    return (c.N + PAD if c.ldc is None else c.ldc) + (8 if c.c_off else 0)


NT_MAX_M, NT_MAX_N = 256 * 20 - 37, 264
NT_NNZ = 32


# ======================================================================================================= NT: operands, reference
def nt_a(M, K):
    """(M, K) int64 in {-1, 0, 1}: row m has its non-zeros at (7 m + 13 i) % K, i < 32 - between them the rows hit every 8-element chunk of every k-step"""
    m = torch.arange(M).unsqueeze(1)
    i = torch.arange(NT_NNZ).unsqueeze(0)
    a = torch.zeros(M, K, dtype=torch.int64)
    a.scatter_(1, (7 * m + 13 * i) % K, torch.where((m + i) % 3 == 0, -1, 1).expand(M, NT_NNZ).contiguous())
    return a


def nt_w(N, K):
    """(N, K) int64 in {-2 .. 2}: seeded draws - no symmetry in (n, k), no two rows or columns alike"""
    return torch.randint(-2, 3, (N, K), generator=torch.Generator().manual_seed(1000 + K))


def nt_bias(N):
    return (5 * torch.arange(N)) % 129 - 64                                    # [-64, 64]


def nt_res(M, N):
    m = torch.arange(M).unsqueeze(1)
    n = torch.arange(N).unsqueeze(0)
    return (3 * m + 11 * n + m // 32) % 201 - 100                              # [-100, 100]


def nt_mask(M, N):
    """(M, N) float in {-2 .. 2}; half of its zeros are -0.0 (a ReLU output is never negative, but the kernel tests sign and magnitude)"""
    m = torch.arange(M).unsqueeze(1)
    n = torch.arange(N).unsqueeze(0)
    v = ((3 * m + 7 * n + m // 8) % 5 - 2).float()
    return torch.where((v == 0) & ((m + n) % 2 == 1), torch.tensor(-0.0), v)


def exact_matmul_nt(a, w):
    """a (M, K) @ w (N, K)^T of small integers, int64: formed in fp64, where it is exact"""
    p = a.double() @ w.double().t()
    assert float(p.abs().max()) < 2.0 ** 52
    q = p.to(torch.int64)
    assert torch.equal(q.double(), p)
    return q


NT_BOUND = 256


def nt_reference(prod, act, bias, res_or_mask):
    """int64 result of one case from the int64 product prod (M, N); asserts that every intermediate is a bf16 integer (|x| <= 256)"""
    M, N = prod.shape

    def bounded(x):
        assert int(x.abs().max()) <= NT_BOUND, f"intermediate of magnitude {int(x.abs().max())} is not exact in bf16"
        return x
    x = bounded(prod)
    if act == ACT_RELU_MASK:
        return torch.where(res_or_mask > 0, x, torch.zeros_like(x))
    if bias is not None:
        x = bounded(x + bias)
    if act == ACT_RELU:
        x = x.clamp_min(0)
    if res_or_mask is not None:
        x = bounded(x + res_or_mask)
    return x


class NtData:
    """Operands and products shared by every NT case of a module: one A (NT_MAX_M, K), W (NT_MAX_N, K) and product per K (a case takes the
    leading rows), bias / res / mask once.  Built on the CPU; `dev` copies live on the device the cases run on."""

    def __init__(self, dev="cpu"):
        self.dev = dev
        self.prod, self.a, self.w = {}, {}, {}
        self.bias = nt_bias(NT_MAX_N)
        self.res = nt_res(NT_MAX_M, NT_MAX_N)
        self.mask = nt_mask(NT_MAX_M, NT_MAX_N)
        self.d_bias = self.bias.float().to(dev)
        self.d_res = self.res.bfloat16().to(dev)
        self.d_mask = self.mask.bfloat16().to(dev)

    def of_k(self, K):
        if K not in self.prod:
            a, w = nt_a(NT_MAX_M, K), nt_w(NT_MAX_N, K)
            self.prod[K] = exact_matmul_nt(a, w)
            self.a[K], self.w[K] = a.bfloat16().to(self.dev), w.bfloat16().to(self.dev)
        return self.a[K], self.w[K], self.prod[K]

    def reference(self, c):
        prod = self.of_k(c.K)[2][:c.M, :c.N]
        extra = None if c.res is None else (self.mask if c.act == ACT_RELU_MASK else self.res)[:c.M, :c.N]
        return nt_reference(prod, c.act, self.bias[:c.N] if c.bias else None, extra)

    def operands(self, c):
        """(a, w, bias, res, out, init): views into NaN-poisoned buffers and the sentinel-filled output buffer with a copy of its initial
        state.  res is out for an in-place case."""
        dev, nan = self.dev, float("nan")
        a_full, w_full, _ = self.of_k(c.K)
        M, N, K = c.M, c.N, c.K
        ldc, off = nt_ldc(c), c.c_off // 2
        abuf = torch.full((M + 2, K + PAD), nan, dtype=torch.bfloat16, device=dev)
        abuf[:M, :K] = a_full[:M]
        wbuf = torch.full((N + 2, K + PAD), nan, dtype=torch.bfloat16, device=dev)
        wbuf[:N, :K] = w_full[:N]
        bias = None
        if c.bias:
            bbuf = torch.full((N + 4,), nan, dtype=torch.float32, device=dev)
            bbuf[:N] = self.d_bias[:N]
            bias = bbuf[:N]
        cbuf = torch.full((M + 2, ldc), SENTINEL_BF16, dtype=torch.bfloat16, device=dev)
        out = cbuf[:M, off:off + N]
        res = None
        if c.res == "inplace":
            out.copy_(self.d_res[:M, :N])
            res = out
        elif c.res is not None:
            rbuf = torch.full((M + 2, ldc), nan, dtype=torch.bfloat16, device=dev)
            res = rbuf[:M, off:off + N]
            res.copy_((self.d_mask if c.act == ACT_RELU_MASK else self.d_res)[:M, :N])
        return abuf[:M, :K], wbuf[:N, :K], bias, res, out, (cbuf, cbuf.clone(), off)


SENTINEL_BF16 = -776.0      # a bf16 value no case produces (results stay within 256)
SENTINEL_F32 = -7777.25


# ======================================================================================================= the checker
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_exact(buf, init, ref, rows, cols, col_off=0, what=""):
    """buf: the whole output buffer after the call, init: a copy of it from before.  buf[:rows, col_off : col_off + cols] must hold the
    integers of ref (int64) bit for bit in buf's number format, and every other element of buf its initial bits."""
    assert buf.shape == init.shape and ref.shape == (rows, cols) and ref.dtype == torch.int64
    want = init.clone()
    want[:rows, col_off:col_off + cols] = ref.to(buf.device).to(buf.dtype)
    assert torch.equal(want[:rows, col_off:col_off + cols].to(torch.int64).cpu(), ref.cpu()), f"{what}: reference not representable"
    bad = _bits(buf) != _bits(want)
    if bool(bad.any()):
        inside = torch.zeros_like(bad)
        inside[:rows, col_off:col_off + cols] = True
        n_in, n_out = int((bad & inside).sum()), int((bad & ~inside).sum())
        r, c = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {n_in} of {rows * cols} results differ from the integer product, {n_out} elements outside the output "
                             f"were written; first at buffer [{r}, {c}]: got {float(buf[r, c])}, want {float(want[r, c])}")


# ======================================================================================================= TN: restatements
def tn_plan(M, N, K, cus):
    """gemm.hip tn_plan(): (ring, rows_per_split, nsplit)"""
    tiles = ceil_div(N, 128) * ceil_div(K, 128)
    max_s = ceil_div(M, 4 * TM)
    s_floor = cus // tiles if cus // tiles > 0 else 1
    if tiles * s_floor * 5 >= cus * 4:
        splits, ring = s_floor, 3
    else:
        splits, ring = ((2 * cus) // tiles if ceil_div(2 * cus, tiles) > 1 else 1), 2
    splits = max(1, min(splits, max_s))
    rows_per_split = ceil_div(ceil_div(M, splits), TM) * TM
    return ring, rows_per_split, ceil_div(M, rows_per_split)


def tn_stagger(M, rows_per_split, nsplit):
    """gemm.hip tn_stagger(): (r0, skew, why) - why names the condition on which the stagger was declined, or is "staggered" / "fewer than 3 splits" """
    if nsplit < 3:
        return rows_per_split, 0, "fewer than 3 splits"
    sk = (rows_per_split * 50 // 100 // (nsplit - 1)) // TM * TM
    tri = nsplit * (nsplit - 1) // 2
    r = ceil_div(ceil_div(M - sk * tri if M - sk * tri > 0 else M, nsplit), TM) * TM
    if sk <= 0:
        return rows_per_split, 0, "declined: skew below one stage"
    if r < 4 * TM:
        return rows_per_split, 0, "declined: first split below 4 stages"
    if r * (nsplit - 1) + sk * ((nsplit - 1) * (nsplit - 2) // 2) >= M:
        return rows_per_split, 0, "declined: last split would start behind M"
    return r, sk, "staggered"


def tn_ranges(M, nsplit, r0, skew):
    """[mbeg, mend) of every split, as gemm_tn_dma_kernel / gemm_tn_multi_kernel compute them"""
    out = []
    for s in range(nsplit):
        mbeg = s * r0 + skew * (s * (s - 1) // 2)
        out.append((mbeg, min(M, mbeg + r0 + skew * s)))
    return out


TnState = collections.namedtuple("TnState", "ring nsplit r0 skew why ranges")


def tn_state(M, N, K, cus):
    ring, rps, nsplit = tn_plan(M, N, K, cus)
    r0, skew, why = tn_stagger(M, rps, nsplit)
    return TnState(ring, nsplit, r0, skew, why, tn_ranges(M, nsplit, r0, skew))


def tn_multi_plan(shapes, cus, option=1):
    """tn_multi_launch(): None when the group goes to the grouped kernel, else (nsplit, r0, skew, why, ranges).  shapes: [(M, N, K)]"""
    M = shapes[0][0]
    if not option or len(shapes) > 4 or M < 4096 or any(s[0] != M for s in shapes):
        return None
    tiles = sum(ceil_div(n, 128) * ceil_div(k, 128) for _, n, k in shapes)
    max_s = ceil_div(M, 4 * TM)
    splits = max(1, min(cus // tiles, max_s))
    if tiles * splits * 5 < cus * 4 and splits < max_s:
        return None
    rps = ceil_div(ceil_div(M, splits), TM) * TM
    nsplit = ceil_div(M, rps)
    r0, skew, why = tn_stagger(M, rps, nsplit)
    return nsplit, r0, skew, why, tn_ranges(M, nsplit, r0, skew)


def tn_grouped_plan(shapes, cus):
    """The R search of asr_gemm_tn_grouped_bf16: (R, [[(mbeg, mend)] per problem])"""
    tiles = [ceil_div(n, 256) * ceil_div(k, 128) for _, n, k in shapes]
    work = sum(t * m for t, (m, _, _) in zip(tiles, shapes))
    max_m = max(m for m, _, _ in shapes)
    R = max(ceil_div(ceil_div(work, cus), TM) * TM, 4 * TM)
    while True:
        blocks = sum(t * ceil_div(m, R) for t, (m, _, _) in zip(tiles, shapes))
        if blocks <= cus or R >= max_m:
            break
        R += TM
    ranges = []
    for m, _, _ in shapes:
        rps = min(R, m)
        ranges.append([(s * rps, min(m, s * rps + rps)) for s in range(ceil_div(m, R))])
    return R, ranges


# ======================================================================================================= TN: case tables
TN_LIMITS = [0, 8]
# nsteps 1 .. 4 in a single split, ragged or not: a prologue shorter than either ring (2 or 3 slots), exactly as long, longer
TN_STAGE_SHAPES = [(M, 128, 128) for M in (1, 63, 64, 65, 128, 129, 192, 200, 256)] + \
    [(M, 384, 128) for M in (1, 64, 129, 200)]      # three tiles: the two-slot ring under cu_limit = 8
# (M, N, K): what each reaches under the whole device and under cu_limit = 8 is asserted in tests/test_gemm_states_cpu.py
TN_SPLIT_SHAPES = [
    (400, 128, 128),       # two splits (256 + 144 rows)
    (577, 128, 128),       # three splits; the stagger would start below 4 stages (declined)
    (1600, 256, 128),      # 8 CUs: 4 splits, r0 = 320, skew = 64 (320, 384, 448, 448 rows); 256 CUs: 7 splits, skew below one stage (declined)
    (1400, 384, 128),      # 8 CUs: ring 2 (3 tiles x 2 = 6 of 8 CUs), 5 splits; 256 CUs: ring 3, 6 splits
    (1540, 128, 128),      # 7 splits of 256, the last of 4 rows (shorter than one stage)
    (1300, 1160, 1032),    # 256 CUs: 90 tiles -> ring 2, 5 splits, the last of 20 rows; 8 CUs: ring 3, one split
    (1600, 1016, 1024),    # 256 CUs: 64 tiles x 4 staggered splits
    (3100, 136, 72),       # 256 CUs: 2 tiles x 13 splits; 8 CUs: 4 staggered splits, ragged last stage, clamped edge columns
]
TN_TAIL_SHAPES = [(200, N, K) for N in (8, 136) for K in (8, 72, 136)]


def tn_shapes():
    return TN_STAGE_SHAPES + TN_SPLIT_SHAPES + TN_TAIL_SHAPES


# grouped launches: [(M, N, K, with_dbias)]
TN_GROUPS = {
    "multi": [(4100, 128, 128, True), (4100, 256, 128, False)],            # same M >= 4096, small N and K: the multi launch (whole device)
    "multi_staggered": [(4100, 128, 128, False), (4100, 120, 72, True)],     # two tiles: qualifies under cu_limit = 8 too, 4 staggered splits there
    "grouped": [(300, 136, 72, True), (1000, 128, 264, False), (70, 8, 8, True)],      # different M: the 256 x 128-tile grouped kernel
}
TN_MAX_M, TN_MAX_N, TN_MAX_K = 4100, 1160, 1032
TN_BOUND = 1 << 24


# ======================================================================================================= TN: operands, reference
def tn_dy(M, N):
    """(M, N) int64 in {-4 .. 4}, seeded draws; a case takes leading rows and columns of the largest"""
    return torch.randint(-4, 5, (TN_MAX_M, TN_MAX_N), generator=torch.Generator().manual_seed(31))[:M, :N]


def tn_x(M, K):
    return torch.randint(-4, 5, (TN_MAX_M, TN_MAX_K), generator=torch.Generator().manual_seed(37))[:M, :K]


def tn_dw0(N, K):
    n = torch.arange(N).unsqueeze(1)
    k = torch.arange(K).unsqueeze(0)
    return (13 * n + 29 * k) % 2001 - 1000


def tn_db0(N):
    return (17 * torch.arange(N)) % 501 - 250


def tn_reference(dy, x, dw0=None, db0=None):
    """(dW, dbias) int64: dw0 + dy^T x and db0 + column sums of dy; asserts that no partial sum can reach 2^24 (the sum of the magnitudes
    bounds every partial sum in every order)"""
    M = dy.shape[0]
    p = dy.double().t() @ x.double()
    worst = dy.double().abs().t() @ x.double().abs()
    start = 0 if dw0 is None else int(dw0.abs().max())
    assert float(worst.max()) + start < TN_BOUND, f"partial sums up to {float(worst.max()) + start} are not exact in fp32"
    q = p.to(torch.int64)
    assert torch.equal(q.double(), p)
    col = dy.sum(0)
    assert int(dy.abs().sum(0).max()) + (0 if db0 is None else int(db0.abs().max())) < TN_BOUND
    return (q if dw0 is None else q + dw0), (col if db0 is None else col + db0)


class TnData:
    """dY (TN_MAX_M, TN_MAX_N) and X (TN_MAX_M, TN_MAX_K) once; a case takes leading rows and columns.  Products per (M, N, K) are cached."""

    def __init__(self, dev="cpu"):
        self.dev = dev
        self.dy, self.x = tn_dy(TN_MAX_M, TN_MAX_N), tn_x(TN_MAX_M, TN_MAX_K)
        self.dw0, self.db0 = tn_dw0(TN_MAX_N, TN_MAX_K), tn_db0(TN_MAX_N)
        self.d_dy, self.d_x = self.dy.bfloat16().to(dev), self.x.bfloat16().to(dev)
        self.d_dw0, self.d_db0 = self.dw0.float().to(dev), self.db0.float().to(dev)
        self._ref = {}

    def reference(self, M, N, K, accumulate):
        """(dW, dbias) int64; dbias always accumulates onto its start value, dW only when `accumulate`"""
        key = (M, N, K)
        if key not in self._ref:
            tn_reference(self.dy[:M, :N], self.x[:M, :K], self.dw0[:N, :K], self.db0[:N])      # the bound, with the start values
            self._ref[key] = tn_reference(self.dy[:M, :N], self.x[:M, :K])
        dw, db = self._ref[key]
        return (dw + self.dw0[:N, :K] if accumulate else dw), db + self.db0[:N]

    def operands(self, M, N, K, accumulate, with_dbias):
        """(dy, x, dw, dbias, wbuf, winit, bbuf, binit): NaN behind N / K / M of the operands; the dW buffer holds its integer start values
        (accumulate) or NaN (overwrite) inside and the sentinel outside; dbias likewise, in a longer vector"""
        dev, nan = self.dev, float("nan")
        ybuf = torch.full((M + 2, N + PAD), nan, dtype=torch.bfloat16, device=dev)
        ybuf[:M, :N] = self.d_dy[:M, :N]
        xbuf = torch.full((M + 2, K + PAD), nan, dtype=torch.bfloat16, device=dev)
        xbuf[:M, :K] = self.d_x[:M, :K]
        wbuf = torch.full((N + 2, K + PAD), SENTINEL_F32, dtype=torch.float32, device=dev)
        if accumulate:
            wbuf[:N, :K] = self.d_dw0[:N, :K]
        else:
            wbuf[:N, :K] = nan
        bbuf = binit = dbias = None
        if with_dbias:
            bbuf = torch.full((1, N + 4), SENTINEL_F32, dtype=torch.float32, device=dev)
            bbuf[0, :N] = self.d_db0[:N]
            binit = bbuf.clone()
            dbias = bbuf[0, :N]
        return ybuf[:M, :N], xbuf[:M, :K], wbuf[:N, :K], dbias, wbuf, wbuf.clone(), bbuf, binit
