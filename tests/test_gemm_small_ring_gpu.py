"""The small-M GEMM's register ring (gemm_small_kernel: four 256-deep k-steps in flight, bias / ReLU mask requested before the k-loop; tuning
option "gemm_small_ring", on by default) against the fp64 product of the same bf16 operands, and bit for bit against the two-step kernel
it stands in front of (option off).

Shapes: K covers every state of the ring - fewer k-steps than stages (nk = 1, 2, 3), exactly as many (4), one more (5), the loop's exit
into a tail of every length but four again (6, 7, 9, 17 steps: tails of 6, 7, 5, 5 after 0, 0, 1, 3 rounds), and a zero-padded partial last
step (8, 264, 1032, 2056, 4232); M and N cover one row, one short of / one past a tile and a third tile row, a single 8-column group, and tiles cut by N.
Leading dimensions are all larger than the rows they hold; rows past M and columns past N of the output buffer keep their sentinel.
Tolerance: the one tests/test_kernels_gpu.py::test_gemm_small uses, on operands drawn the same way."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = [8, 256, 264, 512, 768, 1024, 1032, 1280, 1536, 1792, 2056, 4232]
MS = [1, 63, 65, 130]
NS = [8, 72, 136]
PAD = 8
ACT_NONE, ACT_RELU, ACT_RELU_MASK = 0, 1, 2


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def extras():
    """bias, mask (+0, -0, negative and positive entries) and the sentinel-filled output buffer, shared by every case"""
    g = torch.Generator().manual_seed(11)
    bias = torch.randn(max(NS), generator=g).to(DEV)
    mask = torch.randn(max(MS), max(NS) + PAD, generator=g)
    mask[::3, ::5] = 0.0
    mask[1::4, 2::7] = -0.0
    sentinel = torch.full((max(MS) + 2, max(NS) + PAD), -777.0, dtype=torch.bfloat16, device=DEV)
    return bias, mask.bfloat16().to(DEV), sentinel


@pytest.mark.parametrize("trans_b", [False, True])
@pytest.mark.parametrize("K_", KS)
def test_ring_against_fp64_and_two_step_kernel(K, extras, K_, trans_b):
    bias, mask_buf, sentinel = extras
    g = torch.Generator().manual_seed(1000 * K_ + trans_b)
    a_buf = torch.randn(max(MS), K_ + PAD, generator=g).bfloat16().to(DEV)                                     # lda > K
    b_buf = ((torch.randn(K_, max(NS) + PAD, generator=g) if trans_b else torch.randn(max(NS), K_ + PAD, generator=g)) * 0.25).bfloat16().to(DEV)      # ldb padded
    a = a_buf[:, :K_]
    b_full = b_buf[:, :max(NS)] if trans_b else b_buf[:, :K_]
    ref_full = a.double() @ (b_full.double() if trans_b else b_full.double().t())                              # one reference for every (M, N)
    atol = 2e-2 * math.sqrt(K_ / 64)
    for M in MS:
        for N in NS:
            bm = b_full[:, :N] if trans_b else b_full[:N]
            for act in (ACT_NONE, ACT_RELU, ACT_RELU_MASK):
                for with_bias in (False, True):
                    ref = ref_full[:M, :N] + (bias[:N].double() if with_bias else 0.0)
                    mask = None
                    if act == ACT_RELU:
                        ref = ref.clamp_min(0)
                    elif act == ACT_RELU_MASK:
                        mask = mask_buf[:M, :N]
                        ref = torch.where(mask.double() > 0, ref, torch.zeros_like(ref))
                    outs = []
                    for ring in (1, 0):
                        buf = sentinel.clone()
                        prev = K.set_option("gemm_small_ring", ring)
                        try:
                            K.gemm_small(a[:M], bm, bias[:N] if with_bias else None, buf[:M, :N], trans_b=trans_b, act=act, mask=mask)      # ldc > N
                        finally:
                            K.set_option("gemm_small_ring", prev)
                        outs.append(buf)
                    what = f"gemm_small {M}x{N}x{K_} trans_b={trans_b} act={act} bias={with_bias}"
                    new, old = outs
                    assert torch.equal(new.view(torch.int16), old.view(torch.int16)), f"{what}: ring and two-step kernel differ"
                    assert torch.equal(new[M:].view(torch.int16), sentinel[M:].view(torch.int16)) and \
                        torch.equal(new[:M, N:].view(torch.int16), sentinel[:M, N:].view(torch.int16)), f"{what}: wrote outside C"
                    err = (new[:M, :N].double() - ref).abs()
                    bad = err > atol + 1e-2 * ref.abs()
                    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.3e} (ref max {float(ref.abs().max()):.3e})"
