"""A/B of the small-M GEMM's register ring (tuning option "gemm_small_ring": 1 = four k-steps in flight and bias / mask requested first,
0 = the two-step kernel) at the decoder's shapes: M = 736 rows, bias / activation as the joint step uses them (forward: bias, ReLU on w_1;
input gradient: no bias, ReLU mask on w_2's).  Each launch takes the next of enough operand sets that a set is not met again before 64 MB of other
operands went by (beyond the L2s, as in the step); HIP events around blocks of launches made through the vectorcall trampolines (the host
stays ahead of the GPU), the two option values alternated block by block, the median block of each reported.
python tools/small_gemm_ab.py > profiles/small_ring_small_gemm_ab.txt"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from asr_chinese_e2e_amd import kernels as K, _lib
M = int(os.environ.get("M", "736"))
BLOCK, ROUNDS = 200, 7
ACT_NONE, ACT_RELU, ACT_RELU_MASK = 0, 1, 2
fast, st = _lib.fast, K._stream()
print(f"M={M}; us per launch, median of {ROUNDS} blocks of {BLOCK} launches per option value, alternated")
print(f"{'N':>5s} {'K':>5s} {'TB':>2s} {'act':>4s} {'bias':>4s} {'sets':>4s} {'ring=0':>8s} {'ring=1':>8s} {'gain':>7s}")
for tb in (False, True):
    for N, Kd in ((512, 512), (1536, 512), (1024, 512), (512, 1024), (512, 1536), (512, 4232)):
        act = (ACT_RELU_MASK if tb else ACT_RELU) if (N, Kd) == (1024, 512) else ACT_NONE
        set_bytes = 2 * (M * Kd + N * Kd + M * N * (2 if act == ACT_RELU_MASK else 1))
        nset = max(4, -(-(64 << 20) // set_bytes))
        calls = []
        keep = []
        for _ in range(nset):
            a = torch.randn(M, Kd, device="cuda").bfloat16()
            b = ((torch.randn(Kd, N, device="cuda") if tb else torch.randn(N, Kd, device="cuda")) * 0.05).bfloat16()
            bias = None if tb else torch.randn(N, device="cuda")
            mask = torch.randn(M, N, device="cuda").bfloat16() if act == ACT_RELU_MASK else None
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
            keep.append((a, b, bias, mask, out))
            calls.append((K._p(a), K._p(b), K._p(bias), K._p(mask), K._p(out), M, N, Kd, Kd, N if tb else Kd, N, int(tb), act, st))
        def block():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(BLOCK):
                rc = fast.asr_gemm_small_bf16(*calls[i % nset])
                assert rc == 0, rc
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / BLOCK * 1e3
        t = {0: [], 1: []}
        for rnd in range(ROUNDS + 1):
            for ring in (0, 1):
                prev = K.set_option("gemm_small_ring", ring)
                try:
                    x = block()
                finally:
                    K.set_option("gemm_small_ring", prev)
                if rnd: t[ring].append(x)      # round 0 warms up
        m0, m1 = sorted(t[0])[ROUNDS // 2], sorted(t[1])[ROUNDS // 2]
        print(f"{N:5d} {Kd:5d} {int(tb):2d} {act:4d} {int(not tb):4d} {nset:4d} {m0:8.2f} {m1:8.2f} {100 * (m0 - m1) / m0:6.1f}%", flush=True)
