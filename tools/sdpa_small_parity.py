"""Error of the one-wave attention kernels (option "sdpa_small" = 1) and of the one-workgroup kernels they replace (= 0) against the fp64
reference of tests/test_sdpa_small_gpu.py, every case of that test: max |x - ref| / max |ref| per output.
python tools/sdpa_small_parity.py > profiles/sdpa_small_parity.txt"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asr_chinese_e2e_amd import kernels as K
from tests import test_sdpa_small_gpu as T
print(f"B={T.B} H={T.H} dk={T.DK}, k_len = (1, Tk, Tk // 2 + 1); relative to the largest element of the fp64 reference; old = sdpa_small 0, new = 1")
print(f"{'Tq':>3s} {'Tk':>3s} {'causal':>6s} {'rows':>5s} " + " ".join(f"{n + ' old':>10s} {n + ' new':>10s}" for n in ("o", "lse", "dq", "dk", "dv")))
worst = {}
for Tq, Tk, causal, layout in T.CASES:
    old, new, floor = T.measure(K, Tq, Tk, causal, layout)
    cells = []
    for n in ("o", "lse", "dq", "dk", "dv"):
        (eo, den), (en, _) = old[n], new[n]
        cells.append(f"{eo / den:10.3e} {en / den:10.3e}")
        if eo > 0:
            worst[n] = max(worst.get(n, 0.0), en / eo)
    print(f"{Tq:3d} {Tk:3d} {int(causal):6d} {layout:>5s} " + " ".join(cells), flush=True)
print("largest new / old ratio per output (cases with old > 0): " + ", ".join(f"{n} {r:.2f}" for n, r in worst.items()))
