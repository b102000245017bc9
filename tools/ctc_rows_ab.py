#!/usr/bin/env python3
"""Same bytes from two builds of the library: SHA-256 of every output of ctc_fwd_bwd, ctc_align, cr_ctc, softmax_rows and softmax_bwd_add
on seeded inputs - the tail, width and range (A, A50, F) cases of tests/ctc_range_cases.py, the dense shapes of tests/test_cr_ctc_gpu.py
and tests/test_interctc_gpu.py (with the block that begins one element into its allocation), and the workload shapes once each.

    bash tools/build_rev.sh <rev>
    python tools/ctc_rows_ab.py --parent build_ab/<rev>/asr_chinese_e2e_amd/libasr_hip.so [--out bits.json]

One fresh process per library (the parent's through ASR_HIP_LIB), ASR_DETERMINISTIC=1 (the f32 ctc_grad_kernel adds through LDS atomics by
default).  Exit status 1 if a hash differs."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CAP = 6144
DENSE = ([(R, T, V, None, 0) for R in (1, 3) for T in (1, 9) for V in (2, 5, 64, 257)] +
         [(1, 1, 4232, 4288, 0), (3, 9, 4232, 4288, 0), (1, 2, CAP, None, 0), (1, 2, CAP + 1, None, 0), (1, 2, CAP + 8, None, 0), (1, 2, 64, 72, 1)])
LENS9 = {1: [12, 9], 3: [9, 0, 1, 8, 0, 1]}                                            # tests/test_cr_ctc_gpu.py
LENS = {(1, 1): [1], (1, 9): [9], (3, 1): [0, 1, 1], (3, 9): [0, 1, 12], (1, 2): [2]}      # tests/test_interctc_gpu.py


def child(out_path):
    import numpy as np
    import torch
    from asr_chinese_e2e_amd import kernels as K
    from tests import cr_ctc_ref, ctc_range_cases as C, interctc_ref
    dev = "cuda"
    out = {}

    def sha(t):
        t = t.contiguous().cpu()
        return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()

    def i32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)

    def rows(x, ld, shift):
        """x (R, T, V) on the host -> (the device view [:, :, :V] of zero-padded rows ld apart, `shift` elements into the allocation, the block)"""
        R, T, V = x.shape
        ld = V if ld is None else ld
        flat = torch.zeros(R * T * ld + shift, dtype=x.dtype, device=dev)
        buf = flat[shift:].view(R, T, ld)
        buf[:, :, :V] = x.to(dev)
        return buf[:, :, :V], buf

    def ctc(name, logits, in_len, labels, lab_len, dtype, ld=None):
        x, _ = rows(torch.from_numpy(logits).to(dtype) if isinstance(logits, np.ndarray) else logits, ld, 0)
        il, lab, ll = i32(in_len), i32(labels), i32(lab_len)
        path = torch.full(x.shape[:2], -7, dtype=torch.int32, device=dev)
        dl, dbuf = rows(torch.zeros(x.shape, dtype=dtype), ld, 0)
        nll, _ = K.ctc_fwd_bwd(x, il, lab, ll, K.Workspace(dev), dlogits=dl, best_path=path)
        nll0, _ = K.ctc_fwd_bwd(x, il, lab, ll, K.Workspace(dev), want_grad=False)
        for k, t in (("nll", nll), ("dlogits", dbuf), ("best_path", path), ("nll_no_grad", nll0)):
            out[f"ctc_fwd_bwd/{name}/{k}"] = sha(t)
        for k, t in zip(("path", "spans", "token_logp", "score"), K.ctc_align(x, il, lab, ll)):
            out[f"ctc_align/{name}/{k}"] = sha(t)

    f32, bf16 = torch.float32, torch.bfloat16
    for dtype, V in ((f32, 16), (bf16, 64)):
        for kind, lmaxes, make in (("tail", C.TAIL_LMAX, C.tail_case), ("width", C.WIDTH_LMAX, C.width_case)):
            for Lmax in lmaxes:
                c = make(Lmax, V, dtype)
                ctc(f"{kind}{Lmax}/{dtype}", c.logits, c.in_len, c.labels, c.lab_len, dtype)
    for dtype in (f32, bf16):
        for name in ("A", "A50", "F"):
            c = C.range_case(name, dtype)
            ctc(f"range{name}/{dtype}", c.logits, c.in_len, c.labels, c.lab_len, dtype)
    for dtype in (f32, bf16):
        for R, T, V, ld, shift in DENSE:
            tag = f"{R}x{T}x{V}/ld{ld}+{shift}/{dtype}"
            logits, in_len = cr_ctc_ref.make_case(R, T, V, 1.0, LENS9[R] if T == 9 else None)
            x, _ = rows(torch.from_numpy(logits).to(dtype), ld, shift)
            for acc in (False, True):
                prior = torch.from_numpy(cr_ctc_ref.make_case(R, T, V, 1.0, seed=1)[0]).to(dtype) if acc else torch.zeros(2 * R, T, V, dtype=dtype)
                g, gbuf = rows(prior, ld, shift)
                o = K.cr_ctc(x, i32(in_len), grad_scale=0.37, dlogits=g, accumulate=acc)
                for k, t in (("cr", o["cr"]), ("frame", o["frame"]), ("dlogits", gbuf)):
                    out[f"cr_ctc/{tag}/acc{int(acc)}/{k}"] = sha(t)
            z, dp, prior, n = interctc_ref.make_case(R, T, V, 1.0, LENS[(R, T)])
            z, dp, prior = (torch.from_numpy(a).to(dtype) for a in (z, dp, prior))
            p, pbuf = rows(torch.zeros(R, T, V, dtype=dtype), ld, shift)
            K.softmax_rows(rows(z, ld, shift)[0], i32(n), out=p)
            out[f"softmax_rows/{tag}"] = sha(pbuf)
            for acc in (False, True):
                g, gbuf = rows(prior, ld, shift)
                K.softmax_bwd_add(p, rows(dp, ld, shift)[0], i32(n), g, accumulate=acc)
                out[f"softmax_bwd_add/{tag}/acc{int(acc)}"] = sha(gbuf)
    # the workload shapes, once each
    B, T, V, LD, L = 32, 500, 4232, 4288, 22
    gen = torch.Generator().manual_seed(0)
    x = (torch.randn(B, T, V, generator=gen) * 2).to(bf16)
    lab = torch.randint(4, V, (B, L), generator=gen, dtype=torch.int32).numpy()
    ll = torch.randint(8, L + 1, (B,), generator=gen, dtype=torch.int32).numpy()
    il = torch.randint(T * 3 // 5, T + 1, (B,), generator=gen, dtype=torch.int32).numpy()
    ctc("workload", x, il, lab, ll, bf16, ld=LD)
    two = torch.cat([x, (x.float() + 0.5 * torch.randn(B, T, V, generator=gen)).to(bf16)])
    g, gbuf = rows(torch.zeros(2 * B, T, V, dtype=bf16), LD, 0)
    o = K.cr_ctc(rows(two, LD, 0)[0], i32(np.concatenate([il, il])), grad_scale=0.2 / 32, dlogits=g)
    for k, t in (("cr", o["cr"]), ("frame", o["frame"]), ("dlogits", gbuf)):
        out[f"cr_ctc/workload/{k}"] = sha(t)
    del two, o, g, gbuf
    p, pbuf = rows(torch.zeros(B, T, V, dtype=bf16), LD, 0)
    K.softmax_rows(rows(x, LD, 0)[0], i32(il), out=p)
    out["softmax_rows/workload"] = sha(pbuf)
    dp = rows(torch.randn(B, T, V, generator=gen).to(bf16), LD, 0)[0]
    for acc in (False, True):
        g, gbuf = rows(x, LD, 0)
        K.softmax_bwd_add(p, dp, i32(il), g, accumulate=acc)
        out[f"softmax_bwd_add/workload/acc{int(acc)}"] = sha(gbuf)
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not os.path.isfile(a.parent):
        sys.exit(f"--parent {a.parent!r}: no such library (bash tools/build_rev.sh <rev>)")
    got = {}
    for side, lib in (("parent", os.path.abspath(a.parent)), ("new", "")):
        env = dict(os.environ, ASR_DETERMINISTIC="1")
        env.pop("ASR_HIP_LIB", None)
        if lib:
            env["ASR_HIP_LIB"] = lib
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, f"{side}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, check=True, timeout=600)
            got[side] = json.load(open(path))
    differing = sorted(k for k in set(got["parent"]) | set(got["new"]) if got["parent"].get(k) != got["new"].get(k))
    res = {"compared": len(got["new"]), "differing": differing, "sha256": got["new"]}
    line = json.dumps({"compared": res["compared"], "differing": differing})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(1 if differing or not got["new"] else 0)


if __name__ == "__main__":
    main()
