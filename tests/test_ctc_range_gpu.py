"""The CTC lattice kernels (asr_ctc_fwd_bwd, asr_ctc_align) where the scaled linear-domain lattice is not enough, and at its edges.

Range: blank-dominated posteriors with long label sequences (tests/ctc_range_cases.py; tests/test_ctc_range_cpu.py shows from the
oracle alone that their final states and frame posteriors lie below exp(-745) of the column maxima).  Loss and gradient against
oracle.ctc_ref.ctc_batch (log domain, fp64) on the rounded logits, with torch's fp64 F.ctc_loss as a second opinion, at test_ctc's
tolerances; the alignment against the fp64 Viterbi restatement of tests/test_ctc_align_cpu.py at test_ctc_align_gpu's tolerances.

Edges: full lattice rows and the first Lmax of the next row width (Lmax = 31, 32, 63, 64, 127, 128, 255: the carries between a lane's
registers, the half-wave maximum), and input lengths around the boundaries between the steady state of the recursion's prefetch and
its clamped tail, on plain random logits.

With the scaled linear lattice alone (the parent commit's library on the MI355X) the widths, the tails, the refusals and batch D
passed, and every hazard utterance failed: batches A, A50, B, C, E gave nll = +inf (0 with zero_infinity; oracle 981.1, 967.1, 766.4,
2478.7, 817.6) with an all-zero gradient (max error 0.46 to 1.0), and their alignments were refused (score -inf); batch F gave a
finite nll of 1070.9987 against 1067.4708, the plain softmax (fp32) or NaN (bf16) as the gradient of its middle frames, and an alignment
of score -1100.82 against the best path's -1094.99."""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ctc_ref  # noqa: E402
from tests import ctc_range_cases as C  # noqa: E402
from tests.test_ctc_align_cpu import collapse, log_softmax, rescore, viterbi_ref  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
NLL_TOL = dict(rtol=1e-4, atol=1e-4)                                                # test_ctc's
GRAD_TOL = {F32: dict(rtol=1e-3, atol=2e-5), BF16: dict(rtol=1e-2, atol=4e-3)}      # test_ctc's

@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def ws(K):
    return K.Workspace(DEV)


def close(a, b, rtol, atol, what=""):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    err = (a - b).abs()
    bad = ~(err <= atol + rtol * b.abs())       # a NaN is off
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err[~err.isnan()].max()):.3e} (ref max {float(b.abs().max()):.3e})"


def dev(a):
    return torch.from_numpy(np.asarray(a)).int().to(DEV)


class Ref:
    """Loss and gradient of one batch from the oracle (zero_infinity semantics: 0 and a zero gradient for an infeasible utterance),
    confirmed by torch's fp64 CTC.  Computed once per batch and dtype and never written to."""

    def __init__(self, c):
        self.nll, self.grad = ctc_ref.ctc_batch(c.logits.astype(np.float64), c.in_len, c.labels, c.lab_len, zero_infinity=True)
        x = torch.from_numpy(c.logits).double().requires_grad_(True)
        tn = F.ctc_loss(F.log_softmax(x, -1).transpose(0, 1), torch.from_numpy(c.labels), torch.from_numpy(c.in_len),
                        torch.from_numpy(c.lab_len), blank=0, reduction="none", zero_infinity=True)
        tn.sum().backward()
        assert np.allclose(self.nll, tn.detach().numpy(), rtol=1e-9, atol=1e-9)
        self.tgrad = x.grad
        self.infeasible = [b for b in range(len(c.in_len))
                           if c.in_len[b] < c.lab_len[b] + C.repeats(c.labels[b, : c.lab_len[b]])]
        assert all(self.nll[b] == 0.0 for b in self.infeasible) and all(self.nll[b] > 0.0 for b in range(len(c.in_len)) if b not in self.infeasible)
        self.argmax = torch.from_numpy(c.logits).argmax(-1)
        self.grad_t = torch.from_numpy(self.grad)
        self.nll.setflags(write=False)
        self.grad.setflags(write=False)


@lru_cache(maxsize=None)
def ref_of(kind, *key):
    c = {"range": C.range_case, "width": C.width_case, "tail": C.tail_case}[kind](*key)
    return c, Ref(c)


def check_loss(K, ws, c, r, dtype, zero_infinity=True, inplace=False, grad_scale=0.5):
    B, T, V = c.logits.shape
    x = torch.from_numpy(c.logits).to(dtype).to(DEV)
    assert torch.equal(x.float().cpu(), torch.from_numpy(c.logits))            # the case is already rounded to dtype
    path = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    nll, dl = K.ctc_fwd_bwd(x, dev(c.in_len), dev(c.labels), dev(c.lab_len), ws, zero_infinity=zero_infinity, grad_scale=grad_scale,
                            dlogits=x if inplace else None, best_path=path)
    torch.cuda.synchronize()
    assert (dl.data_ptr() == x.data_ptr()) == inplace
    nll, dl, path = nll.cpu(), dl.float().cpu(), path.cpu()
    for b in range(B):
        print(f"{c.name}[{b}] {dtype} T={c.in_len[b]} L={c.lab_len[b]}: nll {float(nll[b]):.4f} (oracle {r.nll[b]:.4f}), "
              f"max |dlogits - oracle| {float((dl[b] - grad_scale * r.grad_t[b]).abs().max()):.3e}")
    ok = [b for b in range(B) if b not in r.infeasible]
    close(nll[ok], torch.from_numpy(r.nll[ok]), **NLL_TOL, what=f"{c.name} nll")
    for b in r.infeasible:          # from the lengths alone: +inf (0 with zero_infinity), gradient exactly 0
        assert float(nll[b]) == (0.0 if zero_infinity else math.inf), (b, float(nll[b]))
        assert float(dl[b].abs().max()) == 0.0, b
    close(dl, grad_scale * r.grad_t, **GRAD_TOL[dtype], what=f"{c.name} dlogits")
    close(dl, grad_scale * r.tgrad, **GRAD_TOL[dtype], what=f"{c.name} dlogits vs torch")
    for b in range(B):
        Tb = int(c.in_len[b])
        assert float(dl[b, Tb:].abs().max() if Tb < T else 0.0) == 0.0, b      # padded frames: exact zeros
        assert path[b, :Tb].tolist() == r.argmax[b, :Tb].tolist() and int(path[b, Tb:].abs().sum()) == 0, b


# ------------------------------------------------------------------------------------------------------------------ range: loss
@pytest.mark.parametrize("mode", ["zero_infinity", "inf", "inplace"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", C.RANGE_NAMES)
def test_ctc_loss_past_the_fp64_range(K, ws, name, dtype, mode):
    """Batches A (V = 64; A50: V = 50, the generic kernels), B, C, D, E, F: fp32 takes the generic gradient kernel, bf16 with V % 8 == 0
    the rows kernels.  A feasible utterance never reads as infeasible; a truly infeasible one (batch A, utterance 3) still does.
    Batch F is found by its frames (every alpha * beta of the middle frames is 0) while its loss tail is in range."""
    c, r = ref_of("range", name, dtype)
    check_loss(K, ws, c, r, dtype, zero_infinity=mode != "inf", inplace=mode == "inplace", grad_scale=1.0 if mode == "inf" else 0.5)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["A", "F"])
def test_ctc_loss_without_gradient_past_the_fp64_range(K, ws, name, dtype):
    """Forward only: no gradient kernel looks at the frames.  In batch F the loss tail is in range although the scaled alpha dropped
    states that carry most of the path mass on the way (the scaled lattice alone gives 1070.9987 for 1067.4708)."""
    c, r = ref_of("range", name, dtype)
    x = torch.from_numpy(c.logits).to(dtype).to(DEV)
    nll, dl = K.ctc_fwd_bwd(x, dev(c.in_len), dev(c.labels), dev(c.lab_len), ws, want_grad=False)
    nll = nll.cpu()
    print(name, dtype, nll.tolist(), r.nll.tolist())
    assert dl is None
    ok = [b for b in range(len(c.in_len)) if b not in r.infeasible]
    close(nll[ok], torch.from_numpy(r.nll[ok]), **NLL_TOL, what=f"{name} nll, forward only")
    for b in r.infeasible:
        assert math.isinf(float(nll[b])) and float(nll[b]) > 0


# ------------------------------------------------------------------------------------------------------------- alignment
def outputs_of_path(logp, path, labels, Lmax):
    """spans and token_logp (asr_ctc_align's definitions) of a frame-wise path that spells `labels`."""
    spans = np.full((Lmax, 2), -1, dtype=np.int64)
    tlp = np.zeros(Lmax)
    i, prev = -1, 0
    for t, tok in enumerate(path):
        if tok != 0:
            if tok != prev:
                i += 1
                spans[i, 0] = t
            spans[i, 1] = t
            tlp[i] += logp[t, tok]
        prev = tok
    assert i == len(labels) - 1
    return spans, tlp


def check_align(K, c, dtype):
    """As tests/test_ctc_align_gpu.py::_check_against_oracle, with its tolerances; spans and token_logp are compared for every utterance:
    with the oracle's when the kernel found the oracle's path, else (two best paths within the score tolerance: bf16 logits tie) with
    what the kernel's own path gives in fp64."""
    B, T, V = c.logits.shape
    Lmax = c.labels.shape[1]
    x = torch.from_numpy(c.logits).to(dtype).to(DEV)
    path, spans, tlp, score = (a.cpu().numpy() for a in K.ctc_align(x, dev(c.in_len), dev(c.labels), dev(c.lab_len)))
    logp = log_softmax(c.logits.astype(np.float64))
    same = 0
    for b in range(B):
        Tb, L = int(c.in_len[b]), int(c.lab_len[b])
        labels = [int(v) for v in c.labels[b, :L]]
        wsc, states = viterbi_ref(logp[b, :Tb], labels)
        print(f"{c.name}[{b}] {dtype} T={Tb} L={L}: score {score[b]:.4f} (oracle {wsc:.4f})")
        if states is None:
            assert Tb < L + C.repeats(labels)
            assert score[b] == -math.inf and (spans[b] == -1).all() and (tlp[b, :L] == -math.inf).all(), b
            assert (path[b, :Tb] == 0).all() and (path[b, Tb:] == -1).all(), b
            continue
        tol = 1e-5 * max(1.0, abs(wsc))
        assert abs(score[b] - wsc) <= tol, (b, score[b], wsc)
        assert (path[b, Tb:] == -1).all()
        assert collapse(path[b, :Tb].tolist()) == labels, b
        assert abs(rescore(logp[b, :Tb], path[b, :Tb]) - wsc) <= tol, b
        want = [0 if s % 2 == 0 else labels[s // 2] for s in states]
        same += path[b, :Tb].tolist() == want
        wspans, wtlp = outputs_of_path(logp[b, :Tb], want if path[b, :Tb].tolist() == want else path[b, :Tb].tolist(), labels, Lmax)
        assert (spans[b] == wspans).all(), b
        assert np.allclose(tlp[b], wtlp, rtol=1e-5, atol=1e-4), b
    return same


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["A", "A50", "B", "C", "F"])
def test_ctc_align_past_the_fp64_range(K, name, dtype):
    """The best path of a long label sequence under blank-dominated posteriors lies as far below the all-blank prefix as the loss's
    final states do: the alignment must still be found (and the infeasible utterance of batch A still refused)."""
    c = C.range_case(name, dtype)
    same = check_align(K, c, dtype)
    if dtype == F32:      # continuous logits: no ties, the oracle's very path
        assert same == sum(h is not None for h in c.hazard), same


# ------------------------------------------------------------------------------------------------------ row widths, prefetch tails
EDGE_TYPES = [(F32, 16), (BF16, 64)]


@pytest.mark.parametrize("dtype,V", EDGE_TYPES, ids=["f32-V16", "bf16-V64"])
@pytest.mark.parametrize("Lmax", C.WIDTH_LMAX)
def test_ctc_lattice_row_widths(K, ws, Lmax, dtype, V):
    """Entry L in the last lane of the last register (Lmax = 31, 63, 127, 255) and the first Lmax of the next width (32, 64, 128)."""
    c, r = ref_of("width", Lmax, V, dtype)
    assert not r.infeasible
    check_loss(K, ws, c, r, dtype)
    check_align(K, c, dtype)


@pytest.mark.parametrize("dtype,V", EDGE_TYPES, ids=["f32-V16", "bf16-V64"])
@pytest.mark.parametrize("Lmax", C.TAIL_LMAX)
def test_ctc_prefetch_tails(K, ws, Lmax, dtype, V):
    """in_len = 1 .. 130 across (in_len - 1) % 8 and the first steady-state iteration of the prefetch (4 buffers: 57 frames; 2: 25)."""
    c, r = ref_of("tail", Lmax, V, dtype)
    assert not r.infeasible
    check_loss(K, ws, c, r, dtype)
    check_align(K, c, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_lmax_256_is_refused(K, ws, dtype):
    B, T, V, Lmax = 1, 8, 16, 256
    x = torch.zeros(B, T, V, dtype=dtype, device=DEV)
    il, lab, ll = dev([T]), torch.ones(B, Lmax, dtype=torch.int32, device=DEV), dev([2])
    with pytest.raises(RuntimeError, match="longer than 255"):
        K.ctc_fwd_bwd(x, il, lab, ll, ws)
    with pytest.raises(RuntimeError, match="longer than 255"):
        K.ctc_align(x, il, lab, ll)
