"""Intermediate CTC with self-conditioning on the GPU: asr_softmax_rows / asr_softmax_bwd_add against their definition
(tests/interctc_ref.py) on f32 and bf16 frames and on bytes, the training step of a small TransformerCTC with the interctc_* keys against
the definition under autograd, the properties of the model's paths, and two data-parallel ranks (the "gradient final" marks).

Tolerances of the kernels - the gates of tests/test_cr_ctc_gpu.py.  An f32 output: the definition is also evaluated in float32 on the
CPU; the kernel may be further from the float64 definition than that run by a factor 4 (another reduction order), floor 1e-6.  A bf16
output: against the float64 result on the bf16 values the kernel reads, rounded to bf16; one bf16 ulp of the reference value (a single
final rounding can land on the neighbour) plus the f32 allowance.  The figures are printed (pytest -s), attached to the test's report
(record_property) and, when ASR_INTERCTC_PARITY names a file, appended to it as JSON lines; profiles/interctc_parity.json keeps one run of them."""
import json
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import interctc_ref as I  # noqa: E402
from tests.helpers import ROOT, free_port  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = 768.0      # exact in bf16
CAP = 6144            # kernels.INTERCTC_RESIDENT_MAX_V (asserted below): the longest row the kernels keep in registers
# one utterance of length 0, one of length 1 and one full (12 > T is clamped)
LENS = {(1, 1): [1], (1, 9): [9], (3, 1): [0, 1, 1], (3, 9): [0, 1, 12], (1, 2): [2]}
# (B, T, V, ld or None): B in {1, 3}, T in {1, 9}, V in {2, 5, 64, 257} and 4232 in rows of 4288; the cap, the cap plus one (the path that
# reads the rows again, element by element) and a row of whole vectors above the cap; whole vectors in V and ld behind a base address
# that is no multiple of 16 bytes (element by element for the address alone)


class Shifted(int):
    """A row stride whose blocks - the inputs and every output block - begin one element into a 16-byte-aligned allocation."""

    def __repr__(self):
        return "%d+1" % int(self)


SHAPES = ([(B, T, V, None) for B in (1, 3) for T in (1, 9) for V in (2, 5, 64, 257)] +
          [(1, 1, 4232, 4288), (3, 9, 4232, 4288), (1, 2, CAP, None), (1, 2, CAP + 1, None), (1, 2, CAP + 8, None), (1, 2, 64, Shifted(72))])
SPREADS = (1.0, 60.0)


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    assert kernels.INTERCTC_RESIDENT_MAX_V == CAP
    return kernels


@lru_cache(maxsize=None)
def reference(B, T, V, spread, dtype):
    """The inputs as the kernels read them in `dtype` and the definition in float64 and in float32.  Computed once.
    p: softmax_rows of the logits; its rounding to `dtype` is the backward's input, with dp and a prior gradient."""
    z, dp, prior, in_len = I.make_case(B, T, V, spread, LENS[(B, T)])
    z, dp, prior = (torch.from_numpy(a).to(dtype) for a in (z, dp, prior))
    p64, p32 = I.softmax_rows(z.double(), in_len), I.softmax_rows(z.float(), in_len)
    p = p64.to(dtype)
    t64, t32 = I.softmax_bwd(p.double(), dp.double(), in_len), I.softmax_bwd(p.float(), dp.float(), in_len)
    acc32 = (prior.float() + t32).double().numpy()      # the float32 run of accumulate = 1: the sum rounded to float32 as well
    return dict(z=z, dp=dp, prior=prior, in_len=in_len, p=p, p64=p64.numpy(), p32=p32.double().numpy(), t64=t64.numpy(), t32=t32.double().numpy(),
                acc64=prior.double().numpy() + t64.numpy(), acc32=acc32)


def device_rows(x, ld, fill=SENTINEL):
    """x (B, T, V) on the host -> a device view [:, :, :V] of rows `ld` apart (dense when ld is None), the padding holding `fill`."""
    if ld is None:
        return x.to(DEV), None
    B, T, V = x.shape
    buf = torch.full((B, T, ld), fill, dtype=x.dtype)
    buf[:, :, :V] = x
    if isinstance(ld, Shifted):
        flat = torch.empty(buf.numel() + 1, dtype=x.dtype, device=DEV)
        assert flat.data_ptr() % 16 == 0
        flat[1:] = buf.reshape(-1).to(DEV)
        buf = flat[1:].view(B, T, ld)
        assert buf.data_ptr() % 16 == x.element_size()
    else:
        buf = buf.to(DEV)
    return buf[:, :, :V], buf


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def bf16_ulp(v):
    """The spacing of bf16 numbers at |v| (float64 array): 2^(floor(log2 |v|) - 7), at least the smallest subnormal's."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def _gate(got, want, want32, dtype):
    """(passes, figures): the gate of the module docstring on one output block (float64 numpy arrays)."""
    dev_32 = float(np.abs(want32 - want).max())
    allow = max(4.0 * dev_32, 1e-6)
    if dtype == torch.bfloat16:
        w = torch.from_numpy(want).to(torch.bfloat16).double().numpy()      # the float64 result rounded to bf16
        excess = float((np.abs(got - w) - bf16_ulp(w)).max())
        return excess <= allow, dict(kernel=float(np.abs(got - w).max()), float32=dev_32, worst_excess_over_one_ulp=excess)
    dev_k = float(np.abs(got - want).max())
    return dev_k <= allow, dict(kernel=dev_k, float32=dev_32, ratio=dev_k / max(dev_32, 1e-300))


def _keep_parity(row):
    path = os.environ.get("ASR_INTERCTC_PARITY")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("B,T,V,ld", SHAPES)
def test_kernels_match_the_definition(K, B, T, V, ld, spread, dtype, record_property):
    r = reference(B, T, V, spread, dtype)
    in_len, n_dev = r["in_len"], _i32(r["in_len"])
    n = np.clip(in_len, 0, T)
    row = dict(B=B, T=T, V=V, ld=ld, spread=spread, dtype=str(dtype))
    # ---- forward
    x, _ = device_rows(r["z"], ld)
    out, obuf = device_rows(torch.full((B, T, V), SENTINEL, dtype=dtype), ld)
    assert K.softmax_rows(x, n_dev, out=out) is out
    torch.cuda.synchronize()
    got = out.double().cpu().numpy()
    ok, row["softmax_rows"] = _gate(got, r["p64"], r["p32"], dtype)
    print(row)
    assert ok, row
    assert np.isfinite(got).all()
    for b in range(B):      # exact: zeros on the frames past the utterance
        assert (got[b, n[b]:] == 0).all()
    if obuf is not None:     # ... and the padding columns keep their sentinel
        assert obuf.shape[2] == ld > V and bool((obuf[:, :, V:] == SENTINEL).all())
    fresh = K.softmax_rows(x, n_dev)      # out=None: a fresh block laid out like the logits, the same bytes
    assert fresh.stride() == x.stride() and torch.equal(fresh.contiguous().view(torch.uint8), out.contiguous().view(torch.uint8))
    # ---- backward, accumulate off and on
    p, _ = device_rows(r["p"], ld)
    dp, _ = device_rows(r["dp"], ld)
    for acc in (False, True):
        prior = r["prior"] if acc else torch.full((B, T, V), SENTINEL, dtype=dtype)
        g, gbuf = device_rows(prior, ld)
        assert K.softmax_bwd_add(p, dp, n_dev, g, accumulate=acc) is g
        torch.cuda.synchronize()
        got = g.double().cpu().numpy()
        ok, row["softmax_bwd_add acc=%d" % acc] = _gate(got, r["acc64"] if acc else r["t64"], r["acc32"] if acc else r["t32"], dtype)
        print(row)
        assert ok, row
        raw, pr = g.cpu(), prior
        for b in range(B):      # frames past the utterance: untouched under accumulate, zeros otherwise
            if acc:
                assert torch.equal(raw[b, n[b]:].contiguous().view(torch.uint8), pr[b, n[b]:].contiguous().view(torch.uint8))
            else:
                assert bool((raw[b, n[b]:] == 0).all())
        if gbuf is not None:
            assert bool((gbuf[:, :, V:] == SENTINEL).all())
    if n.max() > 0 and spread == 1.0:
        assert np.abs(r["t64"]).max() > 0
    record_property("interctc_parity", row)
    _keep_parity(row)


BYTES_SHAPES = [(3, 9, 257, None), (3, 9, 4232, 4288), (3, 9, 64, None), (1, 2, CAP + 8, None), (1, 2, CAP + 1, None), (1, 2, 64, Shifted(72))]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,V,ld", BYTES_SHAPES)
def test_bytes(K, B, T, V, ld, dtype):
    """Two runs write identical bytes; a -inf logit gives exactly 0 and a row without a finite maximum zeros; a backward term is exactly
    zero wherever p is 0, so accumulate leaves those cells' bytes.  Rows: one logit 60 above the rest (the others' exp(-60) = 9e-27 is
    still a float, the hot class is exactly 1 and its term exactly 0) and one 120 above, where the others do round to 0."""
    r = reference(B, T, V, 1.0, dtype)
    n_dev, n = _i32(r["in_len"]), np.clip(r["in_len"], 0, T)
    x, _ = device_rows(r["z"], ld)

    def out():      # a shifted case gets a shifted output block too; the others leave the block to the call
        return dict(out=device_rows(torch.zeros(B, T, V, dtype=dtype), ld)[0]) if isinstance(ld, Shifted) else {}

    a, b = K.softmax_rows(x, n_dev, **out()), K.softmax_rows(x, n_dev, **out())
    assert torch.equal(_bytes(a), _bytes(b)) and bool((a != 0).any())
    dp, _ = device_rows(r["dp"], ld)
    prior, _ = device_rows(r["prior"], ld)
    g1, _ = device_rows(r["prior"], ld)
    g2, _ = device_rows(r["prior"], ld)
    K.softmax_bwd_add(a, dp, n_dev, g1, accumulate=True)
    K.softmax_bwd_add(a, dp, n_dev, g2, accumulate=True)
    assert torch.equal(_bytes(g1), _bytes(g2)) and not torch.equal(_bytes(g1), _bytes(prior))
    z = r["z"].clone()
    full, hot = int(np.argmax(n)), 3      # the full utterance; the hot class
    z[full, 0, :] = 0.0
    z[full, 0, hot] = 120.0
    z[full, 0, 1] = float("-inf")
    z[full, T - 1, :] = 0.0
    z[full, T - 1, hot] = 60.0
    if T > 2:
        z[full, 1, :] = float("-inf")
    xz, _ = device_rows(z, ld)
    p = K.softmax_rows(xz, n_dev, **out())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(p.float()).all())
    row0, last = p[full, 0].float().cpu(), p[full, T - 1].float().cpu()
    assert float(row0[hot]) == 1.0 and float(row0.abs().sum()) == 1.0      # -inf and exp(-120): exactly 0
    assert float(last[hot]) == 1.0 and float(last.sum()) == 1.0 and float(last.min()) > 0
    if T > 2:
        assert bool((p[full, 1] == 0).all())
    gz, _ = device_rows(r["prior"], ld)
    K.softmax_bwd_add(p, dp, n_dev, gz, accumulate=True)
    torch.cuda.synchronize()
    live = torch.zeros(B, T, dtype=torch.bool)
    for u in range(B):
        live[u, :n[u]] = True
    cells = (p == 0).cpu() & live.unsqueeze(-1)
    assert int(cells.sum()) >= V - 1
    assert torch.equal(_bytes(gz.cpu()[cells]), _bytes(r["prior"][cells]))      # += exactly 0
    gw, _ = device_rows(torch.full((B, T, V), SENTINEL, dtype=dtype), ld)
    K.softmax_bwd_add(p, dp, n_dev, gw, accumulate=False)
    assert bool((gw.cpu()[cells] == 0).all())
    # the hot class of both rows: s = dp[hot] after rounding, the term exactly 0
    assert float(gw[full, 0, hot]) == 0.0 and float(gw[full, T - 1, hot]) == 0.0


def test_refusals_leave_the_outputs_untouched(K):
    from asr_chinese_e2e_amd._lib import AsrHipError
    r = reference(3, 9, 64, 1.0, torch.float32)
    x, n = r["z"].to(DEV), _i32(r["in_len"])
    keep = torch.full_like(x, 5.0)
    both = torch.full((6, 9, 64), 5.0, device=DEV)      # two blocks inside one buffer, overlapping
    with pytest.raises(AsrHipError):      # the output is the logits
        K.softmax_rows(keep, n, out=keep)
    with pytest.raises(AsrHipError):      # ... or overlaps them
        K.softmax_rows(both[:3], n, out=both[2:5])
    with pytest.raises(AsrHipError):      # the gradient block is p / is dp / overlaps p
        K.softmax_bwd_add(keep, x, n, keep)
    with pytest.raises(AsrHipError):
        K.softmax_bwd_add(x, keep, n, keep)
    with pytest.raises(AsrHipError):
        K.softmax_bwd_add(both[:3], x, n, both[2:5])
    with pytest.raises(ValueError):
        K.softmax_rows(x, n[:2], out=keep)
    with pytest.raises(ValueError):
        K.softmax_rows(x, n, out=keep.to(torch.bfloat16))
    with pytest.raises(ValueError):
        K.softmax_bwd_add(x, x[:, :, :32], n, keep)
    with pytest.raises(TypeError):
        K.softmax_rows(x.double(), n, out=keep.double())
    torch.cuda.synchronize()
    assert bool((keep == 5.0).all()) and bool((both == 5.0).all())


# ------------------------------------------------------------------------------------------------ the model
W = 0.3
STEP_CASES = [(dtype, layers, cond) for dtype in ("fp32", "bf16") for layers in ((1,), (1, 2)) for cond in (False, True)]


@lru_cache(maxsize=None)
def _model_case(dtype):
    """(shape, cfg, sd with the conditioning projection, batch): three layers, the issue's shapes."""
    from tests.test_model_gpu import oracle_case
    if dtype == "fp32":
        shape = (2, 30, 16, 40, 6)
        over = dict(d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=3, use_decoder=False, ctc_weight=1.0)
        cfg, sd, batch = oracle_case(*shape, over, seed=5)
    else:      # the widths the MFMA kernels are built for
        shape = (2, 40, 80, 56, 12)
        over = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=3, use_decoder=False, ctc_weight=1.0)
        cfg, sd, batch = oracle_case(*shape, over, seed=9)
    sd = dict(sd)
    sd[I.COND] = I.init_cond(cfg.d_model, shape[3], seed=11)      # Xavier-uniform
    return shape, cfg, sd, batch


def _weights(sd, cond):
    return {k: v for k, v in sd.items() if cond or k != I.COND}


def _build(dtype, layers=(), cond=False, **over):
    from tests.test_model_gpu import build
    (B, T, F_, V, L), cfg, sd, batch = _model_case(dtype)
    keyed = over.pop("keyed", False)      # the keys at their defaults, spelled out
    keys = dict(interctc_weight=W if layers else 0.0, interctc_layers=layers, interctc_condition=cond) if (layers or cond or keyed) else {}
    model = build(cfg, V, "TransformerCTC", dtype=dtype, dropout=0.0, **keys, **over).cuda()
    model.load_state_dict(_weights(sd, cond))
    model._ensure_engine(DEV)
    return model


def _step(dtype, layers=(), cond=False, **over):
    from tests.test_model_gpu import to_pack
    model = _build(dtype, layers, cond, **over)
    model.zero_flat_grads()
    loss, _ = model.train_step(to_pack(_model_case(dtype)[3]))
    torch.cuda.synchronize()
    return model, loss


@lru_cache(maxsize=None)
def _oracle(dtype, layers, cond):
    """tests/interctc_ref.py under autograd with RefTrainer's leaves.  bf16 with conditioning: the engine stores the posteriors in bf16
    (asr_softmax_rows rounds once to the logits' dtype), so the oracle rounds p at that place - and nothing else."""
    from oracle import ref_model as R
    shape, cfg, sd, batch = _model_case(dtype)
    tr = R.RefTrainer(_weights(sd, cond), cfg, warmup=25)
    leaves = {k: tr.sd[k].detach().clone().requires_grad_(True) for k in tr.trainable}
    s = dict(tr.sd)
    s.update(leaves)
    out = I.losses(s, cfg, batch, W, layers, cond, round_p=torch.bfloat16 if (dtype == "bf16" and cond) else None)
    grads = torch.autograd.grad(out["loss"], [leaves[k] for k in tr.trainable], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(tr.trainable, grads)}
    return dict(loss=float(out["loss"].detach()), ctc=float(out["ctc"].detach()), inter=[float(v.detach()) for v in out["inter"]],
                per_utt=out["per_utt"].detach().numpy(), enc_out=out["enc_out"].detach(), grads=grads)


@pytest.mark.parametrize("dtype,layers,cond", STEP_CASES)
def test_step_matches_the_oracle(dtype, layers, cond):
    """w = 0.3 at layers (1,) and (1, 2) of three, with and without self-conditioning: the loss and every gradient tensor - the
    conditioning projection's included - against the oracle, at the gates of tests/test_model_gpu.py (fp32: loss 1e-4, gradients rtol
    3e-4 / atol 3e-6 gmax; bf16: BF16_LOSS_RTOL and bf16_gradient_gate).  The bf16 oracle rounds the posteriors to bf16 where the kernel
    does (see _oracle) and nothing else."""
    from tests.test_model_gpu import BF16_LOSS_RTOL, bf16_gradient_gate
    (B, T, F_, V, L), cfg, sd, batch = _model_case(dtype)
    want = _oracle(dtype, layers, cond)
    gmax = max(float(g.abs().max()) for g in want["grads"].values())
    print(dtype, layers, cond, "oracle loss", want["loss"], "ctc", want["ctc"], "inter", want["inter"], "gmax", gmax)
    assert all(v > 1.0 for v in want["inter"])      # the intermediate terms are not negligible
    if cond:
        share = float(want["grads"][I.COND].abs().max()) / gmax
        print("Wc gradient share", share)
        assert share > 1e-3
    model, loss = _step(dtype, layers, cond)
    names = [n for n, _ in model.named_parameters()]
    assert (I.COND in names) == cond and set(names) == set(want["grads"])
    last = model._engine.last_interctc
    assert last.shape == (len(layers), B)
    rel = abs(float(loss[0]) - want["loss"]) / abs(want["loss"])
    print(dtype, "loss", float(loss[0]), "rel", rel, "interctc", last.cpu().numpy().tolist())
    if dtype == "fp32":
        assert rel < 1e-4, (float(loss[0]), want["loss"])
        assert np.allclose(last.cpu().numpy(), want["per_utt"][:-1], rtol=1e-4)
        for n, p in model.named_parameters():
            assert np.allclose(p.grad.cpu().numpy(), want["grads"][n].numpy(), rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), n
    else:
        worst, worst_name, ratio = bf16_gradient_gate(model, dict(grads=want["grads"]), "interctc")
        print("bf16 worst cosine", worst, worst_name, "norm ratio", ratio, "loss rel", rel)
        assert rel < BF16_LOSS_RTOL, (float(loss[0]), want["loss"])
    # the parent commit ignores the keys: its loss is the plain CTC loss, which this is not
    assert abs(want["loss"] - want["ctc"]) > 1e-3 * abs(want["ctc"])


def test_default_keys_are_todays_step(deterministic_mode):
    """interctc_weight = 0, layers = (): the flat gradient and the loss of the step bit for bit, and nothing of the new stage runs."""
    plain, loss0 = _step("fp32")
    keyed, loss1 = _step("fp32", keyed=True)
    eng = keyed._engine
    assert eng.interctc == ((), 0.0, False) and eng.cond is None and eng.last_interctc is None and keyed._interctc_mean is None and not eng._hold_marks
    assert keyed._flat.index == plain._flat.index
    assert torch.equal(plain._flat.g.view(torch.int32), keyed._flat.g.view(torch.int32)) and torch.equal(loss0, loss1)
    assert float(plain._flat.g.abs().max()) > 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_plain_intermediate_ctc_leaves_inference_alone(dtype):
    from tests.test_model_gpu import to_pack
    pack = to_pack(_model_case(dtype)[3])
    base, plain = _build(dtype), _build(dtype, (1, 2))
    a, b = base.forward(pack), plain.forward(pack)
    assert torch.equal(_bytes(a.encoder_out), _bytes(b.encoder_out)) and torch.equal(_bytes(a.ctc_logits), _bytes(b.ctc_logits))
    assert plain._engine.last_interctc is None      # no loss, no head at the middle layers


@pytest.mark.parametrize("layers", [(1,), (1, 2)])
def test_conditioned_forward_matches_the_definition(layers):
    """Evaluation mode, fp32: the encoder output against the definition at the forward gate of tests/test_model_gpu.py (rtol 1e-4, atol
    2e-5); padded rows exactly 0 (in bf16 too)."""
    from tests.test_model_gpu import to_pack
    want = _oracle("fp32", layers, True)
    batch = _model_case("fp32")[3]
    model = _build("fp32", layers, True).eval()
    out = model.forward(to_pack(batch))
    got = out.encoder_out.cpu()
    assert np.allclose(got.numpy(), want["enc_out"].numpy(), rtol=1e-4, atol=2e-5)
    base = _oracle("fp32", layers, False)["enc_out"]
    assert float((want["enc_out"] - base).abs().max()) > 1e-3      # the conditioning is visible to that gate
    for dtype, o in (("fp32", got), ("bf16", _build("bf16", layers, True).eval().forward(to_pack(_model_case("bf16")[3])).encoder_out.float().cpu())):
        wl = _model_case(dtype)[3]["wave_len"]
        assert int(wl.min()) < o.shape[1]
        for b in range(o.shape[0]):
            assert float(o[b, int(wl[b]):].abs().sum()) == 0.0 and float(o[b, :int(wl[b])].abs().max()) > 0


@pytest.mark.parametrize("cond", [False, True])
def test_interctc_losses_match_the_definition(cond):
    from tests.test_model_gpu import to_pack
    want = _oracle("fp32", (1, 2), cond)
    model = _build("fp32", (1, 2), cond)
    got = model.interctc_losses(to_pack(_model_case("fp32")[3]))
    assert got["layers"] == (1, 2) and len(got["interctc"]) == 2
    assert np.allclose(np.array(got["interctc"] + [got["ctc"]]), want["per_utt"], rtol=1e-4)
    with pytest.raises(ValueError):
        _build("fp32").interctc_losses(to_pack(_model_case("fp32")[3]))


def test_overlap_on_and_off_give_the_same_gradient(monkeypatch):
    """ASR_WGRAD_OVERLAP is read when the engine is built: with the weight gradients on their own stream (the head's and the
    conditioning projection's are issued from the forward AND the backward pass) and on the main stream - against each other and the oracle."""
    want = _oracle("fp32", (1, 2), True)
    gmax = max(float(g.abs().max()) for g in want["grads"].values())
    got = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("ASR_WGRAD_OVERLAP", flag)
        model, loss = _step("fp32", (1, 2), True)
        assert model._engine.overlap_wgrad == (flag == "1")
        got[flag] = ({n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters()}, float(loss[0]))
    assert abs(got["1"][1] - got["0"][1]) <= 1e-6 * abs(got["0"][1])
    for n in got["0"][0]:
        assert np.allclose(got["1"][0][n], got["0"][0][n], rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), n
        for flag in ("1", "0"):
            assert np.allclose(got[flag][0][n], want["grads"][n].numpy(), rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), (n, flag)


def test_metrics_report_the_mean():
    from tests.test_model_gpu import make_opt, to_pack
    (B, T, F_, V, L), cfg, sd, batch = _model_case("fp32")
    model = _build("fp32", (1, 2), True)
    metrics, _ = model.iterate(to_pack(batch), optimizer=make_opt(model, cfg, 25), is_train=True)
    last = model._engine.last_interctc
    want = float(last.mean())
    assert last.shape == (2, B) and abs(float(metrics.interctc) - want) <= 1e-6 * want and want > 1.0
    ev, _ = model.iterate(to_pack(batch), is_train=False)
    assert "interctc" not in ev
    base = _build("fp32")
    plain, _ = base.iterate(to_pack(batch), optimizer=make_opt(base, cfg, 25), is_train=True)
    assert "interctc" not in plain


def test_streaming_refuses_conditioning_and_is_unchanged_without():
    (B, T, F_, V, L), cfg, sd, batch = _model_case("fp32")
    cond = _build("fp32", (1,), True, chunk_size=4)
    for what in ("stream", "sessions"):
        with pytest.raises(ValueError, match="interctc_condition"):
            getattr(cond, what)(B)
    base, plain = _build("fp32", chunk_size=4), _build("fp32", (1, 2), chunk_size=4)
    feats = batch["wave"][:, :8].to(DEV)
    outs = []
    for m in (base, plain):
        st = m.stream(B)
        ids = [st.push(feats[:, :4].contiguous(), [4] * B), st.push(feats[:, 4:8].contiguous(), [4] * B)]
        ss = m.sessions(B)
        ss.open(0)
        ids.append(ss.push(feats[:, :4].contiguous(), [4] + [0] * (B - 1), [False] * B))
        outs.append(ids)
    assert outs[0] == outs[1] and len(outs[0][0]) == B


# ------------------------------------------------------------------------------------------------ two ranks
DP2_WORKER = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
from asr_chinese_e2e_amd import Models, dist as D
from asr_chinese_e2e_amd.data_handler import Vocab, synthetic_pack
from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
from asr_chinese_e2e_amd.Utils import Pack
rank, world = D.init("gloo")          # two ranks share the one GPU of the test box: gloo moves the CUDA buckets
torch.cuda.set_device(0)
def build():
    torch.manual_seed(0)
    M = Models.TransformerCTC
    cfg = M.get_default_config()()
    cfg.fn_build(dict(n_mels=16, lfr_m=1, d_model=64, hidden_size=16, num_head=4, ff_size=128, layer_num=3, dropout=0.0, dtype="fp32",
                      interctc_weight=0.3, interctc_layers=(1, 2), interctc_condition=True))
    m = M(cfg, Vocab.synthetic(40)).cuda()
    return m, NoamOpt(64, 1, 10, FusedAdam(m.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
full = synthetic_pack(6, 24, 16, 40, seed=5, ragged=True, Lmin=2, Lmax=6, device="cuda")
lo, hi = (0, 3) if rank == 0 else (3, 6)
mine = Pack()
mine.add(**{k: full[k][lo:hi].contiguous() for k in ("wave", "wave_len", "tgt_for_input", "tgt_for_metric", "tgt_len")})
m1, o1 = build()                      # single process, whole batch
m2, o2 = build()                      # data parallel, half a batch per rank
dp = D.DataParallel(m2, "cuda", bucket_bytes=16 << 10)      # small buckets: the head and the conditioning projection travel on their own
f = m2._flat
assert len(dp.bucketer.buckets) > 6 and dp.bucketer.buckets[0][0] >= f.index["encoder.layer_stack.2.pos_ffn.w_1.weight"][0]
# (1) the reduced gradients of one backward equal the single-process gradients of the whole batch
m1._ensure_engine("cuda"); m1.zero_flat_grads(); m1.train_step(full)
m2.zero_flat_grads(); dp.bucketer.begin()
m2.train_step(mine, count_hook=dp._counts.start); dp.bucketer.finish()
torch.cuda.synchronize()
assert not m2._engine._hold_marks
for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
    if n.endswith("w_ks.bias"):       # analytically zero gradient (softmax is shift-invariant): pure round-off
        continue
    sc = float(p.grad.abs().max()) + 1e-30
    assert float((p.grad - q.grad).abs().max()) <= 1e-4 * sc, (n, float((p.grad - q.grad).abs().max()), sc)
def same_on_both_ranks(t):
    hi_, lo_ = t.clone(), t.clone()
    torch.distributed.all_reduce(hi_, op=torch.distributed.ReduceOp.MAX)
    torch.distributed.all_reduce(lo_, op=torch.distributed.ReduceOp.MIN)
    return torch.equal(hi_, lo_)
assert same_on_both_ranks(f.g), "the ranks hold different reduced gradients: a bucket left before its last gradient was added"
# (2) a few steps: the ranks hold identical parameters, which follow the single process within a few learning rates
# (Adam, eps 1e-9, turns the round-off of near-zero gradient elements into +-lr)
for _ in range(3):
    a, _ = m1.iterate(full, optimizer=o1)
    b, _ = dp.iterate(mine, optimizer=o2)
    assert "interctc" in b and "interctc" in a
torch.cuda.synchronize()
assert same_on_both_ranks(f.p), "the ranks' parameters diverged"
for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
    assert float((p.detach() - q.detach()).abs().max()) <= 3 * o1._rate, n
torch.distributed.barrier(); torch.distributed.destroy_process_group()
print("rank", rank, "interctc dp2 ok")
"""


def test_two_ranks_hold_the_same_parameters(tmp_path):
    """The conditioned model, layers (1, 2), on two gloo ranks sharing the GPU: with self-conditioning the head's and the conditioning
    projection's gradients are final only once the backward pass has issued the lowest listed layer's branch, so every "gradient final"
    mark above it is withheld (Engine._ready).  A mark raised early sends their bucket out before the backward contributions are added:
    the ranks then hold different gradients.  Built as tests/test_train_loop_gpu.py builds its two-rank test."""
    script = tmp_path / "interctc_dp2_worker.py"
    script.write_text(DP2_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=free_port(), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r), LOCAL_RANK="0"),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} interctc dp2 ok" in o
