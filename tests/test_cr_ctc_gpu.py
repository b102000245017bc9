"""CR-CTC on the GPU: asr_cr_ctc_fwd_bwd against its definition (tests/cr_ctc_ref.py) on f32 and bf16 logits, its exact properties on
bytes, the training step of a small TransformerCTC with config.cr_ctc_weight against the CPU oracle, and the two-view loader.

Tolerances.  frame, cr and the f32 gradient: the definition is also evaluated in float32 on the CPU; the kernel may be further from the
float64 definition than that run by a factor 4 (another reduction order), floor 1e-6 - the gate of tests/test_mwer_gpu.py.  A bf16
gradient block: against the float64 gradient of the bf16-rounded logits, rounded to bf16; one bf16 ulp of the reference value (a single
final rounding can land on the neighbour) plus the f32 allowance.  Both figures are printed (pytest -s) and attached to the test's report
(record_property); profiles/cr_ctc_parity.json keeps one run of them."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cr_ctc_ref as C  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = 768.0      # exact in bf16
CAP = 6144            # kernels.CR_CTC_RESIDENT_MAX_V (asserted below): the longest row the kernel keeps in registers
LENS9 = {1: [12, 9], 3: [9, 0, 1, 8, 0, 1], 4: [9, 0, 1, 5, 9, 0, 1, 4]}      # a zero-length pair, a one-frame pair, views one frame apart; 12 > T is clamped
# (P, T, V, ld or None): P in {1, 3}, T in {1, 9}, V in {2, 5, 64, 257} and 4232 in rows of 4288; the issue's four-pair lengths; the cap and
# the cap plus one (the path that reads the rows again, with vectors and element by element), and a row of whole vectors above the cap;
# whole vectors in V and ld behind a base address that is no multiple of 16 bytes (element by element for the address alone)


class Shifted(int):
    """A row stride whose blocks - the logits and every output block - begin one element into a 16-byte-aligned allocation."""

    def __repr__(self):
        return "%d+1" % int(self)


SHAPES = ([(P, T, V, None) for P in (1, 3) for T in (1, 9) for V in (2, 5, 64, 257)] +
          [(1, 1, 4232, 4288), (3, 9, 4232, 4288), (4, 9, 64, None), (1, 2, CAP, None), (1, 2, CAP + 1, None), (1, 2, CAP + 8, None),
           (1, 2, 64, Shifted(72))])
SPREADS = (1.0, 60.0)      # at 60 float32 probabilities underflow while the loss stays finite


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    assert kernels.CR_CTC_RESIDENT_MAX_V == CAP
    return kernels


def _lens(P, T):
    return None if T != 9 else LENS9[P]


@lru_cache(maxsize=None)
def reference(P, T, V, spread, dtype):
    """(logits f32 numpy, in_len, the definition in float64, in float32) on the values the kernel reads in `dtype`.  Computed once."""
    logits, in_len = C.make_case(P, T, V, spread, _lens(P, T))
    x = torch.from_numpy(logits).to(dtype)
    return logits, in_len, C.autograd(x, in_len), C.autograd(x, in_len, dtype=torch.float32)


def device_rows(x, ld, fill=SENTINEL):
    """x (R, T, V) on the host -> a device view [:, :, :V] of rows `ld` apart (dense when ld is None), the padding holding `fill`."""
    if ld is None:
        return x.to(DEV), None
    R, T, V = x.shape
    buf = torch.full((R, T, ld), fill, dtype=x.dtype)
    buf[:, :, :V] = x
    if isinstance(ld, Shifted):
        flat = torch.empty(buf.numel() + 1, dtype=x.dtype, device=DEV)
        assert flat.data_ptr() % 16 == 0
        flat[1:] = buf.reshape(-1).to(DEV)
        buf = flat[1:].view(R, T, ld)
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


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("P,T,V,ld", SHAPES)
def test_kernel_matches_the_definition(K, P, T, V, ld, spread, dtype, record_property):
    logits, in_len, want, want32 = reference(P, T, V, spread, dtype)
    x, _ = device_rows(torch.from_numpy(logits).to(dtype), ld)
    dl, dbuf = device_rows(torch.full((2 * P, T, V), SENTINEL, dtype=dtype), ld)
    out = K.cr_ctc(x, _i32(in_len), dlogits=dl)
    torch.cuda.synchronize()
    assert out["dlogits"] is dl and out["frame"].shape == (P, T) and out["cr"].shape == (P,)
    got = dict(frame=out["frame"].double().cpu().numpy(), cr=out["cr"].double().cpu().numpy(), grad=dl.double().cpu().numpy())
    row = dict(P=P, T=T, V=V, ld=ld, spread=spread, dtype=str(dtype))
    allow = {}
    for k in ("frame", "cr", "grad"):
        dev_32 = float(np.abs(want32[k] - want[k]).max())
        allow[k] = max(4.0 * dev_32, 1e-6)
        if k == "grad" and dtype == torch.bfloat16:
            w = torch.from_numpy(want[k]).to(torch.bfloat16).double().numpy()      # the float64 gradient rounded to bf16
            excess = np.abs(got[k] - w) - bf16_ulp(w)
            dev_k = float(np.abs(got[k] - w).max())
            row[k] = dict(kernel=dev_k, float32=dev_32, worst_excess_over_one_ulp=float(excess.max()))
            print(row, k)
            assert float(excess.max()) <= allow[k], (k, dev_k, dev_32)
            continue
        dev_k = float(np.abs(got[k] - want[k]).max())
        row[k] = dict(kernel=dev_k, float32=dev_32, ratio=dev_k / max(dev_32, 1e-300))
        print(row, k)
        assert dev_k <= allow[k], (k, dev_k, dev_32)
    record_property("cr_ctc_parity", row)
    print("cr_ctc_parity", json.dumps(row))
    assert np.isfinite(got["frame"]).all() and np.isfinite(got["grad"]).all()
    # exact: zeros past the pair's frames (accumulate = 0 writes them), the padding columns keep their sentinel
    n = np.minimum(np.clip(in_len[:P], 0, T), np.clip(in_len[P:], 0, T))
    raw = dl.float().cpu().numpy()
    for p in range(P):
        assert (raw[p, n[p]:] == 0).all() and (raw[p + P, n[p]:] == 0).all() and (got["frame"][p, n[p]:] == 0).all()
    if n.max() > 0 and spread == 1.0:
        assert np.abs(raw).max() > 0
    if dbuf is not None:
        assert dbuf.shape[2] == ld > V and bool((dbuf[:, :, V:] == SENTINEL).all())
    if dtype == torch.float32:      # view b's gradient is the exact negation of view a's
        assert np.array_equal(raw[:P], -raw[P:])


BYTES_SHAPES = [(3, 9, 257, None), (3, 9, 4232, 4288), (3, 9, 64, None), (1, 2, CAP + 8, None), (1, 2, CAP + 1, None), (1, 2, 64, Shifted(72))]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("P,T,V,ld", BYTES_SHAPES)
def test_bytes(K, P, T, V, ld, dtype):
    """Identical views give exactly zero; swapped halves swap the gradient; two runs write the same bytes; the scale through the device
    scalar; accumulate = 1 over a random prior leaves every byte past the pair's frames and in the padding, and adds in f32 on the rest."""
    logits, in_len, _, _ = reference(P, T, V, 1.0, dtype)
    xh = torch.from_numpy(logits).to(dtype)
    x, _ = device_rows(xh, ld)
    n_dev = _i32(in_len)

    def out():      # a shifted case gets a shifted gradient block too; the others leave the block to the call
        return dict(dlogits=device_rows(torch.zeros(2 * P, T, V, dtype=dtype), ld)[0]) if isinstance(ld, Shifted) else {}

    a = K.cr_ctc(x, n_dev, grad_scale=0.37, **out())
    b = K.cr_ctc(x, n_dev, grad_scale=0.37, **out())
    for k in ("cr", "frame", "dlogits"):
        assert torch.equal(_bytes(a[k]), _bytes(b[k])), k
    assert bool((a["dlogits"] != 0).any())
    # the scale through the device scalar: s = (2 s) / 2
    c = K.cr_ctc(x, n_dev, grad_scale=0.74, grad_scale_div=torch.tensor([2.0], device=DEV), **out())
    assert torch.equal(_bytes(c["dlogits"]), _bytes(a["dlogits"])) and torch.equal(_bytes(c["cr"]), _bytes(a["cr"]))
    # no gradient wanted: the same values
    v = K.cr_ctc(x, n_dev, want_grad=False)
    assert v["dlogits"] is None and torch.equal(_bytes(v["cr"]), _bytes(a["cr"])) and torch.equal(_bytes(v["frame"]), _bytes(a["frame"]))
    # swapped halves: swapped gradient, the same cr and frame
    xs, _ = device_rows(torch.cat([xh[P:], xh[:P]]), ld)
    s = K.cr_ctc(xs, _i32(np.concatenate([in_len[P:], in_len[:P]])), grad_scale=0.37, **out())
    assert torch.equal(_bytes(s["cr"]), _bytes(a["cr"])) and torch.equal(_bytes(s["frame"]), _bytes(a["frame"]))
    assert torch.equal(_bytes(s["dlogits"][:P]), _bytes(a["dlogits"][P:])) and torch.equal(_bytes(s["dlogits"][P:]), _bytes(a["dlogits"][:P]))
    # identical views: exactly zero
    xi, _ = device_rows(torch.cat([xh[:P], xh[:P]]), ld)
    z = K.cr_ctc(xi, n_dev, grad_scale=0.37, **out())
    assert bool((z["frame"] == 0).all()) and bool((z["cr"] == 0).all()) and bool((z["dlogits"] == 0).all())
    # accumulate = 1 over a random prior
    n = np.minimum(np.clip(in_len[:P], 0, T), np.clip(in_len[P:], 0, T))
    live = torch.zeros(2 * P, T, dtype=torch.bool)
    for p in range(P):
        live[p, :n[p]] = True
        live[p + P, :n[p]] = True
    g = torch.Generator().manual_seed(3)
    width = ld if ld is not None else V
    prior_full = torch.randn(2 * P, T, width, generator=g).to(dtype)
    buf = device_rows(prior_full, ld)[1] if isinstance(ld, Shifted) else prior_full.to(DEV)
    K.cr_ctc(x, n_dev, grad_scale=0.37, dlogits=buf[:, :, :V], accumulate=True)
    got_full = buf.cpu()
    got, prior, added = got_full[:, :, :V], prior_full[:, :, :V], a["dlogits"].cpu()
    assert torch.equal(_bytes(got_full[:, :, V:]), _bytes(prior_full[:, :, V:]))
    assert torch.equal(_bytes(got[~live]), _bytes(prior[~live]))
    if dtype == torch.float32:      # the same f32 value is added in f32: exact
        assert torch.equal(got[live], prior[live] + added[live])
    else:                           # the f32 sum is rounded once to bf16; `added` was rounded on its own (2^-9 relative each)
        want = prior[live].float() + added[live].float()
        assert torch.allclose(got[live].float(), want, rtol=2 ** -7, atol=2 ** -8 * float(added.float().abs().max()))


def test_refusals_leave_the_outputs_untouched(K):
    from asr_chinese_e2e_amd._lib import AsrHipError
    logits, in_len, _, _ = reference(3, 9, 64, 1.0, torch.float32)
    x = torch.from_numpy(logits).to(DEV)
    n = _i32(in_len)
    keep = torch.full_like(x, 5.0)
    both = torch.full((12, 9, 64), 5.0, device=DEV)      # logits and gradient block inside one buffer, overlapping
    for kw in (dict(grad_scale=float("nan")), dict(grad_scale=float("inf"))):
        with pytest.raises(AsrHipError):
            K.cr_ctc(x, n, dlogits=keep, **kw)
    with pytest.raises(AsrHipError):      # the gradient block is the logits
        K.cr_ctc(keep, n, dlogits=keep)
    with pytest.raises(AsrHipError):      # ... or overlaps them
        K.cr_ctc(both[:6], n, dlogits=both[3:9])
    with pytest.raises(AsrHipError):      # V < 2
        K.cr_ctc(keep[:, :, :1].contiguous(), n, dlogits=torch.full((6, 9, 1), 5.0, device=DEV))
    with pytest.raises(ValueError):
        K.cr_ctc(x, n, accumulate=True)
    with pytest.raises(ValueError):
        K.cr_ctc(x[:5], n[:5])
    with pytest.raises(ValueError):
        K.cr_ctc(x, n, dlogits=keep.to(torch.bfloat16))
    torch.cuda.synchronize()
    assert bool((keep == 5.0).all()) and bool((both == 5.0).all())


# ------------------------------------------------------------------------------------------------ the model
CR_WEIGHT = 0.2
MASK_T, MASK_F = slice(4, 16), slice(2, 10)      # the block of frames and of mel bins the second view has zeroed


@lru_cache(maxsize=None)
def _model_case(dtype):
    """(shape, cfg, sd, batch of one view, batch of two views): the second half is the first with MASK_T frames and MASK_F bins zeroed."""
    from tests.test_model_gpu import oracle_case
    if dtype == "fp32":
        shape = (2, 30, 16, 40, 6)
        over = dict(d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=2, use_decoder=False, ctc_weight=1.0)
        cfg, sd, one = oracle_case(*shape, over, seed=5)
    else:      # the widths the MFMA kernels are built for
        shape = (2, 40, 80, 56, 12)
        over = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=2, use_decoder=False, ctc_weight=1.0)
        cfg, sd, one = oracle_case(*shape, over, seed=9)
    view1 = one["wave"].clone()
    view1[:, MASK_T, :] = 0
    view1[:, :, MASK_F] = 0
    two = {k: torch.cat([v, v]) for k, v in one.items()}
    two["wave"] = torch.cat([one["wave"], view1])
    return shape, cfg, sd, one, two


def _step(cfg, sd, batch, V, dtype, **over):
    from tests.test_model_gpu import build, to_pack
    model = build(cfg, V, "TransformerCTC", dtype=dtype, dropout=0.0, **over).cuda()
    model.load_state_dict(dict(sd))
    model._ensure_engine(DEV)
    model.zero_flat_grads()
    loss, _ = model.train_step(to_pack(batch))
    torch.cuda.synchronize()
    return model, loss


def test_weight_zero_is_todays_step(deterministic_mode):
    """cr_ctc_weight = 0 on a two-view batch: the flat gradient of the step, bit for bit, and nothing of the consistency stage runs."""
    (B, T, F_, V, L), cfg, sd, one, two = _model_case("fp32")
    plain, loss0 = _step(cfg, sd, two, V, "fp32")
    keyed, loss1 = _step(cfg, sd, two, V, "fp32", cr_ctc_weight=0.0)
    assert keyed._engine.cr_ctc is False and keyed._engine.last_cr is None and keyed._cr_mean is None
    assert torch.equal(plain._flat.g.view(torch.int32), keyed._flat.g.view(torch.int32)) and torch.equal(loss0, loss1)
    assert float(plain._flat.g.abs().max()) > 0


def test_identical_views_add_nothing():
    """cr_ctc_weight > 0, dropout 0, both halves the same rows: the loss and the flat gradient of the plain step on those rows, as numbers
    (the gradient takes the out-of-place path), and metrics.cr == 0."""
    from tests.test_model_gpu import make_opt, to_pack
    (B, T, F_, V, L), cfg, sd, one, two = _model_case("fp32")
    same = {k: torch.cat([v, v]) for k, v in one.items()}
    plain, loss0 = _step(cfg, sd, same, V, "fp32")
    keyed, loss1 = _step(cfg, sd, same, V, "fp32", cr_ctc_weight=CR_WEIGHT)
    frame, cr = keyed._engine.last_cr
    assert frame.shape == (B, T) and cr.shape == (B,) and bool((cr == 0).all()) and bool((frame == 0).all())
    assert abs(float(loss1[0]) - float(loss0[0])) <= 1e-6 * abs(float(loss0[0]))
    g0, g1 = plain._flat.g.float().cpu().numpy(), keyed._flat.g.float().cpu().numpy()
    gmax = float(np.abs(g0).max())
    assert gmax > 0 and np.allclose(g1, g0, rtol=3e-4, atol=3e-6 * max(gmax, 1.0))
    metrics, _ = keyed.iterate(to_pack(same), optimizer=make_opt(keyed, cfg, 25), is_train=True)
    assert float(metrics.cr) == 0.0


def _oracle(cfg, sd, batch, weight):
    """R.ctc_loss over all rows / rows + weight * mean_p cr[p] through oracle.ref_model's encoder, with autograd."""
    from oracle import ref_model as R
    tr = R.RefTrainer(sd, cfg, warmup=25)
    leaves = {k: tr.sd[k].detach().clone().requires_grad_(True) for k in tr.trainable}
    s = dict(tr.sd)
    s.update(leaves)
    enc = R.encoder_forward(s, cfg, batch["wave"], batch["wave_len"])
    logits = R.ctc_logits(s, enc)
    ctc = R.ctc_loss(logits, batch["wave_len"], batch["tgt_for_input"], batch["tgt_len"])
    frame, cr = C.terms(logits, batch["wave_len"].numpy())
    loss = ctc + weight * cr.mean()
    grads = torch.autograd.grad(loss, [leaves[k] for k in tr.trainable], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(tr.trainable, grads)}
    return float(loss.detach()), float(ctc.detach()), cr.detach().numpy(), grads


@lru_cache(maxsize=None)
def _oracle_cached(dtype):
    shape, cfg, sd, one, two = _model_case(dtype)
    return _oracle(cfg, sd, two, CR_WEIGHT)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_matches_the_oracle(dtype):
    """cr_ctc_weight = 0.2 on a two-view batch: the loss and every gradient tensor against the oracle, at the gates of the CTC-only model
    in tests/test_model_gpu.py (fp32: loss 1e-4, gradients rtol 3e-4 / atol 3e-6 gmax; bf16: loss 1e-3, cosine 0.999, norm within 3 %)."""
    from tests.test_model_gpu import BF16_LOSS_RTOL, bf16_gradient_gate, make_opt, to_pack
    (B, T, F_, V, L), cfg, sd, one, two = _model_case(dtype)
    want_loss, want_ctc, want_cr, grads = _oracle_cached(dtype)
    print(dtype, "oracle loss", want_loss, "ctc", want_ctc, "cr", want_cr)
    assert float(want_cr.mean()) > 1e-3      # the term is not negligible
    model, loss = _step(cfg, sd, two, V, dtype, cr_ctc_weight=CR_WEIGHT)
    frame, cr = model._engine.last_cr
    print(dtype, "loss", float(loss[0]), "cr", cr.cpu().numpy())
    rel = abs(float(loss[0]) - want_loss) / abs(want_loss)
    if dtype == "fp32":
        assert rel < 1e-4, (float(loss[0]), want_loss)
        assert np.allclose(cr.cpu().numpy(), want_cr, rtol=1e-4, atol=1e-6)
        gmax = max(float(g.abs().max()) for g in grads.values())
        for n, p in model.named_parameters():
            assert np.allclose(p.grad.cpu().numpy(), grads[n].numpy(), rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), n
    else:
        worst, worst_name, ratio = bf16_gradient_gate(model, dict(grads=grads), "cr_ctc")
        print("bf16 worst cosine", worst, worst_name, "norm ratio", ratio, "loss rel", rel)
        assert rel < BF16_LOSS_RTOL, (float(loss[0]), want_loss)
    # metrics.cr is the mean over the batch's pairs
    model2, _ = _step(cfg, sd, two, V, dtype, cr_ctc_weight=CR_WEIGHT)
    metrics, _ = model2.iterate(to_pack(two), optimizer=make_opt(model2, cfg, 25), is_train=True)
    want_mean = float(model2._engine.last_cr[1].mean())
    assert abs(float(metrics.cr) - want_mean) <= 1e-6 * max(1.0, want_mean) and want_mean > 1e-3
    # evaluation is unchanged: no consistency term, no `cr`
    ev, _ = model2.iterate(to_pack(two), is_train=False)
    assert "cr" not in ev


def test_overlap_on_and_off_give_the_same_gradient(monkeypatch):
    """The hand-over to the weight-gradient stream must come after the consistency gradient is added (ASR_WGRAD_OVERLAP is read when the
    engine is built): both settings against each other and against the oracle, at the fp32 gates."""
    (B, T, F_, V, L), cfg, sd, one, two = _model_case("fp32")
    want_loss, _, _, grads = _oracle_cached("fp32")
    got = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("ASR_WGRAD_OVERLAP", flag)
        model, loss = _step(cfg, sd, two, V, "fp32", cr_ctc_weight=CR_WEIGHT)
        assert model._engine.overlap_wgrad == (flag == "1")
        got[flag] = ({n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters()}, float(loss[0]))
    assert abs(got["1"][1] - got["0"][1]) <= 1e-6 * abs(got["0"][1])
    gmax = max(float(g.abs().max()) for g in grads.values())
    for n in got["0"][0]:
        assert np.allclose(got["1"][0][n], got["0"][0][n], rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), n
    for n in ("ctc_lo.weight", "ctc_lo.bias"):      # the head's gradient reads the block both gradients went into
        for flag in ("1", "0"):
            assert np.allclose(got[flag][0][n], grads[n].numpy(), rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), (n, flag)


def test_odd_batch_is_refused():
    from tests.test_model_gpu import build, to_pack
    (B, T, F_, V, L), cfg, sd, one, two = _model_case("fp32")
    model = build(cfg, V, "TransformerCTC", dtype="fp32", dropout=0.0, cr_ctc_weight=CR_WEIGHT).cuda()
    model.load_state_dict(dict(sd))
    with pytest.raises(ValueError, match="odd"):
        model.train_step(to_pack({k: v[:3] for k, v in two.items()}))


# ------------------------------------------------------------------------------------------------ the loader
POLICY = "t2x20,f2x10"


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_loader_yields_two_views(dtype):
    from asr_chinese_e2e_amd.data_handler import AudioParser, BucketedWaveLoader, specaug
    from tests.test_specaug_gpu import N_UTT, corpus
    ds = corpus(16000, seed=1)
    parser = AudioParser(n_mels=23, lfr_m=4, lfr_n=3, device=DEV)
    lkw = dict(parser=parser, dtype=dtype, shuffle=True, seed=5, bucket_size=6, spec_augment=POLICY)
    one, two = BucketedWaveLoader(ds, 3, **lkw), BucketedWaveLoader(ds, 3, views=2, **lkw)
    policy = specaug.as_policy(POLICY)
    differ = 0
    for epoch in range(2):
        table1 = specaug.draw(5, epoch, N_UTT, policy, view=1)
        seen = 0
        for a, b in zip(one, two):
            B = a.wave.shape[0]
            assert B == 3 and b.wave.shape[0] == 2 * B and b.wave.shape[1:] == a.wave.shape[1:]
            assert _same_bits(b.wave[:B], a.wave)      # view 0 is the one-view loader's batch, bit for bit
            for k in ("wave_len", "tgt_len", "tgt_for_input", "tgt_for_metric"):
                assert torch.equal(b[k][:B], a[k]) and torch.equal(b[k][B:], a[k]), k
            # view 1 = parse_batch of the same waveforms with the second view's ranges
            idx = [int(v) - 4 for v in a.tgt_for_input[:, 0]]      # the first label is the utterance's index (corpus)
            waves = [ds.wave(i) for i in idx]
            S = max(w.size for w in waves)
            wav = torch.zeros(B, S)
            for r, w in enumerate(waves):
                wav[r, :w.size] = torch.from_numpy(w)
            sizes = [w.size for w in waves]
            rows = parser.spec_ranges(policy, table1[idx], sizes)
            want, want_len = parser.parse_batch(wav.to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV), dtype, spec_ranges=rows, spec_policy=policy)
            assert _same_bits(b.wave[B:], want) and torch.equal(b.wave_len[B:], want_len.long())
            differ += int(not _same_bits(b.wave[B:], b.wave[:B]))
            seen += B
        assert seen == N_UTT
    assert differ >= 1      # the second view differs from the first somewhere
    # without a policy the two views are the same rows
    plain = BucketedWaveLoader(ds, 3, parser=parser, dtype=dtype, shuffle=False, views=2)
    for b in plain:
        assert b.wave.shape[0] == 6 and _same_bits(b.wave[:3], b.wave[3:]) and torch.equal(b.tgt_len[:3], b.tgt_len[3:])


def test_iterate_on_a_two_view_batch_reports_cr():
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import AudioParser, BucketedWaveLoader, Vocab
    from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt
    from tests.test_specaug_gpu import corpus
    ds = corpus(16000, seed=1)
    parser = AudioParser(n_mels=23, lfr_m=4, lfr_n=3, device=DEV)
    loader = BucketedWaveLoader(ds, 3, parser=parser, dtype=torch.float32, shuffle=True, seed=5, bucket_size=6, spec_augment=POLICY, views=2)
    mc = Models.TransformerCTC.get_default_config()()
    mc.fn_build(dict(n_mels=23, lfr_m=4, layer_num=1, d_model=32, hidden_size=8, num_head=4, ff_size=64, dtype="fp32", cr_ctc_weight=CR_WEIGHT))
    model = Models.TransformerCTC(mc, Vocab.synthetic(30)).cuda()
    opt = NoamOpt(mc.d_model, 1, 25, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
    pack = next(iter(loader))
    metrics, _ = model.iterate(pack, optimizer=opt, is_train=True)
    torch.cuda.synchronize()
    cr = float(metrics.cr)
    assert np.isfinite(cr) and cr >= 0.0 and np.isfinite(float(metrics.loss))
    assert model._engine.last_cr[0].shape == (3, pack.wave.shape[1])
