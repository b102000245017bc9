"""MWER for the CTC head on the GPU: asr_mwer_errors / asr_ctc_mwer_lattice / asr_ctc_mwer_grad against their definition
(tests/mwer_ref.py) on f32 and bf16 logits, the exact properties of the sparse gradient on bytes, and the training step of a small
TransformerCTC with config.mwer_weight against the CPU oracle.

Tolerances.  err: integers.  ll differences, post, risk: the definition is also evaluated in float32 on the CPU; the kernels may be
further from the float64 definition than that run by a factor 4 (another summation order), floor 1e-6.  The gradient divided by
max(1, max_i e_i): the gates of tests/test_kernels_gpu.py::test_ctc (f32: rtol 1e-3, atol 2e-5; bf16: rtol 1e-2, atol 4e-3).  The measured
ratios are printed (pytest -s) and attached to the test's report (record_property); profiles/mwer_parity.json keeps one run of them."""
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ctc_range_cases as RC  # noqa: E402
from tests import mwer_ref as M  # noqa: E402

DEV = "cuda"
GATES = {torch.float32: dict(rtol=1e-3, atol=2e-5), torch.bfloat16: dict(rtol=1e-2, atol=4e-3)}
DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = 768.0      # exact in bf16
CASES = ("tiny", "ragged", "wave_edge", "long", "vocab", "blank")


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int32))).to(DEV)


def _rows(rng, B, N, Lh, V, lists):
    hyp, hyp_len = np.zeros((B, N, Lh), np.int32), np.full((B, N), -1, np.int32)
    for b in range(B):
        for i, h in enumerate(lists[b]):
            if h is not None:
                hyp[b, i, :len(h)] = h
                hyp_len[b, i] = len(h)
    return hyp, hyp_len


@lru_cache(maxsize=None)
def make_case(name):
    """(logits f32 (B, T, V) numpy, in_len, hyp, hyp_len, ref, ref_len) of the issue's shapes (B, T, V, N, Lh)."""
    rng = np.random.RandomState({n: 11 + k for k, n in enumerate(CASES)}[name])
    tok = lambda n, V: [int(v) for v in rng.randint(1, V, size=n)]      # noqa: E731

    def varied(h, at, V):      # h with the tokens at `at` replaced by other ids
        h = list(h)
        for j in at:
            h[j] = 1 + h[j] % (V - 1)
        return h
    scale = 2.0
    if name == "tiny":                     # (1, 1, 2, 1, 1)
        B, T, V, N, Lh = 1, 1, 2, 1, 1
        lists, refs, in_len = [[[1]]], [[1]], [1]
    elif name == "ragged":                 # (3, 37, 11, 4, 8): in_len 37 / 0 / 1; empty entry, repeats a a, the reference itself, an absent rank
        B, T, V, N, Lh = 3, 37, 11, 4, 8
        refs = [tok(6, V), tok(3, V), [4]]
        lists = [[[], [3, 3, 5, 5, 5, 2], refs[0], None], [tok(2, V), [], refs[1], None], [[], [4], [4, 7], None]]
        in_len = [37, 0, 1]
    elif name == "wave_edge":              # (2, 130, 64, 16, 40): S = 63 / 65 / 67 around one wave's 64 lanes
        B, T, V, N, Lh = 2, 130, 64, 16, 40
        scale = 0.5      # flat enough that several entries of a list carry posterior mass
        refs = [tok(33, V), tok(20, V)]
        lists = []
        for b in range(B):
            rows = [tok(31, V), tok(32, V), tok(33, V), list(refs[b]), tok(40, V), [], tok(1, V)]
            rows += [tok(int(rng.randint(0, 41)), V) for _ in range(N - len(rows) - 1)] + [None]
            lists.append(rows)
        lists[1][4] = list(refs[1][:10]) + list(refs[1][11:])      # one deletion away from the reference
        in_len = [130, 97]
    elif name == "long":                   # (1, 600, 5, 2, 255): a 255-token entry
        B, T, V, N, Lh = 1, 600, 5, 2, 255
        scale = 0.5
        long = tok(255, V)      # the two entries and the reference are a few substitutions apart, so both entries carry mass
        refs = [varied(long, (3, 77, 200), V)[:250]]
        lists = [[long, varied(long, (10, 100, 101, 254), V)]]
        in_len = [600]
    elif name == "vocab":                  # (2, 40, 4232, 4, 12): rows padded to ld = 4288
        B, T, V, N, Lh = 2, 40, 4232, 4, 12
        scale = 0.5
        refs = [tok(9, V), tok(12, V)]
        lists = [[list(refs[b]), list(refs[b][:-1]) + [V - 1], varied(refs[b], (0, 4, 5), V), list(refs[b][1:])] for b in range(B)]
        in_len = [40, 33]
    else:                                  # blank-dominated posteriors: batch A of tests/ctc_range_cases.py (100 labels in 250 frames, boost 12)
        c = RC.range_case("A")
        B, T, V = c.logits.shape
        N, Lh = 4, 100
        refs = [[int(v) for v in c.labels[b, :c.lab_len[b]]] for b in range(B)]
        lists = []
        for b in range(B):
            r = refs[b]      # equal lengths: under a dominant blank one token less is e^12 more probable and would take all the mass
            lists.append([list(r), varied(r, (len(r) // 2,), V), varied(r, (len(r) // 4, len(r) - 1), V), list(r)] if r else [[], [], [], []])
        logits = c.logits.astype(np.float32)
        hyp, hyp_len = _rows(rng, B, N, Lh, V, lists)
        Lr = max(len(r) for r in refs)
        ref = np.zeros((B, Lr), np.int32)
        for b, r in enumerate(refs):
            ref[b, :len(r)] = r
        return logits, np.asarray(c.in_len, np.int32), hyp, hyp_len, ref, np.array([len(r) for r in refs], np.int32)
    logits = (rng.randn(B, T, V) * scale).astype(np.float32)
    hyp, hyp_len = _rows(rng, B, N, Lh, V, lists)
    Lr = max(len(r) for r in refs)
    ref = np.zeros((B, Lr), np.int32)
    for b, r in enumerate(refs):
        ref[b, :len(r)] = r
    return logits, np.array(in_len, np.int32), hyp, hyp_len, ref, np.array([len(r) for r in refs], np.int32)


@lru_cache(maxsize=None)
def reference(name, dtype):
    """The definition on the values the kernel reads in `dtype`: (float64 run, float32 run).  Computed once, shared, never changed."""
    logits, in_len, hyp, hyp_len, ref, ref_len = make_case(name)
    x = torch.from_numpy(logits).to(dtype)
    return (M.autograd(x, in_len, hyp, hyp_len, ref, ref_len), M.autograd(x, in_len, hyp, hyp_len, ref, ref_len, dtype=torch.float32))


def device_case(name, dtype, ld=None):
    logits, in_len, hyp, hyp_len, ref, ref_len = make_case(name)
    B, T, V = logits.shape
    x = torch.from_numpy(logits).to(dtype)
    if ld is not None:
        buf = torch.full((B, T, ld), SENTINEL, dtype=dtype)
        buf[:, :, :V] = x
        x = buf.to(DEV)[:, :, :V]
    else:
        x = x.to(DEV)
    return x, _i32(in_len), _i32(hyp), _i32(hyp_len), _i32(ref), _i32(ref_len)


def _ll_diffs(ll, present):
    """ll_i - ll of the first entry taking part, per utterance; 0 elsewhere."""
    out = np.zeros_like(ll)
    for b in range(ll.shape[0]):
        on = np.flatnonzero(present[b])
        if on.size:
            out[b, on] = ll[b, on] - ll[b, on[0]]
    return out


def _emax(want):
    return np.maximum(1, (want["err"] * want["present"]).max(1)).astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_kernels_match_the_definition(K, name, dtype, record_property):
    want, want32 = reference(name, dtype)
    ld = 4288 if name == "vocab" else None
    x, in_len, hyp, hyp_len, ref, ref_len = device_case(name, dtype, ld)
    B, T, V = x.shape
    dbuf = torch.full((B, T, x.stride(1)), SENTINEL, dtype=dtype, device=DEV)      # the gradient goes into rows laid out like the logits'
    out = K.ctc_mwer(x, in_len, hyp, hyp_len, ref, ref_len, dlogits=dbuf[:, :, :V])
    torch.cuda.synchronize()
    err, flags = M.errors(*make_case(name)[2:])
    assert out["err"].cpu().numpy().tolist() == err.tolist() and out["flags"].cpu().numpy().tolist() == flags.tolist()
    present = out["present"].cpu().numpy()
    assert present.tolist() == want["present"].tolist()
    ll = out["ll"].cpu().numpy()
    assert np.isneginf(ll[present == 0]).all() and np.isfinite(ll[present == 1]).all()
    row = dict(case=name, dtype=str(dtype))
    got = dict(ll=_ll_diffs(ll, present), post=out["post"].double().cpu().numpy(), risk=out["risk"].double().cpu().numpy())
    for k in ("ll", "post", "risk"):
        w64, w32 = (_ll_diffs(w["ll"], present) for w in (want, want32)) if k == "ll" else (want[k], want32[k])
        dev_k, dev_32 = float(np.abs(got[k] - w64).max()), float(np.abs(w32 - w64).max())
        row[k] = dict(kernel=dev_k, float32=dev_32, ratio=dev_k / max(dev_32, 1e-300))
        print(name, dtype, k, row[k])
        assert dev_k <= max(4.0 * dev_32, 1e-6), (k, dev_k, dev_32)
    assert (out["coef"].cpu().numpy()[present == 0] == 0).all() and (got["post"][present == 0] == 0).all()
    g = out["dlogits"].double().cpu().numpy() / _emax(want)[:, None, None]
    w = want["grad"] / _emax(want)[:, None, None]
    row["grad_max_abs_dev"] = float(np.abs(g - w).max())
    row["grad_max"] = float(np.abs(w).max())
    record_property("mwer_parity", row)
    print("mwer_parity", json.dumps(row))
    assert np.allclose(g, w, **GATES[dtype]), (np.abs(g - w).max(), np.abs(w).max())
    # exact: untouched cells and rows past in_len are zero, and the padding columns keep their sentinel
    mask = M.touched(*make_case(name)[2:4], present, make_case(name)[1], T, V)
    raw = out["dlogits"].cpu()
    assert (raw.float().numpy()[~mask] == 0).all()
    if ld is not None:
        assert dbuf.shape[2] == ld > V and bool((dbuf[:, :, V:] == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ("ragged", "wave_edge", "vocab"))
def test_bytes(K, name, dtype):
    """accumulate = 1 over a random prior content leaves every untouched byte, and adds in f32 on the touched cells; two runs write the same
    bytes; ctc_mwer is its three stages."""
    ld = 4288 if name == "vocab" else None
    x, in_len, hyp, hyp_len, ref, ref_len = device_case(name, dtype, ld)
    B, T, V = x.shape
    ldx = x.stride(1)
    a = K.ctc_mwer(x, in_len, hyp, hyp_len, ref, ref_len, grad_scale=0.37)
    b = K.ctc_mwer(x, in_len, hyp, hyp_len, ref, ref_len, grad_scale=0.37)
    for k in ("ll", "post", "coef", "risk", "present", "err", "flags", "dlogits"):
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k
    # the three stages alone, the scale through the device scalar
    err, flags = K.mwer_errors(hyp, hyp_len, ref, ref_len)
    lat = K.ctc_mwer_lattice(x, in_len, hyp, hyp_len, err)
    div = torch.tensor([2.0], device=DEV)
    dl = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=DEV)
    K.ctc_mwer_grad(dl, in_len, hyp, hyp_len, lat["coef"], lat["ws"], grad_scale=0.74, grad_scale_div=div)
    assert torch.equal(err, a["err"]) and torch.equal(flags, a["flags"])
    for k in ("ll", "post", "coef", "risk", "present"):
        assert torch.equal(lat[k].view(torch.uint8), a[k].view(torch.uint8)), k
    assert torch.equal(dl.contiguous().view(torch.uint8), a["dlogits"].contiguous().view(torch.uint8))
    # accumulate = 1 over a random prior
    present = a["present"].cpu().numpy()
    mask = torch.from_numpy(M.touched(*make_case(name)[2:4], present, make_case(name)[1], T, V))
    g = torch.Generator().manual_seed(3)
    prior_full = torch.randn(B, T, ldx, generator=g).to(dtype)
    buf = prior_full.to(DEV)
    acc = buf[:, :, :V]
    K.ctc_mwer_grad(acc, in_len, hyp, hyp_len, lat["coef"], lat["ws"], grad_scale=0.37, accumulate=True)
    got_full = buf.cpu()
    got, prior = got_full[:, :, :V], prior_full[:, :, :V]
    assert torch.equal(got_full[:, :, V:].contiguous().view(torch.uint8), prior_full[:, :, V:].contiguous().view(torch.uint8))
    assert torch.equal(got[~mask].view(torch.uint8), prior[~mask].view(torch.uint8))
    added = a["dlogits"].cpu()
    if dtype == torch.float32:      # the same f32 value is added in f32: exact
        assert torch.equal(got[mask], prior[mask] + added[mask])
    else:                           # the f32 sum is rounded once to bf16; `added` was rounded on its own (2^-9 relative each)
        want = prior[mask].float() + added[mask].float()
        assert torch.allclose(got[mask].float(), want, rtol=2 ** -7, atol=2 ** -8 * float(added.float().abs().max()))
    assert bool((added[mask] != 0).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ("wave_edge", "vocab"))
def test_on_top_of_the_ctc_gradient(K, name, dtype):
    """The engine's order: lattice, the CTC kernels in place over the logits, the risk gradient added on top = the sum of the two references."""
    import torch.nn.functional as F
    logits, in_len_h, hyp_h, hyp_len_h, ref_h, ref_len_h = make_case(name)
    want, _ = reference(name, dtype)
    scale = 1.0 / float(_emax(want).max())
    ld = 4288 if name == "vocab" else None
    x, in_len, hyp, hyp_len, ref, ref_len = device_case(name, dtype, ld)
    B, T, V = x.shape
    xc = torch.from_numpy(logits).to(dtype).double().requires_grad_(True)
    nll = F.ctc_loss(F.log_softmax(xc, -1).transpose(0, 1), torch.from_numpy(ref_h).long(), torch.from_numpy(in_len_h).long(),
                     torch.from_numpy(ref_len_h).long(), blank=0, reduction="none")
    ctc_grad, = torch.autograd.grad(nll.sum(), xc)
    for b in range(B):
        ctc_grad[b, in_len_h[b]:] = 0
    err, _ = K.mwer_errors(hyp, hyp_len, ref, ref_len)
    lat = K.ctc_mwer_lattice(x, in_len, hyp, hyp_len, err)
    got_nll, _ = K.ctc_fwd_bwd(x, in_len, ref, ref_len, K.Workspace(DEV), dlogits=x)
    K.ctc_mwer_grad(x, in_len, hyp, hyp_len, lat["coef"], lat["ws"], grad_scale=scale, accumulate=True)
    torch.cuda.synchronize()
    assert np.allclose(got_nll.cpu().numpy(), nll.detach().numpy(), rtol=1e-4 if dtype == torch.float32 else 1e-3)
    total = ctc_grad.numpy() + scale * want["grad"]
    print(name, dtype, "largest scaled risk gradient", np.abs(scale * want["grad"]).max(), "largest CTC gradient", float(ctc_grad.abs().max()))
    assert np.abs(scale * want["grad"]).max() > 10 * GATES[torch.float32]["atol"]      # the risk term is visible at the f32 gate
    assert np.allclose(x.double().cpu().numpy(), total, **GATES[dtype])


def test_wrapper_refusals(K):
    x, in_len, hyp, hyp_len, ref, ref_len = device_case("ragged", torch.float32)
    err, _ = K.mwer_errors(hyp, hyp_len, ref, ref_len)
    lat = K.ctc_mwer_lattice(x, in_len, hyp, hyp_len, err)
    from asr_chinese_e2e_amd._lib import AsrHipError
    with pytest.raises(ValueError):
        K.mwer_errors(hyp.long(), hyp_len, ref, ref_len)
    with pytest.raises(ValueError):
        K.ctc_mwer_lattice(x, in_len, hyp[:2], hyp_len[:2], err)
    with pytest.raises(ValueError):
        K.ctc_mwer(x, in_len, hyp, hyp_len, ref, ref_len, accumulate=True)
    keep = torch.full_like(x, 5.0)
    for kw in (dict(grad_scale=float("nan")), dict(grad_scale=float("inf")), dict(blank=x.shape[2])):
        with pytest.raises(AsrHipError):
            K.ctc_mwer_grad(keep, in_len, hyp, hyp_len, lat["coef"], lat["ws"], **kw)
    with pytest.raises(AsrHipError):
        K.ctc_mwer_grad(keep, in_len, hyp, hyp_len, lat["coef"], lat["ws"][:-16])
    big = torch.zeros(2, 17, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(AsrHipError):
        K.mwer_errors(big, torch.zeros(2, 17, dtype=torch.int32, device=DEV), ref[:2], ref_len[:2])
    torch.cuda.synchronize()
    assert bool((keep == 5.0).all())


# ------------------------------------------------------------------------------------------------ the model
def _model_case(dtype, seed=5):
    from tests.test_model_gpu import oracle_case
    if dtype == "fp32":
        over = dict(d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=2, use_decoder=False, ctc_weight=1.0)
        return (4, 30, 16, 40, 6), oracle_case(4, 30, 16, 40, 6, over, seed=seed)
    # the widths the MFMA kernels are built for.  A freshly drawn head emits a token on almost every frame, and an entry longer than the row
    # (2 * label width + 8 tokens) takes part in nothing: 40 full frames with transcripts of the length of what the model hears (_heard)
    over = dict(d_model=512, hidden_size=64, num_head=8, ff_size=1024, layer_num=2, use_decoder=False, ctc_weight=1.0)
    cfg, sd, batch = oracle_case(4, 40, 80, 56, 16, over, seed=9, ragged=False)
    return (4, 40, 80, 56, 16), (cfg, sd, _heard(cfg, sd, batch, 56, "bf16"))


def _heard(cfg, sd, batch, V, dtype):
    """The batch with transcripts a few deletions away from the model's own best hypothesis (ids below 4 and two more tokens dropped: a
    deletion keeps a sequence alignable), so that the entries of a list differ in their errors and the risk has a gradient."""
    from tests.test_model_gpu import build, to_pack
    model = build(cfg, V, "TransformerCTC", dtype=dtype).cuda()
    model.load_state_dict(dict(sd))
    lists = model.ctc_prefix_beam_search(to_pack(batch), beam_size=4, nbest=1, frame_topk=7)
    refs = []
    for ent in lists:
        top = [t for t in ent[0]["yseq"] if t >= 4]
        refs.append([t for j, t in enumerate(top) if len(top) <= 4 or j not in (1, len(top) // 2)])
    assert all(len(r) >= 2 for r in refs)
    tgt = torch.zeros(len(refs), max(len(r) for r in refs), dtype=torch.long)
    for b, r in enumerate(refs):
        tgt[b, :len(r)] = torch.tensor(r)
    return dict(batch, tgt_for_input=tgt, tgt_len=torch.tensor([len(r) for r in refs], dtype=torch.long))


def _step(cfg, sd, batch, V, dtype, **over):
    from tests.test_model_gpu import build, to_pack
    model = build(cfg, V, "TransformerCTC", dtype=dtype, **over).cuda()
    model.load_state_dict(dict(sd))
    pack = to_pack(batch)
    model._ensure_engine(DEV)
    model.zero_flat_grads()
    loss, _ = model.train_step(pack)
    torch.cuda.synchronize()
    return model, loss


def test_weight_zero_is_todays_step(deterministic_mode):
    """mwer_weight = 0, with every other key set: the flat gradient of the step, bit for bit, and nothing of the MWER stage runs."""
    (B, T, F_, V, L), (cfg, sd, batch) = _model_case("fp32")
    plain, loss0 = _step(cfg, sd, batch, V, "fp32")
    keyed, loss1 = _step(cfg, sd, batch, V, "fp32", mwer_weight=0.0, mwer_nbest=2, mwer_beam=3, mwer_frame_topk=5, mwer_blank_skip=0.9)
    assert keyed._engine.mwer is None and keyed._engine.last_mwer is None and keyed._mwer_mean is None
    assert torch.equal(plain._flat.g.view(torch.int32), keyed._flat.g.view(torch.int32)) and torch.equal(loss0, loss1)
    assert float(plain._flat.g.abs().max()) > 0


def _oracle(cfg, sd, batch, lists, weight):
    """R.ctc_loss / B + weight * mean risk on the lists the device search made, through oracle.ref_model's encoder, with autograd."""
    from oracle import ref_model as R
    tok, ln, err = (t.cpu().numpy() for t in lists)
    tr = R.RefTrainer(sd, cfg, warmup=25)
    leaves = {k: tr.sd[k].detach().clone().requires_grad_(True) for k in tr.trainable}
    s = dict(tr.sd)
    s.update(leaves)
    enc = R.encoder_forward(s, cfg, batch["wave"], batch["wave_len"])
    logits = R.ctc_logits(s, enc)
    ctc = R.ctc_loss(logits, batch["wave_len"], batch["tgt_for_input"], batch["tgt_len"])
    risk, _ = M.risk_terms(logits, batch["wave_len"].numpy(), tok, ln, err)
    loss = ctc + weight * risk.mean()
    grads = torch.autograd.grad(loss, [leaves[k] for k in tr.trainable], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(tr.trainable, grads)}
    return float(loss.detach()), float(ctc.detach()), risk.detach().numpy(), grads


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_matches_the_oracle(dtype):
    """mwer_weight = 0.5: the loss and every gradient tensor against the oracle on the step's own lists, at the gates of the CTC-only model
    in tests/test_model_gpu.py (fp32: loss 1e-4, gradients rtol 3e-4 / atol 3e-6 gmax; bf16: loss 1e-3, cosine 0.999, norm within 3 %)."""
    from tests.test_model_gpu import BF16_LOSS_RTOL, bf16_gradient_gate, make_opt, to_pack
    (B, T, F_, V, L), (cfg, sd, batch) = _model_case(dtype)
    model, loss = _step(cfg, sd, batch, V, dtype, mwer_weight=0.5)
    tok, ln, err, post, risk = model._engine.last_mwer
    assert tok.shape[:2] == (B, 4) and tok.shape[2] <= 255
    print(dtype, "lengths", ln.cpu().numpy().tolist(), "errors", err.cpu().numpy().tolist(), "posteriors", post.cpu().numpy().round(4).tolist())
    assert int((ln >= 0).sum()) >= 2 * B      # the lists are lists
    assert int(((post > 1e-3).sum(1) >= 2).sum()) >= B // 2      # ... and in half of them more than one entry carries mass
    want_loss, want_ctc, want_risk, grads = _oracle(cfg, sd, batch, (tok, ln, err), 0.5)
    print(dtype, "loss", float(loss[0]), want_loss, "ctc", want_ctc, "risk", risk.cpu().numpy(), want_risk)
    assert float(np.abs(want_risk).max()) > 0.5 and max(float(g.abs().max()) for g in grads.values()) > 0
    ref = dict(grads=grads)
    rel = abs(float(loss[0]) - want_loss) / abs(want_loss)
    if dtype == "fp32":
        assert rel < 1e-4, (float(loss[0]), want_loss)
        assert np.allclose(risk.cpu().numpy(), want_risk, rtol=1e-4, atol=1e-5)
        gmax = max(float(g.abs().max()) for g in grads.values())
        for n, p in model.named_parameters():
            assert np.allclose(p.grad.cpu().numpy(), grads[n].numpy(), rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), n
    else:
        worst, worst_name, ratio = bf16_gradient_gate(model, ref, "mwer")
        print("bf16 worst cosine", worst, worst_name, "norm ratio", ratio, "loss rel", rel)
        assert rel < BF16_LOSS_RTOL, (float(loss[0]), want_loss)
    # metrics.mwer is the definition's mean risk
    model2, _ = _step(cfg, sd, batch, V, dtype, mwer_weight=0.5)
    metrics, _ = model2.iterate(to_pack(batch), optimizer=make_opt(model2, cfg, 25), is_train=True)
    want_mean = float(model2._engine.last_mwer[4].mean())
    assert abs(float(metrics.mwer) - want_mean) <= 1e-6 * max(1.0, want_mean)
    # bf16 logits are 2^-9 |x| <= 0.016 from the oracle's; over 40 frames an entry's ll moves by ~0.05 and its posterior by ~5 %, and the
    # errors of a list's entries are a few apart: the risk may move by a few per cent, bounded here at 5 %
    assert abs(want_mean - float(want_risk.mean())) <= (1e-4 if dtype == "fp32" else 5e-2) * max(1.0, float(want_risk.mean()))


def test_overlap_on_and_off_give_the_same_gradient(monkeypatch):
    """The hand-over to the weight-gradient stream must come after the risk gradient is added (ASR_WGRAD_OVERLAP is read when the engine
    is built).  Both against the oracle's gates of the fp32 CTC-only model, and the head's gradient against each other."""
    (B, T, F_, V, L), (cfg, sd, batch) = _model_case("fp32")
    got = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("ASR_WGRAD_OVERLAP", flag)
        model, loss = _step(cfg, sd, batch, V, "fp32", mwer_weight=0.5)
        assert model._engine.overlap_wgrad == (flag == "1")
        got[flag] = ({n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters()}, float(loss[0]),
                     tuple(t.cpu().numpy() for t in model._engine.last_mwer[:3]))
    for a, b in zip(got["1"][2], got["0"][2]):
        assert np.array_equal(a, b)
    assert abs(got["1"][1] - got["0"][1]) <= 1e-6 * abs(got["0"][1])
    gmax = max(float(np.abs(g).max()) for g in got["0"][0].values())
    for n in got["0"][0]:
        assert np.allclose(got["1"][0][n], got["0"][0][n], rtol=3e-4, atol=3e-6 * max(gmax, 1.0)), n


def test_mwer_risk_is_the_search_plus_the_definition():
    from tests.test_model_gpu import build, to_pack
    (B, T, F_, V, L), (cfg, sd, batch) = _model_case("fp32")
    model = build(cfg, V, "TransformerCTC", dtype="fp32").cuda()
    model.load_state_dict(dict(sd))
    pack = to_pack(batch)
    res = model.mwer_risk(pack, nbest=3, beam_size=4, frame_topk=6)
    lists = model.ctc_prefix_beam_search(pack, beam_size=4, nbest=3, frame_topk=6)
    with torch.no_grad():
        logits = model.forward(pack).ctc_logits.float().cpu()
    refs = [[int(v) for v in batch["tgt_for_input"][b, :int(batch["tgt_len"][b])]] for b in range(B)]
    from asr_chinese_e2e_amd import kernels
    Lh = min(T, 255, 2 * kernels.dec_preprocess(pack.tgt_for_input.contiguous(), 2, 3)[2].shape[1] + 8)      # the row width of the step's lists
    for b in range(B):
        assert res[b]["nbest"] == [e["yseq"][:Lh] for e in lists[b]] and len(res[b]["nbest"]) >= 2
        N = len(res[b]["nbest"])
        hyp, hyp_len = np.zeros((1, N, Lh), np.int32), np.zeros((1, N), np.int32)
        for i, e in enumerate(lists[b]):
            hyp[0, i, :min(len(e["yseq"]), Lh)] = e["yseq"][:Lh]
            hyp_len[0, i] = len(e["yseq"])      # the true length: an entry longer than the row takes part in nothing
        ref = np.array([refs[b] or [0]], np.int32)
        want = M.autograd(logits[b:b + 1], [int(batch["wave_len"][b])], hyp, hyp_len, ref, [len(refs[b])])
        assert res[b]["errors"] == want["err"][0].tolist()
        assert np.allclose(res[b]["posteriors"], want["post"][0], rtol=1e-4, atol=1e-6) and abs(res[b]["risk"] - want["risk"][0]) <= 1e-4 * max(1.0, want["risk"][0])
    with pytest.raises(ValueError):
        model.mwer_risk(pack, nbest=5, beam_size=4)
    with pytest.raises(ValueError):
        model.mwer_risk(pack, blank_skip=0.0)


def test_config_refusals_before_any_launch():
    from tests.test_model_gpu import build
    (B, T, F_, V, L), (cfg, sd, batch) = _model_case("fp32")
    for kw in (dict(mwer_weight=float("nan")), dict(mwer_weight=-0.5), dict(mwer_weight=0.5, mwer_nbest=1), dict(mwer_weight=0.5, mwer_nbest=5),
               dict(mwer_weight=0.5, mwer_beam=8, mwer_nbest=8, mwer_frame_topk=8), dict(mwer_weight=0.5, mwer_blank_skip=1.5)):
        with pytest.raises(ValueError):
            build(cfg, V, "TransformerCTC", dtype="fp32", **kw)
    from oracle import ref_model as R
    joint = R.default_cfg(n_mels=F_, lfr_m=1, d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=1, ctc_weight=0.3)
    with pytest.raises(ValueError):
        build(joint, V, "TransformerOffical", dtype="fp32", mwer_weight=0.5)
