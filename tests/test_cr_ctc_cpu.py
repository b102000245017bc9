"""CR-CTC without a GPU: the definition (tests/cr_ctc_ref.py) against itself, the second view's SpecAugment table, the binding, and every
refusal that needs no launch (the launcher's on host addresses, kernels.cr_ctc's argument checks, the config keys, the loader's views)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import cr_ctc_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = {3: [9, 0, 1, 8, 0, 1], 1: [12, 9]}      # a zero-length pair, a one-frame pair, views one frame apart (n = min); a length past T is clamped
# the shapes of tests/test_cr_ctc_gpu.py that a CPU run affords in both precisions
CASES = [(P, T, V, spread) for P in (1, 3) for T in (1, 9) for V in (2, 5, 64, 257) for spread in (1.0, 60.0)] + [(1, 2, 4232, 1.0), (1, 2, 4232, 60.0)]


def _case(P, T, V, spread):
    lens = [min(v, T) for v in LENS[P]] if T > 1 else None
    return C.make_case(P, T, V, spread, lens)


@pytest.mark.parametrize("P,T,V,spread", CASES)
def test_closed_form_equals_autograd(P, T, V, spread):
    logits, in_len = _case(P, T, V, spread)
    a, e = C.autograd(logits, in_len), C.explicit(logits, in_len)
    for k in ("frame", "cr", "grad"):
        assert np.allclose(a[k], e[k], rtol=1e-12, atol=1e-14), k
    n = np.minimum(np.clip(in_len[:P], 0, T), np.clip(in_len[P:], 0, T))
    for p in range(P):      # exactly zero past the pair's frames, in both views
        assert (a["grad"][p, n[p]:] == 0).all() and (a["grad"][p + P, n[p]:] == 0).all() and (a["frame"][p, n[p]:] == 0).all()
    assert np.array_equal(e["grad"][:P], -e["grad"][P:])
    if spread == 1.0 and n.max() > 0:
        assert np.abs(a["grad"]).max() > 1e-3      # the case says something


@pytest.mark.parametrize("P,T,V,spread", CASES)
def test_term_is_nonnegative_and_zero_for_identical_views(P, T, V, spread):
    logits, in_len = _case(P, T, V, spread)
    a = C.autograd(logits, in_len)
    assert (a["frame"] >= 0).all() and (a["cr"] >= 0).all()
    same = np.concatenate([logits[:P], logits[:P]])
    for fn in (C.autograd, C.explicit):
        s = fn(same, in_len)
        assert (s["frame"] == 0).all() and (s["cr"] == 0).all()
        # the closed form subtracts equal numbers; autograd sums two terms that cancel up to their rounding
        assert (s["grad"] == 0).all() if fn is C.explicit else np.abs(s["grad"]).max() <= 1e-15


@pytest.mark.parametrize("P,T,V,spread", CASES)
def test_float32_restatement_is_a_usable_yardstick(P, T, V, spread):
    """A sanity check of the yardstick, not of the kernel: float32 within 1e-5 relative of float64.  Relative to the result, or to the
    numbers it is a difference of where these cancel (two saturated views: y_a - y_b ~ 1e-7 is below the float32 spacing of y ~ 1): 1 for the
    gradient, a difference of probabilities, and the largest |lp_a - lp_b| for J, whose terms are such differences times that factor."""
    logits, in_len = _case(P, T, V, spread)
    w64, w32 = C.autograd(logits, in_len), C.autograd(logits, in_len, dtype=torch.float32)
    lp = torch.log_softmax(torch.from_numpy(logits).double(), -1)
    floor = dict(grad=1.0, frame=float((lp[:P] - lp[P:]).abs().max()), cr=float((lp[:P] - lp[P:]).abs().max()))
    for k in ("frame", "cr", "grad"):
        assert np.abs(w32[k] - w64[k]).max() <= 1e-5 * max(np.abs(w64[k]).max(), floor[k]), k
    e32 = C.explicit(logits, in_len, dtype=torch.float32)
    assert np.abs(e32["grad"] - w64["grad"]).max() <= 1e-5 * max(np.abs(w64["grad"]).max(), 1.0)


def test_swapping_the_views_swaps_the_gradient():
    logits, in_len = _case(3, 9, 64, 1.0)
    a = C.autograd(logits, in_len)
    b = C.autograd(np.concatenate([logits[3:], logits[:3]]), np.concatenate([in_len[3:], in_len[:3]]))
    assert np.array_equal(a["frame"], b["frame"]) and np.array_equal(a["grad"][:3], b["grad"][3:]) and np.array_equal(a["grad"][3:], b["grad"][:3])


def test_second_view_draws_its_own_table():
    from asr_chinese_e2e_amd.data_handler import specaug
    policy = specaug.as_policy("wenet")
    seed, epoch, n = 7, 3, 6
    v0 = specaug.draw(seed, epoch, n, policy, view=0)
    assert np.array_equal(v0, specaug.draw(seed, epoch, n, policy))      # view 0 is the one-view table
    import random
    rng = random.Random(f"spec_augment/{seed}/{epoch}")      # ... whose generator string has not changed
    assert v0.reshape(-1).tolist() == [rng.getrandbits(32) for _ in range(n * policy.n_draws)]
    v1 = specaug.draw(seed, epoch, n, policy, view=1)
    assert v1.shape == v0.shape and v1.dtype == v0.dtype and not np.array_equal(v0, v1)
    assert np.array_equal(v1, specaug.draw(seed, epoch, n, policy, view=1))
    frames = [120, 90, 300, 64, 250, 33]
    r0, r1 = (specaug.resolve_batch(policy, v, frames, 80) for v in (v0, v1))
    assert r0.shape == r1.shape and sum(not np.array_equal(a, b) for a, b in zip(r0, r1)) >= 1      # an utterance's resolved ranges differ
    for bad in (2, -1, True, "1"):
        with pytest.raises(ValueError):
            specaug.draw(seed, epoch, n, policy, view=bad)


def test_abi_header_binding_and_makefile():
    from asr_chinese_e2e_amd import _lib, kernels
    raw = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    name = "asr_cr_ctc_fwd_bwd"
    assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == 14
    assert int(re.search(r"#define ASR_CR_CTC_RESIDENT_MAX_V (\d+)", raw).group(1)) == kernels.CR_CTC_RESIDENT_MAX_V == _lib.CR_CTC_RESIDENT_MAX_V
    assert kernels.CR_CTC_RESIDENT_MAX_V >= 4232 and kernels.CR_CTC_RESIDENT_MAX_V % (256 * 8) == 0
    assert _lib.ABI_VERSION == 10 == _lib.lib.asr_abi_version()
    make = open(os.path.join(ROOT, "asr_chinese_e2e_amd", "csrc", "Makefile")).read()
    assert "cr_ctc.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1)
    assert callable(kernels.cr_ctc)


def test_launcher_refusals_on_the_host():
    """The launcher refuses before any launch: host addresses stand in for the device pointers, nothing is launched or written."""
    from asr_chinese_e2e_amd import _lib
    P, T, V, ld = 2, 3, 6, 8
    n = 2 * P * T * ld
    block = np.full(2 * n + 8, -7, np.float32)      # the logits, and behind them the gradient block
    in_len, frame, pair, div = np.full(8, -7, np.int32), np.full(P * T + 2, -7, np.float32), np.full(P + 2, -7, np.float32), np.full(4, -7, np.float32)
    p = lambda a: a.ctypes.data      # noqa: E731

    def call(**kw):
        a = dict(logits=p(block), in_len=p(in_len), grad=p(block) + 4 * n, frame=p(frame), pair=p(pair), P=P, T=T, V=V, ld=ld, grad_scale=1.0,
                 grad_scale_div=None, accumulate=0, dtype=0, stream=None)
        a.update(kw)
        return _lib.fast.asr_cr_ctc_fwd_bwd(*a.values())

    span = 4 * ((2 * P * T - 1) * ld + V)
    bad = [dict(logits=None), dict(in_len=None), dict(frame=None), dict(pair=None), dict(logits=p(block) + 2), dict(grad=p(block) + 4 * n + 2),
           dict(in_len=p(in_len) + 2), dict(frame=p(frame) + 1), dict(pair=p(pair) + 2), dict(grad_scale_div=p(div) + 2),
           dict(P=0), dict(P=-1), dict(P=65536), dict(T=0), dict(V=1), dict(V=0), dict(ld=V - 1),
           dict(grad=p(block)), dict(grad=p(block) + span - 4), dict(grad=p(block) + 4 * ld), dict(logits=p(block) + 4 * n, grad=p(block) + 4 * n - span + 4),
           dict(accumulate=1, grad=None), dict(accumulate=2), dict(accumulate=-1),
           dict(grad_scale=float("nan")), dict(grad_scale=float("inf")), dict(grad_scale=float("-inf"))]
    for kw in bad:
        assert call(**kw) == -1 and "asr_cr_ctc_fwd_bwd" in _lib.last_error(), kw      # ASR_EINVAL
    assert call(dtype=2) == -2 and call(dtype=-1) == -2      # ASR_EDTYPE
    assert call(dtype=1, logits=p(block) + 1) == -1 and call(dtype=1, grad=p(block) + 4 * n + 1) == -1
    assert "overlaps" in (call(grad=p(block) + span - 4), _lib.last_error())[1]
    for a in (block, in_len, frame, pair, div):
        assert (a == -7).all()


def test_wrapper_argument_checks():
    """kernels.cr_ctc refuses on the host, before it asks for a device pointer."""
    from asr_chinese_e2e_amd import kernels as K
    x = torch.zeros(4, 3, 6)
    n = torch.full((4,), 3, dtype=torch.int32)
    for args, kw in (((torch.zeros(3, 3, 6), n[:3]), {}), ((torch.zeros(3, 6), n), {}), ((torch.zeros(0, 3, 6), n[:0]), {}),
                     ((x, n[:2]), {}), ((x, n.long()), {}), ((x, n), dict(accumulate=True)),
                     ((x, n), dict(want_grad=False, accumulate=True)), ((x, n), dict(want_grad=False, dlogits=torch.zeros_like(x))),
                     ((x, n), dict(dlogits=torch.zeros(4, 3, 5))), ((x, n), dict(dlogits=torch.zeros(4, 3, 6, dtype=torch.bfloat16))),
                     ((x, n), dict(dlogits=torch.zeros(4, 3, 8)[:, :, :6])), ((x, n), dict(grad_scale_div=torch.ones(2))),
                     ((x, n), dict(grad_scale_div=torch.ones(1, dtype=torch.float64)))):
        with pytest.raises(ValueError):
            K.cr_ctc(*args, **kw)
    with pytest.raises(ValueError, match="CUDA"):      # everything checked: only the device is missing
        K.cr_ctc(x, n)


def test_config_key_defaults_and_refusals():
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab, synthetic_pack
    from asr_chinese_e2e_amd.Models.transformer_official import cr_ctc_setting
    for M_ in (Models.TransformerCTC, Models.TransformerOffical):
        assert M_.get_default_config()().cr_ctc_weight == 0.0
    assert cr_ctc_setting(0.2) == 0.2 and cr_ctc_setting(0) == 0.0
    for bad in (-0.1, float("nan"), float("inf"), "0.2", True, None):
        with pytest.raises(ValueError):
            cr_ctc_setting(bad)

    def build(M_, **kw):
        mc = M_.get_default_config()()
        mc.fn_build(dict(n_mels=8, lfr_m=1, layer_num=1, d_model=16, hidden_size=8, num_head=2, ff_size=16, **kw))
        return M_(mc, Vocab.synthetic(12))
    model = build(Models.TransformerCTC, cr_ctc_weight=0.2)
    assert model.cr_ctc_weight == 0.2 and model._cr_mean is None
    assert build(Models.TransformerOffical).cr_ctc_weight == 0.0 and build(Models.TransformerCTC, mwer_weight=0.5).cr_ctc_weight == 0.0
    for M_, kw in ((Models.TransformerOffical, dict(cr_ctc_weight=0.2)), (Models.TransformerOffical, dict(cr_ctc_weight=0.2, ctc_weight=0.3)),
                   (Models.TransformerCTC, dict(cr_ctc_weight=-1.0)), (Models.TransformerCTC, dict(cr_ctc_weight=float("nan"))),
                   (Models.TransformerCTC, dict(cr_ctc_weight=float("inf"))), (Models.TransformerCTC, dict(cr_ctc_weight=0.2, mwer_weight=0.5))):
        with pytest.raises(ValueError):
            build(M_, **kw)
    # an odd number of rows is refused before anything is launched (so also where there is nothing to launch on)
    with pytest.raises(ValueError, match="odd"):
        model.train_step(synthetic_pack(3, 12, 8, 12, seed=1))


def test_loader_views_refusals():
    from asr_chinese_e2e_amd.data_handler.loader import BucketedWaveLoader, MetaLayout
    for kw in (dict(views=0), dict(views=3), dict(views=True), dict(views="2"), dict(views=2, augment=True)):
        with pytest.raises(ValueError):
            BucketedWaveLoader(None, 4, **kw)
    one, two = MetaLayout(4, 5, spec=12), MetaLayout(4, 5, spec=12, views=2)
    assert "spec1" not in one and two.size == one.size + 4 * 12 and two.at["spec1"][2] == (4, 12) and two.at["spec"] == one.at["spec"]
    assert MetaLayout(4, 5, views=2).size == MetaLayout(4, 5).size      # without a policy the second view adds no words


def test_train_flag_selects_two_views():
    import train
    assert train.loader_views(0.2) == 2 and train.loader_views("0.2") == 2 and train.loader_views(0.0) == 1 and train.loader_views(None) == 1
    assert "--cr_ctc_weight" in train.__doc__
