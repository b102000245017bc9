"""Intermediate CTC without a GPU: the definition (tests/interctc_ref.py) against autograd and against itself, the config keys and their
refusals, the parameter layout with and without the conditioning projection, the binding, and every refusal that needs no launch."""
import os
import re

import numpy as np
import pytest
import torch

from tests import interctc_ref as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = {1: [9], 3: [0, 1, 12]}      # an empty utterance, one frame, a length past T (clamped)
CASES = [(B, T, V, spread) for B in (1, 3) for T in (1, 9) for V in (2, 5, 64, 257) for spread in (1.0, 60.0)]


def _lens(B, T):
    return LENS[B] if T == 9 else None


@pytest.mark.parametrize("B,T,V,spread", CASES)
def test_closed_form_softmax_backward_equals_autograd(B, T, V, spread):
    z, dp, _, in_len = I.make_case(B, T, V, spread, _lens(B, T))
    z64 = torch.from_numpy(z).double().requires_grad_(True)
    dp64 = torch.from_numpy(dp).double()
    p = I.softmax_rows(z64, in_len)
    want, = torch.autograd.grad((p * dp64).sum(), z64)
    p = p.detach()
    got = I.softmax_bwd(p, dp64, in_len)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)
    n = np.clip(in_len, 0, T)
    for b in range(B):      # the frames past the utterance: p exactly 0, no gradient
        assert float(p[b, n[b]:].abs().sum()) == 0.0 and float(got[b, n[b]:].abs().sum()) == 0.0
        if n[b]:
            assert torch.allclose(p[b, :n[b]].sum(-1), torch.ones(n[b], dtype=torch.float64), atol=1e-12)


def test_softmax_rows_edge_rows():
    z = torch.zeros(1, 3, 4, dtype=torch.float64)
    z[0, 0, 1] = float("-inf")
    z[0, 1, :] = float("-inf")
    z[0, 2, 2] = 60.0
    p = I.softmax_rows(z, [3])
    assert p[0, 0, 1] == 0 and torch.allclose(p[0, 0, [0, 2, 3]], torch.full((3,), 1 / 3, dtype=torch.float64))
    assert float(p[0, 1].abs().sum()) == 0.0      # no finite maximum: zeros
    g = I.softmax_bwd(p.float(), torch.randn(1, 3, 4), [3])
    assert float(g[0, 1].abs().sum()) == 0.0 and torch.isfinite(g).all()


def _small_case(layer_num=3):
    from oracle import ref_model as R
    from asr_chinese_e2e_amd.data_handler import synthetic_pack
    B, T, F_, V, L = 2, 30, 16, 40, 6
    cfg = R.default_cfg(n_mels=F_, lfr_m=1, d_model=32, hidden_size=8, num_head=4, ff_size=64, layer_num=layer_num, use_decoder=False, ctc_weight=1.0)
    sd = {k: v.double() for k, v in R.init_state_dict(cfg, V, seed=5).items()}
    sd[I.COND] = I.init_cond(32, V, seed=6, dtype=torch.float64)
    pack = synthetic_pack(B, T, F_, V, seed=7, ragged=True, Lmin=2, Lmax=L)
    batch = {k: pack[k] for k in ("wave", "wave_len", "tgt_for_input", "tgt_len")}
    batch["wave"] = batch["wave"].double()
    return cfg, sd, batch, V


def test_definition_loss_identities():
    """Without layers the definition is R's own CTC-only loss; w -> 0 approaches it continuously; plain intermediate CTC leaves the
    encoder output alone, conditioning moves it and keeps the padded rows exactly zero; the per-utterance losses sum to the batch ones."""
    from oracle import ref_model as R
    cfg, sd, batch, V = _small_case()
    base = R.forward_losses(sd, cfg, batch)
    none = I.losses(sd, cfg, batch, 0.0, (), False)
    assert float(none["loss"]) == float(base["loss"]) and torch.equal(none["enc_out"], base["enc_out"])
    plain = I.losses(sd, cfg, batch, 0.3, (1, 2), False)
    assert torch.equal(plain["enc_out"], base["enc_out"]) and float(plain["ctc"]) == float(base["ctc"])
    want = 0.7 * float(plain["ctc"]) + 0.3 * 0.5 * (float(plain["inter"][0]) + float(plain["inter"][1]))
    assert abs(float(plain["loss"]) - want) <= 1e-12 * abs(want)
    for eps in (1e-3, 1e-6, 1e-9):
        near = I.losses(sd, cfg, batch, eps, (1, 2), False)
        assert abs(float(near["loss"]) - float(base["loss"])) <= 2 * eps * max(abs(float(base["loss"])), max(float(v) for v in near["inter"]))
    cond = I.losses(sd, cfg, batch, 0.3, (1,), True)
    assert not torch.equal(cond["enc_out"], base["enc_out"])
    for b in range(batch["wave"].shape[0]):
        assert float(cond["enc_out"][b, int(batch["wave_len"][b]):].abs().sum()) == 0.0
    B = batch["wave"].shape[0]
    assert torch.allclose(cond["per_utt"].sum(dim=1) / B, torch.stack(cond["inter"] + [cond["ctc"]]), rtol=1e-12)
    # both terms carry gradient into the conditioning projection and the head
    leaves = {k: sd[k].clone().requires_grad_(True) for k in (I.COND, "ctc_lo.weight")}
    out = I.losses({**sd, **leaves}, cfg, batch, 0.3, (1,), True)
    gc, gh = torch.autograd.grad(out["loss"], [leaves[I.COND], leaves["ctc_lo.weight"]])
    assert float(gc.abs().max()) > 0 and float(gh.abs().max()) > 0


def test_settings_and_refusals():
    from asr_chinese_e2e_amd.Models.transformer_official import interctc_settings as S
    assert S(0.0, (), False, 6) == (0.0, (), False)
    assert S(0.3, (3,), True, 6) == (0.3, (3,), True) and S(0.3, [2, 4], False, 6) == (0.3, (2, 4), False)
    assert S(0.3, "3", 1, 6) == (0.3, (3,), True) and S(0.3, "2,4", 0, 6) == (0.3, (2, 4), False) and S(0.3, " 2, 4 ", False, 6)[1] == (2, 4)
    assert S(0.3, 3, False, 6)[1] == (3,) and S(0, "", False, 6) == (0.0, (), False) and S(0.3, (5,), False, 6)[1] == (5,)
    bad = [(-0.1, (3,), False), (1.0, (3,), False), (1.5, (3,), False), (float("nan"), (3,), False), (float("inf"), (3,), False),
           ("0.3", (3,), False), (True, (3,), False), (None, (3,), False),
           (0.3, (), False), (0.0, (3,), False), (0.0, (), True), (0.3, (), True),                     # w > 0 iff layers; conditioning needs layers
           (0.3, (0,), False), (0.3, (6,), False), (0.3, (7,), False), (0.3, (-1,), False),             # out of [1, layer_num - 1]
           (0.3, (3, 3), False), (0.3, (4, 2), False), (0.3, "4,2", False), (0.3, "3,3", False),       # duplicate, unsorted
           (0.3, "a", False), (0.3, "2;4", False), (0.3, "2,,4", False), (0.3, (2.0,), False), (0.3, (True,), False), (0.3, 2.5, False),
           (0.3, {3}, False), (0.3, ("3",), False), (0.3, (3,), "yes"), (0.3, (3,), 2), (0.3, (3,), None)]
    for w, layers, cond in bad:
        with pytest.raises(ValueError):
            S(w, layers, cond, 6)
    with pytest.raises(ValueError):
        S(0.3, (1,), False, 1)      # a one-layer encoder has no middle layer


def _build(M_, layer_num=3, **kw):
    from asr_chinese_e2e_amd.data_handler import Vocab
    mc = M_.get_default_config()()
    mc.fn_build(dict(n_mels=8, lfr_m=1, layer_num=layer_num, d_model=16, hidden_size=8, num_head=2, ff_size=16, **kw))
    return M_(mc, Vocab.synthetic(12))


def test_config_keys_on_the_models():
    from asr_chinese_e2e_amd import Models
    for M_ in (Models.TransformerCTC, Models.TransformerOffical):
        c = M_.get_default_config()()
        assert c.interctc_weight == 0.0 and tuple(c.interctc_layers) == () and c.interctc_condition is False
    m = _build(Models.TransformerCTC, interctc_weight=0.3, interctc_layers="1,2", interctc_condition=1)
    assert (m.interctc_weight, m.interctc_layers, m.interctc_condition) == (0.3, (1, 2), True) and m._interctc_mean is None
    assert _build(Models.TransformerOffical).interctc_layers == ()
    ic = dict(interctc_weight=0.3, interctc_layers=(1,))
    for M_, kw in ((Models.TransformerOffical, ic), (Models.TransformerOffical, dict(ctc_weight=0.3, **ic)),      # the joint model
                   (Models.TransformerCTC, dict(mwer_weight=0.5, **ic)), (Models.TransformerCTC, dict(cr_ctc_weight=0.2, **ic)),
                   (Models.TransformerCTC, dict(interctc_weight=0.3)), (Models.TransformerCTC, dict(interctc_layers=(1,))),
                   (Models.TransformerCTC, dict(interctc_condition=True)), (Models.TransformerCTC, dict(interctc_weight=0.3, interctc_layers=(3,))),
                   (Models.TransformerCTC, dict(interctc_weight=0.3, interctc_layers=(2, 1))),
                   (Models.TransformerCTC, dict(interctc_weight=1.0, interctc_layers=(1,))),
                   (Models.TransformerCTC, dict(interctc_weight=float("nan"), interctc_layers=(1,)))):
        with pytest.raises(ValueError):
            _build(M_, **kw)
    # streaming runs its own encoder tick: refused with conditioning, before anything touches a device
    for what in ("stream", "sessions"):
        with pytest.raises(ValueError, match="interctc_condition"):
            getattr(m, what)(2)


def test_parameter_layout():
    """Default keys: the state dict's keys, their order and the flat offsets of a model built without them.  Conditioning: exactly one
    more key, (d_model, V), directly in front of ctc_lo.weight in the flat buffer and behind the encoder's keys in the state dict."""
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.engine import COND_NAME
    assert COND_NAME == I.COND
    torch.manual_seed(0)
    base = _build(Models.TransformerCTC)
    torch.manual_seed(0)
    keyed = _build(Models.TransformerCTC, interctc_weight=0.0, interctc_layers=(), interctc_condition=False)
    torch.manual_seed(0)
    plain = _build(Models.TransformerCTC, interctc_weight=0.3, interctc_layers=(1, 2))
    for m in (keyed, plain):
        assert list(m.state_dict().keys()) == list(base.state_dict().keys())
        assert m._flat.index == base._flat.index and m._flat.block_range == base._flat.block_range and m._flat.numel == base._flat.numel
        for k, v in base.state_dict().items():      # and the same initial values from the same seed
            assert torch.equal(m.state_dict()[k], v), k
    cond = _build(Models.TransformerCTC, interctc_weight=0.3, interctc_layers=(1,), interctc_condition=True)
    keys, bkeys = list(cond.state_dict().keys()), list(base.state_dict().keys())
    assert [k for k in keys if k not in bkeys] == [COND_NAME] and [k for k in keys if k != COND_NAME] == bkeys
    assert keys.index(COND_NAME) == keys.index("ctc_lo.weight") - 1 and keys[keys.index(COND_NAME) - 1].startswith("encoder.layer_stack.2.")
    assert tuple(cond.state_dict()[COND_NAME].shape) == (16, 12) == cond._flat.index[COND_NAME][1]
    f = cond._flat
    blocks = [[n for n, _ in blk] for blk in f.blocks]
    at = blocks.index([COND_NAME])
    assert blocks[at + 1] == ["ctc_lo.weight"] and blocks[at + 2] == ["ctc_lo.bias"] and at + 3 == len(blocks)
    off, end = f.block_range[at]
    assert end - off == 16 * 12 and f.index["ctc_lo.weight"][0] == (end + 63) // 64 * 64
    for n, (o, shape) in base._flat.index.items():      # everything below the projection keeps its offset
        if not n.startswith("ctc_lo."):
            assert f.index[n] == (o, shape), n
    w = cond.state_dict()[COND_NAME]
    assert float(w.abs().max()) > 0 and abs(float(w.std()) - (2.0 / (16 + 12)) ** 0.5) < 0.5 * (2.0 / (16 + 12)) ** 0.5      # initialised like the projections
    assert not hasattr(getattr(base, "encoder"), "conditioning_layer")


def test_binding_and_header():
    from asr_chinese_e2e_amd import _lib, kernels
    raw = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    for name in ("asr_softmax_rows", "asr_softmax_bwd_add"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and re.search(r"\bint %s\(" % name, raw)
    assert int(re.search(r"#define ASR_INTERCTC_RESIDENT_MAX_V (\d+)", raw).group(1)) == kernels.INTERCTC_RESIDENT_MAX_V == _lib.INTERCTC_RESIDENT_MAX_V
    assert kernels.INTERCTC_RESIDENT_MAX_V >= 4232 and kernels.INTERCTC_RESIDENT_MAX_V % (256 * 8) == 0
    assert _lib.ABI_VERSION == 10 == _lib.lib.asr_abi_version()
    make = open(os.path.join(ROOT, "asr_chinese_e2e_amd", "csrc", "Makefile")).read()
    assert "interctc.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1)
    assert callable(kernels.softmax_rows) and callable(kernels.softmax_bwd_add)


def test_launcher_refusals_on_the_host():
    """The launchers refuse before any launch: host addresses stand in for the device pointers, nothing is launched or written."""
    from asr_chinese_e2e_amd import _lib
    B, T, V, ld = 2, 3, 6, 8
    n = B * T * ld
    block = np.full(3 * n + 8, -7, np.float32)      # three blocks back to back: logits | out,  p | dp | grad
    in_len = np.full(8, -7, np.int32)
    p = lambda a: a.ctypes.data      # noqa: E731
    span = 4 * ((B * T - 1) * ld + V)

    def fwd(**kw):
        a = dict(logits=p(block), in_len=p(in_len), out=p(block) + 4 * n, B=B, T=T, V=V, ld=ld, dtype=0, stream=None)
        a.update(kw)
        return _lib.fast.asr_softmax_rows(*a.values())

    def bwd(**kw):
        a = dict(p=p(block), dp=p(block) + 4 * n, in_len=p(in_len), grad=p(block) + 8 * n, B=B, T=T, V=V, ld=ld, accumulate=1, dtype=0, stream=None)
        a.update(kw)
        return _lib.fast.asr_softmax_bwd_add(*a.values())

    shapes = [dict(B=0), dict(B=-1), dict(B=65536), dict(T=0), dict(T=-2), dict(V=0), dict(V=-1), dict(ld=V - 1), dict(in_len=None), dict(in_len=p(in_len) + 2)]
    for kw in shapes + [dict(logits=None), dict(out=None), dict(logits=p(block) + 2), dict(out=p(block) + 4 * n + 2),
                        dict(out=p(block)), dict(out=p(block) + span - 4), dict(out=p(block) + 4 * ld),
                        dict(logits=p(block) + 4 * n, out=p(block) + 4 * n - span + 4)]:
        assert fwd(**kw) == -1 and "asr_softmax_rows" in _lib.last_error(), kw      # ASR_EINVAL
    assert fwd(dtype=2) == -2 and fwd(dtype=-1) == -2      # ASR_EDTYPE
    assert fwd(dtype=1, logits=p(block) + 1) == -1 and fwd(dtype=1, out=p(block) + 4 * n + 1) == -1
    assert "overlaps" in (fwd(out=p(block) + span - 4), _lib.last_error())[1]
    for kw in shapes + [dict(p=None), dict(dp=None), dict(grad=None), dict(p=p(block) + 2), dict(dp=p(block) + 4 * n + 2), dict(grad=p(block) + 8 * n + 2),
                        dict(accumulate=2), dict(accumulate=-1),
                        dict(grad=p(block)), dict(grad=p(block) + span - 4), dict(grad=p(block) + 4 * n), dict(grad=p(block) + 4 * n + span - 4),
                        dict(grad=p(block) + 4 * n - span + 4), dict(p=p(block) + 8 * n + 4 * ld)]:
        assert bwd(**kw) == -1 and "asr_softmax_bwd_add" in _lib.last_error(), kw
    assert bwd(dtype=2) == -2 and bwd(dtype=-1) == -2
    assert bwd(dtype=1, grad=p(block) + 8 * n + 1) == -1
    assert "overlaps" in (bwd(grad=p(block) + 4 * n), _lib.last_error())[1]
    assert (block == -7).all() and (in_len == -7).all()


def test_wrapper_argument_checks():
    """kernels.softmax_rows / softmax_bwd_add refuse on the host, before they ask for a device pointer."""
    from asr_chinese_e2e_amd import kernels as K
    x = torch.zeros(2, 3, 6)
    n = torch.full((2,), 3, dtype=torch.int32)
    for args, kw in (((torch.zeros(3, 6), n), {}), ((x, n[:1]), {}), ((x, n.long()), {}), ((x, n), dict(out=torch.zeros(2, 3, 5))),
                     ((x, n), dict(out=torch.zeros(2, 3, 6, dtype=torch.bfloat16))), ((x, n), dict(out=torch.zeros(2, 3, 8)[:, :, :6]))):
        with pytest.raises(ValueError):
            K.softmax_rows(*args, **kw)
    for args in ((torch.zeros(3, 6), torch.zeros(3, 6), n, torch.zeros(3, 6)), (x, x, n[:1], x.clone()), (x, x, n.long(), x.clone()),
                 (x, torch.zeros(2, 3, 5), n, x.clone()), (x, x, n, torch.zeros(2, 3, 8)[:, :, :6]), (x, x.to(torch.bfloat16), n, x.clone()),
                 (x, x, n, x.clone().to(torch.bfloat16))):
        with pytest.raises(ValueError):
            K.softmax_bwd_add(*args)
    with pytest.raises(ValueError, match="CUDA"):      # everything checked: only the device is missing
        K.softmax_rows(x, n)
    with pytest.raises(ValueError, match="CUDA"):
        K.softmax_bwd_add(x, x.clone(), n, x.clone())


def test_train_flags_are_documented():
    import train
    for flag in ("--interctc_weight", "--interctc_layers", "--interctc_condition"):
        assert flag in train.__doc__
    flags = train.parse_flags(["--interctc_weight=0.3", "--interctc_layers=2,4", "--interctc_condition=1"])
    from asr_chinese_e2e_amd.Models.transformer_official import interctc_settings as S
    assert S(flags["interctc_weight"], flags["interctc_layers"], flags["interctc_condition"], 6) == (0.3, (2, 4), True)
    assert S(0.3, train.parse_flags(["--interctc_layers=3"])["interctc_layers"], False, 6)[1] == (3,)
