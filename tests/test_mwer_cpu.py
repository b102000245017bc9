"""MWER for the CTC head, what needs no GPU: the two statements of the definition (tests/mwer_ref.py) against each other, the exact
sparsity of the gradient, the entries that take part in nothing, the bindings and every refusal the launchers and the model make on the
host."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import mwer_ref as M
from tests import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("asr_ctc_mwer_workspace_bytes", "asr_mwer_errors", "asr_ctc_mwer_lattice", "asr_ctc_mwer_grad")


def case(seed=0, B=2, T=7, V=6, N=4, Lh=4):
    """Random logits; per utterance an empty entry, a doubled token, an entry equal to the reference, a random one."""
    rng = np.random.RandomState(seed)
    logits = torch.from_numpy(rng.randn(B, T, V) * 1.5)
    ref = rng.randint(1, V, size=(B, 3)).astype(np.int32)
    ref_len = np.array([3, 2][:B] + [3] * max(B - 2, 0), np.int32)
    hyp = np.zeros((B, N, Lh), np.int32)
    hyp_len = np.zeros((B, N), np.int32)
    for b in range(B):
        rows = [[], [2, 2, 1], list(ref[b, :ref_len[b]]), list(rng.randint(1, V, size=Lh))][:N]
        for i, h in enumerate(rows):
            hyp[b, i, :len(h)] = h
            hyp_len[b, i] = len(h)
    in_len = np.array([T, T - 1][:B] + [T] * max(B - 2, 0), np.int32)
    return logits, in_len, hyp, hyp_len, ref, ref_len


def both(logits, in_len, hyp, hyp_len, ref, ref_len, **kw):
    return M.autograd(logits, in_len, hyp, hyp_len, ref, ref_len, **kw), M.explicit(logits, in_len, hyp, hyp_len, ref, ref_len, **kw)


def test_explicit_form_equals_autograd():
    """The alpha / beta form against torch.autograd through F.ctc_loss and a softmax over the list, float64, the gate of
    tests/test_oracle_ctc.py for the same comparison (rtol 1e-9; atol 1e-10 as there, for the cells that are zero)."""
    for seed in range(3):
        a, e = both(*case(seed), scale=0.7)
        assert a["present"].tolist() == e["present"].tolist() and a["present"].sum() == 8
        on = a["present"] == 1
        for k in ("ll", "post", "coef"):
            assert np.allclose(e[k][on], a[k][on], rtol=1e-9, atol=1e-12), k
        assert np.allclose(e["risk"], a["risk"], rtol=1e-9) and math.isclose(e["loss"], a["loss"], rel_tol=1e-9)
        assert np.allclose(e["grad"], a["grad"], rtol=1e-9, atol=1e-10)
        assert np.abs(a["grad"]).max() > 1e-3


def test_gradient_is_exactly_sparse():
    """Columns of no entry's tokens and rows past T_b: exactly zero in the explicit form, rounding in autograd's; row sums: rounding."""
    logits, in_len, hyp, hyp_len, ref, ref_len = case(1, V=9)
    hyp = np.where(hyp == 5, 4, hyp)      # no entry emits 5 .. 8
    hyp = np.where(hyp > 5, 3, hyp)
    a, e = both(logits, in_len, hyp, hyp_len, ref, ref_len)
    mask = M.touched(hyp, hyp_len, e["present"], in_len, logits.shape[1], 9)
    assert not mask[:, :, 5:].any() and mask[:, :, 0].any()
    assert (e["grad"][~mask] == 0).all()
    assert np.abs(a["grad"][~mask]).max() <= 1e-15
    # a row sums to sum_i c_i * (the state posteriors of entry i at the frame, which sum to 1 up to the rounding of T * S additions)
    tol = 4 * np.finfo(np.float64).eps * logits.shape[1] * (2 * hyp.shape[2] + 1) * np.abs(e["coef"]).sum(1).max()
    assert tol < 1e-12 and np.abs(e["grad"].sum(-1)).max() <= tol and np.abs(a["grad"].sum(-1)).max() <= tol
    assert (e["grad"][1, in_len[1]:] == 0).all() and (a["grad"][1, in_len[1]:] == 0).all()


def test_single_entry_and_equal_errors_give_no_gradient():
    logits, in_len, hyp, hyp_len, ref, ref_len = case(2)
    one = M.explicit(logits, in_len, hyp[:, 2:3], hyp_len[:, 2:3], ref, ref_len)
    assert np.allclose(one["post"], 1.0) and (one["risk"] == 0).all() and np.abs(one["grad"]).max() == 0
    one = M.explicit(logits, in_len, hyp[:, 1:2], hyp_len[:, 1:2], ref, ref_len)      # one wrong entry: risk = its errors, still no gradient
    assert (one["risk"] == one["err"][:, 0]).all() and (one["err"] > 0).all() and np.abs(one["grad"]).max() == 0
    same = np.full((2, 4), 3, np.int32)
    a, e = both(logits, in_len, hyp, hyp_len, ref, ref_len, err=same)
    # risk = 3 sum_i P_i = 3 up to N roundings, so |c_i| <= 3 N eps P_i and no cell is further from 0 than their sum
    tol = 2 * 3 * 4 * np.finfo(np.float64).eps
    assert np.allclose(e["risk"], 3.0) and np.abs(e["grad"]).max() <= tol and np.abs(a["grad"]).max() <= tol


def test_entries_that_take_part_in_nothing():
    """Absent, longer than the row, infeasible and out-of-vocabulary entries: the result is that of the list without them."""
    logits, in_len, hyp, hyp_len, ref, ref_len = case(3, N=4, Lh=4)
    V, T = logits.shape[2], logits.shape[1]
    base = M.explicit(logits, in_len, hyp[:, :2], hyp_len[:, :2], ref, ref_len)
    for what in ("absent", "long", "infeasible", "oov", "blank", "negative"):
        h, n = hyp.copy(), hyp_len.copy()
        il = in_len.copy()
        if what == "absent":
            n[:, 2:] = -1
        elif what == "long":
            n[:, 2:] = 5      # the search reports the true length of an entry it truncated to Lh = 4
        elif what == "infeasible":
            il[:] = 4         # [2, 2, 1] needs 4 frames and stays; four equal tokens need 7
            h[:, 2:] = 3
            n[:, 2:] = 4
        else:
            h[:, 2:, 1] = {"oov": V, "blank": 0, "negative": -1}[what]
            n[:, 2:] = 3
        ref_il = il
        want = base if what != "infeasible" else M.explicit(logits, il, hyp[:, :2], hyp_len[:, :2], ref, ref_len)
        a, e = both(logits, ref_il, h, n, ref, ref_len)
        for r in (a, e):
            assert r["present"].tolist() == [[1, 1, 0, 0]] * 2, what
            assert (r["post"][:, 2:] == 0).all() and (r["coef"][:, 2:] == 0).all() and np.isneginf(r["ll"][:, 2:]).all()
            assert np.allclose(r["risk"], want["risk"], rtol=1e-12) and np.allclose(r["grad"], want["grad"], rtol=1e-9, atol=1e-12), what
    err, flags = M.errors(hyp, np.array([[-1, 5, 4, 0]] * 2), ref, ref_len)
    assert flags.tolist() == [[1, 2, 0, 0]] * 2 and (err[:, :2] == 0).all() and err[:, 3].tolist() == ref_len.tolist()


def test_empty_utterances():
    """T_b = 0, and an utterance none of whose entries takes part: risk 0, posteriors 0, gradient 0; the others are not disturbed."""
    logits, in_len, hyp, hyp_len, ref, ref_len = case(4, B=3)
    alone = M.explicit(logits[2:], in_len[2:], hyp[2:], hyp_len[2:], ref[2:], ref_len[2:])
    in_len = in_len.copy()
    in_len[0] = 0
    hyp_len = hyp_len.copy()
    hyp_len[1] = -1
    a, e = both(logits, in_len, hyp, hyp_len, ref, ref_len)
    for r in (a, e):
        assert (r["present"][:2] == 0).all() and (r["risk"][:2] == 0).all() and (r["post"][:2] == 0).all() and (r["grad"][:2] == 0).all()
        assert np.allclose(r["grad"][2], alone["grad"][0], rtol=1e-9, atol=1e-12) and np.allclose(r["risk"][2], alone["risk"][0])
    assert M.explicit(logits, in_len * 0, hyp, hyp_len, ref, ref_len)["loss"] == 0.0


def test_duplicate_entries_share_the_mass():
    logits, in_len, hyp, hyp_len, ref, ref_len = case(5)
    hyp, hyp_len = hyp.copy(), hyp_len.copy()
    hyp[:, 3], hyp_len[:, 3] = hyp[:, 1], hyp_len[:, 1]
    a, e = both(logits, in_len, hyp, hyp_len, ref, ref_len)
    assert np.allclose(e["post"][:, 1], e["post"][:, 3], rtol=1e-12) and np.allclose(e["ll"][:, 1], e["ll"][:, 3], rtol=1e-12)
    assert np.allclose(e["grad"], a["grad"], rtol=1e-9, atol=1e-10) and np.allclose(e["post"].sum(1), 1.0)


def test_errors_are_score_refs_distance():
    rng = np.random.RandomState(6)
    hyp = rng.randint(1, 5, size=(3, 4, 9)).astype(np.int32)
    hyp_len = rng.randint(0, 10, size=(3, 4)).astype(np.int32)
    ref = rng.randint(1, 5, size=(3, 7)).astype(np.int32)
    ref_len = np.array([7, 0, 4], np.int32)
    err, flags = M.errors(hyp, hyp_len, ref, ref_len)
    assert (flags == 0).all()
    for b in range(3):
        for i in range(4):
            assert err[b, i] == R.align(ref[b, :ref_len[b]], hyp[b, i, :hyp_len[b, i]])["distance"]
    assert err[1].tolist() == hyp_len[1].tolist()


def test_abi_header_binding_and_makefile():
    from asr_chinese_e2e_amd import _lib, kernels
    raw = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    consts = {k: int(v) for k, v in re.findall(r"#define (ASR_MWER_\w+) (\d+)", raw)}
    assert consts == {"ASR_MWER_MAX_N": kernels.MWER_MAX_N, "ASR_MWER_MAX_LEN": kernels.MWER_MAX_LEN, "ASR_MWER_ABSENT": kernels.MWER_ABSENT,
                      "ASR_MWER_LONG": kernels.MWER_LONG}
    assert (kernels.MWER_MAX_N, kernels.MWER_MAX_LEN) == (16, 255)
    assert _lib.ABI_VERSION == 10 == _lib.lib.asr_abi_version()
    make = open(os.path.join(ROOT, "asr_chinese_e2e_amd", "csrc", "Makefile")).read()
    assert "mwer.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1)
    for fn in ("mwer_errors", "ctc_mwer_lattice", "ctc_mwer_grad", "ctc_mwer_workspace_bytes", "ctc_mwer"):
        assert callable(getattr(kernels, fn))


def test_workspace_query():
    from asr_chinese_e2e_amd import _lib, kernels
    small, big = kernels.ctc_mwer_workspace_bytes(2, 4, 10, 8), kernels.ctc_mwer_workspace_bytes(2, 4, 10, 9)
    # at least the frames' log-sum-exp, fp64 alpha and f32 posteriors of every state, and the two chain words of every slot
    assert small >= 2 * 10 * 8 + 2 * 4 * 10 * 17 * 12 + 2 * 4 * 8 * 8 and small % 16 == 0 and big > small
    for bad in ((0, 4, 10, 8), (2, 0, 10, 8), (2, 17, 10, 8), (2, 4, 0, 8), (2, 4, 10, 0), (2, 4, 10, 256)):
        assert _lib.fast.asr_ctc_mwer_workspace_bytes(*bad) == 0 and "asr_ctc_mwer_workspace_bytes" in _lib.last_error()
        with pytest.raises(ValueError):
            kernels.ctc_mwer_workspace_bytes(*bad)


def test_launcher_refusals_on_the_host():
    """Every launcher refuses before any launch: host addresses stand in for the device pointers, nothing is launched or written."""
    from asr_chinese_e2e_amd import _lib
    B, N, Lh, Lr, T, V, ld = 2, 3, 4, 5, 6, 7, 8
    i32 = [np.full(64, -7, np.int32) for _ in range(8)]
    f32 = [np.full(64, -7, np.float32) for _ in range(4)]
    f64 = np.full(64, -7.0)
    need = int(_lib.fast.asr_ctc_mwer_workspace_bytes(B, N, T, Lh))
    ws = np.full(need // 8 + 4, -7.0)
    wsp = ws.ctypes.data + (-ws.ctypes.data) % 16
    frames = np.full(B * T * ld, -7, np.float32)
    p = lambda a: a.ctypes.data      # noqa: E731

    def errors(**kw):
        a = dict(hyp=p(i32[0]), hyp_len=p(i32[1]), ref=p(i32[2]), ref_len=p(i32[3]), err=p(i32[4]), flags=p(i32[5]), B=B, N=N, Lh=Lh, ldn=Lh, ldb=N * Lh,
                 Lr=Lr, ldr=Lr, stream=None)
        a.update(kw)
        return _lib.fast.asr_mwer_errors(*a.values())

    def lattice(**kw):
        a = dict(logits=p(frames), in_len=p(i32[6]), hyp=p(i32[0]), hyp_len=p(i32[1]), err=p(i32[4]), ll=p(f64), post=p(f32[0]), coef=p(f32[1]), risk=p(f32[2]),
                 present=p(i32[7]), B=B, T=T, V=V, ld=ld, N=N, Lh=Lh, ldn=Lh, ldb=N * Lh, blank=0, ws=wsp, ws_bytes=need, dtype=0, stream=None)
        a.update(kw)
        return _lib.fast.asr_ctc_mwer_lattice(*a.values())

    def grad(**kw):
        a = dict(dlogits=p(frames), in_len=p(i32[6]), hyp=p(i32[0]), hyp_len=p(i32[1]), coef=p(f32[1]), B=B, T=T, V=V, ld=ld, N=N, Lh=Lh, ldn=Lh, ldb=N * Lh,
                 blank=0, grad_scale=1.0, grad_scale_div=None, accumulate=0, ws=wsp, ws_bytes=need, dtype=0, stream=None)
        a.update(kw)
        return _lib.fast.asr_ctc_mwer_grad(*a.values())

    lists = [dict(B=0), dict(B=65536), dict(N=0), dict(N=17), dict(Lh=0), dict(Lh=256), dict(ldn=Lh - 1), dict(ldb=(N - 1) * Lh + Lh - 1), dict(hyp=None),
             dict(hyp_len=None), dict(hyp=p(i32[0]) + 2), dict(hyp_len=p(i32[1]) + 1)]
    frames_bad = [dict(T=0), dict(V=1), dict(ld=V - 1), dict(blank=-1), dict(blank=V), dict(in_len=None), dict(ws=None), dict(ws=wsp + 8)]
    for fn, call, cases in (
            ("asr_mwer_errors", errors, lists + [dict(ref=None), dict(ref_len=None), dict(err=None), dict(flags=None), dict(Lr=0), dict(Lr=256), dict(ldr=Lr - 1),
                                                 dict(ref=p(i32[2]) + 2), dict(err=p(i32[4]) + 2)]),
            ("asr_ctc_mwer_lattice", lattice, lists + frames_bad + [dict(logits=None), dict(logits=p(frames) + 2), dict(err=None), dict(ll=None), dict(ll=p(f64) + 4),
                                                                  dict(post=None), dict(coef=None), dict(risk=None), dict(present=None), dict(post=p(f32[0]) + 2)]),
            ("asr_ctc_mwer_grad", grad, lists + frames_bad + [dict(dlogits=None), dict(dlogits=p(frames) + 1), dict(coef=None), dict(coef=p(f32[1]) + 2),
                                                            dict(grad_scale=float("nan")), dict(grad_scale=float("inf")), dict(grad_scale=float("-inf")),
                                                            dict(accumulate=2), dict(accumulate=-1), dict(grad_scale_div=p(f32[3]) + 2)])):
        for kw in cases:
            assert call(**kw) == -1 and fn in _lib.last_error(), (fn, kw)      # ASR_EINVAL
    for call in (lattice, grad):
        assert call(dtype=2) == -2      # ASR_EDTYPE
        assert call(ws_bytes=need - 1) == -3 and "workspace" in _lib.last_error()      # ASR_EWORKSPACE
    assert lattice(dtype=1, logits=p(frames) + 1) == -1 and grad(dtype=1, dlogits=p(frames) + 1) == -1
    for a in i32 + f32 + [f64, ws, frames]:
        assert (a == -7).all()


def test_config_defaults_and_refusals():
    from asr_chinese_e2e_amd import Models
    from asr_chinese_e2e_amd.data_handler import Vocab
    from asr_chinese_e2e_amd.Models.transformer_official import mwer_settings
    for M_ in (Models.TransformerCTC, Models.TransformerOffical):
        c = M_.get_default_config()()
        assert (c.mwer_weight, c.mwer_nbest, c.mwer_beam, c.mwer_frame_topk, c.mwer_blank_skip) == (0.0, 4, 4, 7, None)
    assert mwer_settings(0.5, 4, 4, 7, None) == (0.5, dict(nbest=4, beam=4, frame_topk=7, thr=None))
    assert mwer_settings(0.0, 2, 8, 7, 0.98)[1]["thr"] == float(np.float32(np.log(np.float32(0.98))))
    for bad in ((-0.1, 4, 4, 7, None), (float("nan"), 4, 4, 7, None), (float("inf"), 4, 4, 7, None), ("0.5", 4, 4, 7, None), (True, 4, 4, 7, None),
                (0.5, 1, 4, 7, None), (0.5, 5, 4, 7, None), (0.5, 4, 4, 16, None), (0.5, 8, 8, 8, None), (0.5, 4, 17, 1, None), (0.5, 4.0, 4, 7, None),
                (0.5, 4, 4, 0, None), (0.5, 4, 4, 7, 0.0), (0.5, 4, 4, 7, 1.5), (0.5, 4, 4, 7, "x")):
        with pytest.raises(ValueError):
            mwer_settings(*bad)

    def build(M_, **kw):
        mc = M_.get_default_config()()
        mc.fn_build(dict(n_mels=8, lfr_m=1, layer_num=1, d_model=16, hidden_size=8, num_head=2, ff_size=16, **kw))
        return M_(mc, Vocab.synthetic(12))
    assert build(Models.TransformerCTC, mwer_weight=0.5).mwer_weight == 0.5
    assert build(Models.TransformerOffical).mwer_weight == 0.0
    for M_, kw in ((Models.TransformerOffical, dict(mwer_weight=0.5)), (Models.TransformerOffical, dict(mwer_weight=0.5, ctc_weight=0.3)),
                   (Models.TransformerCTC, dict(mwer_weight=-1.0)), (Models.TransformerCTC, dict(mwer_weight=0.5, mwer_nbest=1)),
                   (Models.TransformerCTC, dict(mwer_nbest=5)), (Models.TransformerCTC, dict(mwer_beam=8, mwer_frame_topk=8)),
                   (Models.TransformerCTC, dict(mwer_blank_skip=2.0))):
        with pytest.raises(ValueError):
            build(M_, **kw)
