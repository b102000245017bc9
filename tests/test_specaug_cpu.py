"""SpecAugment policies, host side (no GPU): data_handler/specaug.py against the definition (tests/specaug_ref.py), the definition's own
identities and a hand-computed warp, the draws, the policy strings and every refusal, the meta layout, and the names of the entry points."""
import os
import random
import re

import numpy as np
import pytest

from tests import specaug_ref as SR
from tests.helpers import ROOT


def _policy(p):
    from asr_chinese_e2e_amd.data_handler.specaug import SpecAugmentPolicy
    return SpecAugmentPolicy(**p._asdict())


def _random_policy(rng, F):
    return SR.Policy(warp=rng.choice((0, 0, 1, 2, 5, 40, 64)), n_t=rng.randrange(9), max_t=rng.choice((1, 2, 7, 50, 1000)),
                     t_permille=rng.choice((1, 50, 200, 999, 1000)), n_f=rng.randrange(9), max_f=rng.randrange(1, F + 1), n_s=rng.randrange(9),
                     sub_t=rng.choice((1, 3, 30, 500)))


def _check_row(p, row, T, F):
    """The invariants of a resolved row: every range inside the utterance, non-empty or (0, 0); p <= s; the warp inside (0, T)."""
    wc, ww = int(row[0]), int(row[1])
    if p.warp > 0 and T - 2 * p.warp > 0:
        assert p.warp <= wc <= T - p.warp - 1 and 1 <= ww <= T - 1 and abs(ww - wc) <= p.warp, (p, T, wc, ww)
    else:
        assert wc == ww == 0
    k = 2
    cap = min(p.max_t, T * p.t_permille // 1000)
    for _ in range(p.n_t):
        t0, t1 = int(row[k]), int(row[k + 1])
        assert (0 <= t0 < t1 <= T and t1 - t0 <= cap) or (t0 == t1 == 0 and (T == 0 or cap == 0)), (p, T, t0, t1)
        k += 2
    for _ in range(p.n_f):
        f0, f1 = int(row[k]), int(row[k + 1])
        assert 0 <= f0 < f1 <= F and f1 - f0 <= p.max_f, (p, F, f0, f1)
        k += 2
    for _ in range(p.n_s):
        s, e, q = (int(v) for v in row[k:k + 3])
        assert (0 <= s < e <= T and e - s <= p.sub_t and 0 <= q <= s) or (T == 0 and s == e == q == 0), (p, T, s, e, q)
        k += 3
    assert k == len(row)


def test_resolve_against_the_definition_and_its_invariants():
    from asr_chinese_e2e_amd.data_handler import specaug
    rng = random.Random(11)
    cases = []
    for i in range(2000):
        F = rng.choice((1, 23, 40, 80))
        p = _random_policy(rng, F)
        W = max(p.warp, 1)
        T = rng.choice((0, 1, 2, 2 * W, 2 * W + 1, 2 * W + 2, rng.randrange(3, 40), rng.randrange(40, 3000)))
        cases.append((p, T, F))
    # the corners by name: no frame, one, two, T = 2W (no warp), T = 2W + 1 (one position), cap = 0 (T * permille // 1000 == 0)
    cases += [(SR.Policy(warp=5, n_t=2, max_t=50, n_f=2, max_f=10, n_s=2, sub_t=30), T, 80) for T in (0, 1, 2, 10, 11)]
    cases += [(SR.Policy(n_t=3, max_t=50, t_permille=200), T, 80) for T in (4, 5)]
    seen_cap0 = seen_warp_edge = False
    for i, (p, T, F) in enumerate(cases):
        d = [rng.getrandbits(32) for _ in range(SR.n_draws(p))]
        if i % 7 == 0:      # extreme numbers
            d = [rng.choice((0, 1, 2 ** 32 - 1, 2 ** 31)) for _ in d]
        want = SR.resolve(p, d, T, F)
        pol = _policy(p)
        got = specaug.resolve(pol, d, T, F)
        assert got.dtype == np.int32 and got.shape == (pol.width,) == (pol.n_draws,) == (SR.n_draws(p),)
        assert np.array_equal(got, want), (p, T, F, d)
        _check_row(p, got, T, F)
        seen_cap0 |= p.n_t > 0 and T > 0 and min(p.max_t, T * p.t_permille // 1000) == 0
        seen_warp_edge |= p.warp > 0 and T == 2 * p.warp + 1
    assert seen_cap0 and seen_warp_edge
    # a batch at once, from the table of draws
    p = SR.Policy(warp=5, n_t=2, max_t=50, t_permille=200, n_f=2, max_f=10, n_s=3, sub_t=30)
    table = SR.draw(3, 1, 6, p)
    frames = [0, 1, 11, 57, 300, 2999]
    rows = specaug.resolve_batch(_policy(p), table, frames, 80)
    assert rows.dtype == np.int32 and np.array_equal(rows, np.stack([SR.resolve(p, table[i], frames[i], 80) for i in range(6)]))


def test_draw_is_a_pure_function_of_seed_epoch_and_index():
    from asr_chinese_e2e_amd.data_handler import specaug
    from asr_chinese_e2e_amd.data_handler.loader import BatchPlan
    p = SR.Policy(warp=5, n_t=2, max_t=50, n_f=2, max_f=10, n_s=3, sub_t=30)
    pol = _policy(p)
    plan = BatchPlan([100, 200, 300, 400], 2, seed=7)      # the generator a loader hands to the reference's SpecAugment and the batch order
    random.seed(99)
    state, plan_state = random.getstate(), plan.rng.getstate()
    a = specaug.draw(7, 3, 10, pol)
    b = specaug.draw(7, 3, 10, pol)
    assert random.getstate() == state and plan.rng.getstate() == plan_state
    assert a.dtype == np.uint32 and a.shape == (10, pol.n_draws) == (10, 19)
    assert np.array_equal(a, b) and np.array_equal(a, SR.draw(7, 3, 10, p))
    assert np.array_equal(specaug.draw(7, 3, 4, pol), a[:4]) and np.array_equal(specaug.draw(7, 3, 1000, pol)[:10], a)      # row i does not depend on n
    assert not np.array_equal(specaug.draw(7, 4, 10, pol), a) and not np.array_equal(specaug.draw(8, 3, 10, pol), a)
    assert specaug.draw(7, 3, 0, pol).shape == (0, 19)
    assert len(set(a.reshape(-1).tolist())) > 180 and int(a.max()) > 2 ** 31      # 32-bit numbers, not small ones


def _frames(T, F, seed=0):
    return np.random.default_rng(seed).standard_normal((T, F)).astype(np.float32)


def test_apply_identities():
    x = _frames(9, 5)
    # an all-zero row
    assert np.array_equal(SR.apply(x, np.zeros(2 + 4 + 4 + 6, np.int32), 2, 2, 2).view(np.uint32), x.view(np.uint32))
    assert SR.apply(_frames(0, 5), [0] * 5, 0, 0, 1).shape == (0, 5)
    # p = 0: a substitution by the frame itself; the time mask still zeroes its frames (+0.0), every other frame keeps its bits
    y = SR.apply(x, [0, 0, 6, 8, 2, 7, 0], 1, 0, 1)
    assert np.array_equal(np.delete(y, (6, 7), 0).view(np.uint32), np.delete(x, (6, 7), 0).view(np.uint32))
    assert not y[6:8].view(np.uint32).any()
    # a warp that moves nothing (ww == wc): weight 0, the frames' bits
    assert np.array_equal(SR.apply(x, [4, 4], 0, 0, 0).view(np.uint32), x.view(np.uint32))
    # masks: zero is +0.0; a mel mask covers every frame, substituted ones too
    y = SR.apply(x, [0, 0, 1, 3, 2, 4, 5, 7, 3], 1, 1, 1)
    assert not y[:, 2:4].view(np.uint32).any() and not y[1:3].view(np.uint32).any()
    assert not y[5].any() and np.array_equal(y[6, :2], x[3, :2]) and np.array_equal(y[6, 4:], x[3, 4:])      # frame 5 reads masked frame 2
    # substitutions never chain: frames 6, 7 read ORIGINAL frames 4, 5 although frames 4, 5 are themselves substituted; the last one wins
    y = SR.apply(x, [0, 0, 4, 6, 4, 6, 8, 2, 7, 8, 1], 0, 0, 3)
    assert np.array_equal(y[4:6], x[0:2]) and np.array_equal(y[6], x[4]) and np.array_equal(y[7], x[6])
    # a hostile row is clamped: negative, past T, e < s, p > s, a warp boundary outside (0, T)
    y = SR.apply(x, [9, 3, -5, 2, 7, 100, -3, 2, 3, 5, 50, 12, 40, 40], 2, 1, 2)
    want = SR.apply(x, [0, 0, 0, 2, 7, 9, 0, 2, 3, 5, 3, 9, 9, 9], 2, 1, 2)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)) and np.array_equal(y[3:5, 2:], np.zeros((2, 3), np.float32)) and y[5:7, 2:].all()
    assert SR.clamp_row([9, 3, 5, 2, 6, 2, 50], 1, 0, 1, 9, 5) == (0, 0, [(5, 5)], [], [(6, 6, 6)])      # e < s: empty


def test_apply_warp_by_hand():
    """T = 5, the boundary between frames 1 | 2 moved to 2 | 3: three output frames from two input frames, two from three."""
    f32 = np.float32
    x = np.array([[1.0, -3.0], [2.5, 0.1], [7.0, 0.2], [-1.0, 0.3], [4.0, 1e-3]], dtype=f32)
    y = SR.apply(x, [2, 3], 0, 0, 0)
    lerp = lambda a, b, num, den: a + (f32(num) / f32(den)) * (b - a)      # float32 operands: every operation rounds to float32
    want = np.stack([
        lerp(x[0], x[1], 0, 6),      # o = 0: num = max(1 * 2 - 3, 0) = 0
        lerp(x[0], x[1], 3, 6),      # o = 1: num = 3 * 2 - 3 = 3 -> i0 = 0, w = 3 / 6
        lerp(x[1], x[1], 1, 6),      # o = 2: num = 5 * 2 - 3 = 7 -> i0 = 1 = i1 (the segment's last frame), w = 1 / 6
        lerp(x[2], x[3], 1, 4),      # o = 0 of the right segment: num = 1 * 3 - 2 = 1, den = 4
        lerp(x[3], x[4], 3, 4),      # o = 1: num = 3 * 3 - 2 = 7 -> i0 = 1, w = 3 / 4
    ]).astype(f32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(y[0], x[0]) and np.array_equal(y[2], x[1]) and y[1, 0] == f32(1.75) and y[3, 0] == f32(5.0) and y[4, 0] == f32(2.75)
    # the stacking rule of the kernels on top of it
    out, Tl = SR.stack(y, 4, 3, 3)
    assert Tl == 2 and not out[2].any() and np.array_equal(out[1], np.concatenate([y[3], y[4], y[4], y[4]]))


def test_policy_strings():
    from asr_chinese_e2e_amd.data_handler.specaug import GRAMMAR, SpecAugmentPolicy as P, as_policy
    assert P.from_string("wenet") == P(n_t=2, max_t=50, n_f=2, max_f=10) == P.from_string("t2x50,f2x10")
    assert P.from_string("espnet") == P(warp=5, n_t=2, max_t=40, n_f=2, max_f=30)
    full = P.from_string(" W5, t2x50 ,f2x10,s3x30,r200 ")
    assert full == P(warp=5, n_t=2, max_t=50, t_permille=200, n_f=2, max_f=10, n_s=3, sub_t=30)
    assert full.n_draws == full.width == 2 + 4 + 4 + 9 and P().width == 2 and P.from_string("wenet").t_permille == 1000
    assert as_policy(None) is None and as_policy("") is None and as_policy(full) is full and as_policy("wenet") == P.from_string("wenet")
    assert "SpecAugmentPolicy(warp=5" in repr(full)
    for bad in ("", "kaldi", "t2", "t2x", "tx50", "t2x50,t1x10", "w5,w6", "t2x50;f2x10", "q3", "t-1x5", "t2x50,,f2x10", "r", "w5.0", 5):
        with pytest.raises(ValueError) as e:
            P.from_string(bad)
        assert GRAMMAR in str(e.value), bad


def test_policy_refusals():
    from asr_chinese_e2e_amd.data_handler import AudioParser, build_dataloader
    from asr_chinese_e2e_amd.data_handler.loader import BucketedWaveLoader
    from asr_chinese_e2e_amd.data_handler.specaug import SpecAugmentPolicy as P
    for bad in (dict(warp=-1), dict(warp=65), dict(n_t=9), dict(n_t=-1), dict(n_f=9), dict(n_s=9), dict(max_t=0), dict(max_f=0), dict(sub_t=0),
                dict(t_permille=0), dict(t_permille=1001), dict(n_t=1.5), dict(warp=True), dict(max_t="50")):
        with pytest.raises(ValueError):
            P(**bad)
    for text in ("w65", "t9x5", "t2x0", "r0", "r1001", "s9x3"):      # well-formed, out of range
        with pytest.raises(ValueError):
            P.from_string(text)
    P(warp=64, n_t=8, n_f=8, n_s=8, t_permille=1)      # the limits themselves
    with pytest.raises(ValueError, match="max_f=30"):
        P.from_string("espnet").check_mels(23)
    assert P.from_string("espnet").check_mels(30).max_f == 30 and P(max_f=99).check_mels(23).n_f == 0      # no mel mask: its cap is not used
    # the loader and the parser refuse before they touch a device
    with pytest.raises(ValueError, match="augment=True"):
        BucketedWaveLoader(None, 2, augment=True, spec_augment="wenet", device="cpu")
    with pytest.raises(ValueError, match="w<W>"):
        BucketedWaveLoader(None, 2, spec_augment="t2", device="cpu")
    with pytest.raises(ValueError, match="augment=True"):
        build_dataloader("nowhere", None, 2, part="train", augment=True, spec_augment="wenet")
    with pytest.raises(ValueError, match="max_f=30"):
        build_dataloader("nowhere", None, 2, part="train", n_mels=23, spec_augment="espnet")
    with pytest.raises(ValueError, match="w<W>"):
        build_dataloader("nowhere", None, 2, part="dev", spec_augment="masks")
    parser = AudioParser(n_mels=23, device="cpu")
    with pytest.raises(ValueError, match="max_f=30"):
        parser.spec_ranges(P.from_string("espnet"), np.zeros((1, 10), np.uint32), [1600])
    import torch
    wav, wl = torch.zeros(2, 1600), torch.tensor([1600, 800], dtype=torch.int32)
    pol = P.from_string("wenet")
    rows = parser.spec_ranges(pol, np.zeros((2, pol.n_draws), np.uint32), [1600, 800])
    for kw in (dict(spec_policy=pol), dict(spec_ranges=rows), dict(spec_policy=pol, spec_ranges=rows, augment=True),
               dict(spec_policy=pol, spec_ranges=rows[:1]), dict(spec_policy=pol, spec_ranges=rows[:, :5]),
               dict(spec_policy=P.from_string("espnet"), spec_ranges=rows)):
        with pytest.raises(ValueError, match="parse_batch|max_f"):      # its own refusals, before the first launch would fail for want of a GPU
            parser.parse_batch(wav, wl, **kw)


def test_spec_ranges_counts_frames_as_the_front_ends_do():
    from asr_chinese_e2e_amd.data_handler import AudioParser
    from asr_chinese_e2e_amd.data_handler.specaug import SpecAugmentPolicy as P
    p = SR.Policy(warp=2, n_t=2, max_t=20, n_f=1, max_f=7, n_s=1, sub_t=9)
    pol, table = P(**p._asdict()), SR.draw(1, 0, 6, p)
    lengths = [0, 1, 399, 400, 5000, 16000]
    for frontend, frames in (("reference", [0, 1, 3, 3, 32, 101]), ("kaldi", [0, 0, 0, 1, 29, 98])):
        parser = AudioParser(n_mels=23, device="cpu", frontend=frontend)
        assert [parser.num_frames(l) for l in lengths] == frames
        rows = parser.spec_ranges(pol, table, lengths)
        assert rows.shape == (6, pol.width) and rows.dtype == np.int32
        assert np.array_equal(rows, np.stack([SR.resolve(p, table[i], frames[i], 23) for i in range(6)]))
        # rows narrower than the longest utterance cut the frame count as the kernels cut it
        cut = parser.spec_ranges(pol, table, lengths, S=4000)
        T = parser.num_frames(4000)
        assert np.array_equal(cut[4], SR.resolve(p, table[4], T, 23)) and np.array_equal(cut[:4], rows[:4])


def test_meta_layout_and_pack_meta():
    from asr_chinese_e2e_amd.data_handler.loader import MetaLayout, pack_meta
    off, zero = MetaLayout(3, 4, factor=True, aug=True), MetaLayout(3, 4, factor=True, aug=True, spec=0)
    assert off.size == zero.size and off.at == zero.at and "spec" not in zero
    on = MetaLayout(3, 4, factor=True, aug=True, spec=7)
    assert on.size == off.size + 21 and all(on.at[k] == off.at[k] for k in off.at) and on.at["spec"] == (off.size, off.size + 21, (3, 7))
    lay = MetaLayout(3, 4, spec=7)
    meta = np.full(lay.size, -1, dtype=np.int32)
    rows = np.arange(21, dtype=np.int32).reshape(3, 7) - 5
    sizes, tgt = [1600, 800, 0], [[1, 2], [3], [4, 5, 6, 7]]
    m = pack_meta(lay, meta, sizes, tgt, spec=rows)
    assert np.array_equal(lay.field(meta, "spec"), rows) and lay.field(meta, "n_samples").tolist() == sizes and m.len_out == sizes
    seen = []
    m2 = pack_meta(lay, meta, sizes, tgt, spec=lambda lens: seen.append(list(lens)) or rows + 1)      # rows made from the lengths decided there
    assert seen == [sizes] and np.array_equal(lay.field(meta, "spec"), rows + 1) and m2 == m
    with pytest.raises(TypeError):
        pack_meta(lay, meta, sizes, tgt, None, None, None, None, None, rows)      # keyword-only
    plain = MetaLayout(3, 4)
    buf = np.zeros(plain.size, dtype=np.int32)
    assert pack_meta(plain, buf, sizes, tgt) == m and np.array_equal(buf, meta[:plain.size])      # off: the words of before


def test_train_flag(monkeypatch):
    import torch
    import train

    class Built(Exception):
        pass

    assert train.TrainConfig().spec_aug == ""
    for flag, want in (("--spec_aug=w5,t2x50,f2x10,s3x30,r200", "w5,t2x50,f2x10,s3x30,r200"), ("--spec_aug=wenet", "wenet"), ("--spec_aug=", None), (None, None)):
        calls = []

        def fake_loader(**kw):
            calls.append(kw)
            if len(calls) == 3:
                raise Built
            return []

        monkeypatch.setattr(train, "build_dataloader", fake_loader)
        monkeypatch.setattr(train.Vocab, "load", staticmethod(lambda path: train.Vocab.synthetic(10)))
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(torch.cuda, "set_device", lambda i: None)
        monkeypatch.delenv("WORLD_SIZE", raising=False)
        with pytest.raises(Built):
            train.train(**train.parse_flags(["--model_name=TransformerOffical"] + ([flag] if flag else [])))
        assert [c["part"] for c in calls] == ["train", "test", "dev"]
        assert calls[0]["spec_augment"] == want and all("spec_augment" not in c for c in calls[1:])      # the train part only


def test_entry_points_are_named_and_validate_on_the_host():
    from asr_chinese_e2e_amd import _lib, kernels
    from asr_chinese_e2e_amd.data_handler import specaug
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    assert int(re.search(r"#define\s+ASR_SPECAUG_MAX_RANGES\s+(\d+)", text).group(1)) == _lib.SPECAUG_MAX_RANGES == specaug.MAX_RANGES == 8
    for name in ("asr_utt_norm_specaug_lfr_fwd", "asr_global_norm_specaug_lfr_fwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text) and name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1])
    assert callable(kernels.utt_norm_specaug_lfr) and callable(kernels.global_norm_specaug_lfr)
    assert _lib.lib.asr_abi_version() == 10
    ok = 4096      # any non-null address: every call below is refused before it would be read
    for lib in (_lib.lib, _lib.fast):
        for f, stats in ((lib.asr_utt_norm_specaug_lfr_fwd, ()), (lib.asr_global_norm_specaug_lfr_fwd, (ok, ok))):
            call = lambda feat=ok, wl=ok, rg=ok, ld=19, nt=2, nf=2, ns=3, st=stats, out=ok, ol=ok, B=2, Tmax=8, F=40, m=4, n=3, Tl=3, dt=0: \
                f(feat, wl, rg, ld, nt, nf, ns, *st, out, ol, B, Tmax, F, m, n, Tl, dt, None)
            for kw in (dict(feat=None), dict(wl=None), dict(rg=None), dict(out=None), dict(ol=None)):
                assert call(**kw) == -1 and "null pointer" in _lib.last_error(), kw
            if stats:
                assert call(st=(None, ok)) == -1 and call(st=(ok, None)) == -1 and "null pointer" in _lib.last_error()
                assert call(B=65536) == -1 and "B=65536" in _lib.last_error()
                assert call(Tl=2 ** 30, m=4, F=40) == -1 and "does not fit" in _lib.last_error()
            for kw, word in ((dict(nt=9), "n_t=9"), (dict(nf=9), "n_f=9"), (dict(ns=9), "n_s=9"), (dict(nt=-1), "n_t=-1"), (dict(ld=18), "ld=18"),
                             (dict(ld=0), "ld=0"), (dict(B=0), "B=0"), (dict(Tmax=0), "Tmax=0"), (dict(F=0), "n_mels=0"), (dict(m=0), "m=0"),
                             (dict(n=0), "n=0"), (dict(Tl=0), "Tlfr_max=0")):
                assert call(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
            assert call(nt=8, nf=8, ns=8, ld=57) == -1 and "ld=57" in _lib.last_error()      # 2 + 16 + 16 + 24 = 58 words
            assert call(dt=7) == -2 and "dtype 7" in _lib.last_error()
