"""Token-level scoring on the GPU, integer for integer against its definition (tests/score_ref.py): asr_edit_align over the lengths around
the 64-column block, alphabets where ties are everywhere, shared and permuted references, strides, clamped lengths, extreme ids, the
counts-only mode, the placement of the direction masks at the LDS budget and past it, the launcher's refusals; model.evaluate on a small
model.  Every comparison is of integers: there is no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import score_ref as R  # noqa: E402

DEV = "cuda"
LENS = (0, 1, 2, 63, 64, 65, 128, 129)
KEYS = ("distance", "cor", "sub", "del", "ins")


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _seq(rng, n, V):
    return rng.integers(0, V, n).tolist()


def _check(got, refs, hyps, ref_of=None, ops=True):
    assert len(got) == len(hyps)
    cache = {}
    for p, g in enumerate(got):
        r = refs[p if ref_of is None else ref_of[p]]
        key = (tuple(r), tuple(hyps[p]))
        if key not in cache:
            cache[key] = R.align(r, hyps[p])
        want = cache[key]
        assert {k: g[k] for k in KEYS} == {k: want[k] for k in KEYS}, (p, len(r), len(hyps[p]))
        if ops:
            assert g["ops"] == want["ops"], (p, len(r), len(hyps[p]))
        else:
            assert "ops" not in g


@pytest.mark.parametrize("V", [2, 3, 4232])
def test_every_length_around_the_block(V):
    from asr_chinese_e2e_amd.scoring import align_ids
    rng = np.random.default_rng(V)
    refs = [_seq(rng, m, V) for m in LENS for _ in LENS]
    hyps = [_seq(rng, n, V) for _ in LENS for n in LENS]
    _check(align_ids(hyps, refs), refs, hyps)
    _check(align_ids(hyps, refs, ops=False), refs, hyps, ops=False)


def test_identical_disjoint_repeated_and_extreme_ids():
    from asr_chinese_e2e_amd.scoring import align_ids
    rng = np.random.default_rng(5)
    V = 4232
    a = _seq(rng, 129, V)
    big = 2 ** 31 - 1
    pairs = [(a, a), (a, [x + V for x in a]), ([7] * 65, [7] * 129), ([7] * 129, [7] * 64), ([7] * 70, [8] * 66), (a[:64], a[1:65]), (a[1:65], a[:64]),
             ([0, V - 1, big, 0], [big, 0, V - 1]), ([big] * 3, [big - 1, big, 0, big]), ([0], [0]), ([0, 0, 0], [])]
    refs, hyps = [p[0] for p in pairs], [p[1] for p in pairs]
    _check(align_ids(hyps, refs), refs, hyps)
    _check(align_ids(hyps, refs, ops=False), refs, hyps, ops=False)


@pytest.mark.parametrize("P", [1, 7, 130])
def test_shared_references_in_permuted_order(P):
    from asr_chinese_e2e_amd.scoring import align_ids
    rng = np.random.default_rng(P)
    nref = (P + 9) // 10
    refs = [_seq(rng, int(rng.integers(0, 40)), 3) for _ in range(nref)]
    ref_of = [p // 10 for p in range(P)]      # an n-best of 10 per reference
    ref_of = [ref_of[i] for i in rng.permutation(P)]
    hyps = []
    for p in range(P):      # the reference with a few edits, so that the list looks like an n-best
        h = list(refs[ref_of[p]])
        for _ in range(int(rng.integers(0, 4))):
            at = int(rng.integers(0, len(h) + 1))
            if rng.random() < 0.5 and at < len(h):
                del h[at]
            else:
                h.insert(at, int(rng.integers(0, 3)))
        hyps.append(h)
    _check(align_ids(hyps, refs, ref_of=ref_of), refs, hyps, ref_of)
    _check(align_ids(hyps, refs, ref_of=ref_of, ops=False), refs, hyps, ref_of, ops=False)


def _unpack(counts, ops, n_ops):
    counts, ops, n_ops = counts.cpu().numpy(), ops.cpu().numpy(), n_ops.cpu().tolist()
    return [dict(zip(KEYS, counts[p].tolist()), ops=list(zip(*ops[p, :, :n_ops[p]].tolist())) if n_ops[p] else []) for p in range(len(n_ops))]


def test_padded_rows_and_clamped_lengths(K):
    rng = np.random.default_rng(9)
    P_, Lh, Lr = 5, 70, 66
    hbuf, rbuf = rng.integers(0, 3, (P_, Lh + 7)).astype(np.int32), rng.integers(0, 3, (P_, Lr + 3)).astype(np.int32)
    hl, rl = [70, 3, 1000, 0, 2 ** 31 - 1], [66, 900, 5, 67, -4]      # past Lh / Lr and below 0: clamped
    ro = [4, 3, 2, 1, 0]
    d_h, d_r = torch.from_numpy(hbuf).to(DEV)[:, :Lh], torch.from_numpy(rbuf).to(DEV)[:, :Lr]
    assert d_h.stride(0) == Lh + 7 and d_r.stride(0) == Lr + 3
    got = _unpack(*K.edit_align(d_h, _i32(hl), d_r, _i32(rl), _i32(ro), hl, rl, ro))
    refs = [rbuf[q, :min(max(rl[q], 0), Lr)].tolist() for q in range(P_)]
    hyps = [hbuf[p, :min(max(hl[p], 0), Lh)].tolist() for p in range(P_)]
    _check(got, refs, hyps, ro)
    counts, none, none2 = K.edit_align(d_h, _i32(hl), d_r, _i32(rl), _i32(ro), hl, rl, ro, ops=False)
    assert none is None and none2 is None
    assert counts.cpu().tolist() == [[g[k] for k in KEYS] for g in got]


# ------------------------------------------------------------------------------------------------ where the direction masks live
@pytest.fixture(scope="module")
def long_pair():
    rng = np.random.default_rng(77)
    ref, hyp = _seq(rng, 1100, 4), _seq(rng, 1000, 4)
    return ref, hyp, R.align(ref, hyp)


def test_mask_placement_at_the_lds_budget(K):
    from asr_chinese_e2e_amd.scoring import align_ids
    rng = np.random.default_rng(31)
    n, m = 128, K.EDIT_LDS_DIR_BYTES // 32
    assert m * 2 * 16 == K.EDIT_LDS_DIR_BYTES
    ref, hyp = _seq(rng, m + 1, 3), _seq(rng, n, 3)
    assert K.edit_align_workspace_bytes([n], [m], [0], n, m) == 0
    assert K.edit_align_workspace_bytes([n], [m + 1], [0], n, m + 1) == (m + 1) * 2 * 16
    _check(align_ids([hyp], [ref[:m]]), [ref[:m]], [hyp])
    _check(align_ids([hyp], [ref]), [ref], [hyp])


def test_long_pair_uses_the_workspace_and_mixes_with_short_pairs(K, long_pair):
    from asr_chinese_e2e_amd.scoring import align_ids
    ref, hyp, want = long_pair
    assert K.edit_align_workspace_bytes([len(hyp)], [len(ref)], [0], len(hyp), len(ref)) == len(ref) * 16 * 16 > K.EDIT_LDS_DIR_BYTES
    alone = align_ids([hyp], [ref])[0]
    assert alone == want
    counts = align_ids([hyp], [ref], ops=False)[0]
    assert counts == {k: want[k] for k in KEYS}
    rng = np.random.default_rng(3)
    refs = [_seq(rng, 15, 3) for _ in range(6)]
    hyps = [_seq(rng, int(rng.integers(0, 20)), 3) for _ in range(6)]
    short = align_ids(hyps, refs)
    _check(short, refs, hyps)
    mixed = align_ids(hyps[:3] + [hyp] + hyps[3:] + [hyp[:900]], refs[:3] + [ref] + refs[3:], ref_of=[0, 1, 2, 3, 4, 5, 6, 3])
    assert mixed[:3] == short[:3] and mixed[4:7] == short[3:] and mixed[3] == want
    assert mixed[7] == R.align(ref, hyp[:900])


# ------------------------------------------------------------------------------------------------ refusals, before any launch
def test_refusals_leave_the_outputs_alone(K):
    from asr_chinese_e2e_amd import _lib
    P_, Rn, Lh, Lr = 3, 2, 8, 8
    hyp, ref = torch.ones(P_, Lh, dtype=torch.int32, device=DEV), torch.ones(Rn, Lr, dtype=torch.int32, device=DEV)
    hl, rl, ro = np.array([8, 4, 0], np.int32), np.array([8, 3], np.int32), np.array([0, 1, 1], np.int32)
    d_hl, d_rl, d_ro = _i32(hl), _i32(rl), _i32(ro)
    ldo = Lh + Lr
    counts = torch.full((P_, 5), -7, dtype=torch.int32, device=DEV)
    ops = torch.full((P_, 3, ldo), -7, dtype=torch.int32, device=DEV)
    n_ops = torch.full((P_,), -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def args(**kw):
        a = dict(hyp=hyp.data_ptr(), hyp_len=d_hl.data_ptr(), Lh=Lh, ldh=Lh, ref=ref.data_ptr(), ref_len=d_rl.data_ptr(), Lr=Lr, ldr=Lr, ref_of=d_ro.data_ptr(),
                 h_hl=hl.ctypes.data, h_rl=rl.ctypes.data, h_ro=ro.ctypes.data, P=P_, R=Rn, counts=counts.data_ptr(), ops=ops.data_ptr(), n_ops=n_ops.data_ptr(),
                 ldo=ldo, ws=None, ws_bytes=0, stream=stream)
        a.update(kw)
        return list(a.values())

    bad_ro = np.array([0, 2, 1], np.int32)
    neg_ro = np.array([0, -1, 1], np.int32)
    cases = [dict(hyp=None), dict(ref=None), dict(hyp_len=None), dict(ref_len=None), dict(ref_of=None), dict(counts=None), dict(n_ops=None),
             dict(h_hl=None), dict(h_rl=None), dict(h_ro=None), dict(hyp=hyp.data_ptr() + 2), dict(counts=counts.data_ptr() + 1), dict(ops=ops.data_ptr() + 2),
             dict(P=0), dict(P=-1), dict(R=0), dict(Lh=-1), dict(Lr=-1), dict(ldh=Lh - 1), dict(ldr=Lr - 1), dict(ldo=ldo - 1),
             dict(h_ro=bad_ro.ctypes.data), dict(h_ro=neg_ro.ctypes.data)]
    for kw in cases:
        assert _lib.fast.asr_edit_align(*args(**kw)) == -1, kw      # ASR_EINVAL
        assert "asr_edit_align" in _lib.last_error()
    # a pair past the LDS budget with no workspace, and with one a byte short of the size query's answer
    m = K.EDIT_LDS_DIR_BYTES // 16 + 1
    bref = torch.ones(1, m, dtype=torch.int32, device=DEV)
    bl, bo, one = np.array([m], np.int32), np.array([0, 0, 0], np.int32), _i32([m])
    need = K.edit_align_workspace_bytes(hl, bl, bo, Lh, m)
    assert need == 2 * m * 16      # the 8-token hypothesis and the 4-token one; the empty one needs none
    bops = torch.full((P_, 3, Lh + m), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    big = dict(ref=bref.data_ptr(), ref_len=one.data_ptr(), Lr=m, ldr=m, R=1, h_rl=bl.ctypes.data, h_ro=bo.ctypes.data, ops=bops.data_ptr(), ldo=Lh + m)
    assert _lib.fast.asr_edit_align(*args(**big)) == -3      # ASR_EWORKSPACE
    assert _lib.fast.asr_edit_align(*args(ws=ws.data_ptr(), ws_bytes=need - 1, **big)) == -3
    assert _lib.fast.asr_edit_align(*args(ws=ws.data_ptr() + 8, ws_bytes=need, **big)) == -1      # misaligned workspace
    too = np.array([K.EDIT_MAX_REF + 1], np.int32)
    assert _lib.fast.asr_edit_align(*args(**dict(big, Lr=K.EDIT_MAX_REF + 1, ldr=K.EDIT_MAX_REF + 1, h_rl=too.ctypes.data, ops=None, n_ops=None))) == -1
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((ops == -7).all()) and bool((n_ops == -7).all()) and bool((bops == -7).all())
    # the same arguments, unchanged, are accepted
    assert _lib.fast.asr_edit_align(*args()) == 0
    assert counts.cpu().tolist() == [[0, 8, 0, 0, 0], [1, 3, 0, 0, 1], [3, 0, 0, 3, 0]] and n_ops.cpu().tolist() == [8, 4, 3]
    assert _lib.fast.asr_edit_align(*args(ws=ws.data_ptr(), ws_bytes=need, **big)) == 0
    assert counts.cpu().tolist() == [[m - 8, 8, 0, m - 8, 0], [m - 4, 4, 0, m - 4, 0], [m, 0, 0, m, 0]] and n_ops.cpu().tolist() == [m, m, m]


# ------------------------------------------------------------------------------------------------ the model
def _batches(V):
    from asr_chinese_e2e_amd.data_handler import synthetic_pack
    return [synthetic_pack(3, 60, 320, V, seed=41, ragged=True, Lmin=3, Lmax=9, device=DEV),
            synthetic_pack(2, 48, 320, V, seed=42, ragged=True, Lmin=2, Lmax=12, device=DEV)]


def _gold(batches):
    out = []
    for pack in batches:
        tgt, n = pack.tgt_for_input.cpu(), pack.tgt_len.cpu().tolist()
        out += [tgt[b, :n[b]].tolist() for b in range(tgt.shape[0])]
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_model_evaluate_equals_the_definition(dtype):
    from asr_chinese_e2e_amd.scoring import Scorer
    from tests.test_align_long_gpu import _model
    model = _model(dtype)
    batches = _batches(30)
    got = model.evaluate(batches, beam_size=3)
    hyps = [r["ids"] for pack in batches for r in model.transcribe(pack, beam_size=3, timestamps=False)]
    gold = _gold(batches)
    want = Scorer(model.vocab)
    keys = [f"utt{i}" for i in range(5)]
    want.add_aligned(keys, [R.align(want._clean(r), want._clean(h)) for r, h in zip(gold, hyps)], hyps, gold)
    assert got.utts == want.utts and got.summary() == want.summary()
    assert got.summary()["utterances"] == 5 and got.summary()["ref_tokens"] == sum(len(g) for g in gold) > 0
    assert got.per_token() == want.per_token() and got.confusions() == want.confusions()


def test_oracle_cer_of_the_ctc_nbest():
    from tests.test_align_long_gpu import _model
    model = _model("fp32")
    batches = _batches(30)
    got = model.evaluate(batches, search="ctc_prefix_beam", nbest=4, beam_size=4)
    gold = _gold(batches)
    lists = [utt for pack in batches for utt in model.ctc_prefix_beam_search(pack, 4, 4)]
    assert len(lists) == 5 and max(len(u) for u in lists) > 1
    best, hist = 0, [0, 0, 0, 0]
    for utt, g in zip(lists, gold):
        d = [R.align(g, [x for x in h["yseq"] if x not in (0, 2, 3)])["distance"] for h in utt]
        best += min(d)
        hist[d.index(min(d))] += 1
    s = got.summary()
    assert s["oracle_cer"] == best / sum(len(g) for g in gold) and s["oracle_rank_hist"] == hist[:len(s["oracle_rank_hist"])] and sum(hist) == 5
    assert s["oracle_cer"] <= s["cer"]
    with pytest.raises(ValueError, match="nbest"):
        model.evaluate(batches, nbest=2)
    with pytest.raises(ValueError, match="search"):
        model.evaluate(batches, search="greedy")
