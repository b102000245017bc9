"""Consensus decoding on the GPU, integer for integer against its definition (tests/consensus_ref.py): asr_nbest_consensus over the
lengths around the 64-column block, every list size at which a stage takes another path, absent entries, alphabets where ties are
everywhere, duplicates, zero weights, risk ties and slot ties, more distinct alternatives than are kept, insertion runs, strides, clamped
lengths, the launcher's refusals; consensus_ids / consensus_packed on the prototype's generator; model.consensus and model.evaluate on a
small model.  Every comparison is of integers: there is no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import consensus_ref as C  # noqa: E402
from tests import score_ref as R  # noqa: E402

DEV = "cuda"
LENS = (0, 1, 2, 63, 64, 65, 128, 129, 255, 256)
EPS = C.EPS


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int32))).to(DEV)


def _compare(host, u, hyps, weights, alts, S):
    """Every array of utterance u against the definition."""
    want = C.consensus(hyps, weights, alts)
    N, m = len(hyps), len(want["mbr"])
    assert host["d"][u, :N, :N].tolist() == want["d"]
    assert host["risk"][u, :N].tolist() == want["risk"] and int(host["pivot"][u]) == want["pivot"] and int(host["W"][u]) == want["W"]
    assert host["votes"][u, :N, :2 * m + 1].tolist() == want["votes"] and bool((host["votes"][u, :, 2 * m + 1:] == EPS).all())
    assert host["extra"][u, :N].tolist() == want["extra"]
    assert host["n_alts"][u, :2 * m + 1].tolist() == [s["n_alts"] for s in want["slots"]] and bool((host["n_alts"][u, 2 * m + 1:] == 0).all())
    assert host["pivot_w"][u, :2 * m + 1].tolist() == [s["pivot_weight"] for s in want["slots"]]
    fill = [(EPS, 0)] * alts
    assert [[tuple(a) for a in s] for s in host["alts"][u, :2 * m + 1].tolist()] == [(s["alts"] + fill)[:alts] for s in want["slots"]]
    assert all(tuple(a) == (EPS, 0) for s in host["alts"][u, 2 * m + 1:].tolist() for a in s) and S >= 2 * m + 1
    return want


def _run(K, lists, weights, alts=4, twice=False):
    """lists (None = absent) and weights through the kernels; the output's host views, compared with the definition list by list."""
    from asr_chinese_e2e_amd.consensus import _host_arrays
    tok, ln, w = _host_arrays(lists, weights, None, 1.0)
    U, N, L = tok.shape
    args = (_i32(tok), _i32(ln), _i32(w), ln, w)
    out = K.nbest_consensus(*args, alts=alts)
    if twice:      # no atomics, a fixed order: the same bytes in every run
        assert torch.equal(out, K.nbest_consensus(*args, alts=alts))
    host = K.nbest_unpack(out.cpu().numpy(), U, N, L, alts)
    wants = []
    for u, l in enumerate(lists):
        hyps = list(l) + [None] * (N - len(l))
        wants.append(_compare(host, u, hyps, w[u].tolist(), alts, 2 * L + 1))
    return host, wants


def _edits(rng, base, V, k):
    h = list(base)
    for _ in range(k):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(h) + 1))
        if kind == 0 and at < len(h):
            del h[at]
        elif kind == 1 and at < len(h):
            h[at] = int(rng.integers(0, V))
        else:
            h.insert(at, int(rng.integers(0, V)))
    return h[:C.MAX_LEN]


@pytest.mark.parametrize("V", [2, 3, 4232])
def test_every_length_around_the_block(K, V):
    rng = np.random.default_rng(V)
    mixed = [rng.integers(0, V, n).tolist() for n in LENS]
    base = rng.integers(0, V, 129).tolist()
    near = [_edits(rng, base, V, int(rng.integers(0, 6))) for _ in range(10)]      # a list that looks like an n-best: the pivot is long
    long_ = [_edits(rng, rng.integers(0, V, 256).tolist(), V, 0)] * 2 + [_edits(rng, base + base[:127], V, 9) for _ in range(8)]
    order = rng.permutation(10).tolist()
    lists = [mixed, near, long_, [mixed[i] for i in order]]
    weights = [rng.integers(0, 100000, 10).tolist() for _ in lists]
    _, wants = _run(K, lists, weights, alts=4, twice=True)
    assert len(wants[1]["mbr"]) > 64 and len(wants[2]["mbr"]) > 128


@pytest.mark.parametrize("N,U", [(1, 1), (2, 33), (5, 33), (63, 1), (64, 2)])
def test_list_sizes_absent_entries_duplicates_and_zero_weights(K, N, U):
    rng = np.random.default_rng(100 * N + U)
    lists, weights = [], []
    for u in range(U):
        base = rng.integers(0, 3, int(rng.integers(0, 13))).tolist()
        l = [_edits(rng, base, 3, int(rng.integers(0, 4))) for _ in range(N)]
        if N >= 5:
            l[3] = list(l[1])                                  # a duplicate
            gone = {0: [0], 1: [N // 2], 2: [N - 1], 3: [0, 1, N - 1]}.get(u % 5, [])      # absent at the front, in the middle, at the end
            for k in gone:
                l[k] = None
        w = rng.integers(0, 50000, N)
        w[rng.random(N) < 0.3] = 0                             # zero weights still vote
        if u % 7 == 6:
            w[:] = 0
        lists.append(l)
        weights.append(w.tolist())
    _run(K, lists, weights, alts=3)


def test_ties_and_more_alternatives_than_are_kept(K):
    # equal weights on a symmetric list: every risk ties, the lowest index wins; every slot ties, the first voter wins
    sym = [[1, 2], [2, 1], [1, 2], [2, 1]]
    # 12 distinct tokens in one slot, weights with ties: the top A are kept and n_alts is exact
    many = [[10 + k] for k in range(12)]
    many_w = [5, 9, 9, 1, 7, 7, 7, 2, 3, 9, 4, 6]
    gaps = [[1], [3, 1], [4, 1], [5, 1], [6, 1], [7, 1], [8, 1], [9, 1], [3, 1], [10, 1], [11, 1]]      # 10 alternatives in a gap slot
    gaps_w = [50, 2, 3, 3, 4, 5, 6, 7, 1, 8, 9]
    lists, weights = [sym, many, gaps, [None, [7], []]], [[250] * 4, many_w, gaps_w, [100, 500, 500]]
    for alts in (1, 8):
        host, wants = _run(K, lists, weights, alts=alts)
        assert wants[0]["risk"] == [1000] * 4 + [0] * 8      # the shorter lists are padded with absent entries
        assert wants[0]["pivot"] == 0 and wants[0]["slots"][1]["alts"][0] == (1, 500)
        assert wants[1]["pivot"] == 1 and wants[1]["slots"][1]["n_alts"] == 12 and wants[1]["slots"][1]["alts"][:min(alts, 4)] == [(11, 9), (12, 9), (19, 9), (14, 7)][:alts]
        assert wants[2]["pivot"] == 0 and wants[2]["slots"][0]["n_alts"] == 10 and wants[2]["slots"][0]["alts"][0] == (EPS, 50)
        assert wants[3]["pivot"] == 1 and wants[3]["consensus"] == [7]      # [7] before []: the risks tie and 1 < 2
        assert int(host["n_alts"][1, 1]) == 12


def test_insertion_runs_of_two_and_three(K):
    lists = [[[1, 2], [1, 7, 8, 9, 2], [5, 6, 1, 2]], [[1, 2, 3], [1, 2, 3, 4, 4], [1, 2, 3, 4, 4, 4], [9, 9, 1, 2, 3]]]
    _, wants = _run(K, lists, [[3, 2, 1], [5, 2, 2, 1]])
    assert wants[0]["votes"][1] == [EPS, 1, 7, 2, EPS] and wants[0]["votes"][2] == [5, 1, EPS, 2, EPS] and wants[0]["extra"] == [0, 2, 1, 0]
    assert wants[1]["extra"] == [0, 1, 2, 1] and wants[1]["slots"][6]["alts"] == [(EPS, 6), (4, 4)]


def test_padded_rows_and_clamped_lengths(K):
    rng = np.random.default_rng(9)
    U, N, L = 3, 4, 70
    buf = rng.integers(0, 3, (U, N + 1, L + 7)).astype(np.int32)
    d_tok = torch.from_numpy(buf).to(DEV)[:, :N, :L]
    assert d_tok.stride(0) == (N + 1) * (L + 7) and d_tok.stride(1) == L + 7
    dev_ln = np.array([[70, 1000, -5, 3], [2 ** 31 - 1, 0, 66, -(2 ** 31)], [-1, 65, 64, 300]], np.int32)      # past L and below -1: clamped
    ln = np.clip(dev_ln, -1, L).astype(np.int32)
    w = rng.integers(0, 1000, (U, N)).astype(np.int32)
    out = K.nbest_consensus(d_tok, _i32(dev_ln), _i32(w), ln, w, alts=2)
    host = K.nbest_unpack(out.cpu().numpy(), U, N, L, 2)
    for u in range(U):
        _compare(host, u, [buf[u, k, :ln[u, k]].tolist() if ln[u, k] >= 0 else None for k in range(N)], w[u].tolist(), 2, 2 * L + 1)


def test_stages_alone_equal_the_three_in_one(K):
    from asr_chinese_e2e_amd.consensus import _host_arrays
    rng = np.random.default_rng(4)
    lists = [[_edits(rng, [1, 2, 3, 4, 5], 6, 2) for _ in range(6)] for _ in range(3)]
    tok, ln, w = _host_arrays(lists, [[7, 6, 5, 4, 3, 2]] * 3, None, 1.0)
    args = (_i32(tok), _i32(ln), _i32(w), ln, w)
    whole = K.nbest_consensus(*args, alts=4)
    parts = torch.full_like(whole, -7)
    for stage in ("pair_dist", "pivot_votes", "slot_vote"):
        K.nbest_consensus(*args, alts=4, out=parts, stage=stage)
    assert torch.equal(whole, parts)
    with pytest.raises(ValueError, match="stage"):
        K.nbest_consensus(*args, stage="votes")


# ------------------------------------------------------------------------------------------------ refusals, before any launch
def test_refusals_leave_the_outputs_alone(K):
    from asr_chinese_e2e_amd import _lib
    U, N, L, A = 2, 3, 4, 2
    tok = torch.ones(U, N, L, dtype=torch.int32, device=DEV)
    ln, w = np.array([[4, -1, 2], [0, 1, -1]], np.int32), np.array([[5, 9, 5], [1, 1, 1]], np.int32)
    d_ln, d_w = _i32(ln), _i32(w)
    need = K.nbest_out_words(U, N, L, A) * 4
    out = torch.full((need // 4,), -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(fn="asr_nbest_consensus", **kw):
        a = dict(tok=tok.data_ptr(), len=d_ln.data_ptr(), weights=d_w.data_ptr(), L=L, ldn=L, ldu=N * L, h_len=ln.ctypes.data, h_w=w.ctypes.data, U=U, N=N, A=A,
                 out=out.data_ptr(), out_bytes=need, stream=stream)
        a.update(kw)
        return getattr(_lib.fast, fn)(*a.values())

    def mirror(src, at, value):
        m = src.copy()
        m[at] = value
        return m
    neg_w, big_w, long_len, none_present = mirror(w, (0, 2), -1), mirror(w, (1, 0), 2 ** 30), mirror(ln, (0, 0), 257), mirror(ln, (1, slice(None)), -1)
    cases = [dict(tok=None), dict(len=None), dict(weights=None), dict(h_len=None), dict(h_w=None), dict(out=None), dict(tok=tok.data_ptr() + 2),
             dict(len=d_ln.data_ptr() + 1), dict(out=out.data_ptr() + 4), dict(U=0), dict(U=-1), dict(U=65536), dict(N=0), dict(N=65), dict(L=-1), dict(L=257),
             dict(A=0), dict(A=9), dict(ldn=L - 1), dict(ldu=N * L - 1), dict(h_w=neg_w.ctypes.data), dict(h_w=big_w.ctypes.data),
             dict(h_len=long_len.ctypes.data), dict(h_len=none_present.ctypes.data)]
    for fn in ("asr_nbest_consensus", "asr_nbest_pair_dist", "asr_nbest_pivot_votes", "asr_nbest_slot_vote"):
        for kw in cases:
            assert call(fn, **kw) == -1 and fn in _lib.last_error(), (fn, kw)      # ASR_EINVAL
        assert call(fn, out_bytes=need - 1) == -3      # ASR_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    # the same arguments, unchanged, are accepted; so is a huge weight on an absent entry, which does not count
    masked = mirror(w, (0, 1), 2 ** 30)
    assert call() == 0
    first = out.clone()
    assert call(h_w=masked.ctypes.data) == 0 and torch.equal(first, out)
    host = K.nbest_unpack(out.cpu().numpy(), U, N, L, A)
    _compare(host, 0, [[1, 1, 1, 1], None, [1, 1]], [5, 9, 5], A, 2 * L + 1)
    _compare(host, 1, [[], [1], None], [1, 1, 1], A, 2 * L + 1)


# ------------------------------------------------------------------------------------------------ the Python interface
def _as_reference(got, lists, weights, alts):
    for g, l, w in zip(got, lists, weights):
        want = C.consensus(l, w, alts)
        W = want["W"]
        assert g["pivot"] == want["pivot"] and g["mbr"] == want["mbr"] and g["consensus"] == want["consensus"] and g["risk"] == want["risk"]
        assert g["confidence"] == want["confidence"] and g["expected_errors"] == want["expected_errors"] and g["extra_insertions"] == want["extra_insertions"]
        assert g["weights"] == [int(x) for x in w] and len(g["slots"]) == len(want["slots"])
        for s, (gs, ws) in enumerate(zip(g["slots"], want["slots"])):
            assert gs["pivot_pos"] == (s // 2 if s & 1 else None) and gs["n_alternatives"] == ws["n_alts"]
            assert gs["alternatives"] == [(None if t == EPS else t, x / W if W else 0.0) for t, x in ws["alts"]]


@pytest.fixture(scope="module")
def prototype():
    from tests.test_consensus_cpu import prototype_lists
    lists, scores = prototype_lists(150)
    return lists, scores, [C.nbest_weights(s).tolist() for s in scores]


def test_consensus_ids_on_the_prototype_generator(prototype):
    from asr_chinese_e2e_amd.consensus import consensus_ids
    lists, scores, weights = prototype
    got = consensus_ids(lists, scores=scores, alts=4)
    _as_reference(got, lists, weights, 4)
    assert any(g["pivot"] != 0 for g in got) and any(g["consensus"] not in l for g, l in zip(got, lists)) and any(g["extra_insertions"] > 0 for g in got)
    assert consensus_ids(lists, weights=weights, alts=4) == got
    scaled = consensus_ids(lists[:20], scores=scores[:20], scale=0.25, alts=2)
    _as_reference(scaled, lists[:20], [C.nbest_weights(s, 0.25).tolist() for s in scores[:20]], 2)
    flat = consensus_ids(lists[:5])      # neither weights nor scores: every entry counts alike
    _as_reference(flat, lists[:5], [[(1 << 20) // len(l)] * len(l) for l in lists[:5]], 4)


def test_consensus_packed_equals_consensus_ids(prototype, K):
    from asr_chinese_e2e_amd.consensus import _host_arrays, consensus_ids, consensus_packed, unpack_results
    lists, scores, weights = prototype
    tok, ln, w = _host_arrays(lists, weights, None, 1.0)
    views = consensus_packed(_i32(tok), _i32(ln), _i32(w), ln, w, alts=4)
    assert all(v.is_cuda for v in views.values()) and views["risk"].dtype == torch.int64 and views["alts"].shape == (150, 2 * tok.shape[2] + 1, 4, 2)
    host = K.nbest_unpack(views["buffer"].cpu().numpy(), *tok.shape, 4)
    assert unpack_results(host, tok, ln, w, 4, sizes=[len(l) for l in lists]) == consensus_ids(lists, weights=weights, alts=4)
    assert views["pivot"].cpu().tolist() == [C.consensus(l, x)["pivot"] for l, x in zip(lists, weights)]


# ------------------------------------------------------------------------------------------------ the model
def _batches(V):
    from asr_chinese_e2e_amd.data_handler import synthetic_pack
    return [synthetic_pack(3, 60, 320, V, seed=41, ragged=True, Lmin=3, Lmax=9, device=DEV),
            synthetic_pack(2, 48, 320, V, seed=42, ragged=True, Lmin=2, Lmax=12, device=DEV)]


def _strip(seq):
    seq = list(seq)
    seq = seq[1:] if seq and seq[0] == 2 else seq
    return seq[:-1] if seq and seq[-1] == 3 else seq


@pytest.mark.parametrize("search", ["ctc_prefix_beam", "attention_beam"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_model_consensus_equals_the_definition(dtype, search):
    from tests.test_align_long_gpu import _model
    model = _model(dtype)
    pack = _batches(30)[0]
    got = model.consensus(pack, search=search, beam_size=4, nbest=4, posterior_scale=0.5, alts=3)
    fn = model.ctc_prefix_beam_search if search == "ctc_prefix_beam" else model.beam_search
    with torch.no_grad():
        found = fn(pack, 4, 4)
    assert len(got) == len(found) == 3 and max(len(u) for u in found) > 1
    for g, utt in zip(got, found):
        lists, w = [_strip(h["yseq"]) for h in utt], C.nbest_weights([h["score"] for h in utt], 0.5)
        want = C.consensus(lists, w, 3)
        assert g["nbest"] == utt and g["best_ids"] == lists[0]
        assert g["ids"] == want["consensus"] and g["mbr_ids"] == want["mbr"] and g["mbr_rank"] == want["pivot"] and g["confidence"] == want["confidence"]
        assert [s["n_alternatives"] for s in g["slots"]] == [s["n_alts"] for s in want["slots"]]
        assert [[t for t, _ in s["alternatives"]] for s in g["slots"]] == [[None if t == EPS else t for t, _ in s["alts"]] for s in want["slots"]]
        assert g["text"] == "".join(model.vocab._id2token[i] for i in g["ids"])
    with pytest.raises(ValueError, match="nbest"):
        model.consensus(pack, nbest=65)
    with pytest.raises(ValueError, match="posterior_scale"):
        model.consensus(pack, posterior_scale=0.0)


def test_model_evaluate_with_consensus_equals_a_host_recomputation():
    from tests.test_align_long_gpu import _model
    model = _model("fp32")
    batches = _batches(30)
    got = model.evaluate(batches, search="ctc_prefix_beam", nbest=4, beam_size=4, consensus=True, posterior_scale=0.5).summary()
    plain = model.evaluate(batches, search="ctc_prefix_beam", nbest=4, beam_size=4).summary()
    assert set(plain) == {"utterances", "ref_tokens", "cor", "sub", "del", "ins", "cer", "ser", "empty_refs", "cer_ref_convention", "oracle_cer", "oracle_rank_hist"}
    assert {k: got[k] for k in plain} == plain and set(got) - set(plain) == {"mbr_cer", "consensus_cer", "mbr_rank_hist"}
    mbr = cons = tokens = 0
    hist = [0, 0, 0, 0]
    for pack in batches:
        tgt, n = pack.tgt_for_input.cpu(), pack.tgt_len.cpu().tolist()
        with torch.no_grad():
            found = model.ctc_prefix_beam_search(pack, 4, 4)
        for b, utt in enumerate(found):
            gold = tgt[b, :n[b]].tolist()
            lists = [[x for x in h["yseq"] if x not in (0, 2, 3)] for h in utt] or [[]]
            want = C.consensus(lists, C.nbest_weights([h["score"] for h in utt] or [0.0], 0.5), 1)
            mbr += R.align(gold, want["mbr"])["distance"]
            cons += R.align(gold, want["consensus"])["distance"]
            hist[want["pivot"]] += 1
            tokens += len(gold)
    assert got["mbr_cer"] == mbr / tokens and got["consensus_cer"] == cons / tokens and got["mbr_rank_hist"] == hist[:len(got["mbr_rank_hist"])] and sum(hist) == 5
    with pytest.raises(ValueError, match="n-best search"):
        model.evaluate(batches, consensus=True)
    with pytest.raises(ValueError, match="posterior_scale"):
        model.evaluate(batches, search="ctc_prefix_beam", nbest=2, consensus=True, posterior_scale=-1.0)
