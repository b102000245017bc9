"""Consensus decoding without a GPU: the definition (tests/consensus_ref.py) against an independent two-row DP and a hand case, the
weights, the properties the definition promises, every refusal that needs no launch, the binding, and the Scorer's new summary keys on
host-made results.  Integers throughout; the only floats are the divisions by W."""
import os
import re

import numpy as np
import pytest

from tests import consensus_ref as C
from tests import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("asr_nbest_out_bytes", "asr_nbest_pair_dist", "asr_nbest_pivot_votes", "asr_nbest_slot_vote", "asr_nbest_consensus")


def _two_row(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[-1]


def prototype_lists(count, seed=0):
    """The generator the feature was prototyped on: an alphabet of 6 ids, 2 to 10 entries, a reference of 3 to 11 tokens with up to 3 random
    edits per entry, weights from sorted normal scores (sd 1.5)."""
    rng = np.random.default_rng(seed)
    lists, scores = [], []
    for _ in range(count):
        ref = rng.integers(0, 6, int(rng.integers(3, 12))).tolist()
        ent = []
        for _ in range(int(rng.integers(2, 11))):
            h = list(ref)
            for _ in range(int(rng.integers(0, 4))):
                kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(h) + 1))
                if kind == 0 and at < len(h):
                    del h[at]
                elif kind == 1 and at < len(h):
                    h[at] = int(rng.integers(0, 6))
                else:
                    h.insert(at, int(rng.integers(0, 6)))
            ent.append(h)
        lists.append(ent)
        scores.append(np.sort(rng.normal(0.0, 1.5, len(ent)))[::-1].tolist())
    return lists, scores


def test_reference_against_brute_force():
    lists, scores = prototype_lists(60)
    off_rank0 = outside = extra = 0
    for l, s in zip(lists, scores):
        w = C.nbest_weights(s)
        got = C.consensus(l, w)
        d = [[_two_row(a, b) for b in l] for a in l]
        assert got["d"] == d and all(d[i][k] == d[k][i] for i in range(len(l)) for k in range(len(l)))
        risk = [sum(int(w[k]) * d[i][k] for k in range(len(l))) for i in range(len(l))]
        assert got["risk"] == risk and got["pivot"] == risk.index(min(risk)) and got["W"] == int(w.sum())
        assert got["mbr"] == l[got["pivot"]] and len(got["votes"][0]) == 2 * len(got["mbr"]) + 1
        for sl in got["slots"]:      # every present entry votes once per slot
            assert sl["n_alts"] >= len(sl["alts"]) >= 1 and sum(x for _, x in sl["alts"]) <= got["W"]
        off_rank0 += got["pivot"] != 0
        outside += got["consensus"] not in l
        extra += got["extra_insertions"] > 0
    assert off_rank0 and outside and extra      # the generator reaches every branch


def test_hand_case():
    got = C.consensus([[1, 2, 3], [1, 4, 3], [1, 2, 3, 5], [1, 2]], [400000, 300000, 200000, 148576])
    assert got["risk"] == [648576, 1097152, 1297152, 1400000] and got["pivot"] == 0 and got["W"] == 1048576
    assert got["consensus"] == [1, 2, 3] and got["mbr"] == [1, 2, 3]
    assert got["confidence"] == [1.0, 748576 / 1048576, 900000 / 1048576]
    assert got["slots"][6] == {"alts": [(C.EPS, 848576), (5, 200000)], "n_alts": 2, "pivot_weight": 848576}
    assert got["slots"][3]["alts"] == [(2, 748576), (4, 300000)] and got["slots"][5]["alts"] == [(3, 900000), (C.EPS, 148576)]
    assert got["extra_insertions"] == 0 and got["expected_errors"][0] == 648576 / 1048576


def test_insertion_runs_vote_once():
    got = C.consensus([[1, 2], [1, 7, 8, 9, 2], [5, 6, 1, 2]], [3, 2, 1])
    assert got["pivot"] == 0 and got["votes"][1] == [C.EPS, 1, 7, 2, C.EPS] and got["votes"][2] == [5, 1, C.EPS, 2, C.EPS]
    assert got["extra"] == [0, 2, 1] and got["extra_insertions"] == 3 and got["consensus"] == [1, 2]


def test_nbest_weights():
    from asr_chinese_e2e_amd.consensus import nbest_weights
    rng = np.random.default_rng(1)
    for n in (1, 2, 10, 64):
        s = np.sort(rng.normal(0, 3, n))[::-1]
        w = nbest_weights(s)
        assert w.dtype == np.int32 and abs(int(w.sum()) - 2 ** 20) <= n / 2 and (w >= 0).all()
        assert (w == C.nbest_weights(s)).all() and (np.diff(w) <= 0).all()      # sorted scores: weights that never rise
    assert nbest_weights([-3.5]).tolist() == [2 ** 20]
    assert nbest_weights([0.0, -np.inf, 0.0]).tolist() == [2 ** 19, 0, 2 ** 19]
    assert nbest_weights([-np.inf, -np.inf]).tolist() == [0, 0]
    assert nbest_weights([0.0, -1.0], scale=2.0).tolist() == nbest_weights([0.0, -2.0]).tolist() != nbest_weights([0.0, -1.0]).tolist()
    assert nbest_weights([0.0, np.log(0.5)]).tolist() == [699051, 349525]      # 2/3 and 1/3 of 2**20, rounded half up
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="scale"):
            nbest_weights([0.0], scale=bad)
    with pytest.raises(ValueError, match="NaN"):
        nbest_weights([0.0, np.nan])


def test_properties_of_the_reference():
    one = C.consensus([[4, 5, 6]], [2 ** 20])
    assert one["consensus"] == [4, 5, 6] and one["confidence"] == [1.0, 1.0, 1.0] and one["pivot"] == 0
    l = [[1, 2, 3], [9, 9], [1, 2, 4, 3]]
    all_on_one = C.consensus(l, [0, 2 ** 20, 0])
    assert all_on_one["pivot"] == 1 and all_on_one["consensus"] == [9, 9] and all_on_one["confidence"] == [1.0, 1.0]
    pooled = C.consensus([[1, 2], [3, 4], [3, 4]], [400, 300, 300])      # the duplicates pool their weight: 600 against 400
    assert pooled["pivot"] == 1 and pooled["consensus"] == [3, 4] and pooled["slots"][1]["alts"] == [(3, 600), (1, 400)]
    tie = C.consensus([[], [7]], [500, 500])
    assert tie["pivot"] == 0 and tie["consensus"] == [] and tie["slots"] == [{"alts": [(C.EPS, 500), (7, 500)], "n_alts": 2, "pivot_weight": 500}]
    zero = C.consensus([[1], [2]], [0, 0])
    assert zero["W"] == 0 and zero["pivot"] == 0 and zero["confidence"] == [0.0] and zero["expected_errors"] == [0.0, 0.0] and zero["consensus"] == [1]
    absent = C.consensus([None, [1, 2], None, [1, 3]], [9, 1, 9, 1])
    assert absent["pivot"] == 1 and absent["W"] == 2 and absent["risk"] == [0, 1, 0, 1] and absent["votes"][0] == [C.EPS] * 5
    assert absent["slots"][3]["alts"] == [(2, 1), (3, 1)]      # equal weights: the first voter wins


def test_refusals_without_a_launch():
    from asr_chinese_e2e_amd import consensus as M
    from asr_chinese_e2e_amd import kernels as K
    with pytest.raises(ValueError, match="no lists"):
        M.consensus_ids([])
    with pytest.raises(ValueError, match="between 1 and 64"):
        M.consensus_ids([[[1]] * 65])
    with pytest.raises(ValueError, match="between 1 and 64"):
        M.consensus_ids([[]])
    with pytest.raises(ValueError, match="256"):
        M.consensus_ids([[[1] * 257]])
    with pytest.raises(ValueError, match="no entry"):
        M.consensus_ids([[None, None]])
    with pytest.raises(ValueError, match="alts"):
        M.consensus_ids([[[1]]], alts=0)
    with pytest.raises(ValueError, match="alts"):
        M.consensus_ids([[[1]]], alts=9)
    with pytest.raises(ValueError, match="2\\*\\*30"):
        M.consensus_ids([[[1], [2]]], weights=[[2 ** 30, 1]])
    with pytest.raises(ValueError, match=">= 0"):
        M.consensus_ids([[[1], [2]]], weights=[[5, -1]])
    with pytest.raises(ValueError, match="entry for entry"):
        M.consensus_ids([[[1], [2]]], weights=[[5]])
    with pytest.raises(ValueError, match="not both"):
        M.consensus_ids([[[1]]], weights=[[5]], scores=[[0.0]])
    with pytest.raises(ValueError, match="id outside"):
        M.consensus_ids([[[-1]]])
    for U, N, L, A in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 65, 1, 1), (1, 1, 257, 1), (1, 1, -1, 1), (1, 1, 1, 0), (1, 1, 1, 9)):
        with pytest.raises(ValueError, match="bad shape"):
            K.nbest_out_words(U, N, L, A)
    U, N, L, A = 3, 5, 7, 4
    S = 2 * L + 1
    assert K.nbest_out_words(U, N, L, A) == U * (2 * N + N * N + 2 + N + 2 * S + N * S + S * A * 2)
    flat = np.arange(K.nbest_out_words(U, N, L, A), dtype=np.int32)
    v = K.nbest_unpack(flat, U, N, L, A)
    assert v["risk"].shape == (U, N) and v["risk"].dtype == np.int64 and v["alts"].shape == (U, S, A, 2) and int(v["alts"][-1, -1, -1, -1]) == flat[-1]
    assert int(v["d"][0, 0, 0]) == 2 * U * N and v["votes"].shape == (U, N, S)


def test_model_refusals_come_before_the_search():
    from asr_chinese_e2e_amd.consensus import model_consensus

    class Never:
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")
    for kw in (dict(nbest=65), dict(nbest=0), dict(posterior_scale=0.0), dict(posterior_scale=float("nan")), dict(posterior_scale=float("inf")),
               dict(alts=9), dict(search="greedy")):
        with pytest.raises(ValueError):
            model_consensus(Never(), None, **kw)


def test_abi_header_binding_and_makefile():
    from asr_chinese_e2e_amd import _lib, kernels
    raw = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    consts = {k: int(v.strip("()")) for k, v in re.findall(r"#define (ASR_NBEST_\w+) (\(?-?\d+\)?)", raw)}
    assert consts == {"ASR_NBEST_MAX_N": kernels.NBEST_MAX_N == C.MAX_N and C.MAX_N, "ASR_NBEST_MAX_LEN": kernels.NBEST_MAX_LEN == C.MAX_LEN and C.MAX_LEN,
                      "ASR_NBEST_MAX_ALTS": kernels.NBEST_MAX_ALTS == C.MAX_ALTS and C.MAX_ALTS, "ASR_NBEST_EPS": kernels.NBEST_EPS == C.EPS and C.EPS}
    assert _lib.ABI_VERSION == 10 == _lib.lib.asr_abi_version()
    make = open(os.path.join(ROOT, "asr_chinese_e2e_amd", "csrc", "Makefile")).read()
    assert "consensus.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1)


def test_launcher_refusals_on_the_host():
    """The launcher reads only its host mirrors before it refuses: host addresses stand in for the device pointers, nothing is launched."""
    from asr_chinese_e2e_amd import _lib
    U, N, L, A = 2, 3, 4, 2
    tok = np.zeros((U, N, L), np.int32)
    ln, w = np.array([[4, -1, 2], [0, 1, -1]], np.int32), np.array([[5, 9, 5], [1, 1, 1]], np.int32)
    need = int(_lib.fast.asr_nbest_out_bytes(U, N, L, A))
    out = np.full(need // 4 + 2, -7, np.int32)
    base = out.ctypes.data + (out.ctypes.data % 8)

    def call(fn="asr_nbest_consensus", **kw):
        a = dict(tok=tok.ctypes.data, len=ln.ctypes.data, weights=w.ctypes.data, L=L, ldn=L, ldu=N * L, h_len=ln.ctypes.data, h_w=w.ctypes.data, U=U, N=N, A=A,
                 out=base, out_bytes=need, stream=None)
        a.update(kw)
        return getattr(_lib.fast, fn)(*a.values())

    def mirror(at, value, which):
        m = (ln if which == "len" else w).copy()
        m[at] = value
        return m
    neg_w, big_w, long_len, none_present = mirror((0, 2), -1, "w"), mirror((1, 0), 2 ** 30, "w"), mirror((0, 0), 257, "len"), mirror((1, slice(None)), -1, "len")
    masked_w = mirror((0, 1), 2 ** 30, "w")      # an absent entry's weight does not count
    cases = [dict(tok=None), dict(len=None), dict(weights=None), dict(h_len=None), dict(h_w=None), dict(out=None), dict(tok=tok.ctypes.data + 2),
             dict(out=base + 4), dict(U=0), dict(U=-1), dict(U=65536), dict(N=0), dict(N=65), dict(L=-1), dict(L=257), dict(A=0), dict(A=9), dict(ldn=L - 1),
             dict(ldu=(N - 1) * L + L - 1), dict(h_w=neg_w.ctypes.data), dict(h_w=big_w.ctypes.data), dict(h_len=long_len.ctypes.data),
             dict(h_len=none_present.ctypes.data)]
    for fn in NAMES[1:]:
        for kw in cases:
            assert call(fn, **kw) == -1 and fn in _lib.last_error(), (fn, kw)      # ASR_EINVAL
        assert call(fn, out_bytes=need - 1) == -3 and "asr_nbest_out_bytes" in _lib.last_error()
    assert (out == -7).all()
    assert masked_w[0, 1] == 2 ** 30 and ln[0, 1] == -1      # accepted by the checks: covered on the GPU, where the launch can follow


def test_evaluate_cli_flags():
    import evaluate as E
    assert "consensus" in E.CLI_KEYS and "posterior_scale" in E.CLI_KEYS
    search, num = E.eval_options({"search": "ctc_prefix_beam", "nbest": 10, "beam_size": 10, "consensus": 1, "posterior_scale": 0.5})
    assert search == "ctc_prefix_beam" and num["consensus"] == 1 and num["posterior_scale"] == 0.5
    assert E.eval_options({})[1]["consensus"] == 0 and E.eval_options({})[1]["posterior_scale"] == 1.0
    for bad in ({"consensus": 1}, {"search": "ctc_prefix_beam", "consensus": 1, "posterior_scale": 0}, {"posterior_scale": "x"},
                {"search": "attention_beam", "consensus": 1, "nbest": 65, "beam_size": 65}):
        with pytest.raises(SystemExit):
            E.eval_options(bad)


def _scorer():
    from asr_chinese_e2e_amd.scoring import Scorer
    return Scorer(["$", "%", "^", "&", "a", "b", "c", "d"])


def test_scorer_summary_with_consensus_keys():
    A_, B_, C_, D_ = 4, 5, 6, 7
    refs = [[A_, B_, C_], [A_, A_], [B_, D_, C_, A_]]
    nbest = [[[A_, C_, C_], [A_, B_, C_], [A_, B_, C_, D_]], [[A_, A_], [A_]], [[D_, C_, C_], [B_, D_, C_]]]
    weights = [[300, 400, 300], [900, 100], [500, 500]]
    s = _scorer()
    res = [[R.align(r, x) for x in h] for r, h in zip(refs, nbest)]
    cons = [C.consensus(h, w) for h, w in zip(nbest, weights)]
    assert [c["pivot"] for c in cons] == [1, 0, 0] and [c["consensus"] for c in cons] == [[A_, B_, C_], [A_, A_], [D_, C_, C_]]
    extra = [{"mbr_rank": c["pivot"], "mbr": R.align(r, c["mbr"]), "consensus": R.align(r, c["consensus"])} for c, r in zip(cons, refs)]
    s.add_aligned(list("xyz"), res, nbest, refs, consensus=extra)
    got = s.summary()
    assert got["cer"] == 3 / 9 and got["oracle_cer"] == 1 / 9 and got["mbr_cer"] == 2 / 9 and got["consensus_cer"] == 2 / 9 and got["mbr_rank_hist"] == [2, 1, 0]
    plain = _scorer()
    plain.add_aligned(list("xyz"), res, nbest, refs)
    assert {k: got[k] for k in plain.summary()} == plain.summary() and set(got) - set(plain.summary()) == {"mbr_cer", "consensus_cer", "mbr_rank_hist"}
    with pytest.raises(ValueError, match="mbr_rank"):
        _scorer().add_aligned(["x"], res[:1], nbest[:1], refs[:1], consensus=[dict(extra[0], mbr_rank=3)])
    with pytest.raises(ValueError, match="one entry for every"):
        _scorer().add_aligned(list("xy"), res[:2], nbest[:2], refs[:2], consensus=extra[:1])
    mixed = _scorer()
    mixed.add_aligned(["x"], res[:1], nbest[:1], refs[:1], consensus=extra[:1])
    mixed.add_aligned(["y"], res[1:2], nbest[1:2], refs[1:2])
    with pytest.raises(ValueError, match="n-best scores for every"):
        mixed.summary()
