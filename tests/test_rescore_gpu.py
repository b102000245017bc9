"""Rescoring of n-best lists on the GPU: asr_lm_score_nbest against NgramLM.score / walk and asr_nbest_sweep against the definition
(tests/rescore_ref.py), integers and float bits with no tolerance; the launchers' refusals; rescore.sweep / rescore / lm_scores; and the
model level (model.rescore, model.tune, model.evaluate(rescore=))."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lm_ref  # noqa: E402
from tests import rescore_ref as D  # noqa: E402
from tests import score_ref as R  # noqa: E402
from tests.test_rescore_cpu import generate, present_of, quarter_grid, random_grid, random_lm_table  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from asr_chinese_e2e_amd import kernels
    return kernels


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ------------------------------------------------------------------------------------------------ asr_lm_score_nbest
def _lms():
    from asr_chinese_e2e_amd.lm import NgramLM
    V = 14
    out = {"table": NgramLM(lm_ref.table(True), lm_ref.ORDER, lm_ref.V, weight=1.0, ins=0.0),
           "table_no_bos": NgramLM(lm_ref.table(False), lm_ref.ORDER, lm_ref.V, weight=1.0, ins=0.0),
           "order1": NgramLM(random_lm_table(1, V, 1), 1, V, weight=1.0, ins=0.0),
           "order3_no_eos": NgramLM(random_lm_table(3, V, 3, with_eos=False), 3, V, weight=0.7, ins=0.25),
           "order5": NgramLM(random_lm_table(5, V, 5), 5, V, weight=1.0, ins=0.0)}
    assert not out["order3_no_eos"].has_eos and out["order5"].has_eos and out["table_no_bos"].start == 0 and out["table"].start != 0
    return out


def _hyps(P, V, seed):
    """P hypotheses: the lengths 0, 1, 2, 63, 64, 65 and 300 first (as far as P reaches), then short random ones; ids from -2 to V + 1, so
    tokens without a unigram and ids outside [0, V) are among them; every seventh entry is absent."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2, 63, 64, 65, 300]
    hyps = []
    for p in range(P):
        n = lens[p] if p < len(lens) else int(rng.integers(0, 20))
        hyps.append(None if p % 7 == 5 and p >= len(lens) else rng.integers(-2, V + 2, n).tolist())
    return hyps


@pytest.mark.parametrize("name", ["table", "table_no_bos", "order1", "order3_no_eos", "order5"])
def test_lm_score_nbest_equals_the_host_methods_bit_for_bit(K, name):
    lm = _lms()[name]
    V = lm.vocab_size
    for P, pad in ((1, 0), (63, 0), (64, 3), (65, 0), (1000, 0)):
        hyps = _hyps(P, V, seed=P)
        L = max(len(h) for h in hyps if h is not None) + pad      # ld above the longest length
        tok = np.full((P, max(L, 1)), 7, np.int32)
        ln = np.full(P, -1, np.int32)
        for p, h in enumerate(hyps):
            if h is not None:
                ln[p] = len(h)
                tok[p, :len(h)] = h
        d_tok, d_ln = torch.from_numpy(tok).to(DEV), torch.from_numpy(ln).to(DEV)
        first = torch.empty(6 * P, dtype=torch.int32, device=DEV)
        score, bias, state, ntok = (x.cpu().numpy() for x in K.lm_score_nbest(d_tok, d_ln, ln, lm, out=first))
        again = torch.empty(6 * P, dtype=torch.int32, device=DEV)
        K.lm_score_nbest(d_tok, d_ln, ln, lm, out=again)
        assert torch.equal(first, again)      # two runs, the same bytes
        want = D.lm_scores(lm, [hyps])[0]
        assert _bits(score).tolist() == _bits([w[0] for w in want]).tolist(), (name, P)
        assert _bits(bias).tolist() == _bits([w[1] for w in want]).tolist(), (name, P)
        assert state.tolist() == [w[2] for w in want] and ntok.tolist() == [w[3] for w in want], (name, P)
        if P == 1000:
            assert sum(h is None for h in hyps) > 100 and any(s != b for s, b in zip(score.tolist(), bias.tolist())) == lm.has_eos


def test_lm_score_nbest_equals_the_fused_search_lm_score(K):
    """A fused LM of weight 0.3: what the CTC prefix beam search reports for every entry of a random lattice is this kernel's score of the
    entry's tokens."""
    from asr_chinese_e2e_amd.lm import NgramLM
    from asr_chinese_e2e_amd.rescore import lm_scores_packed
    lm = NgramLM(lm_ref.table(), lm_ref.ORDER, lm_ref.V, weight=0.3, ins=0.2, device=DEV)
    B, T, k, beam = 3, 24, 5, 8
    logits = torch.randn(B, T, lm_ref.V, generator=torch.Generator().manual_seed(3)) * 1.5
    vals, ids, blank_lp = K.ctc_frame_topk(logits.reshape(B * T, lm_ref.V).to(DEV), k, 0)
    in_len = torch.tensor([T, 17, 9], dtype=torch.int32, device=DEV)
    tok, ln, sc, bias, state = K.ctc_prefix_beam(vals, ids, blank_lp, in_len, B, T, beam, beam, 0, lm=lm)
    got = lm_scores_packed(tok, ln, lm)
    assert all(got[n].shape == (B, beam) and got[n].is_cuda for n in ("lm_score", "bias", "state", "tokens"))
    h_ln, h_bias, h_state = ln.cpu().tolist(), bias.cpu().tolist(), state.cpu().tolist()
    h_tok = tok.cpu().tolist()
    g_score, g_bias, g_state, g_n = (got[n].cpu().tolist() for n in ("lm_score", "bias", "state", "tokens"))
    seen = 0
    for b in range(B):
        for r in range(beam):
            if h_ln[b][r] < 0:
                assert (g_score[b][r], g_bias[b][r], g_state[b][r], g_n[b][r]) == (0.0, 0.0, -1, 0)
                continue
            seen += 1
            assert g_score[b][r] == lm.final(h_state[b][r], h_bias[b][r]) == lm.score(h_tok[b][r][:h_ln[b][r]])
            assert (g_bias[b][r], g_state[b][r], g_n[b][r]) == (h_bias[b][r], h_state[b][r], h_ln[b][r])
    assert seen > B


# ------------------------------------------------------------------------------------------------ asr_nbest_sweep
def _run_sweep(K, f, lists, err, grid, totals=True):
    from asr_chinese_e2e_amd.rescore import _device_sweep
    return _device_sweep(f, lists, err, grid, totals=totals, device=DEV)


def _want_totals(f, pres, grid):
    G, (U, N, _) = len(grid), f.shape
    out = np.full((G, U, N), -math.inf)
    for g in range(G):
        for u in range(U):
            for e, t in enumerate(D.totals(f[u], pres[u], grid[g])):
                if t is not None:
                    out[g, u, e] = t
    return out


def _assert_sweep(K, f, lists, err, grid, refs):
    pres = present_of(lists)
    want = D.sweep(f, pres, err, grid, [len(r) for r in refs])
    pick, tot, total = _run_sweep(K, f, lists, err, grid)
    assert pick.dtype == np.int32 and tot.dtype == np.int64 and total.dtype == np.float64
    assert np.array_equal(pick, want["pick"]) and np.array_equal(tot, want["tot"])
    assert np.array_equal(_bits(total), _bits(_want_totals(f, pres, grid)))
    pick2, tot2, none = _run_sweep(K, f, lists, err, grid, totals=False)      # out_total == NULL
    assert none is None and np.array_equal(pick2, pick) and np.array_equal(tot2, tot)
    return want, pick, total


SWEEP_CASES = [(1, 1, 1, 1), (63, 2, 4, 1000), (64, 5, 8, 33), (65, 5, 4, 125), (257, 5, 4, 33), (65, 64, 8, 2), (257, 64, 1, 2), (2, 1, 8, 2)]


@pytest.mark.parametrize("U,N,Kc,G", SWEEP_CASES)
def test_sweep_equals_the_definition(K, U, N, Kc, G):
    refs, lists, f, err = generate(U, N, Kc, seed=U + N, absent=True, neg_inf=True)
    grid = quarter_grid(Kc) if G == 125 else random_grid(G, Kc, seed=G)
    want, pick, total = _assert_sweep(K, f, lists, err, grid, refs)
    if (U, N, Kc, G) == (65, 5, 4, 125):      # what this case is there for
        pres = present_of(lists)
        assert (pick != 0).any() and len({int(x) for x in want["tot"][:, :3].sum(axis=1)}) >= 3
        assert any(lists[u][e] is None for u in range(U) for e in (0, N // 2, N - 1))
        assert (grid < 0).any() and (grid == 0).any() and np.isinf(f).any()
        ties = sum(sum(1 for x in total[g, u] if x == total[g, u, pick[g, u]] and x != -math.inf) > 1 for g in range(G) for u in range(U))
        assert ties > 0
        assert any(t is None and on for g in (0, 124) for u in range(U) for t, on in zip(D.totals(f[u], pres[u], grid[g]), pres[u]))      # unscorable entries


def test_sweep_every_entry_unscorable_and_zero_weights_skip_minus_inf(K):
    refs, lists, f, err = generate(70, 4, 3, seed=9, absent=True)
    f[:, :, 1] = -math.inf                      # a column of -inf
    f[::3, :, 2] = -math.inf                    # and another one for every third utterance
    grid = np.asarray([[1.0, 0.0, 0.0], [1.0, 0.5, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.25], [0.0, 0.0, 0.0]])
    want, pick, total = _assert_sweep(K, f, lists, err, grid, refs)
    pres = present_of(lists)
    first = [p.index(True) for p in pres]
    assert pick[1].tolist() == first and (total[1] == -math.inf).all()              # nothing scorable: the first present entry
    assert np.isfinite(total[0][np.asarray(pres)]).all()                            # the zero weights skip both -inf columns
    assert pick[2, 0::3].tolist() == first[0::3] and pick[4].tolist() == first      # all-zero weights: every total 0.0, the lowest index


def test_sweep_does_not_contract_the_product_into_the_sum(K):
    rng = np.random.default_rng(2)
    U, N = 64, 8
    f = rng.standard_normal((U, N, 3)) * 3.0      # many mantissa bits
    lists = [[[5]] * N for _ in range(U)]
    w = [0.1, 0.3, 0.7]
    unfused = np.zeros((U, N))
    fused = np.zeros((U, N))
    for u in range(U):
        for e in range(N):
            t = 0.0
            z = 0.0
            for k in range(3):
                t = t + (w[k] * float(f[u, e, k]))
                z = float(Fraction(w[k]) * Fraction(float(f[u, e, k])) + Fraction(z))      # one rounding: what an fma gives
            unfused[u, e], fused[u, e] = t, z
    differ = int((_bits(unfused) != _bits(fused)).sum())
    print(f"{differ} of {U * N} totals differ between product-then-sum and fused multiply-add")
    assert differ > 0
    assert _bits(unfused).tolist() == _bits(_want_totals(f, present_of(lists), [w])[0]).tolist()
    pick, tot, total = _run_sweep(K, f, lists, np.zeros((U, N, 3), np.int32), [w])
    assert np.array_equal(_bits(total[0]), _bits(unfused))
    assert pick[0].tolist() == [int(np.argmax(unfused[u])) for u in range(U)]


# ------------------------------------------------------------------------------------------------ refusals, before any launch
def test_refusals_leave_the_outputs_alone(K):
    from asr_chinese_e2e_amd import _lib
    from asr_chinese_e2e_amd.lm import NgramLM
    stream = torch.cuda.current_stream().cuda_stream
    lm = NgramLM(lm_ref.table(), lm_ref.ORDER, lm_ref.V, weight=1.0, ins=0.0, device=DEV)
    good = ctypes.addressof(lm.on(DEV)[1])
    from asr_chinese_e2e_amd.lm import LmTables
    bad = LmTables.from_buffer_copy(lm.on(DEV)[1])
    bad.order = 6
    P, ld = 3, 4
    tok = torch.full((P, ld), 5, dtype=torch.int32, device=DEV)
    ln = np.array([4, -1, 0], np.int32)
    d_ln = torch.from_numpy(ln).to(DEV)
    out = torch.full((6 * P,), -7, dtype=torch.int32, device=DEV)
    o = out.data_ptr()

    def lm_call(**kw):
        a = dict(tok=tok.data_ptr(), len=d_ln.data_ptr(), h_len=ln.ctypes.data, P=P, ld=ld, lm=good, has_eos=1, eos=3, score=o, bias=o + 8 * P, state=o + 16 * P,
                 ntok=o + 20 * P, stream=stream)
        a.update(kw)
        return _lib.fast.asr_lm_score_nbest(*a.values())
    long_len, low_len = ln.copy(), ln.copy()
    long_len[0], low_len[1] = 5, -2
    for kw in (dict(tok=None), dict(len=None), dict(h_len=None), dict(lm=None), dict(score=None), dict(ntok=None), dict(score=o + 4), dict(tok=tok.data_ptr() + 2),
               dict(P=0), dict(P=-3), dict(ld=3), dict(ld=-1), dict(h_len=long_len.ctypes.data), dict(h_len=low_len.ctypes.data), dict(lm=ctypes.addressof(bad))):
        assert lm_call(**kw) == -1 and "asr_lm_score_nbest" in _lib.last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    assert lm_call() == 0
    got = out.cpu().numpy()
    assert got[:2 * P].view(np.float64).tolist() == [lm.score([5, 5, 5, 5]), 0.0, lm.score([])] and got[4 * P:].tolist() == [lm.walk([5] * 4)[0], -1, lm.start, 4, 0, 0]

    U, N, Kc, G = 3, 2, 2, 2
    feat, grid = np.zeros((Kc, N, U), np.float64), np.array([[1.0, 0.0], [0.5, -1.0]], np.float64)
    feat[0, 1] = [1.0, 2.0, 3.0]
    pres, err = np.array([[0, -1, 0], [-1, 0, 0]], np.int32), np.arange(3 * N * U, dtype=np.int32).reshape(3, N, U)
    d_f, d_g = torch.from_numpy(feat).to(DEV), torch.from_numpy(grid).to(DEV)
    d_p, d_e = torch.from_numpy(pres).to(DEV), torch.from_numpy(err).to(DEV)
    need = K.nbest_sweep_workspace_bytes(U, N, Kc, G)
    buf = torch.full((G * 4 + G * U * N + need // 8 + G * U,), -7, dtype=torch.int64, device=DEV)
    b = buf.data_ptr()
    o_tot, o_total, o_ws, o_pick = b, b + G * 32, b + G * 32 + G * U * N * 8, b + G * 32 + G * U * N * 8 + need

    def sw_call(**kw):
        a = dict(feat=d_f.data_ptr(), len=d_p.data_ptr(), err=d_e.data_ptr(), grid=d_g.data_ptr(), h_feat=feat.ctypes.data, h_len=pres.ctypes.data,
                 h_grid=grid.ctypes.data, U=U, N=N, K=Kc, G=G, pick=o_pick, tot=o_tot, total=o_total, ws=o_ws, ws_bytes=need, stream=stream)
        a.update(kw)
        return _lib.fast.asr_nbest_sweep(*a.values())
    nan_f, inf_f, nan_g, none = feat.copy(), feat.copy(), grid.copy(), pres.copy()
    nan_f[1, 0, 0], inf_f[0, 0, 1], nan_g[1, 1] = math.nan, math.inf, math.nan
    none[:, 1] = -1
    for kw in (dict(feat=None), dict(len=None), dict(err=None), dict(grid=None), dict(h_feat=None), dict(h_len=None), dict(h_grid=None), dict(pick=None), dict(tot=None),
               dict(ws=None), dict(feat=d_f.data_ptr() + 4), dict(total=o_total + 4), dict(pick=o_pick + 2), dict(U=0), dict(N=0), dict(N=65), dict(K=0), dict(K=9),
               dict(G=0), dict(G=65537), dict(h_feat=nan_f.ctypes.data), dict(h_feat=inf_f.ctypes.data), dict(h_grid=nan_g.ctypes.data), dict(h_len=none.ctypes.data)):
        assert sw_call(**kw) == -1 and "asr_nbest_sweep" in _lib.last_error(), kw
    assert sw_call(ws_bytes=need - 1) == -3
    torch.cuda.synchronize()
    assert bool((buf == -7).all())
    assert sw_call() == 0 and sw_call(total=None) == 0
    host = buf.cpu().numpy()
    pick = host[(o_pick - b) // 8:].view(np.int32)[:G * U].reshape(G, U)
    lists = [[[5] if pres[e, u] >= 0 else None for e in range(N)] for u in range(U)]
    want = D.sweep(feat.transpose(2, 1, 0), present_of(lists), err.transpose(2, 1, 0), grid, [1] * U)
    assert np.array_equal(pick, want["pick"]) and np.array_equal(host[:G * 4].reshape(G, 4), want["tot"])


# ------------------------------------------------------------------------------------------------ the Python interface
def test_lm_scores_and_rescore_and_sweep(K):
    from asr_chinese_e2e_amd.lm import NgramLM
    from asr_chinese_e2e_amd.rescore import Grid, features, lm_scores, rescore, sweep
    lm = NgramLM(random_lm_table(3, 12, 8), 3, 12, weight=1.0, ins=0.0, device=DEV)
    refs, lists, f, err = generate(40, 5, 3, seed=4, absent=True)
    got = lm_scores(lists, lm)
    want = D.lm_scores(lm, lists)
    assert [[(h["lm_score"], h["bias"], h["state"], h["tokens"]) for h in row] for row in got] == want
    # what a search returns: the present entries, sos / eos spelled, a score and a ctc_score each
    rng = np.random.default_rng(6)
    found = [[{"yseq": [2] + h + [3], "score": -0.125 * e, "ctc_score": float(rng.integers(-40, 1)) / 8.0 if rng.random() > 0.1 else -math.inf}
              for e, h in enumerate(l) if h is not None] for l in lists]
    kept = [[h for h in l if h is not None] for l in lists]
    names, ff, stripped = features(found, lm=lm, columns=["ctc_score", "lm", "len"])
    assert names == ["ctc_score", "lm", "len"] and [[h for h in l if h is not None] for l in stripped] == kept
    for u, l in enumerate(kept):
        for e, h in enumerate(l):
            assert ff[u, e].tolist() == [found[u][e]["ctc_score"], lm.score(h), float(len(h))]
    assert features(found, lm=lm)[0] == ["ctc_score", "lm"]
    grid = Grid(ctc_score=[1.0, 0.0], lm=[0.0, 0.25, 0.5], len=[-0.5, 0.0, 0.5])
    res = sweep(found, refs, grid, lm=lm, picks=True)
    pres = [[h is not None for h in l] for l in stripped]
    errs = np.zeros((40, 5, 3), np.int32)
    for u, l in enumerate(stripped):
        for e, h in enumerate(l):
            if h is not None:
                a = R.align(refs[u], h)
                errs[u, e] = (a["sub"], a["del"], a["ins"])
    want = D.sweep(ff, pres, errs, grid.points, [len(r) for r in refs])
    assert np.array_equal(res.pick, want["pick"]) and res.sub.tolist() == want["tot"][:, 0].tolist() and res.dele.tolist() == want["tot"][:, 1].tolist()
    assert res.ins.tolist() == want["tot"][:, 2].tolist() and res.wrong.tolist() == want["tot"][:, 3].tolist() and res.cer.tolist() == want["cer"].tolist()
    assert res.best == want["best"] and res.ref_tokens == want["ref_tokens"] and res.utterances == 40 and res.names == names
    dist = errs.sum(axis=2)
    assert res.rank0 == sum(int(dist[u, 0]) for u in range(40)) and res.oracle == sum(min(int(dist[u, e]) for e in range(len(kept[u]))) for u in range(40))
    assert res.oracle_cer <= min(res.cer) and len({int(x) for x in res.sub + res.dele + res.ins}) >= 3
    same = sweep((names, ff, stripped), refs, grid)      # features' own result in place of the lists
    assert same.pick is None and same.to_dict() == res.to_dict()
    half = sweep(found[:17], refs[:17], grid, lm=lm).add(sweep(found[17:], refs[17:], grid, lm=lm))
    assert half.to_dict() == res.to_dict()
    # rescore: the order of the definition, copies, the input untouched
    weights = {"ctc_score": 1.0, "lm": 0.25, "len": 0.5}
    before = [[dict(h) for h in l] for l in found]
    new = rescore(found, weights, lm=lm)
    assert found == before and len(new) == 40
    moved = 0
    for u, l in enumerate(new):
        n = len(found[u])
        order = D.order(ff[u, :n], [True] * n, [1.0, 0.25, 0.5])
        tot = D.totals(ff[u, :n], [True] * n, [1.0, 0.25, 0.5])
        assert [h["first_rank"] for h in l] == order
        moved += order != list(range(n))
        for h in l:
            e = h["first_rank"]
            assert h["score"] == (tot[e] if tot[e] is not None else -math.inf) and h["lm"] == lm.score(kept[u][e]) and h["len"] == len(kept[u][e])
            assert {k: v for k, v in h.items() if k not in ("score", "first_rank", "lm", "len")} == {k: v for k, v in found[u][e].items() if k != "score"}
    assert moved > 0 and any(h["score"] == -math.inf for l in new for h in l)
    only = rescore(found, {"ctc_score": 1.0})
    assert all("lm" not in h and "len" not in h for l in only for h in l)


# ------------------------------------------------------------------------------------------------ the model
def _batches(V):
    from asr_chinese_e2e_amd.data_handler import synthetic_pack
    return [synthetic_pack(3, 60, 320, V, seed=41, ragged=True, Lmin=3, Lmax=9, device=DEV),
            synthetic_pack(2, 48, 320, V, seed=42, ragged=True, Lmin=2, Lmax=12, device=DEV)]


def _strip(seq):
    seq = list(seq)
    seq = seq[1:] if seq and seq[0] == 2 else seq
    return seq[:-1] if seq and seq[-1] == 3 else seq


def _model_lm(V):
    from asr_chinese_e2e_amd.lm import NgramLM
    return NgramLM(random_lm_table(3, V, 13), 3, V, weight=1.0, ins=0.0, device=DEV)


def _definition_of(found, names, w, lm):
    """(features, stripped lists) of what a search returned, by the definition's own means."""
    out = []
    for utt in found:
        ids = [_strip(h["yseq"]) for h in utt]
        out.append(([[lm.score(i) if c == "lm" else float(len(i)) if c == "len" else float(h[c]) for c in names] for h, i in zip(utt, ids)], ids))
    return out


@pytest.mark.parametrize("search", ["ctc_prefix_beam", "attention_beam"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_model_rescore_equals_the_definition(dtype, search):
    from tests.test_align_long_gpu import _model
    model = _model(dtype)
    lm = _model_lm(30)
    pack = _batches(30)[0]
    weights = {"score": 1.0, "lm": 0.5, "len": 1.5}
    got = model.rescore(pack, weights, search=search, beam_size=4, nbest=4, lm=lm)
    fn = model.ctc_prefix_beam_search if search == "ctc_prefix_beam" else model.beam_search
    with torch.no_grad():
        found = fn(pack, 4, 4)
    assert len(got) == len(found) == 3 and max(len(u) for u in found) > 1
    for g, utt, (f, ids) in zip(got, found, _definition_of(found, list(weights), None, lm)):
        pres, w = [True] * len(utt), list(weights.values())
        tot = D.totals(f, pres, w)
        assert [h["first_rank"] for h in g] == D.order(f, pres, w) and g[0]["first_rank"] == D.pick(f, pres, w)
        for h in g:
            e = h["first_rank"]
            assert h["yseq"] == utt[e]["yseq"] and h["score"] == tot[e] and h["lm"] == f[e][1] and h["len"] == len(ids[e])
    with pytest.raises(ValueError, match="nbest"):
        model.rescore(pack, weights, nbest=65, lm=lm)
    with pytest.raises(ValueError, match="from_arpa"):
        model.rescore(pack, weights, search=search, beam_size=4, nbest=4)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_model_tune_and_evaluate_with_rescore(dtype):
    from asr_chinese_e2e_amd.rescore import Grid
    from tests.test_align_long_gpu import _model
    model = _model(dtype)
    lm = _model_lm(30)
    batches = _batches(30)
    grid = Grid(score=[1.0, 0.0], lm=[0.0, 0.5, 1.0], len=[-2.0, 0.0, 2.0])
    res = model.tune(batches, grid, search="ctc_prefix_beam", beam_size=4, nbest=4, lm=lm)
    tot = np.zeros((len(grid), 4), np.int64)
    tokens = rank0 = 0
    for pack in batches:
        tgt, n = pack.tgt_for_input.cpu(), pack.tgt_len.cpu().tolist()
        with torch.no_grad():
            found = model.ctc_prefix_beam_search(pack, 4, 4)
        feats, pres, errs, lens = [], [], [], []
        for b, (utt, (f, ids)) in enumerate(zip(found, _definition_of(found, grid.names, None, lm))):
            gold = tgt[b, :n[b]].tolist()
            al = [R.align(gold, i) for i in ids]
            feats.append(f)
            pres.append([True] * len(utt))
            errs.append([(a["sub"], a["del"], a["ins"]) for a in al])
            lens.append(len(gold))
            rank0 += al[0]["distance"]
        want = D.sweep(feats, pres, errs, grid.points, lens)
        tot += want["tot"]
        tokens += want["ref_tokens"]
    assert np.array_equal(np.stack([res.sub, res.dele, res.ins, res.wrong], axis=1), tot)
    assert (res.ref_tokens, res.utterances, res.rank0) == (tokens, 5, rank0) and res.cer.tolist() == [int(e) / tokens for e in tot[:, :3].sum(axis=1)]
    best = min(range(len(grid)), key=lambda g: (int(tot[g, :3].sum()), int(tot[g, 3]), g))
    assert res.best == best and res.best_weights == dict(zip(grid.names, grid.points[best].tolist()))
    # evaluate with the tuned weights reports the tuned counts; without rescore= it reports the lists as the search ranked them
    tuned = model.evaluate(batches, search="ctc_prefix_beam", nbest=4, beam_size=4, rescore=res.best_weights, rescore_lm=lm).summary()
    assert (tuned["sub"], tuned["del"], tuned["ins"]) == (int(res.sub[best]), int(res.dele[best]), int(res.ins[best])) and tuned["cer"] == res.cer[best]
    plain = model.evaluate(batches, search="ctc_prefix_beam", nbest=4, beam_size=4).summary()
    assert plain["sub"] + plain["del"] + plain["ins"] == rank0 == res.rank0 and plain["oracle_cer"] == res.oracle_cer == tuned["oracle_cer"]
    same = model.evaluate(batches, search="ctc_prefix_beam", nbest=4, beam_size=4, rescore={"score": 1.0}).summary()
    assert same == plain      # the search's own score as the only column keeps the search's order
    cons = model.evaluate(batches, search="ctc_prefix_beam", nbest=4, beam_size=4, rescore=res.best_weights, rescore_lm=lm, consensus=True).summary()
    assert {k: cons[k] for k in tuned} == tuned and "mbr_cer" in cons
    with pytest.raises(ValueError, match="n-best search"):
        model.evaluate(batches, rescore=res.best_weights, rescore_lm=lm)
