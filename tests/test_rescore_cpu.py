"""Rescoring of n-best lists without a GPU: the definition (tests/rescore_ref.py) against a literal per-entry loop and a hand case, its LM
part against tests/lm_ref.py, the generator the GPU tests reuse and the properties it must show, Grid and the axis parser, SweepResult,
features' column choice, every refusal that needs no launch, and the binding."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from tests import lm_ref
from tests import rescore_ref as D
from tests import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("asr_lm_score_nbest", "asr_nbest_sweep_workspace_bytes", "asr_nbest_sweep")
QUARTERS = [-0.5, -0.25, 0.0, 0.25, 0.5]


# ------------------------------------------------------------------------------------------------ the generator the GPU tests reuse
def generate(U, N, K, seed=0, absent=False, neg_inf=False):
    """U references of 0 to 8 tokens (ids 4 .. 9), N random edits of each, K features per entry on a grid of eighths in [-5, 0] with the
    token count as the last column (K >= 2).  absent: some entries are None, at the front, in the middle and at the back (never all of a
    list); neg_inf: some features are -inf.  Returns (refs, lists, f (U, N, K) float64, err (U, N, 3) int32 from score_ref.align)."""
    rng = np.random.default_rng(seed)
    refs, lists = [], []
    f = rng.integers(-40, 1, (U, N, K)).astype(np.float64) / 8.0
    err = np.zeros((U, N, 3), dtype=np.int32)
    for u in range(U):
        ref = rng.integers(4, 10, int(rng.integers(0, 9))).tolist()
        ent = []
        for e in range(N):
            h = list(ref)
            for _ in range(int(rng.integers(0, 4))):
                kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(h) + 1))
                if kind == 0 and at < len(h):
                    del h[at]
                elif kind == 1 and at < len(h):
                    h[at] = int(rng.integers(4, 10))
                else:
                    h.insert(at, int(rng.integers(4, 10)))
            ent.append(h)
        if absent and N > 1:
            kind = int(rng.integers(0, 4))      # 0: none, 1: the front, 2: the middle, 3: the back
            gone = {0: [], 1: [0], 2: [N // 2], 3: [N - 1]}[kind]
            for e in gone:
                ent[e] = None
        for e, h in enumerate(ent):
            if h is None:
                continue
            if K >= 2:
                f[u, e, K - 1] = float(len(h))
            a = R.align(ref, h)
            err[u, e] = (a["sub"], a["del"], a["ins"])
        refs.append(ref)
        lists.append(ent)
    if neg_inf:
        f[rng.random((U, N, K)) < 0.06] = -math.inf
    return refs, lists, f, err


def quarter_grid(K):
    """Weights in quarters: column 0 has weight 1, up to three more columns run over -0.5 .. 0.5 (125 points for K >= 4), the rest 0.25."""
    from itertools import product
    axes = [[1.0]] + [QUARTERS] * min(K - 1, 3) + [[0.25]] * max(K - 4, 0)
    return np.asarray(list(product(*axes)), dtype=np.float64)


def random_grid(G, K, seed):
    """G weight vectors in quarters in [-1, 1], zeros and negative values among them."""
    return np.random.default_rng(seed).integers(-4, 5, (G, K)).astype(np.float64) / 4.0


def present_of(lists):
    return [[h is not None for h in l] for l in lists]


def random_lm_table(order, V, seed, with_eos=True, with_bos=True):
    """A random back-off table of `order` over V tokens with holes: tokens V - 1 and 1 have no unigram, a third of the contexts no back-off
    column, higher orders are listed whether or not their prefixes are."""
    import random
    rng = random.Random(seed)
    table = {}
    for a in range(2, V - 1):
        if (a == lm_ref.EOS and not with_eos) or (a == lm_ref.BOS and not with_bos):
            continue
        table[(a,)] = (-0.5 - 2.0 * rng.random(), None if rng.random() < 0.3 else -1.5 * rng.random())
    for n in range(2, order + 1):
        for _ in range(6 * V):
            g = tuple(2 + int(rng.random() * (V - 2)) for _ in range(n - 1)) + (3 + int(rng.random() * (V - 3)),)
            if lm_ref.EOS in g[:-1] or (g[-1] == lm_ref.EOS and not with_eos) or lm_ref.BOS in g[1:] or (g[0] == lm_ref.BOS and not with_bos):
                continue
            table[g] = (-0.05 - 1.5 * rng.random(), None if n == order or rng.random() < 0.35 else -1.2 * rng.random())
    return table


# ------------------------------------------------------------------------------------------------ the definition
def _literal(feats, present, w):
    """The pick and the order of one utterance, written entry by entry with numpy scalars."""
    w = np.asarray(w, dtype=np.float64)
    rows = []
    for e, (f, on) in enumerate(zip(feats, present)):
        if not on:
            continue
        f = np.asarray(f, dtype=np.float64)
        used = w != 0.0
        if not np.isfinite(f[used]).all():
            rows.append((e, None))
            continue
        t = np.float64(0.0)
        for k in range(w.shape[0]):
            if used[k]:
                t = np.float64(t + np.float64(w[k] * f[k]))
        rows.append((e, float(t)))
    good = [(e, t) for e, t in rows if t is not None]
    if good:
        top = max(t for _, t in good)
        pick = min(e for e, t in good if t == top)
    else:
        pick = rows[0][0]
    order = [e for e, _ in sorted(good, key=lambda r: (-r[1], r[0]))] + [e for e, t in rows if t is None]
    return pick, order


def test_definition_against_a_literal_loop():
    refs, lists, f, err = generate(40, 5, 4, seed=3, absent=True, neg_inf=True)
    pres = present_of(lists)
    grid = np.concatenate((quarter_grid(4)[::7], random_grid(10, 4, 1)))
    got = D.sweep(f, pres, err, grid, [len(r) for r in refs])
    tot = np.zeros((grid.shape[0], 4), dtype=np.int64)
    unscorable = 0
    for g, w in enumerate(grid):
        for u in range(40):
            p, o = _literal(f[u], pres[u], w)
            assert got["pick"][g, u] == p == D.pick(f[u], pres[u], w) and D.order(f[u], pres[u], w) == o
            unscorable += any(t is None and on for t, on in zip(D.totals(f[u], pres[u], w), pres[u]))
            s, d, i = err[u, p]
            tot[g] += (s, d, i, s + d + i > 0)
    assert np.array_equal(got["tot"], tot) and unscorable > 0
    errs = tot[:, :3].sum(axis=1)
    assert got["cer"].tolist() == [e / sum(len(r) for r in refs) for e in errs.tolist()]
    b = got["best"]
    assert all((errs[b], tot[b, 3], b) <= (errs[g], tot[g, 3], g) for g in range(grid.shape[0]))


def test_hand_case_tie_unscorable_and_skipped_zero_weight():
    inf = math.inf
    feats = [[1.0, -inf, 2.0],      # unscorable under a non-zero middle weight, scorable when that weight is 0
             [0.5, -1.0, 1.0],
             [1.5, -1.0, 0.0],      # ties entry 1 under (1, 1, 1): 0.5 = 0.5
             [9.0, 0.0, 9.0]]       # absent
    present = [True, True, True, False]
    assert D.totals(feats, present, [1.0, 1.0, 1.0]) == [None, 0.5, 0.5, None]
    assert D.pick(feats, present, [1.0, 1.0, 1.0]) == 1 and D.order(feats, present, [1.0, 1.0, 1.0]) == [1, 2, 0]
    assert D.totals(feats, present, [1.0, 0.0, 1.0]) == [3.0, 1.5, 1.5, None]      # 0 * -inf never happens
    assert D.pick(feats, present, [1.0, 0.0, 1.0]) == 0 and D.order(feats, present, [1.0, 0.0, 1.0]) == [0, 1, 2]
    assert D.pick(feats, present, [-1.0, 0.0, 0.0]) == 1      # negative weights: the smallest feature wins
    only = [[-inf, 0.0], [-inf, 1.0]]
    assert D.pick(only, [False, True], [1.0, 1.0]) == 1 and D.order(only, [True, True], [1.0, 1.0]) == [0, 1]      # nothing scorable: the first present
    with pytest.raises(ValueError, match="no present"):
        D.pick(only, [False, False], [1.0, 1.0])
    for bad in (math.nan, inf):
        with pytest.raises(ValueError, match="NaN or"):
            D.pick([[bad, 0.0]], [True], [1.0, 1.0])
    with pytest.raises(ValueError, match="finite"):
        D.pick(only, [True, True], [1.0, inf])
    # the rounding order: the product first, then the sum (0.1 * 3 = 0.30000000000000004 on its own)
    assert D.total([3.0, 1.0], [0.1, 0.3]) == (True, (0.1 * 3.0) + 0.3)


def test_generator_shows_what_the_gpu_tests_rely_on():
    refs, lists, f, err = generate(65, 5, 4, seed=0)
    pres = present_of(lists)
    grid = quarter_grid(4)
    assert grid.shape == (125, 4)
    got = D.sweep(f, pres, err, grid, [len(r) for r in refs])
    ties = 0
    for g in range(0, 125):
        for u in range(65):
            t = D.totals(f[u], pres[u], grid[g])
            ties += sum(1 for x in t if x == t[got["pick"][g, u]]) > 1
    off0 = int((got["pick"] != 0).sum())
    distinct = len({int(x) for x in got["tot"][:, :3].sum(axis=1)})
    print(f"top ties {ties}, picks off index 0 {off0}, distinct error totals {distinct}")
    assert ties > 0 and off0 > 0 and distinct >= 3
    assert min(len(r) for r in refs) == 0 and max(len(r) for r in refs) == 8


@pytest.mark.parametrize("with_bos", [True, False])
def test_lm_scores_against_the_fp64_restatement(with_bos):
    from asr_chinese_e2e_amd.lm import NgramLM
    table = lm_ref.table(with_bos)
    lm = NgramLM(table, lm_ref.ORDER, lm_ref.V, weight=1.0, ins=0.0)
    ref = lm_ref.Model(table, lm_ref.ORDER, 1.0, 0.0)
    rng = np.random.default_rng(5)
    lists = [[rng.integers(4, lm_ref.V, int(rng.integers(0, 12))).tolist() if rng.random() > 0.15 else None for _ in range(4)] for _ in range(30)]
    got = D.lm_scores(lm, lists)
    for l, row in zip(lists, got):
        for h, (score, bias, state, n) in zip(l, row):
            if h is None:
                assert (score, bias, state, n) == (0.0, 0.0, -1, 0)
            else:
                assert score == ref.lm_score(h) and bias == ref.bias(h) and (state, bias) == lm.walk(h) and n == len(h)


@pytest.mark.parametrize("order,with_eos", [(1, True), (3, False), (5, True)])
def test_random_tables_of_other_orders_agree_with_the_restatement(order, with_eos):
    from asr_chinese_e2e_amd.lm import NgramLM
    V = 14
    table = random_lm_table(order, V, seed=order, with_eos=with_eos)
    lm = NgramLM(table, order, V, weight=0.7, ins=0.2)
    ref = lm_ref.Model(table, order, 0.7, 0.2)
    assert lm.has_eos == with_eos
    rng = np.random.default_rng(order)
    for _ in range(60):
        h = rng.integers(4, V, int(rng.integers(0, 15))).tolist()
        assert lm.score(h) == ref.lm_score(h)


# ------------------------------------------------------------------------------------------------ Grid, the parser, SweepResult
def test_grid_and_axis_parser():
    from asr_chinese_e2e_amd.rescore import Grid, parse_axis, parse_grid
    g = Grid(ctc_score=[1.0], att_score=[0.5, 1, 2], lm=np.arange(0, 1.01, 0.5))
    assert g.names == ["ctc_score", "att_score", "lm"] and g.points.shape == (9, 3) and len(g) == 9
    assert g.points[:4].tolist() == [[1.0, 0.5, 0.0], [1.0, 0.5, 0.5], [1.0, 0.5, 1.0], [1.0, 1.0, 0.0]]      # row-major, the last axis fastest
    assert parse_axis("0:1:0.1") == [0.0 + i * 0.1 for i in range(11)] and parse_axis("-1:2:0.5") == [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]
    assert parse_axis("0:1:0.3") == [0.0, 0.3, 0.6, 0.3 * 3] and parse_axis("2") == [2.0] and parse_axis("1,0.5,-3") == [1.0, 0.5, -3.0]
    assert parse_axis("0.3:0.3:1") == [0.3]
    p = parse_grid("att_score=1;ctc_score=0:1:0.25;lm=0:1:0.1;len=-1:2:0.5")
    assert p.names == ["att_score", "ctc_score", "lm", "len"] and len(p) == 1 * 5 * 11 * 7
    assert p.points[-1].tolist() == [1.0, 1.0, 0.1 * 10, 2.0]
    e = Grid.explicit(["a", "b"], [[1, 2], [3, 4]])
    assert e.names == ["a", "b"] and e.points.tolist() == [[1.0, 2.0], [3.0, 4.0]]
    for bad in ("1:0:0.1", "0:1:0", "0:1", "0:1:-1", "", "0:1e9:1e-3", "0:inf:1"):
        with pytest.raises(ValueError):
            parse_axis(bad)
    for bad in ("lm", "lm=1;lm=2"):
        with pytest.raises(ValueError):
            parse_grid(bad)
    with pytest.raises(ValueError, match="65536"):
        Grid(a=np.arange(257), b=np.arange(256))      # G = 65792
    assert len(Grid(a=np.arange(256), b=np.arange(256))) == 65536
    with pytest.raises(ValueError, match="axes"):
        Grid(**{f"c{i}": [1.0] for i in range(9)})
    with pytest.raises(ValueError, match="finite"):
        Grid(a=[1.0, math.nan])
    with pytest.raises(ValueError, match="finite"):
        Grid.explicit(["a"], [[math.inf]])


def _result(seed, pick=True):
    from asr_chinese_e2e_amd.rescore import SweepResult
    rng = np.random.default_rng(seed)
    G, U = 6, 4
    c = rng.integers(0, 9, (4, G))
    return SweepResult(["a", "len"], np.arange(12).reshape(6, 2) / 4.0, c[0], c[1], c[2], np.minimum(c[3], U), 37 + seed, U, 11, 3,
                       rng.integers(0, 3, (G, U)).astype(np.int32) if pick else None)


def test_sweep_result_add_and_save(tmp_path):
    from asr_chinese_e2e_amd.rescore import SweepResult, load_weights
    a, b = _result(1), _result(2)
    s = a.add(b)
    assert s.sub.tolist() == (a.sub + b.sub).tolist() and s.dele.tolist() == (a.dele + b.dele).tolist() and getattr(s, "del") is s.dele
    assert s.ins.tolist() == (a.ins + b.ins).tolist() and s.wrong.tolist() == (a.wrong + b.wrong).tolist()
    assert (s.ref_tokens, s.utterances, s.rank0, s.oracle) == (38 + 39, 8, 22, 6) and s.pick.shape == (6, 8)
    errs = (s.sub + s.dele + s.ins).tolist()
    assert s.cer.tolist() == [e / 77 for e in errs] and list(s.ser) == [w / 8 for w in s.wrong.tolist()]
    assert s.best == min(range(6), key=lambda g: (errs[g], int(s.wrong[g]), g)) and s.best_weights == {"a": s.grid[s.best, 0], "len": s.grid[s.best, 1]}
    assert s.rank0_cer == 22 / 77 and s.oracle_cer == 6 / 77 and a.add(_result(3, pick=False)).pick is None
    path = tmp_path / "weights.json"
    s.save(str(path))
    d = json.loads(path.read_text())
    assert d["best"] == s.best and d["best_weights"] == s.best_weights and d["sub"] == s.sub.tolist() and d["del"] == s.dele.tolist()
    assert d["names"] == ["a", "len"] and d["cer"] == s.cer.tolist() and d["ref_tokens"] == 77
    assert load_weights(str(path)) == s.best_weights and SweepResult.load(str(path)).to_dict() == s.to_dict()
    (tmp_path / "plain.json").write_text('{"att_score": 1, "lm": 0.3}')
    assert load_weights(str(tmp_path / "plain.json")) == {"att_score": 1.0, "lm": 0.3}
    other = SweepResult(["a", "len"], a.grid + 1.0, a.sub, a.dele, a.ins, a.wrong, 1, 1, 0, 0)
    with pytest.raises(ValueError, match="different grids"):
        a.add(other)
    # ties of the best point: the fewest errors, then the fewest wrong utterances, then the lowest index
    t = SweepResult(["a"], [[0.0], [1.0], [2.0], [3.0]], [2, 1, 1, 1], [0, 1, 0, 1], [0, 0, 1, 0], [2, 2, 1, 1], 10, 3, 2, 0)
    assert t.best == 2


# ------------------------------------------------------------------------------------------------ features and the refusals without a launch
def _found(keys, n=(2, 3)):
    out = []
    for u, k in enumerate(n):
        out.append([dict({"yseq": [2, 5 + e, 6, 3][: 4 - (e % 2)], "score": -1.0 * e - u}, **{c: -0.5 * e - u - i for i, c in enumerate(keys)}) for e in range(k)])
    return out


def test_features_column_choice():
    from asr_chinese_e2e_amd.rescore import features
    names, f, lists = features(_found(["ctc_score", "att_score"]))
    assert names == ["ctc_score", "att_score"] and f.shape == (2, 3, 2) and f.dtype == np.float64
    assert lists == [[[5, 6], [6, 6], None], [[5, 6], [6, 6], [7, 6]]]      # sos and a trailing eos stripped, the short list padded
    assert f[0, 1].tolist() == [-0.5, -1.5] and f[0, 2].tolist() == [0.0, 0.0]
    assert features(_found(["ctc_score", "bias"]))[0] == ["ctc_score", "bias"]
    assert features(_found(["bias"]))[0] == ["score"] and features(_found([]))[0] == ["score"]
    mixed = _found(["ctc_score", "att_score"])
    del mixed[1][2]["att_score"]
    assert features(mixed)[0] == ["ctc_score"]      # only what all entries carry
    names, f, _ = features(_found(["lm_score"]), columns=["lm_score", "len", "score"])
    assert names == ["lm_score", "len", "score"] and f[1, :, 1].tolist() == [2.0, 2.0, 2.0] and f[1, 2, 2] == -3.0
    with pytest.raises(ValueError, match="carries no 'att_score'"):
        features(_found(["ctc_score"]), columns=["att_score"])
    with pytest.raises(ValueError, match="twice"):
        features(_found([]), columns=["score", "score"])


def test_refusals_that_need_no_launch():
    from asr_chinese_e2e_amd.lm import NgramLM
    from asr_chinese_e2e_amd.rescore import Grid, _device_sweep, features, rescore, sweep
    from asr_chinese_e2e_amd.scoring import evaluate
    fused = NgramLM(lm_ref.table(), lm_ref.ORDER, lm_ref.V, weight=0.3, ins=0.0)
    bonus = NgramLM(lm_ref.table(), lm_ref.ORDER, lm_ref.V, weight=1.0, ins=0.5)
    for lm in (fused, bonus):
        with pytest.raises(ValueError, match=r"NgramLM\.from_arpa\(\.\.\., weight=1\.0, ins=0\.0\)"):
            features(_found([]), lm=lm)
    with pytest.raises(ValueError, match=r"NgramLM\.from_arpa\(\.\.\., weight=1\.0, ins=0\.0\)"):
        rescore(_found([]), {"score": 1.0, "lm": 0.5})
    for bad in (math.nan, math.inf):
        found = _found(["ctc_score"])
        found[1][1]["ctc_score"] = bad
        with pytest.raises(ValueError, match="NaN or \\+inf"):
            features(found)
    found = _found(["ctc_score"])
    found[0][0]["ctc_score"] = -math.inf      # taken
    assert features(found)[1][0, 0, 0] == -math.inf
    with pytest.raises(ValueError, match="no entry"):
        features([_found([])[0], []])
    with pytest.raises(ValueError, match="between 1 and 64"):
        features([[{"yseq": [5], "score": 0.0}] * 65])
    with pytest.raises(ValueError, match="between 1 and 8"):
        features(_found([f"c{i}" for i in range(9)]), columns=[f"c{i}" for i in range(9)])
    with pytest.raises(ValueError, match="65536"):
        Grid(score=np.arange(65537))
    f = np.zeros((2, 3, 2))
    lists = [[[5], None, [6]], [None, None, None]]
    with pytest.raises(ValueError, match="utterance 1 has no present entry"):
        _device_sweep(f, lists, np.zeros((2, 3, 3), np.int32), [[1.0, 1.0]])
    with pytest.raises(ValueError, match="columns"):
        sweep((["a", "b"], f, lists), [[5], [6]], Grid(a=[1.0], c=[1.0]))
    with pytest.raises(ValueError, match="weights name"):
        from asr_chinese_e2e_amd.rescore import _weight_vector
        _weight_vector(["a"], {"b": 1.0})

    class Never:
        vocab = ["a"]

        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name})")
    with pytest.raises(ValueError, match="n-best search"):
        evaluate(Never(), [], search="transcribe", rescore={"score": 1.0})
    from asr_chinese_e2e_amd.rescore import model_rescore, model_tune
    with pytest.raises(ValueError, match="search must be"):
        model_rescore(Never(), None, {"score": 1.0}, search="transcribe")
    with pytest.raises(ValueError, match="nbest"):
        model_tune(Never(), [None], Grid(score=[1.0]), nbest=65)


def test_abi_header_binding_and_makefile():
    from asr_chinese_e2e_amd import _lib, kernels, rescore
    raw = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    consts = {k: int(v) for k, v in re.findall(r"#define (ASR_RESCORE_\w+) (\d+)", raw)}
    assert consts == {"ASR_RESCORE_MAX_N": D.MAX_N, "ASR_RESCORE_MAX_K": D.MAX_K, "ASR_RESCORE_MAX_G": D.MAX_G, "ASR_RESCORE_MAX_U": kernels.RESCORE_MAX_U}
    assert (kernels.RESCORE_MAX_N, kernels.RESCORE_MAX_K, kernels.RESCORE_MAX_G) == (rescore.MAX_N, rescore.MAX_K, rescore.MAX_G) == (D.MAX_N, D.MAX_K, D.MAX_G)
    assert _lib.ABI_VERSION == 10 == _lib.lib.asr_abi_version()
    make = open(os.path.join(ROOT, "asr_chinese_e2e_amd", "csrc", "Makefile")).read()
    assert "rescore.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1)


def host_lm_struct(lm):
    """An asr_ngram_lm whose tables are the LM's host arrays: enough for the launchers' checks, which read no table."""
    from asr_chinese_e2e_amd.lm import _TABLES, LmTables
    m = lm._meta
    return LmTables(*[lm._arrays[n].ctypes.data for n in _TABLES], lm.S, lm.A, m["V"], m["order"], m["start"], m["ins"])


def test_launcher_refusals_on_the_host():
    """The launchers read only their host mirrors and the LM struct before they refuse: host addresses stand in for the device pointers,
    nothing is launched."""
    from asr_chinese_e2e_amd import _lib
    from asr_chinese_e2e_amd.lm import NgramLM
    lm = NgramLM(lm_ref.table(), lm_ref.ORDER, lm_ref.V, weight=1.0, ins=0.0)
    st = host_lm_struct(lm)
    P, ld = 3, 4
    tok, ln = np.zeros((P, ld), np.int32), np.array([4, -1, 0], np.int32)
    outs = np.full(8 * P, -7.0, np.float64)
    base = outs.ctypes.data

    def lm_call(**kw):
        a = dict(tok=tok.ctypes.data, len=ln.ctypes.data, h_len=ln.ctypes.data, P=P, ld=ld, lm=ctypes.addressof(st), has_eos=1, eos=3, score=base, bias=base + 8 * P,
                 state=base + 16 * P, ntok=base + 20 * P, stream=None)
        a.update(kw)
        return _lib.fast.asr_lm_score_nbest(*a.values())

    def with_len(at, v):
        m = ln.copy()
        m[at] = v
        return m
    long_len, low_len = with_len(0, 5), with_len(1, -2)
    bad = [host_lm_struct(lm) for _ in range(5)]
    bad[0].order, bad[1].start, bad[2].ins, bad[3].arc_term, bad[4].uni_term = 6, lm.S, math.nan, None, bad[4].uni_term + 4
    cases = [dict(tok=None), dict(len=None), dict(h_len=None), dict(lm=None), dict(score=None), dict(bias=None), dict(state=None), dict(ntok=None),
             dict(tok=tok.ctypes.data + 2), dict(score=base + 4), dict(state=base + 16 * P + 1), dict(P=0), dict(P=-1), dict(ld=-1),
             dict(h_len=long_len.ctypes.data), dict(h_len=low_len.ctypes.data), dict(ld=3)] + [dict(lm=ctypes.addressof(b)) for b in bad]
    for kw in cases:
        assert lm_call(**kw) == -1 and "asr_lm_score_nbest" in _lib.last_error(), kw      # ASR_EINVAL
    assert (outs == -7.0).all()

    U, N, K, G = 3, 2, 2, 2
    feat, grid = np.zeros((K, N, U), np.float64), np.array([[1.0, 0.0], [0.5, -1.0]], np.float64)
    feat[1, 0, 2] = -math.inf      # taken
    pres, err = np.array([[0, -1, 0], [-1, 0, 0]], np.int32), np.zeros((3, N, U), np.int32)
    need = int(_lib.fast.asr_nbest_sweep_workspace_bytes(U, N, K, G))
    assert need == G * 1 * 4 * 8 and int(_lib.fast.asr_nbest_sweep_workspace_bytes(65, 1, 1, 3)) == 3 * 2 * 32
    for shape in ((0, N, K, G), (U, 0, K, G), (U, 65, K, G), (U, N, 0, G), (U, N, 9, G), (U, N, K, 0), (U, N, K, 65537), (2 ** 20 + 1, N, K, G)):
        assert int(_lib.fast.asr_nbest_sweep_workspace_bytes(*shape)) == 0 and "asr_nbest_sweep_workspace_bytes" in _lib.last_error(), shape
    out = np.full(G * U + 2 * G * 4 + 2 * G * U * N + need // 4 + 2, -7, np.int32)
    ob = out.ctypes.data + (out.ctypes.data % 8)
    o_tot, o_total, o_ws, o_pick = ob, ob + G * 32, ob + G * 32 + G * U * N * 8, ob + G * 32 + G * U * N * 8 + need

    def sw_call(**kw):
        a = dict(feat=feat.ctypes.data, len=pres.ctypes.data, err=err.ctypes.data, grid=grid.ctypes.data, h_feat=feat.ctypes.data, h_len=pres.ctypes.data,
                 h_grid=grid.ctypes.data, U=U, N=N, K=K, G=G, pick=o_pick, tot=o_tot, total=o_total, ws=o_ws, ws_bytes=need, stream=None)
        a.update(kw)
        return _lib.fast.asr_nbest_sweep(*a.values())

    def feat_with(v):
        m = feat.copy()
        m[0, 1, 1] = v
        return m
    nan_f, inf_f = feat_with(math.nan), feat_with(math.inf)
    nan_g, inf_g = grid.copy(), grid.copy()
    nan_g[1, 0], inf_g[0, 1] = math.nan, -math.inf
    none = pres.copy()
    none[:, 1] = -1
    cases = [dict(feat=None), dict(len=None), dict(err=None), dict(grid=None), dict(h_feat=None), dict(h_len=None), dict(h_grid=None), dict(pick=None),
             dict(tot=None), dict(ws=None), dict(feat=feat.ctypes.data + 4), dict(len=pres.ctypes.data + 2), dict(tot=o_tot + 4), dict(total=o_total + 4),
             dict(ws=o_ws + 4), dict(U=0), dict(N=0), dict(N=65), dict(K=0), dict(K=9), dict(G=0), dict(G=65537), dict(h_feat=nan_f.ctypes.data),
             dict(h_feat=inf_f.ctypes.data), dict(h_grid=nan_g.ctypes.data), dict(h_grid=inf_g.ctypes.data), dict(h_len=none.ctypes.data)]
    for kw in cases:
        assert sw_call(**kw) == -1 and "asr_nbest_sweep" in _lib.last_error(), kw      # ASR_EINVAL
    assert sw_call(ws_bytes=need - 1) == -3 and "asr_nbest_sweep_workspace_bytes" in _lib.last_error()      # ASR_EWORKSPACE
    assert (out == -7).all()


def test_cli_flags():
    import evaluate as E
    import tune as T
    assert "rescore" in E.CLI_KEYS
    with pytest.raises(SystemExit, match="--rescore needs"):
        E.eval_options({"rescore": "weights.json"})
    assert E.eval_options({"rescore": "weights.json", "search": "attention_beam"})[0] == "attention_beam"
    search, num, grid = T.tune_options({"grid": "att_score=1;lm=0:1:0.5;len=-1,0,1", "lm": "lm.arpa"})
    assert search == "attention_beam" and num["beam_size"] == 10 and num["nbest"] == 10
    assert grid.names == ["att_score", "lm", "len"] and grid.points.shape == (9, 3)
    for bad, why in (({"grid": "lm=0:1:0.5"}, "--lm"), ({}, "--grid"), ({"grid": "score=1", "search": "transcribe", "nbest": 1}, "--search"),
                     ({"grid": "score=1:0:1"}, "--grid"), ({"grid": "score=1", "nbest": 65, "beam_size": 65}, "--nbest")):
        with pytest.raises(SystemExit, match=why):
            T.tune_options(bad)
