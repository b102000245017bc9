"""Token-level scoring without a GPU: the definition (tests/score_ref.py) against a brute-force enumeration of every monotone alignment
and against Utils.score.edit_distance, its pinned tie cases, and the host half of scoring.Scorer (add_aligned, summary, per_token,
confusions, write_jsonl) against values written out here.  Integers throughout."""
import itertools
import json
import os
import re

import numpy as np
import pytest

from tests import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("distance", "cor", "sub", "del", "ins")


def _all_alignments(r, h):
    """(cost, cor, sub, del, ins) of every monotone alignment of r and h: every order of diagonal, down and right steps."""
    out = set()

    def go(i, j, c, s, d, n):
        if i == len(r) and j == len(h):
            out.add((s + d + n, c, s, d, n))
            return
        if i < len(r) and j < len(h):
            eq = r[i] == h[j]
            go(i + 1, j + 1, c + eq, s + (not eq), d, n)
        if i < len(r):
            go(i + 1, j, c, s, d + 1, n)
        if j < len(h):
            go(i, j + 1, c, s, d, n + 1)
    go(0, 0, 0, 0, 0, 0)
    return out


def test_definition_against_brute_force():
    for m in range(5):
        for n in range(5):
            for r in itertools.product((0, 1), repeat=m):
                for h in itertools.product((0, 1), repeat=n):
                    a = R.align(r, h)
                    every = _all_alignments(r, h)
                    assert a["distance"] == min(e[0] for e in every)
                    assert tuple(a[k] for k in KEYS) in every


def _replay(ref, hyp, ops):
    """The hypothesis the ops turn ref into; the positions must run through both strings without a gap."""
    out, i, j = [], 0, 0
    for op, ri, hj in ops:
        if op in (R.COR, R.SUB, R.DEL):
            assert ri == i
            i += 1
        else:
            assert ri == -1
        if op in (R.COR, R.SUB, R.INS):
            assert hj == j
            j += 1
        else:
            assert hj == -1
        if op == R.COR:
            assert ref[ri] == hyp[hj]
            out.append(ref[ri])
        elif op == R.SUB:
            assert ref[ri] != hyp[hj]
            out.append(hyp[hj])
        elif op == R.INS:
            out.append(hyp[hj])
    assert i == len(ref) and j == len(hyp)
    return out


@pytest.mark.parametrize("V", [2, 3, 50])
def test_definition_on_random_pairs(V):
    from asr_chinese_e2e_amd.Utils.score import edit_distance
    rng = np.random.default_rng(V)
    for _ in range(120):
        ref, hyp = rng.integers(0, V, int(rng.integers(0, 41))).tolist(), rng.integers(0, V, int(rng.integers(0, 41))).tolist()
        a = R.align(ref, hyp)
        assert a["distance"] == edit_distance(ref, hyp)
        assert a["cor"] + a["sub"] + a["del"] == len(ref) and a["cor"] + a["sub"] + a["ins"] == len(hyp)
        assert a["sub"] + a["del"] + a["ins"] == a["distance"]
        assert _replay(ref, hyp, a["ops"]) == hyp


def test_pinned_ties():
    a, b, x = 10, 11, 12
    assert R.align([a, b], [b, a]) == {"distance": 2, "cor": 0, "sub": 2, "del": 0, "ins": 0, "ops": [(R.SUB, 0, 0), (R.SUB, 1, 1)]}
    assert R.align([a], [b, a]) == {"distance": 1, "cor": 1, "sub": 0, "del": 0, "ins": 1, "ops": [(R.INS, -1, 0), (R.COR, 0, 1)]}
    assert R.align([], []) == {"distance": 0, "cor": 0, "sub": 0, "del": 0, "ins": 0, "ops": []}
    assert R.align([], [x]) == {"distance": 1, "cor": 0, "sub": 0, "del": 0, "ins": 1, "ops": [(R.INS, -1, 0)]}
    assert R.align([x], []) == {"distance": 1, "cor": 0, "sub": 0, "del": 1, "ins": 0, "ops": [(R.DEL, 0, -1)]}
    d = R.directions([a, b], [b, a])
    assert d[0].tolist() == [R.LEFT] * 3 and d[:, 0].tolist() == [R.LEFT, R.UP, R.UP]


# ------------------------------------------------------------------------------------------------ the host half of the Scorer
TOKENS = ["$", "%", "^", "&", "a", "b", "c", "d"]      # ids 4 .. 7 spell a .. d
A, B, C, D = 4, 5, 6, 7
REFS = [[A, B, C], [A, A], [], [B, D, C, A]]
NBEST = [[[A, C, C], [A, B, C]],            # rank 0: one substitution b -> c; rank 1 is right
         [[A, A], [A]],                     # right at rank 0; the tie goes to the first rank anyway
         [[B], []],                         # an empty reference: one insertion; rank 1 is right
         [[2, D, C, C, 3, 0], [B, D, C]]]   # sos / eos / pad are dropped: d c c against b d c a


def _scorer(ignore=()):
    from asr_chinese_e2e_amd.scoring import Scorer
    return Scorer(TOKENS, ignore_ids=ignore)


def _fed(nbest=True, ignore=()):
    s = _scorer(ignore)
    res = [[R.align(s._clean(r), s._clean(x)) for x in h] for r, h in zip(REFS, NBEST)]
    if nbest:
        s.add_aligned(list("wxyz"), res, NBEST, REFS)
    else:
        s.add_aligned(list("wxyz"), [r[0] for r in res], [h[0] for h in NBEST], REFS)
    return s


def test_scorer_summary_of_a_hand_made_corpus():
    from asr_chinese_e2e_amd.Utils.score import calculate_cer
    s = _fed()
    # z: ref b d c a, hyp d c c -> D[4][3] = 2: delete b, keep d, keep c, substitute a -> c
    assert s.utts[3]["ops"] == [(R.DEL, 0, -1), (R.COR, 1, 0), (R.COR, 2, 1), (R.SUB, 3, 2)] and s.utts[3]["hyp"] == [D, C, C]
    got = s.summary()
    conv = [calculate_cer("a c c", "a b c"), calculate_cer("a a", "a a"), calculate_cer("b", ""), calculate_cer("d c c", "b d c a")]
    assert got == {"utterances": 4, "ref_tokens": 9, "cor": 6, "sub": 2, "del": 1, "ins": 1, "cer": 4 / 9, "ser": 3 / 4, "empty_refs": 1,
                   "cer_ref_convention": sum(conv) / 4, "oracle_cer": 1 / 9, "oracle_rank_hist": [1, 3]}
    assert conv == [1 / 3, 0.0, 1.0, 3 / 4]      # the string convention counts the spaces: another figure than the token-level one
    plain = _fed(nbest=False).summary()
    assert "oracle_cer" not in plain and "oracle_rank_hist" not in plain and {k: plain[k] for k in plain} == {k: got[k] for k in plain}


def test_scorer_per_token_and_confusions():
    s = _fed()
    assert s.per_token() == [{"id": B, "token": "b", "cor": 0, "sub": 1, "del": 1, "ins": 1},      # most errors first, then by id
                             {"id": A, "token": "a", "cor": 3, "sub": 1, "del": 0, "ins": 0},
                             {"id": C, "token": "c", "cor": 2, "sub": 0, "del": 0, "ins": 0},
                             {"id": D, "token": "d", "cor": 1, "sub": 0, "del": 0, "ins": 0}]
    assert [t["token"] for t in s.per_token(top=2)] == ["b", "a"]
    assert s.confusions() == [{"ref_id": A, "hyp_id": C, "ref": "a", "hyp": "c", "count": 1}, {"ref_id": B, "hyp_id": C, "ref": "b", "hyp": "c", "count": 1}]
    assert s.confusions(top=1) == s.confusions()[:1]
    assert _scorer().per_token() == [] and _scorer().confusions() == []


def test_scorer_ignore_ids_remove_from_both_sides():
    s = _fed(ignore=(C,))
    assert [u["ref"] for u in s.utts] == [[A, B], [A, A], [], [B, D, A]] and [u["hyp"] for u in s.utts] == [[A], [A, A], [B], [D]]
    got = s.summary()
    assert (got["ref_tokens"], got["cor"], got["sub"], got["del"], got["ins"]) == (7, 4, 0, 3, 1) and got["cer"] == 4 / 7
    with pytest.raises(ValueError, match="does not belong"):
        _scorer().add_aligned(["k"], [R.align([A], [A])], [[A, B]], [[A]])
    with pytest.raises(ValueError, match="keys"):
        _scorer().add_aligned(["k"], [], [[A]], [[A]])


def test_write_jsonl_round_trips(tmp_path):
    s = _fed()
    path = tmp_path / "scores.jsonl"
    s.write_jsonl(str(path))
    lines = [json.loads(x) for x in open(path, encoding="utf-8").read().splitlines()]
    assert len(lines) == 5 and lines[-1] == {"summary": s.summary()}
    assert lines[0] == {"key": "w", "ref": "a b c", "hyp": "a c c", "distance": 1, "cor": 2, "sub": 1, "del": 0, "ins": 0,
                        "ops": [["=", "a", "a"], ["S", "b", "c"], ["=", "c", "c"]]}
    assert lines[2]["ops"] == [["I", None, "b"]] and lines[3]["ops"][0] == ["D", "b", None]
    names = {"=": R.COR, "S": R.SUB, "D": R.DEL, "I": R.INS}
    for u, line in zip(s.utts, lines):      # back to what went in
        assert line["ref"].split() == [TOKENS[i] for i in u["ref"]] and line["hyp"].split() == [TOKENS[i] for i in u["hyp"]]
        assert [names[o[0]] for o in line["ops"]] == [o[0] for o in u["ops"]]
        assert tuple(line[k] for k in KEYS) == tuple(u[k] for k in KEYS)


def test_abi_header_binding_and_makefile():
    from asr_chinese_e2e_amd import _lib, kernels
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asr_hip.h")).read(), flags=re.S)
    for name in ("asr_edit_align", "asr_edit_align_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and hasattr(_lib.fast, name)
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    raw = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (ASR_EDIT_\w+) (\d+)", raw)}
    assert consts == {"ASR_EDIT_LDS_DIR_BYTES": kernels.EDIT_LDS_DIR_BYTES, "ASR_EDIT_MAX_REF": kernels.EDIT_MAX_REF, "ASR_EDIT_COR": R.COR,
                      "ASR_EDIT_SUB": R.SUB, "ASR_EDIT_DEL": R.DEL, "ASR_EDIT_INS": R.INS}
    # the masks of an LDS pair, its boundary column and the counts-only columns of the longest reference stay inside asr_cer's 150 KB
    assert kernels.EDIT_LDS_DIR_BYTES + 4 * (kernels.EDIT_LDS_DIR_BYTES // 16 + 1) + 16 <= 150 * 1024 and 8 * (kernels.EDIT_MAX_REF + 1) <= 150 * 1024
    assert _lib.ABI_VERSION == 10 == _lib.lib.asr_abi_version()
    make = open(os.path.join(ROOT, "asr_chinese_e2e_amd", "csrc", "Makefile")).read()
    assert "score.hip" in re.search(r"^SRCS\s*=(.*)$", make, re.M).group(1)


def test_size_query_and_refusals_need_no_gpu():
    """The size query and the launcher's checks run on the host before any launch: with host mirrors alone they answer without a device."""
    from asr_chinese_e2e_amd import _lib, kernels
    B = kernels.EDIT_LDS_DIR_BYTES
    assert kernels.edit_align_workspace_bytes([15] * 320, [15] * 320, range(320), 15, 15) == 0
    assert kernels.edit_align_workspace_bytes([128], [B // 32], [0], 128, B // 32) == 0
    assert kernels.edit_align_workspace_bytes([128], [B // 32 + 1], [0], 128, B // 32 + 1) == B + 32
    assert kernels.edit_align_workspace_bytes([129, 5], [B // 48, 9], [0, 1], 129, B // 48) == 0
    assert kernels.edit_align_workspace_bytes([1000, 15, 1000], [1100, 15], [0, 1, 0], 1000, 1100) == 2 * 1100 * 16 * 16
    assert kernels.edit_align_workspace_bytes([2000], [3000], [0], 1000, 1100) == 1100 * 16 * 16      # lengths clamp to Lh / Lr
    assert kernels.edit_align_workspace_bytes([5], [5], [1], 5, 5) == 0 and "ref_of[0] = 1" in _lib.last_error()
