"""asr_ctc_align_long_filler on the device against its definition (tests/align_filler_ref.py), bit for bit: score (fp64), path with its -2
frames, spans and the token sums / extremes - no tolerance anywhere.  Then its identities with asr_ctc_align_long on the device, a ragged
launch, and end to end through model.align_long(filler=...).

Label counts as tests/test_align_long_gpu.py's: L = 1, 64 reach P = 1 (one wave), 65, 256 P = 2, 257, 1024 P = 4, 1025, 8192 P = 8 - both
edges of every instantiation.  A pair with index 64 P w sits at lane 0 of wave w and takes its neighbour's label state through LDS; the
pair before it sits at lane 63 of the wave before."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import align_filler_ref as F  # noqa: E402
from tests import align_long_ref as A  # noqa: E402
from tests.test_align_long_gpu import _model, as_dtype, classes, same_bits  # noqa: E402
from tests.test_align_long_gpu import run as run_plain  # noqa: E402

DEV = "cuda"
NEG = -np.inf


def run(recs, dtype=torch.float32, ld=None, blank=0):
    """recs: [(rows float32 as the device holds them, lse, star, labels, gap, gap_tail)] -> per recording dict(score, path, spans, tok)
    from ONE launch of the filler export."""
    from asr_chinese_e2e_amd import kernels as K
    V = recs[0][0].shape[1]
    Ts, Ls = [r[0].shape[0] for r in recs], [len(r[3]) for r in recs]
    buf = torch.zeros(max(sum(Ts), 1), ld or V, dtype=dtype, device=DEV)
    if sum(Ts):
        buf[:sum(Ts), :V] = torch.from_numpy(np.concatenate([r[0] for r in recs])).to(DEV).to(dtype)
    lse = torch.from_numpy(np.concatenate([np.asarray(r[1], np.float32) for r in recs])).to(DEV)
    star = torch.from_numpy(np.concatenate([np.asarray(r[2], np.float32) for r in recs])).to(DEV)
    ro, lo = np.concatenate(([0], np.cumsum(Ts))), np.concatenate(([0], np.cumsum(Ls)))
    lab = np.concatenate([np.asarray(r[3], np.int64).reshape(-1) for r in recs])
    gap = np.concatenate([np.asarray(r[4], np.uint8).reshape(-1) for r in recs])
    path, spans, tok, score = K.ctc_align_long_filler(buf[:sum(Ts), :V], lse, star, ro, lab, lo, gap, [int(r[5]) for r in recs], blank=blank)
    torch.cuda.synchronize()
    path, spans, tok, score = path.cpu().numpy(), spans.cpu().numpy(), tok.cpu().numpy(), score.cpu().numpy()
    return [dict(score=score[r], path=path[ro[r]:ro[r + 1]], spans=spans[lo[r]:lo[r + 1]], tok=tok[lo[r]:lo[r + 1]]) for r in range(len(recs))]


def check(rows, star, lab, gap, tail, dtype=torch.float32, ld=None, blank=0, lse=None, want=None):
    """The kernel on (rows as `dtype` holds them) against the definition on the same values; star is given per frame and used as it is."""
    x = as_dtype(rows, dtype)
    if lse is None:
        lse = A.lse_of(x) if x.shape[0] else np.zeros(0, np.float32)
    want = F.align(x, lse, star, lab, gap, tail, blank) if want is None else want
    got = run([(x, lse, star, lab, gap, tail)], dtype, ld, blank)[0]
    same_bits(got, want, (x.shape, len(lab), dtype, ld))
    return got, want


# ------------------------------------------------------------------------------------ kernel against definition
def flagged_pairs(L, seed):
    """Pair 0, random pairs, and - where a second wave has pairs (L = 65 fills 33 lanes of one) - the pair 64 P w at lane 0 of the last
    wave that has pairs and the pair just before it."""
    P = classes(L)
    rng = np.random.RandomState(seed)
    pairs = {0} | set(int(i) for i in rng.choice(L, min(L, max(1, L // 50)), replace=False))
    later = 64 * P * ((L - 1) // (64 * P)) or None
    if later:
        pairs |= {later, later - 1}
    return sorted(pairs), later


@functools.lru_cache(maxsize=None)
def filler_inputs(L, seed):
    """tests/align_filler_ref.filler_case with V = 12: foreign frames (class 11, in no label) in front of every flagged pair, in front of
    two pairs that are NOT flagged (the path has to spend plain states on them) and behind the last token; the tail is wide."""
    pairs, later = flagged_pairs(L, seed)
    rows, lse, star, lab, gap, tail = F.filler_case(L, 12, seed, pairs, unflagged=[L // 3 + 1, L // 2 + 1] if L >= 8 else [])
    return rows, star, lab, gap, tail, later


def properties(want, star, lab, gap, tail, x, lse, later):
    """What a case must have, asserted on the reference before the kernel runs."""
    L, T = len(lab), x.shape[0]
    assert np.isfinite(want["score"])
    states = np.array(F.states_of(want["path"], T))
    wide = F.wide_states(L, gap, tail)
    fill = want["path"] == -2
    assert (fill & (states == 2 * L)).any(), "no filler frame in the tail"
    assert ((want["path"] == -1) & wide[states]).any(), "no plain-blank frame in a wide state"
    assert (fill & (states == 0)).any(), "no filler frame in front of pair 0"
    if later is not None:
        assert later >= 64 * classes(L) and (fill & (states == 2 * later)).any(), "no filler frame in a flagged pair of a later wave"
        assert (fill & (states == 2 * (later - 1))).any(), "no filler frame in the pair before it"


@pytest.mark.parametrize("L", [1, 64, 65, 256, 257, 1024, 1025])
def test_kernel_is_the_definition(L):
    """T = 2 L + the inserted foreign frames + 1; f32 and bf16 rows, ld = V and a padded ld."""
    rows, star, lab, gap, tail, later = filler_inputs(L, 300 + L)
    assert rows.shape[0] > 2 * L and classes(L) == {1: 1, 64: 1, 65: 2, 256: 2, 257: 4, 1024: 4, 1025: 8}[L]
    for dtype, lds in ((torch.float32, (None, 24)), (torch.bfloat16, (None, 16))):
        x = as_dtype(rows, dtype)
        lse = A.lse_of(x)
        want = F.align(x, lse, star, lab, gap, tail)
        properties(want, star, lab, gap, tail, x, lse, later)
        for ld in lds:
            check(rows, star, lab, gap, tail, dtype, ld, lse=lse, want=want)


@pytest.mark.parametrize("dtype,ld", [(torch.float32, None), (torch.bfloat16, 24)])
def test_kernel_at_the_limit(dtype, ld):
    """L = 8192 (P = 8, every pair of all 1024 threads): f32 dense rows, bf16 rows in a padded buffer."""
    rows, star, lab, gap, tail, later = filler_inputs(8192, 17)
    assert later == 7680
    x = as_dtype(rows, dtype)
    lse = A.lse_of(x)
    want = F.align(x, lse, star, lab, gap, tail)
    properties(want, star, lab, gap, tail, x, lse, later)
    check(rows, star, lab, gap, tail, dtype, ld, lse=lse, want=want)


# ------------------------------------------------------------------------------------ edges
def _random(T, L, V, seed, star_at=-1.0):
    rng = np.random.RandomState(seed)
    rows = rng.normal(0.0, 2.0, (T, V)).astype(np.float32)
    lab = rng.randint(1, V, L)
    if L >= 3:
        lab[1] = lab[0]
    star = rng.normal(star_at, 1.5, T).astype(np.float32)
    gap = (rng.uniform(size=L) < 0.5).astype(np.uint8)
    return rows, star, lab, gap


def test_empty_sides():
    rows, star, lab, gap = _random(9, 0, 12, 3)
    got, _ = check(rows, star, lab, gap, 1)                                       # L = 0, the tail wide: the sum of the wide emission
    plain, _ = check(rows, star, lab, gap, 0)                                     # L = 0, not wide: every frame blank
    assert (got["path"] == -2).any() and (got["path"] <= -1).all() and (plain["path"] == -1).all() and got["score"] > plain["score"]
    same_bits(plain, A.align(rows, A.lse_of(rows), lab))
    none = np.zeros((0, 12), np.float32)
    for tail in (0, 1):
        got, _ = check(none, np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.uint8), tail)      # T = 0, L = 0
        assert got["score"] == 0.0
        got, _ = check(none, np.zeros(0, np.float32), np.array([3, 4, 4]), np.array([1, 1, 1], np.uint8), tail)      # T = 0, L = 3
        assert got["score"] == NEG and (got["spans"] == -1).all()
        rows, star = _random(1, 0, 12, 4)[0], np.array([1.0], np.float32)          # T = 1: v[0] is all there is; star above any log posterior
        got, _ = check(rows, star, np.zeros(0, np.int64), np.zeros(0, np.uint8), tail)
        assert got["path"].tolist() == [-2 if tail else -1]
        got, _ = check(rows, star, np.array([5]), np.array([1], np.uint8), tail)      # the token takes the frame or the path does not end
        assert got["path"].tolist() == [0]
        got, _ = check(rows, star, np.array([5, 6]), np.array([1, 1], np.uint8), tail)
        assert got["score"] == NEG and got["path"].tolist() == [-1]


def test_feasibility_edge():
    """T exactly at feasibility, every gap and the tail wide, star far above every blank: no frame is left for a filler; one frame less
    is infeasible - a wide blank is still a state that takes a frame."""
    for L in (5, 70, 300, 1100):
        rng = np.random.RandomState(40 + L)
        lab = rng.randint(1, 12, L)
        lab[1] = lab[0]
        T = L + A.repeats(lab)
        rows = rng.normal(0.0, 2.0, (T, 12)).astype(np.float32)
        star, gap = np.full(T, 5.0, np.float32), np.ones(L, np.uint8)
        got, want = check(rows, star, lab, gap, 1)
        assert np.isfinite(got["score"]) and (got["spans"][:, 0] == got["spans"][:, 1]).all()
        assert (got["path"] == -2).sum() == A.repeats(lab)                      # the blanks the repeats need are wide, and star is above them
        got, _ = check(rows[:-1], star[:-1], lab, gap, 1)
        assert got["score"] == NEG and (got["spans"] == -1).all() and (got["path"] == -1).all() and np.isneginf(got["tok"]).all()


def test_minus_infinity_and_ties():
    """Rows holding -inf; star = -inf on some frames; star with the bits of the blank's emission on others (the blank wins: -1)."""
    rng = np.random.RandomState(32)
    rows, star, lab, gap = _random(400, 130, 12, 31)
    rows = rows.copy()
    rows[rng.uniform(size=rows.shape) < 0.3] = -np.inf
    rows[:, 0] = rng.normal(-1.0, 1.0, 400).astype(np.float32)               # the blank stays finite: no row is -inf throughout
    gap[:] = 1
    for dtype in (torch.float32, torch.bfloat16):
        x = as_dtype(rows, dtype)
        lse = A.lse_of(x)
        eb = A.emissions(x, lse)[:, 0]
        st = star.copy()
        st[0::4] = NEG
        st[1::4] = eb[1::4]                                                    # a tie, bit for bit
        st[2::4] = np.nextafter(eb[2::4], np.float32(np.inf))                 # one ulp above
        got, want = check(rows, st, lab, gap, 1, dtype, lse=lse)
        assert not np.isnan(got["score"]) and not np.isnan(got["tok"]).any()
        blankish = got["path"] < 0
        assert not (got["path"][0::4] == -2).any() and not (got["path"][1::4] == -2).any()
        assert (got["path"][2::4][blankish[2::4]] == -2).all() and blankish[1::4].any() and blankish[2::4].any()      # every gap is wide


def test_full_vocabulary():
    pairs, _ = flagged_pairs(300, 11)
    rows, lse, star, lab, gap, tail = F.filler_case(300, 4232, 11, pairs)
    got, _ = check(rows, star, lab, gap, tail, torch.bfloat16, None)
    assert (got["path"] == -2).any()
    rng = np.random.RandomState(12)                                            # another blank id, a padded buffer
    rows, lab = rng.normal(0.0, 2.0, (700, 4232)).astype(np.float32), rng.randint(0, 4231, 300)
    star = rng.normal(-6.0, 2.0, 700).astype(np.float32)
    got, _ = check(rows, star, lab, np.ones(300, np.uint8), 1, torch.float32, 4240, blank=4231)
    assert (got["path"] == -2).any() and (got["path"] == -1).any()


# ------------------------------------------------------------------------------------ identities on the device
@pytest.mark.parametrize("L", [40, 100, 300, 1100])
def test_identities_on_the_device(L):
    """One case per instantiation (P = 1, 2, 4, 8, f32 and bf16): with all flags 0 (star above most blanks), and with star = -inf
    everywhere (every flag set), the four outputs have the bits of asr_ctc_align_long's on the same inputs."""
    rows, star, lab, _ = _random(L + L // 2, L, 12, 60 + L, star_at=0.0)
    T = rows.shape[0]
    for dtype, ld in ((torch.float32, 16), (torch.bfloat16, None)):
        x = as_dtype(rows, dtype)
        lse = A.lse_of(x)
        plain = run_plain([(x, lse, lab)], dtype, ld)[0]
        assert np.isfinite(plain["score"])
        same_bits(run([(x, lse, star, lab, np.zeros(L, np.uint8), 0)], dtype, ld)[0], plain, (L, dtype, "flags 0"))
        same_bits(run([(x, lse, np.full(T, NEG, np.float32), lab, np.ones(L, np.uint8), 1)], dtype, ld)[0], plain, (L, dtype, "star -inf"))
        some = run([(x, lse, star, lab, np.ones(L, np.uint8), 1)], dtype, ld)[0]      # and the feature does something here
        assert (some["path"] == -2).any() and some["score"] > plain["score"]


def test_ragged_launch_and_determinism():
    """R = 7: all four classes, flagged and unflagged recordings, an infeasible and an empty one share a launch; each has the bits it has
    alone and the definition's, and a second run gives the same bits."""
    recs = []
    for (T, L, seed, flagged) in ((2400, 1100, 21, True), (900, 600, 22, False), (6, 9, 23, True), (0, 0, 24, True), (300, 70, 25, True), (90, 30, 26, False),
                                  (120, 40, 27, True)):
        rows, star, lab, gap = _random(T, L, 12, seed)
        if not flagged:
            gap[:] = 0
        recs.append((rows, A.lse_of(rows) if T else np.zeros(0, np.float32), star, lab, gap, int(flagged)))
    alone = [run([r])[0] for r in recs]
    together, again = run(recs), run(recs)
    for r, (a, b, c) in enumerate(zip(alone, together, again)):
        same_bits(b, a, r)
        same_bits(c, a, r)
        same_bits(a, F.align(*recs[r]), r)
    assert np.isfinite(alone[0]["score"]) and alone[2]["score"] == NEG and alone[3]["score"] == 0.0
    assert (alone[0]["path"] == -2).any() and not (alone[1]["path"] == -2).any() and not (alone[5]["path"] == -2).any()
    same_bits(alone[1], A.align(recs[1][0], recs[1][1], recs[1][3]), "unflagged")


# ------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module", params=["fp32", "bf16"])
def filler_setup(request):
    from asr_chinese_e2e_amd.data_handler import AudioParser
    from tests import vad_cases as C
    model = _model(request.param)
    parser = AudioParser(n_mels=80, lfr_m=4, lfr_n=3, device=DEV, frontend="kaldi")
    x = C.long_case()
    wav = torch.from_numpy(x[None]).to(DEV)
    tr = model.transcribe_long(parser, wav, [len(x)], batch_size=2, beam_size=3, joint="ctc_rescore", **C.LONG_OPTS)[0]
    segs = [(s["start_sample"], int(round(s["end_s"] * 16000))) for s in tr["segments"]]
    return model, parser, x, wav, tr, C, segs, host_stats(model, parser, x, segs, 2)


def host_stats(model, parser, x, segs, batch_size):
    """The recording's concatenated CTC rows with lse, best_lp and blank_lp as align_long lays them out, built batch by batch on the
    host side of the kernels: (rows (T, V) float32, lse, best_lp, blank_lp (T,) float32, rows per segment)."""
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.Utils import Pack
    rows, lse, best, blank, counts = [], [], [], [], []
    for i in range(0, len(segs), batch_size):
        part = segs[i:i + batch_size]
        S = max(1, max(b - a for a, b in part))
        wav = np.zeros((len(part), S), dtype=np.float32)
        for r, (a, b) in enumerate(part):
            wav[r, :b - a] = x[a:b]
        feats, flen = parser.parse_batch(torch.from_numpy(wav).cuda(), torch.tensor([b - a for a, b in part], dtype=torch.int32).cuda())
        logits = model._ctc_logits(Pack(wave=feats, wave_len=flen))
        _, bl, kl, l, _ = K.ctc_frame_stats(logits, flen.to(torch.int32), 0)
        for r, n in enumerate(flen.tolist()):
            rows.append(logits[r, :n].float().cpu().numpy())
            lse.append(l[r, :n].cpu().numpy())
            best.append(bl[r, :n].cpu().numpy())
            blank.append(kl[r, :n].cpu().numpy())
            counts.append(int(n))
    return np.concatenate(rows), np.concatenate(lse), np.concatenate(best), np.concatenate(blank), counts


@pytest.mark.parametrize("scope", ["lines", "tokens"])
def test_align_long_with_filler_end_to_end(filler_setup, scope):
    """The 12 s, five-burst recording against a script that only partly matches it: every second token of transcribe_long's own ids,
    each written twice, three tokens a line (and an empty second line).  The tiny model never prefers the blank, so blank states are
    taken only where the script forces them: a doubled token needs a blank between its two copies, inside a line (wide with scope
    "tokens" only) or across a line start (wide with both scopes).  p = the median of best_lp - blank_lp over the frames, so some of
    those frames lie above it (filler) and some below (plain): asserted on the reference first.  fillers, filler_frames, the token
    frames and the score are the definition's on the same rows, lse and best_lp - p; filler=None is today's call."""
    from asr_chinese_e2e_amd.align_long import filler_gaps, stitch_fillers
    model, parser, x, wav, tr, C, segs, (rows, lse, best, blank_lp, counts) = filler_setup
    ids = [i for i in tr["ids"] if i != 0]
    assert len(ids) >= 6
    seq = [t for i in ids[1::2] for t in (i, i)]
    texts = [seq[k:k + 3] for k in range(0, len(seq), 3)]
    texts = texts[:1] + [[]] + texts[1:]
    mine = seq
    p = float(np.median(best - blank_lp))
    assert p >= 0.0 and np.isfinite(p)
    star = (best - np.float32(p)).astype(np.float32)
    lines = [{"ids": t} for t in texts]
    gap = filler_gaps(lines, len(mine), scope)
    assert sum(gap) == (len(texts) - 1 if scope == "lines" else len(mine))
    want = F.align(rows, lse, star, mine, gap, 1)
    assert np.isfinite(want["score"]) and (want["path"] == -2).any() and (want["path"] == -1).any()      # filler and plain frames
    res = model.align_long(parser, wav, [len(x)], [texts], batch_size=2, filler=p, filler_scope=scope, **C.LONG_OPTS)
    assert len(res) == 1
    res = res[0]
    assert res["frames"] == rows.shape[0] and np.float64(res["score"]).view(np.int64) == np.float64(want["score"]).view(np.int64)
    assert [(t["start_frame"], t["end_frame"]) for t in res["tokens"]] == [tuple(int(v) for v in s) for s in want["spans"]]
    assert [t["logp"] for t in res["tokens"]] == [float(v) for v in want["tok"][:, 0]]
    line_of = [k for k, t in enumerate(texts) for _ in t]
    n, runs = stitch_fillers(want["path"].tolist(), line_of, len(texts), segs, counts, model.frame_seconds())
    assert res["filler_frames"] == n == int((want["path"] == -2).sum()) and res["fillers"] == runs and len(runs) >= 1
    assert all(r["before_line"] != 1 and r["before_line"] == (line_of + [len(texts)])[r["before_token"]] for r in runs)      # never the empty line
    if scope == "lines":      # only a line's first token and the tail have a wide gap
        assert all(r["before_token"] == len(mine) or gap[r["before_token"]] for r in runs)
    # off: the result of today's call, with no new key
    off = model.align_long(parser, wav, [len(x)], [texts], batch_size=2, filler=None, **C.LONG_OPTS)[0]
    today = model.align_long(parser, wav, [len(x)], [texts], batch_size=2, **C.LONG_OPTS)[0]
    assert off == today and "fillers" not in off and "filler_frames" not in off
    plain = A.align(rows, lse, mine)
    assert np.float64(off["score"]).view(np.int64) == np.float64(plain["score"]).view(np.int64) and res["score"] >= off["score"]
