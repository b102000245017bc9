"""Definitions the confidence kernels (csrc/confidence.hip) are checked against: numpy float64, no GPU.  Unpinned by WeNet's and
NeMo's binaries - the measures are restated from their descriptions (WeNet: the largest frame posterior along the best path; NeMo: entropy
-based frame confidences, Shannon entropy with linear normalisation, aggregated per token).

frame_stats        per frame: best (first maximum), best_lp, blank_lp, lse, ent = 1 - H / ln V; a class with p = 0 adds exactly 0 to H
token_measures     a token on frames s..e: {post_max, post_min, post_mean, ent_mean, ent_min}
greedy_runs        the maximal runs of equal non-blank classes of a frame-wise path: the tokens of the CTC collapse with their frames
stream_tokens      greedy_runs with each run's measures: what a timed greedy stream reports once its input has ended
utterance          the arithmetic mean of the tokens' values (None without one)
frame_bounds       how far fp32 arithmetic of the kernel's shape may lie from frame_stats - derived below from the arithmetic alone
token_bounds       the same for the five measures of a token
frame_stats_f32    a float32 restatement of the kernel's arithmetic (lane-strided sequential sums, a 6-level tree), which keeps
                   frame_bounds on the CPU (tests/test_confidence_cpu.py)

The bounds.  eps = 2^-24 is the unit roundoff of fp32 (round to nearest); expf and logf are taken as accurate to 1 ulp = 2 eps relative
(the HIP math library's documented accuracy; numpy's float32 routines are at least that good); division is correctly rounded.  A lane adds
n = ceil(V / 64) terms one after the other and the 64 lanes meet in a 6-level tree, so a sum of terms of one sign carries a relative
error of at most (n + 6) eps.  Products of eps are dropped and the first-order total is scaled by SLACK = 1.01 to cover them (the
first-order terms are ~1e-5 at most, their products below 1e-10).  With d_i = x_i - m <= 0, e_i = exp(d_i), s = sum e_i >= 1,
U = -sum d_i e_i >= 0, Q = sum d_i^2 e_i (float64 values of the row):
  d_i     one rounding: |err| <= eps |d_i|
  e_i     relative 2 eps (expf) + eps |d_i| (the error of d_i in the exponent), absolute + TINY = 2^-126 (a result below the smallest
          normal number may be flushed to 0)
  s       rel_s = (n + 6 + 2) eps + eps U / s + V TINY
  lse     = fl(m + logf(s)):  err_lse = rel_s + 2 eps ln s + eps |lse|
  lp_y    = fl(x_y - lse):    err_lp  = err_lse + eps |lp_y|           (best_lp, blank_lp, and the lp of any class a token names)
  u       terms d_i e_i: relative eps (d) + 2 eps + eps |d_i| (e) + eps (the product, fused or not); the sum (n + 6) eps:
          abs_u = (n + 10) eps U + eps Q + V TINY max|d_i finite|
  u / s   err_q = abs_u / s + (U / s) (rel_s + eps)
  H       = fl(logf(s) - u / s):  err_H = rel_s + 2 eps ln s + err_q + eps H
  ent     = fl(1 - fl(H / logf(V))): the quotient carries err_H / ln V + 3 eps (logf(V): 2 eps, the division: eps; H / ln V <= 1), the
          subtraction eps: err_ent = err_H / ln V + 4 eps.  Clamping to [0, 1] moves a value towards the definition's, never away.
A token on n frames (fp32 sums from 0.f in ascending t):
  max / min of lp_t: the largest err_lp of its frames;  sum of lp_t: sum err_lp_t + (n - 1) eps sum |lp_t|;  the mean: + eps |mean|
  post_* = expf(v): |err| <= post (expm1(err_v) + 2 eps) + TINY
  ent_mean: (sum err_ent_t + (n - 1) eps sum ent_t) / n + eps mean;  ent_min: the largest err_ent of its frames
"""
import math

import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126
SLACK = 1.01
MEASURES = ("post_max", "post_min", "post_mean", "ent_mean", "ent_min")


def _rows(logits):
    x = np.asarray(logits, dtype=np.float64)
    assert x.ndim == 2 and x.shape[1] >= 2
    return x


def _parts(x):
    """(m, d, e, s, U, Q) of the rows; d = -inf rows entries give e = 0 and add 0 to U and Q."""
    m = x.max(axis=1, keepdims=True)
    d = x - m
    e = np.exp(d)
    with np.errstate(invalid="ignore"):
        de = np.where(e > 0.0, d * e, 0.0)
        dde = np.where(e > 0.0, d * d * e, 0.0)
    return m[:, 0], d, e, e.sum(axis=1), -de.sum(axis=1), dde.sum(axis=1)


def frame_stats(logits, blank=0):
    """logits (R, V) -> dict(path (R,) int, best_lp, blank_lp, lse, ent (R,) float64, logp (R, V) float64)."""
    x = _rows(logits)
    V = x.shape[1]
    m, d, e, s, U, _ = _parts(x)
    lse = m + np.log(s)
    path = x.argmax(axis=1)      # numpy's argmax returns the first maximum
    H = np.log(s) + U / s
    ent = np.clip(1.0 - H / math.log(V), 0.0, 1.0)
    logp = x - lse[:, None]
    return dict(path=path, best_lp=logp[np.arange(len(x)), path], blank_lp=logp[:, blank], lse=lse, ent=ent, logp=logp)


def frame_bounds(logits):
    """dict(lse (R,), lp (R, V), ent (R,)): the bounds of the module docstring for every row (lp: for every class of the row)."""
    x = _rows(logits)
    V = x.shape[1]
    n = -(-V // 64)
    m, d, e, s, U, Q = _parts(x)
    lns = np.log(s)
    lse = m + lns
    dmax = np.where(np.isfinite(d), -d, 0.0).max(axis=1)
    rel_s = (n + 8) * EPS + EPS * U / s + V * TINY
    err_lse = rel_s + 2 * EPS * lns + EPS * np.abs(lse)
    with np.errstate(invalid="ignore"):
        lp = x - lse[:, None]
        err_lp = err_lse[:, None] + EPS * np.where(np.isfinite(lp), np.abs(lp), 0.0)
    abs_u = (n + 10) * EPS * U + EPS * Q + V * TINY * dmax
    err_q = abs_u / s + (U / s) * (rel_s + EPS)
    H = lns + U / s
    err_H = rel_s + 2 * EPS * lns + err_q + EPS * H
    err_ent = err_H / math.log(V) + 4 * EPS
    return dict(lse=SLACK * err_lse, lp=SLACK * err_lp, ent=SLACK * err_ent)


def token_measures(logp, ent, y, s, e):
    """The five measures of class y on frames s..e inclusive; logp (T, V), ent (T,) float64 (frame_stats')."""
    lp = np.asarray(logp, dtype=np.float64)[s:e + 1, y]
    en = np.asarray(ent, dtype=np.float64)[s:e + 1]
    n = e - s + 1
    return dict(post_max=math.exp(lp.max()), post_min=math.exp(lp.min()), post_mean=math.exp(lp.sum() / n), ent_mean=en.sum() / n, ent_min=en.min())


def token_bounds(logp, ent, err_lp, err_ent, y, s, e):
    """The bounds of token_measures' five values; err_lp (T, V), err_ent (T,): frame_bounds' lp and ent."""
    lp = np.asarray(logp, dtype=np.float64)[s:e + 1, y]
    en = np.asarray(ent, dtype=np.float64)[s:e + 1]
    b_lp, b_en = np.asarray(err_lp)[s:e + 1, y], np.asarray(err_ent)[s:e + 1]
    n = e - s + 1
    mean = lp.sum() / n
    b_mean = (b_lp.sum() + (n - 1) * EPS * np.abs(lp).sum()) / n + EPS * abs(mean)
    post = lambda v, b: math.exp(v) * (math.expm1(b) + 2 * EPS) + TINY      # noqa: E731
    return dict(post_max=SLACK * post(lp.max(), b_lp.max()), post_min=SLACK * post(lp.min(), b_lp.max()), post_mean=SLACK * post(mean, SLACK * b_mean),
                ent_mean=SLACK * ((b_en.sum() + (n - 1) * EPS * en.sum()) / n + EPS * en.sum() / n), ent_min=float(b_en.max()))


def greedy_runs(path, blank=0):
    """[(id, first frame, last frame)] of the maximal runs of equal non-blank classes: a repeat separated by a blank is a new token."""
    runs, last = [], blank
    for t, c in enumerate(int(v) for v in path):
        if c != blank and c != last:
            runs.append([c, t, t])
        elif c != blank:
            runs[-1][2] = t
        last = c
    return [tuple(r) for r in runs]


def stream_tokens(logits, blank=0):
    """One utterance (T, V) -> [dict(id, start_frame, end_frame, measures)] of the greedy path, the run open at the end included."""
    st = frame_stats(logits, blank)
    return [dict(id=y, start_frame=s, end_frame=e, measures=token_measures(st["logp"], st["ent"], y, s, e)) for y, s, e in greedy_runs(st["path"], blank)]


def utterance(values):
    vals = [float(v) for v in values if v is not None]
    return math.fsum(vals) / len(vals) if vals else None


def frame_stats_f32(logits, blank=0):
    """The kernel's arithmetic in numpy float32: lane l adds classes l, l + 64, ... one after the other from 0.f, the 64 lanes meet in a
    6-level pairwise tree, one exp / log each.  -> dict(best_lp, blank_lp, lse, ent) float32."""
    x = np.asarray(logits, dtype=np.float32)
    R, V = x.shape
    n = -(-V // 64)
    m = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = (x - m).astype(np.float32)
        e = np.exp(d).astype(np.float32)
        t = np.where(e > 0, (d * e).astype(np.float32), np.float32(0))

    def wave_sum(v):
        pad = np.zeros((R, n * 64), dtype=np.float32)
        pad[:, :V] = v
        lanes = np.zeros((R, 64), dtype=np.float32)
        for k in range(n):
            lanes = (lanes + pad[:, k * 64:(k + 1) * 64]).astype(np.float32)
        while lanes.shape[1] > 1:
            h = lanes.shape[1] // 2
            lanes = (lanes[:, :h] + lanes[:, h:]).astype(np.float32)
        return lanes[:, 0]
    s, u = wave_sum(e), wave_sum(t)
    lns = np.log(s).astype(np.float32)
    lse = (m[:, 0] + lns).astype(np.float32)
    h = (lns - (u / s).astype(np.float32)).astype(np.float32)
    ent = np.clip((np.float32(1) - (h / np.log(np.float32(V))).astype(np.float32)).astype(np.float32), np.float32(0), np.float32(1))
    path = x.argmax(axis=1)
    return dict(best_lp=(m[:, 0] - lse).astype(np.float32), blank_lp=(x[:, blank] - lse).astype(np.float32), lse=lse, ent=ent, path=path)


# ---------------------------------------------------------------------------------------------- the timed step's fixed input
STEP_SLOTS, STEP_T, STEP_V = 3, 200, 20
STEP_LENS = (200, 193, 200)
STEP_SEED = 20


def _plan(rng, T, lead, tail_open):
    """A frame-wise class plan: `lead` (class, frames) segments, then random ones; tail_open: the last frames belong to a run."""
    seg = list(lead)
    used = sum(n for _, n in seg)
    last = seg[-1][0] if seg else 0
    while used < T:
        c = int(rng.integers(0, STEP_V)) if rng.random() < 0.7 else 0
        if c == last:
            c = 0 if c else 1 + int(rng.integers(0, STEP_V - 1))
        n = min(T - used, int(rng.choice([1, 1, 2, 3, 5, 9])))
        seg.append((c, n))
        used, last = used + n, c
    plan = [c for c, n in seg for _ in range(n)][:T]
    if tail_open:
        plan[-3:] = [7, 7, 7] if plan[-4] != 7 else [8, 8, 8]
    else:
        plan[-2:] = [0, 0]
    return plan


def step_logits(seed=STEP_SEED):
    """The (3, 200, 20) float32 logits of the timed-step and greedy-against-Viterbi tests, drawn from a seeded generator: a planned class
    per frame lifted by 6 over unit normal noise.  Slot 0 holds runs of 1, 2 and 70 frames (the long one lies across frames 64, 65, 128
    and 130, the cuts of the 64- and 65-frame chunks) and a repeat separated by one blank, slot 1 is shorter (STEP_LENS), slot 2 ends on
    an open run.  Rows past a slot's length are zero."""
    rng = np.random.default_rng(seed)
    lead0 = [(0, 3), (5, 1), (0, 2), (7, 2), (0, 1), (7, 3), (3, 4), (4, 1), (0, 40), (9, 75), (0, 2), (11, 2)]      # 9: frames 57..131
    plans = [_plan(rng, STEP_LENS[0], lead0, False), _plan(rng, STEP_LENS[1], [(2, 6), (0, 1), (2, 1)], False), _plan(rng, STEP_LENS[2], [(0, 10), (6, 17)], True)]
    x = np.zeros((STEP_SLOTS, STEP_T, STEP_V), dtype=np.float32)
    for b, plan in enumerate(plans):
        z = rng.standard_normal((len(plan), STEP_V)).astype(np.float32)
        z[np.arange(len(plan)), plan] += np.float32(6.0)
        x[b, :len(plan)] = z
    return x


def top2_gap(logits):
    """Per row the difference of the two largest log-probabilities (= of the two largest logits), float64."""
    x = np.sort(_rows(logits), axis=1)
    return x[:, -1] - x[:, -2]
