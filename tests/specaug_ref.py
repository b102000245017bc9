"""The definition of the SpecAugment policies (several time and mel masks with zero fill, a linear time warp, spectral substitution), in
plain Python integers and numpy float32.  Parity is unpinned by WeNet's and ESPnet's code: the rules are restated from their descriptions
(WeNet spec_aug / spec_sub, ESPnet's time_warp with a linear instead of a bicubic interpolation, so that every value is a named IEEE
operation) and THIS file is what asr_chinese_e2e_amd/data_handler/specaug.py and the two kernels asr_*_norm_specaug_lfr_fwd are tested
against.  Nothing here imports the package.

A policy is any object with the integer fields warp, n_t, max_t, t_permille, n_f, max_f, n_s, sub_t (Policy below).
draw    -> (n, n_draws) uint32: the random numbers of a data set's utterances for one epoch.
resolve -> the int32 row [wc, ww | (t0, t1) x n_t | (f0, f1) x n_f | (s, e, p) x n_s] of an utterance of T frames and F bins.
apply   -> the augmented frames of one utterance from its normalised frames and its row."""
import collections
import random

import numpy as np

Policy = collections.namedtuple("Policy", "warp n_t max_t t_permille n_f max_f n_s sub_t", defaults=(0, 0, 1, 1000, 0, 1, 0, 1))


def n_draws(p):
    return 2 + 2 * p.n_t + 2 * p.n_f + 3 * p.n_s


def draw(seed, epoch, n, p):
    """One generator per (seed, epoch), consumed as getrandbits(32) in utterance order, n_draws numbers per utterance whatever they
    decide: a pure function of (seed, epoch, utterance index)."""
    rng = random.Random(f"spec_augment/{int(seed)}/{int(epoch)}")
    k = n_draws(p)
    return np.array([[rng.getrandbits(32) for _ in range(k)] for _ in range(n)], dtype=np.uint32).reshape(n, k)


def resolve(p, d, T, F):
    """Integer arithmetic only.  d: the utterance's n_draws numbers."""
    d = [int(v) for v in d]
    T, F, W = int(T), int(F), int(p.warp)
    row, k = [0, 0], 2
    if W > 0 and T - 2 * W > 0:
        wc = W + d[0] % (T - 2 * W)
        row = [wc, wc - W + 1 + d[1] % (2 * W)]
    cap = min(int(p.max_t), T * int(p.t_permille) // 1000)
    for _ in range(p.n_t):
        if T == 0 or cap == 0:
            row += [0, 0]
        else:
            start = d[k] % T
            row += [start, min(T, start + 1 + d[k + 1] % cap)]
        k += 2
    for _ in range(p.n_f):
        start = d[k] % F
        row += [start, min(F, start + 1 + d[k + 1] % int(p.max_f))]
        k += 2
    for _ in range(p.n_s):
        if T == 0:
            row += [0, 0, 0]
        else:
            s = d[k] % T
            row += [s, min(T, s + 1 + d[k + 1] % int(p.sub_t)), d[k + 2] % (s + 1)]
        k += 3
    return np.array(row, dtype=np.int32)


def clamp_row(row, n_t, n_f, n_s, T, F):
    """What the consumer makes of a row before it uses it -> (wc, ww, [(t0, t1)], [(f0, f1)], [(s, e, p)]); wc = ww = 0: no warp."""
    row = [int(v) for v in row]
    clip = lambda v, lo, hi: min(max(v, lo), hi)
    wc, ww = row[0], row[1]
    if not (0 < wc < T and 0 < ww < T):
        wc = ww = 0
    k, tm, fm, sb = 2, [], [], []
    for _ in range(n_t):
        t0 = clip(row[k], 0, T)
        tm.append((t0, clip(row[k + 1], t0, T)))
        k += 2
    for _ in range(n_f):
        f0 = clip(row[k], 0, F)
        fm.append((f0, clip(row[k + 1], f0, F)))
        k += 2
    for _ in range(n_s):
        s = clip(row[k], 0, T)
        sb.append((s, clip(row[k + 1], s, T), clip(row[k + 2], 0, s)))
        k += 3
    return wc, ww, tm, fm, sb


def apply(x, row, n_t, n_f, n_s):
    """x (T, F) float32 normalised frames -> y (T, F): every output cell is pulled through substitution source, masks, warp."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    T, F = x.shape
    wc, ww, tm, fm, sb = clamp_row(row, n_t, n_f, n_s, T, F)
    y = np.zeros((T, F), dtype=np.float32)
    mel_masked = [any(f0 <= f < f1 for f0, f1 in fm) for f in range(F)]
    for t in range(T):
        u = t
        for s, e, p in sb:                      # the last matching substitution wins
            if s <= t < e:
                u = t - p
        if any(t0 <= u < t1 for t0, t1 in tm):
            continue
        if ww == 0:
            src = x[u]
        else:
            o, n_out, base, n_in = (u, ww, 0, wc) if u < ww else (u - ww, T - ww, wc, T - wc)
            num, den = max((2 * o + 1) * n_in - n_out, 0), 2 * n_out
            i0 = num // den
            i1 = min(i0 + 1, n_in - 1)
            w = np.float32(num % den) / np.float32(den)
            v0, v1 = x[base + i0], x[base + i1]
            src = (v0 + w * (v1 - v0)).astype(np.float32)      # float32 arrays: each operation rounds on its own
        for f in range(F):
            if not mel_masked[f]:
                y[t, f] = src[f]
    return y


def stack(y, m, n, rows):
    """LFR stacking as the kernels do it: row r, column j F + f holds y[min(r n + j, T - 1), f]; zero rows past ceil(T / n)."""
    T, F = y.shape
    out = np.zeros((rows, m * F), dtype=np.float32)
    Tl = min(-(-T // n), rows)
    for r in range(Tl):
        for j in range(m):
            out[r, j * F:(j + 1) * F] = y[min(r * n + j, T - 1)]
    return out, Tl
