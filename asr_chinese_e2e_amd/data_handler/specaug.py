"""Host side of the SpecAugment policies (several time and mel masks with zero fill, a linear time warp, spectral substitution: the
augmentation of the WeNet / ESPnet AISHELL recipes; the reference has one mask per axis with mean fill - processor.sample_spec_augment -
so parity is unpinned by the reference, and the definition is tests/specaug_ref.py).  A policy says how many ranges of which width an
utterance gets; draw() gives every utterance of the data set its random numbers for one epoch, resolve() turns an utterance's numbers and
its frame count into the int32 row the kernels asr_utt_norm_specaug_lfr_fwd / asr_global_norm_specaug_lfr_fwd consume:

    [wc, ww | (t0, t1) x n_t | (f0, f1) x n_f | (s, e, p) x n_s]

wc, ww: the warp moves frame boundary wc to ww (both 0: no warp); frames [t0, t1) and bins [f0, f1) become 0, the mean under both
normalisations; frames [s, e) are replaced by the frames p earlier.  Frames are the front end's 10 ms frames, before LFR stacking.
Everything here is integer arithmetic on the host: the lengths come from the loader's pack_meta, nothing is read back from the device."""
import random
import re

import numpy as np

MAX_RANGES = 8        # ASR_SPECAUG_MAX_RANGES of include/asr_hip.h: ranges of one kind in a row
MAX_WARP = 64
GRAMMAR = ("'wenet', 'espnet', or comma-separated items w<W> (warp window), t<N>x<WIDTH> (time masks), f<N>x<WIDTH> (mel masks), "
           "s<N>x<WIDTH> (substitutions), r<PERMILLE> (time masks cover at most that share of an utterance), e.g. w5,t2x50,f2x10,s3x30,r200")
PRESETS = {"wenet": "t2x50,f2x10", "espnet": "w5,t2x40,f2x30"}


class SpecAugmentPolicy:
    """warp: the warp window W in frames (0 = off); n_t time masks of at most max_t frames and at most t_permille / 1000 of the utterance;
    n_f mel masks of at most max_f bins; n_s substitutions of at most sub_t frames."""

    FIELDS = ("warp", "n_t", "max_t", "t_permille", "n_f", "max_f", "n_s", "sub_t")

    def __init__(self, warp=0, n_t=0, max_t=1, t_permille=1000, n_f=0, max_f=1, n_s=0, sub_t=1):
        vals = (warp, n_t, max_t, t_permille, n_f, max_f, n_s, sub_t)
        for name, v in zip(self.FIELDS, vals):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"SpecAugmentPolicy: {name}={v!r} is not an integer")
            setattr(self, name, int(v))
        if not 0 <= self.warp <= MAX_WARP:
            raise ValueError(f"SpecAugmentPolicy: warp={self.warp}, the window is 0 (off) .. {MAX_WARP} frames")
        for name in ("n_t", "n_f", "n_s"):
            if not 0 <= getattr(self, name) <= MAX_RANGES:
                raise ValueError(f"SpecAugmentPolicy: {name}={getattr(self, name)}, at most {MAX_RANGES} ranges of a kind")
        for name in ("max_t", "max_f", "sub_t"):
            if getattr(self, name) < 1:
                raise ValueError(f"SpecAugmentPolicy: {name}={getattr(self, name)}, a width cap is at least 1")
        if not 1 <= self.t_permille <= 1000:
            raise ValueError(f"SpecAugmentPolicy: t_permille={self.t_permille}, 1 .. 1000")

    @property
    def n_draws(self):
        """Random numbers per utterance, whatever they decide."""
        return 2 + 2 * self.n_t + 2 * self.n_f + 3 * self.n_s

    @property
    def width(self):
        """Words of an utterance's resolved row."""
        return 2 + 2 * self.n_t + 2 * self.n_f + 3 * self.n_s

    def check_mels(self, n_mels):
        if self.n_f and self.max_f > n_mels:
            raise ValueError(f"SpecAugmentPolicy: max_f={self.max_f} is wider than the {n_mels} mel bins of the front end")
        return self

    def __eq__(self, other):
        return isinstance(other, SpecAugmentPolicy) and all(getattr(self, n) == getattr(other, n) for n in self.FIELDS)

    def __hash__(self):
        return hash(tuple(getattr(self, n) for n in self.FIELDS))

    def __repr__(self):
        return "SpecAugmentPolicy(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.FIELDS) + ")"

    @classmethod
    def from_string(cls, text):
        """GRAMMAR.  Each kind of item at most once; a kind left out is off."""
        if not isinstance(text, str) or not text.strip():
            raise ValueError(f"spec_augment={text!r}: {GRAMMAR}")
        kw = {}
        for item in PRESETS.get(text.strip().lower(), text).split(","):
            item = item.strip().lower()
            m = re.fullmatch(r"([tfs])(\d+)x(\d+)", item)
            single = re.fullmatch(r"([wr])(\d+)", item)
            if m:
                count, cap = {"t": ("n_t", "max_t"), "f": ("n_f", "max_f"), "s": ("n_s", "sub_t")}[m.group(1)]
                new = {count: int(m.group(2)), cap: int(m.group(3))}
            elif single:
                new = {{"w": "warp", "r": "t_permille"}[single.group(1)]: int(single.group(2))}
            else:
                raise ValueError(f"spec_augment={text!r}: cannot read {item!r}; {GRAMMAR}")
            if any(k in kw for k in new):
                raise ValueError(f"spec_augment={text!r}: {item!r} repeats an item; {GRAMMAR}")
            kw.update(new)
        return cls(**kw)


def as_policy(v):
    """None / empty -> None, a SpecAugmentPolicy -> itself, a string -> from_string."""
    if v is None or v is False or (isinstance(v, str) and not v.strip()):
        return None
    return v if isinstance(v, SpecAugmentPolicy) else SpecAugmentPolicy.from_string(v)


def draw(seed, epoch, n, policy, view=0):
    """(n, policy.n_draws) uint32: the random numbers of every utterance 0 .. n-1 of the data set - a pure function of (seed, epoch,
    utterance index), like speed.draw_factors: one generator seeded from a string that names this augmentation, consumed in index order,
    n_draws numbers per utterance whatever they decide.  It never touches the loader's rng, and every data-parallel rank draws the same.
    view: 0 = the table of a one-view loader; 1 = the independent table of the second view of CR-CTC training (BucketedWaveLoader(views=2)),
    from a generator whose string also names the view."""
    if view not in (0, 1) or isinstance(view, bool):
        raise ValueError(f"specaug.draw: view={view!r} (0 or 1)")
    rng = random.Random(f"spec_augment/{int(seed)}/{int(epoch)}" + (f"/view{int(view)}" if view else ""))
    k = policy.n_draws
    bits = rng.getrandbits(32 * n * k) if n else 0      # the same words as n k calls of getrandbits(32): each takes one generator word
    return np.frombuffer(bits.to_bytes(4 * n * k, "little"), dtype="<u4").astype(np.uint32).reshape(n, k)


def resolve(policy, d, T, F, out=None):
    """The int32 row of an utterance of T frames and F bins from its numbers d (n_draws of them).  Integer arithmetic only; every range
    lies inside the utterance (an empty one is (0, 0)), so the kernels' clamps change nothing."""
    T, F, W = int(T), int(F), policy.warp
    d = [int(v) for v in d]
    row = np.zeros(policy.width, dtype=np.int32) if out is None else out
    row[:] = 0
    if W > 0 and T - 2 * W > 0:
        row[0] = W + d[0] % (T - 2 * W)
        row[1] = int(row[0]) - W + 1 + d[1] % (2 * W)
    k = 2
    cap = min(policy.max_t, T * policy.t_permille // 1000)
    for _ in range(policy.n_t):
        if T > 0 and cap > 0:
            row[k] = d[k] % T
            row[k + 1] = min(T, int(row[k]) + 1 + d[k + 1] % cap)
        k += 2
    for _ in range(policy.n_f):
        row[k] = d[k] % F
        row[k + 1] = min(F, int(row[k]) + 1 + d[k + 1] % policy.max_f)
        k += 2
    for _ in range(policy.n_s):
        if T > 0:
            s = d[k] % T
            row[k], row[k + 1], row[k + 2] = s, min(T, s + 1 + d[k + 1] % policy.sub_t), d[k + 2] % (s + 1)
        k += 3
    return row


def resolve_batch(policy, draws, frames, F):
    """(len(frames), policy.width) int32: resolve() for each utterance of a batch; draws: its rows of draw()'s table."""
    rows = np.zeros((len(frames), policy.width), dtype=np.int32)
    for r, T in enumerate(frames):
        resolve(policy, draws[r], T, F, out=rows[r])
    return rows
