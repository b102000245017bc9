"""Host restatement of the engine's dropout masks (csrc/asr_common.h: drop_hash / drop_keep / drop_keep_at / drop_thr16), in numpy.

The engine draws no random numbers: every element's keep bit is a pure function of (element counter, seed), and the backward pass
regenerates the mask of its forward pass from the same two numbers.  One 32-bit hash covers a PAIR of elements (counter >> 1): the low
16 bits decide the even element, the high 16 bits the odd one; an element is kept when its 16 bits are >= thr16 = round(p * 65536).
Kept elements are scaled by 1 / (1 - p) (the engine's scale; not 1 / (1 - thr16 / 65536)).

Counters:
  * LayerNorm / embedding sites (csrc/ln.hip, csrc/misc.hip embed): row * d + c over the (rows, d) activation.
  * attention probabilities (csrc/sdpa.hip): ((b * H + h) * Tq + q) * ((Tk + 1) & ~1) + k - each query row's stride is padded to an
    even number of keys, so a pair never straddles two rows.
"""
import numpy as np

_M1, _M2 = 0x2C1B3D, 0x297A2D


def umul24(a, b):
    """__umul24: the low 32 bits of the product of the low 24 bits of a and b."""
    a = np.asarray(a, dtype=np.uint64) & np.uint64(0xFFFFFF)
    b = np.uint64(b & 0xFFFFFF)
    return ((a * b) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def drop_hash(pair, seed):
    h = np.asarray(pair, dtype=np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)
    h = h ^ (h >> np.uint32(15))
    h = umul24(h, _M1)
    h = h ^ (h >> np.uint32(13))
    h = umul24(h, _M2)
    return h ^ (h >> np.uint32(16))


def drop_thr16(p):
    """(uint32_t)(p * 65536.f + 0.5f) in fp32, p as the kernels receive it (a C float); 0 for p <= 0."""
    p = np.float32(p)
    if p <= 0:
        return 0
    return int(np.float32(p * np.float32(65536.0) + np.float32(0.5)))


def drop_keep(h, half, thr16):
    return ((np.asarray(h, dtype=np.uint32) >> np.uint32(16 * half)) & np.uint32(0xFFFF)) >= np.uint32(thr16)


def drop_keep_at(elem, seed, thr16):
    elem = np.asarray(elem, dtype=np.uint32)
    h = drop_hash(elem >> np.uint32(1), seed)
    return ((h >> (np.uint32(16) * (elem & np.uint32(1)))) & np.uint32(0xFFFF)) >= np.uint32(thr16)


def keep_bits(rows, cols, p, seed, stride=None):
    """(rows, cols) bool keep mask with element counter r * stride + c (stride defaults to cols)."""
    stride = cols if stride is None else stride
    r = np.arange(rows, dtype=np.uint64).reshape(-1, 1)
    c = np.arange(cols, dtype=np.uint64).reshape(1, -1)
    elem = ((r * np.uint64(stride) + c) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return drop_keep_at(elem, seed, drop_thr16(p))


def _scaled(keep, p):
    return keep.astype(np.float64) / (1.0 - float(p)) if p > 0 else np.ones(keep.shape)


def ln_mask(rows, d, p, seed):
    """Scaled keep mask (rows, d) of a LayerNorm / embedding dropout site: counter row * d + c."""
    return _scaled(keep_bits(rows, d, p, seed), p)


def sdpa_mask(B, H, Tq, Tk, p, seed, stride=None):
    """Scaled keep mask (B, H, Tq, Tk) of an attention-probability site: counter ((b*H+h)*Tq+q) * ((Tk+1) & ~1) + k.
    `stride` overrides the padded row stride (negative controls only)."""
    stride = ((Tk + 1) & ~1) if stride is None else stride
    return _scaled(keep_bits(B * H * Tq, Tk, p, seed, stride), p).reshape(B, H, Tq, Tk)


def swap_pair_halves(mask):
    """The mask with the two elements of every (even, odd) column pair exchanged (a negative control: the halves of each hash swapped).
    An odd last column has no partner and stays."""
    m = np.array(mask, copy=True)
    n = m.shape[-1] // 2 * 2
    m[..., 0:n:2], m[..., 1:n:2] = mask[..., 1:n:2], mask[..., 0:n:2]
    return m


def engine_site_seed(step_seed, site):
    """Engine._drop's per-site seed (asr_chinese_e2e_amd/engine.py), restated."""
    return (step_seed * 0x9E3779B1 + site * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF
