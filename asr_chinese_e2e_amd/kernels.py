"""Tensor-level wrappers over the C ABI: each takes torch CUDA tensors, checks what the kernel
assumes (device, dtype, contiguity, shapes) ON THE HOST before launching, and passes raw device
pointers + the current HIP stream.  PyTorch is only the allocator / stream provider here.
"""
import math
import threading
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import ASR_BF16, ASR_F32, ACT_NONE, ACT_RELU, LN_REDUCE_MAX, TN_GROUP_MAX, LnReduceItem, TnProblem, check
from ._lib import fast as lib      # vectorcall trampolines into the C ABI (_lib.py); pointers and stream handles are plain ints

_DT = {torch.float32: ASR_F32, torch.bfloat16: ASR_BF16}


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype} (float32 or bfloat16)")


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")
    return t.data_ptr()


_DEV_INDEX = None
_TLS = threading.local()   # .own_stream = True on a helper thread (the loader's): its launches never follow STREAM_OVERRIDE, which the
                           # training thread sets around ITS side-stream launches
STREAM_OVERRIDE = None     # raw stream handle (int) the next launches go to instead of torch's current stream:
                           # the engine sets it around its side-stream launches of own kernels, which saves the
                           # `with torch.cuda.stream(...)` context switch (~6 us of host time, 25 times per step)


def _stream():
    """Raw handle of torch's current stream.  torch.cuda.current_stream() builds a Stream object and
    resolves the device index through several Python layers (~8 us, ~160 calls per step); the
    private raw getter is a single C call."""
    global _DEV_INDEX
    if STREAM_OVERRIDE is not None and not getattr(_TLS, "own_stream", False):
        return STREAM_OVERRIDE
    if _DEV_INDEX is None:
        _DEV_INDEX = torch.cuda.current_device()   # one process per GPU: bind_device() (engine construction) or the first launch sets it
    return torch._C._cuda_getCurrentRawStream(_DEV_INDEX)


def stream_fork(to_stream_handle, from_stream_handle=None):
    """Work queued on `to` from now on runs after what is queued on `from` (default: torch's current stream) so far.
    Raw stream handles (ints); ~2 us of host time against ~12 us for torch.cuda.Event record + wait."""
    frm = _stream() if from_stream_handle is None else from_stream_handle
    check(lib.asr_stream_fork(frm, to_stream_handle), "asr_stream_fork")


def stream_arm(to_stream_handle, from_stream_handle=None):
    """The next armed-capable entry point (include/asr_hip.h: asr_stream_arm) signals `to` from its last kernel on `from`."""
    frm = _stream() if from_stream_handle is None else from_stream_handle
    check(lib.asr_stream_arm(frm, to_stream_handle), "asr_stream_arm")


def stream_arm_pending():
    """True when the arm was NOT taken by a launch (cleared either way): fall back to stream_fork."""
    return bool(lib.asr_stream_arm_pending())


def bind_device(device):
    """One process drives ONE GPU: the launch stream is looked up on this device from now on.  Called when a model
    builds its engine; a model on a device other than torch's current one is refused (its kernels would be issued
    on the current device's stream against the other device's memory)."""
    global _DEV_INDEX
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    if idx != torch.cuda.current_device():
        raise RuntimeError(f"the model lives on cuda:{idx} but torch's current device is cuda:{torch.cuda.current_device()}: call "
                           f"torch.cuda.set_device({idx}) first (one process per GPU)")
    if _DEV_INDEX is not None and _DEV_INDEX != idx:
        raise RuntimeError(f"this process already launches on cuda:{_DEV_INDEX}; a second GPU (cuda:{idx}) needs its own process")
    _DEV_INDEX = idx


def _chk_f32(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("expected a contiguous float32 tensor")


def _chk_i32(*ts):
    for t in ts:
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError("expected a contiguous int32 tensor")


class LaunchTimer:
    """HIP-event timing of selected launches on the stream they are issued on (bench.py's roofline / kernels
    legs).  `work` is the algorithmic FLOP count of the launch, `nbytes` its algorithmic HBM bytes (0 = not stated)."""

    def __init__(self, names):
        self.names = set(names)
        self.rec = {n: [] for n in names}

    def run(self, name, work, fn, nbytes=0.0):
        if name not in self.names:
            return fn()
        st = torch.cuda.ExternalStream(STREAM_OVERRIDE) if STREAM_OVERRIDE is not None else None   # side-stream launches: record there
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st) if st is not None else e0.record()
        out = fn()
        e1.record(st) if st is not None else e1.record()
        self.rec[name].append((e0, e1, work, nbytes))
        return out

    def summary(self):
        """name -> dict(launches, total_ms, avg_us, work_per_s, work_per_launch, bytes_per_s, bytes_per_launch)
        (call after a device sync)."""
        out = {}
        for n, r in self.rec.items():
            if not r:
                continue
            ms = [a.elapsed_time(b) for a, b, _, _ in r]
            tot, work, nb = sum(ms), sum(x[2] for x in r), sum(x[3] for x in r)
            sec = tot * 1e-3
            out[n] = dict(launches=len(r), total_ms=tot, avg_us=1e3 * tot / len(r), work_per_s=work / sec if tot > 0 else 0.0,
                          work_per_launch=work / len(r), bytes_per_s=nb / sec if tot > 0 else 0.0, bytes_per_launch=nb / len(r))
        return out


TIMER = None   # set to a LaunchTimer by bench.py


def timed(name, work, fn, nbytes=0.0):
    if TIMER is None:
        return fn()
    return TIMER.run(name, work, fn, nbytes)


class Workspace:
    """Grow-only scratch buffer (never shrinks, so pointers stay valid under graph replay once
    the high-water mark has been reached during warm-up)."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes):
        nbytes = max(int(nbytes), 16)
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self.buf


# --------------------------------------------------------------------------------- LayerNorm
def add_ln_fwd(x, res, gamma, beta, pe, lens, B, T, y=None, xhat=None, rstd=None, drop_p=0.0, drop_seed=0, drop_mode=0):
    """y = LN(x + res) * gamma + beta (+ pe[t]), rows t >= lens[b] zeroed.  xhat may alias x.
    drop_mode 1: dropout on x before the residual add; 2: dropout on the output."""
    d = x.shape[-1]
    assert x.is_contiguous() and x.numel() == B * T * d
    if res is not None:
        assert res.is_contiguous() and res.shape == x.shape and res.dtype == x.dtype
    _chk_f32(gamma, beta, pe)
    _chk_i32(lens)
    assert gamma.numel() == d and beta.numel() == d
    if pe is not None:
        assert pe.shape[-1] == d and pe.shape[-2] >= T
    if lens is not None:
        assert lens.numel() == B
    y = torch.empty_like(x) if y is None else y
    xhat = torch.empty_like(x) if xhat is None else xhat
    rstd = torch.empty(B * T, dtype=torch.float32, device=x.device) if rstd is None else rstd
    nb = (3 + (res is not None)) * x.numel() * x.element_size()      # x, (res), y, xhat: SURVEY 8(d) "LN/add/mask"
    timed("add_ln_fwd", 0.0, lambda: check(
        lib.asr_add_ln_fwd(_p(x), _p(res), _p(gamma), _p(beta), _p(pe), _p(lens), _p(y), _p(xhat), _p(rstd),
                           B, T, d, float(drop_p), int(drop_seed) & 0xFFFFFFFF, int(drop_mode), _dt(x), _stream()), "asr_add_ln_fwd"), nb)
    return y, xhat, rstd


def add_ln_bwd(dy, dy2, xhat, rstd, gamma, lens, dgamma, dbeta, dbias, B, T, ws, dz=None, drop_p=0.0, drop_seed=0, drop_mode=0,
               partials=None):
    """Returns (dz, dx): dz = gradient wrt the residual input; dx = gradient wrt x (the same tensor
    unless pre-residual dropout is active, then dz * keep / (1-p)).
    partials: a uint8 buffer of add_ln_bwd_workspace_bytes(B * T, d) that receives the per-workgroup partial sums of
    the parameter gradients INSTEAD of their reduction into dgamma / dbeta / dbias; the caller reduces several
    sites at once with add_ln_bwd_reduce_batched."""
    d = dy.shape[-1]
    assert dy.is_contiguous() and xhat.is_contiguous() and dy.numel() == B * T * d == xhat.numel()
    assert xhat.dtype == dy.dtype and (dy2 is None or (dy2.dtype == dy.dtype and dy2.is_contiguous() and dy2.numel() == dy.numel()))
    _chk_f32(rstd, gamma, dgamma, dbeta, dbias)
    _chk_i32(lens)
    assert rstd.numel() == B * T and dgamma.numel() == d and dbeta.numel() == d and (dbias is None or dbias.numel() == d)
    dz = torch.empty_like(dy) if dz is None else dz
    dx = torch.empty_like(dy) if (drop_p > 0 and drop_mode == 1) else None
    nbytes = lib.asr_add_ln_bwd_workspace_bytes(B * T, d)
    if partials is not None:
        assert partials.dtype == torch.uint8 and partials.numel() >= nbytes
        w, dgamma, dbeta = partials, None, None
    else:
        w = ws.get(nbytes)
    nb = (3 + (dy2 is not None) + (dx is not None)) * dy.numel() * dy.element_size()     # dy, (dy2), xhat, dz, (dx)
    timed("add_ln_bwd", 0.0, lambda: check(
        lib.asr_add_ln_bwd(_p(dy), _p(dy2), _p(xhat), _p(rstd), _p(gamma), _p(lens), _p(dz), _p(dx), _p(dgamma), _p(dbeta),
                           _p(dbias), _p(w), w.numel(), B, T, d, float(drop_p), int(drop_seed) & 0xFFFFFFFF, int(drop_mode),
                           _dt(dy), _stream()), "asr_add_ln_bwd"), nb)
    return dz, (dx if dx is not None else dz)


def add_ln_bwd_workspace_bytes(rows, d):
    return lib.asr_add_ln_bwd_workspace_bytes(rows, d)


def add_ln_bwd_reduce_batched(items, d):
    """items: list of (partials, dgamma, dbeta, dbias or None, rows) left by add_ln_bwd(partials=...)."""
    for i in range(0, len(items), LN_REDUCE_MAX):
        chunk = items[i:i + LN_REDUCE_MAX]
        arr = (LnReduceItem * len(chunk))()
        for q, (part, dg, db, dbias, rows) in zip(arr, chunk):
            _chk_f32(dg, db, dbias)
            assert dg.numel() == d and db.numel() == d and (dbias is None or dbias.numel() == d)
            assert part.numel() >= lib.asr_add_ln_bwd_workspace_bytes(rows, d)
            q.ws, q.dgamma, q.dbeta, q.dbias, q.rows = _p(part), _p(dg), _p(db), _p(dbias), rows
        check(lib.asr_add_ln_bwd_reduce_batched(ctypes.addressof(arr), len(chunk), d, _stream()), "asr_add_ln_bwd_reduce_batched")


# --------------------------------------------------------------------------------- attention
def _strided_rows(t, H, dk):
    """t is a (rows, >=H*dk) view whose last dim is contiguous; returns row stride in elements."""
    assert t.dim() == 2 and t.stride(1) == 1 and t.shape[1] == H * dk
    return t.stride(0)


def _sdpa_entries(name):
    return (getattr(lib, name + "_fwd"), name + "_fwd"), (getattr(lib, name + "_bwd"), name + "_bwd"), getattr(lib, name + "_bwd_workspace_bytes")


_SDPA_PLAIN, _SDPA_CHUNK = _sdpa_entries("asr_sdpa"), _sdpa_entries("asr_sdpa_chunk")


def _sdpa_mask(causal, window, chunk, left_chunks):
    """The entry points of a mask and the two integers they take for it: ((fwd, its name), (bwd, its name), workspace_bytes, a, b).
    chunk > 0 is the chunk mask of asr_sdpa_chunk_*, which replaces causal / window."""
    if chunk > 0:
        assert not causal and window < 0, "a chunk mask replaces causal / window"
        return *_SDPA_CHUNK, int(chunk), int(left_chunks)
    return *_SDPA_PLAIN, int(causal), int(window)


def sdpa_fwd(q, k, v, k_len, B, H, Tq, Tk, dk, causal=False, window=-1, scale=None, o=None, lse=None, drop_p=0.0, drop_seed=0, o_lo=None,
             chunk=0, left_chunks=-1):
    """q: (B*Tq, H*dk) view, k/v: (B*Tk, H*dk) views (may be column slices of a fused buffer).
    o_lo: a tensor of o's shape and strides for the low-order piece of the bf16 output (asr_hip.h; hand it to sdpa_bwd), or None.
    chunk > 0: the chunk mask of asr_sdpa_chunk_fwd (chunk frames, left_chunks chunks of left context, -1 = all) instead of
    causal / window, which must then be off."""
    ldq, ldk, ldv = _strided_rows(q, H, dk), _strided_rows(k, H, dk), _strided_rows(v, H, dk)
    assert q.shape[0] == B * Tq and k.shape[0] == B * Tk and v.shape[0] == B * Tk
    assert q.dtype == k.dtype == v.dtype
    _chk_i32(k_len)
    assert k_len is None or k_len.numel() == B
    o = torch.empty(B * Tq, H * dk, dtype=q.dtype, device=q.device) if o is None else o
    ldo = _strided_rows(o, H, dk)
    lse = torch.empty(B, H, Tq, dtype=torch.float32, device=q.device) if lse is None else lse
    assert o_lo is None or (o_lo.dtype == o.dtype == torch.bfloat16 and o_lo.shape == o.shape and o_lo.stride() == o.stride())
    scale = float(dk) ** -0.5 if scale is None else float(scale)
    e = q.element_size()
    (fwd, name), _, _, a, b = _sdpa_mask(causal, window, chunk, left_chunks)
    timed("sdpa_fwd", 4.0 * B * H * Tq * Tk * dk, lambda: check(
        fwd(_p(q), _p(k), _p(v), _p(o), _p(lse), _p(k_len), B, H, Tq, Tk, dk, ldq, ldk, ldv, ldo,
            a, b, scale, float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(o_lo), _dt(q), _stream()), name),
          2.0 * B * H * (Tq + Tk) * dk * e)          # Q, O + K, V (4 B H T dk e at Tq = Tk)
    return o, lse


def sdpa_bwd(q, k, v, o, do, lse, k_len, B, H, Tq, Tk, dk, dq, dk_, dv, causal=False, window=-1, scale=None, delta=None,
             drop_p=0.0, drop_seed=0, o_lo=None, chunk=0, left_chunks=-1):
    ldq, ldk, ldv, ldo = (_strided_rows(t, H, dk) for t in (q, k, v, o))
    assert _strided_rows(do, H, dk) == ldo and _strided_rows(dq, H, dk) == ldq
    assert _strided_rows(dk_, H, dk) == ldk and _strided_rows(dv, H, dk) == ldv
    assert q.dtype == k.dtype == v.dtype == o.dtype == do.dtype == dq.dtype == dk_.dtype == dv.dtype
    _chk_i32(k_len)
    _chk_f32(lse)
    assert o_lo is None or (o_lo.dtype == o.dtype == torch.bfloat16 and o_lo.shape == o.shape and o_lo.stride() == o.stride())
    _, (bwd, name), workspace_bytes, a, b = _sdpa_mask(causal, window, chunk, left_chunks)
    if delta is None:      # scratch: row sums of dO o O, or the band kernel's dQ partials of the tiles on a key-block boundary
        need = workspace_bytes(B, H, Tq, Tk, dk, a, b, _dt(q))
        delta = torch.empty((need + 3) // 4, dtype=torch.float32, device=q.device)
    scale = float(dk) ** -0.5 if scale is None else float(scale)
    e = q.element_size()
    timed("sdpa_bwd", 10.0 * B * H * Tq * Tk * dk, lambda: check(
        bwd(_p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(delta), delta.numel() * 4, _p(dq), _p(dk_), _p(dv), _p(k_len),
            B, H, Tq, Tk, dk, ldq, ldk, ldv, ldo, a, b, scale, float(drop_p),
            int(drop_seed) & 0xFFFFFFFF, _p(o_lo), _dt(q), _stream()), name),
          B * H * (4.0 * Tq + 4.0 * Tk) * dk * e)    # Q, O, dO, dQ + K, V, dK, dV (8 x 16.4 MB at config 2); 5 products
    return dq, dk_, dv


# --------------------------------------------------------------------------------- losses
def _frame_rows(logits):
    """Row stride (elements) of a (B, T, V) tensor of frames: dense, or a view of rows padded to `ld` >= V elements."""
    B, T, V = logits.shape
    ld = logits.stride(1) if B * T > 1 else V
    assert logits.stride(2) == 1 and ld >= V and (B == 1 or logits.stride(0) == T * ld), f"frames must be rows of one (B*T, ld) buffer: {logits.stride()}"
    return ld


def ctc_fwd_bwd(logits, in_len, labels, lab_len, ws, blank=0, grad_scale=1.0, zero_infinity=False, dlogits=None,
                want_grad=True, nll=None, grad_scale_div=None, best_path=None):
    """logits (B,T,V); returns (nll (B,), dlogits or None).  dlogits may alias logits.
    grad_scale_div: optional 1-element f32 device tensor; the gradient scale is then grad_scale / grad_scale_div[0].
    best_path: optional (B, T) int32 tensor that receives the frame-wise argmax of the logits (the greedy CTC path; see ctc_collapse)."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len, labels, lab_len)
    Lmax = labels.shape[1]
    assert labels.shape[0] == B and in_len.numel() == B and lab_len.numel() == B
    nll = torch.empty(B, dtype=torch.float32, device=logits.device) if nll is None else nll
    if want_grad and dlogits is None:
        dlogits = torch.empty_strided(logits.shape, logits.stride(), dtype=logits.dtype, device=logits.device)
    if dlogits is not None:
        assert dlogits.shape == logits.shape and dlogits.stride() == logits.stride() and dlogits.dtype == logits.dtype
    w = ws.get(lib.asr_ctc_workspace_bytes(B, T, Lmax))
    _chk_f32(grad_scale_div)
    _chk_i32(best_path)
    assert best_path is None or best_path.numel() == B * T
    timed("ctc", 0.0, lambda: check(
        lib.asr_ctc_fwd_bwd(_p(logits), _p(dlogits), _p(in_len), _p(labels), _p(lab_len), _p(nll), B, T, V, ld, Lmax,
                            int(blank), float(grad_scale), _p(grad_scale_div), int(zero_infinity), _p(best_path), _p(w), w.numel(), _dt(logits), _stream()),
        "asr_ctc_fwd_bwd"), (3.0 if dlogits is not None else 1.0) * logits.numel() * logits.element_size())   # 3 B T V e

    return nll, dlogits


def ctc_align(logits, in_len, labels, lab_len, blank=0, ws=None):
    """CTC forced alignment (Viterbi, asr_ctc_align): the best single path of each utterance's labels through its frames.
    logits (B, T, V) f32 / bf16, dense or rows padded as the engine lays them out; in_len (B,), labels (B, Lmax) with every entry
    (padding included) a class id in [0, V), lab_len (B,): int32 on the device.  Lmax <= 255; Lmax = 0 is allowed.
    Returns (path (B, T) int32: token id per frame, `blank` on blank frames, -1 past in_len; spans (B, Lmax, 2) int32: first and last
    frame of each token, -1 past lab_len; token_logp (B, Lmax) f32: sum of log softmax over a token's frames; score (B,) f32:
    log-probability of the best path, -inf when the labels cannot be aligned in the frames).  Semantics: include/asr_hip.h."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len, labels, lab_len)
    assert labels.dim() == 2 and labels.shape[0] == B and in_len.numel() == B and lab_len.numel() == B
    Lmax = labels.shape[1]
    dev = logits.device
    lab = labels if Lmax > 0 else torch.zeros(B, 1, dtype=torch.int32, device=dev)     # the entry point takes Lmax >= 1
    La = lab.shape[1]
    path = torch.empty(B, T, dtype=torch.int32, device=dev)
    spans = torch.empty(B, La, 2, dtype=torch.int32, device=dev)
    token_logp = torch.empty(B, La, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    nbytes = lib.asr_ctc_align_workspace_bytes(B, T, La)
    w = ws.get(nbytes) if ws is not None else torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    timed("ctc_align", 0.0, lambda: check(
        lib.asr_ctc_align(_p(logits), _p(in_len), _p(lab), _p(lab_len), _p(path), _p(spans), _p(token_logp), _p(score), B, T, V, ld, La,
                          int(blank), _p(w), w.numel(), _dt(logits), _stream()),
        "asr_ctc_align"), logits.numel() * logits.element_size())
    return path, spans[:, :Lmax], token_logp[:, :Lmax], score


def ctc_greedy_decode(logits, in_len, blank=0):
    """logits (B,T,V) -> (ids (B,T) int32, collapsed and 0-padded; lens (B,) int32)."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len)
    ids = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    lens = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(lib.asr_ctc_greedy_decode(_p(logits), _p(in_len), _p(ids), _p(lens), B, T, V, ld, int(blank), _dt(logits), _stream()),
          "asr_ctc_greedy_decode")
    return ids, lens


def ctc_frame_argmax(logits, in_len, blank=0):
    """logits (B,T,V) -> the frame-wise best path (B, T) int32 (frames t >= in_len[b] as asr_ctc_frame_argmax leaves them)."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len)
    path = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    check(lib.asr_ctc_frame_argmax(_p(logits), _p(in_len), _p(path), B, T, V, ld, int(blank), _dt(logits), _stream()), "asr_ctc_frame_argmax")
    return path


def ctc_collapse(path, in_len, blank=0):
    """CTC collapse IN PLACE of a frame-wise best path (B, T) int32 (ctc_fwd_bwd's best_path): repeats merged, blanks dropped, 0-padded.
    Returns (path, lens (B,) int32)."""
    B, T = path.shape
    _chk_i32(path, in_len)
    lens = torch.empty(B, dtype=torch.int32, device=path.device)
    check(lib.asr_ctc_collapse(_p(path), _p(in_len), _p(lens), B, T, int(blank), _stream()), "asr_ctc_collapse")
    return path, lens


def decode_attn(q, k, v, H, dk, Tk_cap, kv_div=1, k_len=None, k_len_uniform=0, len_div=1, scale=None, o=None):
    """Single-query attention of R = q.shape[0] rows over cached keys/values (see include/asr_hip.h)."""
    R = q.shape[0]
    ldq, ldk, ldv = _strided_rows(q, H, dk), _strided_rows(k, H, dk), _strided_rows(v, H, dk)
    assert q.dtype == k.dtype == v.dtype
    _chk_i32(k_len)
    o = torch.empty(R, H * dk, dtype=q.dtype, device=q.device) if o is None else o
    scale = float(dk) ** -0.5 if scale is None else float(scale)
    check(lib.asr_decode_attn(_p(q), _p(k), _p(v), _p(o), _p(k_len), int(k_len_uniform), int(len_div), R, H, dk, int(Tk_cap), int(kv_div),
                              ldq, ldk, ldv, _strided_rows(o, H, dk), scale, _dt(q), _stream()), "asr_decode_attn")
    return o


def logsoftmax_topk(logits, beam):
    R, V = logits.shape
    assert logits.stride(1) == 1
    vals = torch.empty(R, beam, dtype=torch.float32, device=logits.device)
    ids = torch.empty(R, beam, dtype=torch.int32, device=logits.device)
    check(lib.asr_logsoftmax_topk(_p(logits), _p(vals), _p(ids), R, V, logits.stride(0), int(beam), _dt(logits), _stream()), "asr_logsoftmax_topk")
    return vals, ids


def ctc_frame_topk(logits, k, blank=0):
    """logits (R, V) -> (vals (R, k) f32 log_softmax of the k best classes per frame, ids (R, k) int32, blank_lp (R) f32)."""
    R, V = logits.shape
    assert logits.stride(1) == 1
    vals = torch.empty(R, k, dtype=torch.float32, device=logits.device)
    ids = torch.empty(R, k, dtype=torch.int32, device=logits.device)
    blank_lp = torch.empty(R, dtype=torch.float32, device=logits.device)
    check(lib.asr_ctc_frame_topk(_p(logits), _p(vals), _p(ids), _p(blank_lp), R, V, logits.stride(0), int(k), int(blank), _dt(logits), _stream()),
          "asr_ctc_frame_topk")
    return vals, ids, blank_lp


def _context_roots(context, roots, B, device):
    """The per-utterance roots of a ContextGraph as host ints and as an int32 device tensor (roots=None: graph 0 for all)."""
    host = [context.root(0)] * B if roots is None else [int(r) for r in roots]
    if len(host) != B or any(r < -1 or r >= context.S for r in host):
        raise ValueError(f"context roots must hold {B} states in [-1, {context.S}), got {host}")
    return host, torch.tensor(host, dtype=torch.int32, device=device)


def _no_lm_with_context(lm, context):
    if lm is not None and context is not None:
        raise ValueError("an n-gram LM (lm=...) and a hotword context (context=...) cannot be combined: the search runs one of the two")


def _no_times_with_bias(times, context, lm):
    if times and (context is not None or lm is not None):
        raise ValueError("token times of the prefix beam search (beam_times) are not combined with a hotword context or an n-gram LM: the plain search carries them")


# The four modes of the CTC prefix beam search (csrc/prefix_beam.hip), a row each: the suffix of its entry points (asr_ctc_prefix_beam<sfx>,
# asr_ctc_prefix_beam_chunk<sfx>, asr_ctc_prefix_beam<sfx>_state_init / _reset), its size queries (offline workspace, resumable workspace,
# state) and the outputs it adds to the plain search's as (name, dtype, kind) in the order of the packed result.
_PB_ENTRY, _PB_TOKEN, _PB_UTT = "entry", "token", "utterance"      # an output's shape: (B, nbest), (B, nbest, Lcap), (B)
_PB_PLAIN_OUT = (("tok", torch.int32, _PB_TOKEN), ("len", torch.int32, _PB_ENTRY), ("score", torch.float32, _PB_ENTRY), ("stable", torch.int32, _PB_UTT))
_PB_BIAS_OUT = (("bias", torch.float64, _PB_ENTRY), ("state", torch.int32, _PB_ENTRY))
_PB_TIMES_OUT = (("vit", torch.float64, _PB_ENTRY), ("start", torch.int32, _PB_TOKEN), ("end", torch.int32, _PB_TOKEN), ("mx", torch.float32, _PB_TOKEN),
                 ("mn", torch.float32, _PB_TOKEN), ("sm", torch.float32, _PB_TOKEN), ("final", torch.int32, _PB_UTT))
_PB_MODES = {
    "plain": ("", lib.asr_ctc_prefix_beam_workspace_bytes, lib.asr_ctc_prefix_beam_stream_workspace_bytes, lib.asr_ctc_prefix_beam_state_bytes, ()),
    "ctx": ("_ctx", lib.asr_ctc_prefix_beam_workspace_bytes, lib.asr_ctc_prefix_beam_stream_workspace_bytes, lib.asr_ctc_prefix_beam_ctx_state_bytes, _PB_BIAS_OUT),
    "lm": ("_lm", lib.asr_ctc_prefix_beam_lm_workspace_bytes, lib.asr_ctc_prefix_beam_lm_workspace_bytes, lib.asr_ctc_prefix_beam_lm_state_bytes, _PB_BIAS_OUT),
    "timed": ("_timed", lib.asr_ctc_prefix_beam_timed_workspace_bytes, lib.asr_ctc_prefix_beam_timed_workspace_bytes, lib.asr_ctc_prefix_beam_timed_state_bytes,
              _PB_TIMES_OUT),
}


def _pb_mode(context=None, lm=None, times=False):
    """The row of _PB_MODES a search with these options runs."""
    _no_lm_with_context(lm, context)
    _no_times_with_bias(times, context, lm)
    return "timed" if times else "lm" if lm is not None else "ctx" if context is not None else "plain"


def _pb_tables(mode, context, lm, device):
    """The mode's table argument, [] or [the address of the ContextGraph's / NgramLM's struct of device tables] (the object keeps the struct)."""
    src = context if mode == "ctx" else lm if mode == "lm" else None
    return [] if src is None else [ctypes.addressof(src.on(device)[1])]


def _pb_call(name, *args):
    check(getattr(lib, name)(*args), name)


def prefix_beam_layout(B, nbest, Lcap, mode="plain"):
    """The packed int32 result of ctc_prefix_beam_chunk: ([(name, dtype, kind, shape, first word, words)], words in all).  The plain search's
    B * (nbest * (Lcap + 2) + 1) words: tok, len, score, stable; behind them the mode's own outputs, after one pad word if that count is odd
    (the first of them is fp64 and 8-aligned): ctx / lm: bias (2 words per entry), state; timed: vit (2 words per entry), start, end, mx, mn,
    sm (Lcap words per entry each), final (a word per utterance)."""
    shapes = {_PB_TOKEN: ((B, nbest, Lcap), B * nbest * Lcap), _PB_ENTRY: ((B, nbest), B * nbest), _PB_UTT: ((B,), B)}
    fields, n = [], 0
    for group in (_PB_PLAIN_OUT, _PB_MODES[mode][4]):
        if group:
            n += n & 1
        for name, dtype, kind in group:
            shape, words = shapes[kind]
            if dtype == torch.float64:
                words *= 2
            fields.append((name, dtype, kind, shape, n, words))
            n += words
    return fields, n


def _pb_views(buf, fields):
    """The fields of prefix_beam_layout as views of the int32 buffer that holds them."""
    out = []
    for _, dtype, _, shape, first, words in fields:
        v = buf[first:first + words]
        if dtype != torch.int32:
            v = v.view(dtype)
        out.append(v if len(shape) == 1 else v.view(shape))
    return tuple(out)


def prefix_beam_unpack(buf, B, nbest, Lcap, mode="plain"):
    """(tokens (B, nbest, Lcap) int32, lengths (B, nbest) int32, scores (B, nbest) f32, stable (B) int32) as views of the int32 buffer of
    B * (nbest * (Lcap + 2) + 1) words that ctc_prefix_beam_chunk fills (on the device or copied to the host).  mode "ctx" / "lm" / "timed":
    the buffer of that mode's state (prefix_beam_layout); the mode's outputs follow the four as views too - (bias (B, nbest) float64,
    state (B, nbest) int32), or (vit (B, nbest) float64, start, end (B, nbest, Lcap) int32, mx, mn, sm (B, nbest, Lcap) float32, final (B) int32)."""
    fields, n = prefix_beam_layout(B, nbest, Lcap, mode)
    assert buf.dtype == torch.int32 and buf.numel() == n and buf.is_contiguous()
    return _pb_views(buf, fields)


def ctc_prefix_beam(vals, ids, blank_lp, in_len, B, T, beam, nbest, blank=0, max_len=None, context=None, roots=None, lm=None, times=False):
    """CTC prefix beam search on the device over the per-frame candidates of ctc_frame_topk (include/asr_hip.h).
    Returns (tokens (B, nbest, Lcap) int32, lengths (B, nbest) int32 with -1 for missing ranks, scores (B, nbest) float32).
    context (a context.ContextGraph): the hotword-biased search (asr_ctc_prefix_beam_ctx) - roots = the root state of each utterance's
    graph (-1: not biased; None: graph 0 for all); the result gains (bias (B, nbest) float64, the raw bias before held(state) is taken
    off, state (B, nbest) int32), and the entries are in the beam's rank order (log p + raw bias).
    lm (an lm.NgramLM): n-gram LM shallow fusion (asr_ctc_prefix_beam_lm); the result gains (bias (B, nbest) float64, the entries' LM bias
    without the end-of-sentence term, state (B, nbest) int32, their LM state), in the beam's rank order (log p + bias).  Not with a context.
    times=True (the plain search only): asr_ctc_prefix_beam_timed; the result gains (vit (B, nbest) float64, the log-probability of each
    entry's best single alignment, and that alignment's records per token: start, end (B, nbest, Lcap) int32 frames, mx, mn, sm (B, nbest,
    Lcap) float32 - the largest, smallest and summed log-posterior over the token's run); positions past an entry's length are zero."""
    mode = _pb_mode(context, lm, times)
    sfx, ws_bytes = _PB_MODES[mode][:2]
    k = vals.shape[1]
    assert vals.shape == (B * T, k) and ids.shape == (B * T, k) and blank_lp.numel() == B * T
    _chk_f32(vals, blank_lp)
    _chk_i32(ids, in_len)
    Lcap = int(T if max_len is None else max_len)
    dev = vals.device
    ws = torch.empty(ws_bytes(B, T, beam), dtype=torch.uint8, device=dev)
    # the per-utterance outputs (stable, final) are the resumable search's; per-token outputs are zero past an entry's length
    outs = [(torch.zeros if kind == _PB_TOKEN else torch.empty)(shape, dtype=dtype, device=dev)
            for _, dtype, kind, shape, _, _ in prefix_beam_layout(B, nbest, Lcap, mode)[0] if kind != _PB_UTT]
    lead = [_p(_context_roots(context, roots, B, dev)[1])] if mode == "ctx" else []
    _pb_call("asr_ctc_prefix_beam" + sfx, _p(vals), _p(ids), _p(blank_lp), _p(in_len), *lead, *_pb_tables(mode, context, lm, dev), _p(ws), ws.numel(),
             *(_p(t) for t in outs), B, T, k, int(beam), int(nbest), Lcap, int(blank), _stream())
    return tuple(outs)


class PrefixBeamState:
    """The resumable prefix beam search's device memory (include/asr_hip.h): `state` (the beam of each utterance between chunks) and
    `ws` (the trie, room for T_cap frames per utterance); `frames` = frames consumed per utterance, kept on the host so that a
    chunk past T_cap is refused before any launch.  context: the ContextGraph of a context state (None: a plain state) - a context state
    is larger (bias, context state and root per utterance) and only ever reaches the _ctx entry points.  lm: the NgramLM of an LM state
    (bias and LM state per entry), which only ever reaches the _lm entry points.  times: a timed state (the entries' best single alignments
    and a second trie for their records), which only ever reaches the _timed entry points.  mode: the state's row of the mode table."""

    def __init__(self, state, ws, B, beam, T_cap, context=None, roots=None, lm=None, times=False):
        self.state, self.ws, self.B, self.beam, self.T_cap = state, ws, B, beam, T_cap
        self.frames = [0] * B
        self.context, self.roots, self.lm, self.times = context, roots, lm, bool(times)
        self.mode = _pb_mode(context, lm, times)


def ctc_prefix_beam_state(B, beam, T_cap, device="cuda", context=None, roots=None, lm=None, times=False):
    """A fresh PrefixBeamState: the empty-prefix beam for B utterances of at most T_cap frames each.  context / roots: a context
    state for the hotword-biased search (roots as ctc_prefix_beam's).  lm: an LM state, every utterance on the LM's start state.
    times: a timed state (asr_ctc_prefix_beam_chunk_timed); its workspace holds both tries, 10 words per node."""
    mode = _pb_mode(context, lm, times)
    sfx, _, ws_bytes, state_bytes, _ = _PB_MODES[mode]
    B, beam, T_cap = int(B), int(beam), int(T_cap)
    if B < 1 or beam < 1 or T_cap < 1:
        raise ValueError(f"ctc_prefix_beam_state: B, beam and T_cap must be >= 1 (got {B}, {beam}, {T_cap})")
    host, root_dev = _context_roots(context, roots, B, device) if mode == "ctx" else (None, None)
    state = torch.zeros(state_bytes(B, beam) // 8, dtype=torch.int64, device=device)      # 8-aligned
    ws = torch.empty(ws_bytes(B, T_cap, beam), dtype=torch.uint8, device=device)
    # a context state takes its roots (the graph reaches the chunks), an LM state the LM (for its start state)
    lead = [_p(root_dev)] if mode == "ctx" else _pb_tables(mode, context, lm, device)
    _pb_call(f"asr_ctc_prefix_beam{sfx}_state_init", _p(state), _p(ws), *lead, B, beam, T_cap, _stream())
    return PrefixBeamState(state, ws, B, beam, T_cap, context, host, lm, times)


def ctc_prefix_beam_chunk(st, vals, ids, blank_lp, n_valid, C, nbest, blank=0, max_len=None, packed=False, nv_dev=None, extra_words=0):
    """One chunk of the resumable search: vals / ids (B*C, k), blank_lp (B*C) = the chunk's rows of ctc_frame_topk; n_valid = the
    frames of each utterance to consume (a list of B ints in [0, C]).  A chunk that would take an utterance past st.T_cap frames raises
    before anything is launched.  Returns (tokens (B, nbest, Lcap) int32, lengths (B, nbest) int32 with -1 for missing ranks, scores
    (B, nbest) f32, stable (B) int32 = the length of the prefix every beam entry shares) - views of one int32 buffer (prefix_beam_unpack);
    packed=True returns (that buffer, Lcap) instead, so that one copy brings all four to the host.  Lcap = max_len, by default the most
    frames any utterance has consumed after this chunk: no prefix is longer than that.  nv_dev: n_valid as an int32 device tensor the
    caller has uploaded already; extra_words (packed only): int32 words left free behind the results in the returned buffer, for
    what else travels to the host in the same copy.
    A context state (st.context): the biased search (asr_ctc_prefix_beam_chunk_ctx); the result gains bias (B, nbest) float64 (raw) and
    state (B, nbest) int32, and the packed buffer grows by them (prefix_beam_layout; prefix_beam_unpack(..., "ctx") reads all six).
    An LM state (st.lm): the search with the n-gram LM (asr_ctc_prefix_beam_chunk_lm); the same two additions, bias without the
    end-of-sentence term and the LM state.
    A timed state (st.times): asr_ctc_prefix_beam_chunk_timed; the result gains (vit, start, end, mx, mn, sm) as ctc_prefix_beam(times=True)
    and final (B) int32 = how many leading records of every list no later frame can change; the packed buffer grows by the seven."""
    B, beam, k = st.B, st.beam, vals.shape[1]
    C, nbest = int(C), int(nbest)
    nv = [int(x) for x in n_valid]
    if len(nv) != B or any(x < 0 or x > C for x in nv):
        raise ValueError(f"ctc_prefix_beam_chunk: n_valid must hold {B} values in [0, {C}], got {nv}")
    for b in range(B):
        if st.frames[b] + nv[b] > st.T_cap:
            raise ValueError(f"ctc_prefix_beam_chunk: utterance {b} would reach {st.frames[b] + nv[b]} frames, the trie holds {st.T_cap}")
    assert vals.shape == (B * C, k) and ids.shape == (B * C, k) and blank_lp.numel() == B * C
    _chk_f32(vals, blank_lp)
    _chk_i32(ids)
    Lcap = int(max(1, max(f + n for f, n in zip(st.frames, nv))) if max_len is None else max_len)
    fields, n_all = prefix_beam_layout(B, nbest, Lcap, st.mode)
    out = torch.zeros(n_all + (int(extra_words) if packed else 0), dtype=torch.int32, device=vals.device)
    views = _pb_views(out, fields)
    if nv_dev is None:
        nv_dev = torch.tensor(nv, dtype=torch.int32, device=vals.device)
    _chk_i32(nv_dev)
    assert nv_dev.numel() == B
    # the entry points take the per-utterance outputs (stable, final) behind the others
    outs = [_p(v) for f, v in zip(fields, views) if f[2] != _PB_UTT] + [_p(v) for f, v in zip(fields, views) if f[2] == _PB_UTT]
    _pb_call("asr_ctc_prefix_beam_chunk" + _PB_MODES[st.mode][0], _p(vals), _p(ids), _p(blank_lp), _p(nv_dev), _p(st.state), _p(st.ws), st.ws.numel(),
             *_pb_tables(st.mode, st.context, st.lm, vals.device), *outs, B, C, k, beam, nbest, Lcap, st.T_cap, int(blank), _stream())
    for b in range(B):
        st.frames[b] += nv[b]
    return (out, Lcap) if packed else views


def ctc_prefix_beam_state_reset(st, flags, slots=(), roots=None, lm=None):
    """Re-initialise the utterances of a PrefixBeamState whose flags[b] != 0 (flags: (B) int32 on the device; `slots`: the same
    utterances as host ints, for the host-side frame counters): byte for byte what ctc_prefix_beam_state leaves for them.
    A context state: roots = the B roots after the reset (those of the flagged utterances are applied; None: all as they are).
    An LM state: the flagged utterances restart on the LM's start state (lm, if given, is the state's own)."""
    _chk_i32(flags)
    assert flags.numel() == st.B
    if lm is not None and lm is not st.lm:
        raise ValueError("ctc_prefix_beam_state_reset: lm must be the NgramLM the state was made with (one LM serves every utterance)")
    if roots is not None and st.mode != "ctx":
        raise ValueError("ctc_prefix_beam_state_reset: roots apply to a context state")
    dev = st.state.device
    host, root_dev = _context_roots(st.context, st.roots if roots is None else roots, st.B, dev) if st.mode == "ctx" else (None, None)
    lead = [_p(root_dev)] if st.mode == "ctx" else _pb_tables(st.mode, st.context, st.lm, dev)      # as ctc_prefix_beam_state's
    _pb_call(f"asr_ctc_prefix_beam{_PB_MODES[st.mode][0]}_state_reset", _p(st.state), _p(st.ws), _p(flags), *lead, st.B, st.beam, st.T_cap, _stream())
    for b in slots:
        st.frames[int(b)] = 0
        if host is not None:
            st.roots[int(b)] = host[int(b)]


# --------------------------------------------------------------------------------- blank-frame skipping (csrc/blank_skip.hip)
def blank_skip_threshold(p):
    """The kernel argument of blank_skip=p: float32(log(float32(p))) as a Python float; p outside (0, 1] or not finite raises ValueError."""
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise ValueError(f"blank_skip must be a probability in (0, 1] (got {p!r})") from None
    if not (math.isfinite(p) and 0.0 < p <= 1.0):
        raise ValueError(f"blank_skip must be a probability in (0, 1] (got {p!r})")
    with np.errstate(divide="ignore"):      # a p below float32's range: log 0 = -inf, every frame with a posterior is high
        return float(np.float32(np.log(np.float32(p))))


class BlankSkipState:
    """The resumable compaction's device memory: `state` (B, 4) int32 {carry bit, frames seen, frames kept, 0} and `frame_map` (B, T_cap)
    int32, the real frame of every kept row so far (include/asr_hip.h: asr_ctc_blank_skip_compact)."""

    def __init__(self, B, T_cap, device):
        self.B, self.T_cap = int(B), int(T_cap)
        self.state = torch.zeros(self.B, 4, dtype=torch.int32, device=device)
        self.frame_map = torch.zeros(self.B, self.T_cap, dtype=torch.int32, device=device)


def ctc_blank_skip_compact(vals, ids, blank_lp, count, thr, B, T, st=None, reset=None):
    """Drop the frames whose blank log-posterior and whose predecessor's are above thr (asr_ctc_blank_skip_compact): vals / ids (B*T, k),
    blank_lp (B*T) from ctc_frame_topk, count (B) int32 on the device (None: T each), thr = blank_skip_threshold(p).  Returns (vals, ids,
    blank_lp in the same layout with the kept rows first, out_len (B) int32, frame_map) - frame_map (B, T) int32 = the frame of every
    kept row, zero behind them; with st (a BlankSkipState: the chunks of a stream, T = the chunk's rows) st.frame_map, extended by this
    chunk's kept rows.  reset (B) int32 on the device, with st: the flagged utterances start over before this chunk."""
    B, T, k = int(B), int(T), vals.shape[1]
    assert vals.shape == (B * T, k) and ids.shape == (B * T, k) and blank_lp.numel() == B * T
    assert vals.is_contiguous() and ids.is_contiguous() and blank_lp.is_contiguous()
    _chk_f32(vals, blank_lp)
    _chk_i32(ids, count, reset)
    assert (count is None or count.numel() == B) and (reset is None or (st is not None and reset.numel() == B)) and (st is None or st.B == B)
    dev = vals.device
    out_vals, out_ids, out_blank_lp = torch.empty_like(vals), torch.empty_like(ids), torch.empty_like(blank_lp)
    out_len = torch.zeros(B, dtype=torch.int32, device=dev)
    frame_map = torch.zeros(B, T, dtype=torch.int32, device=dev) if st is None else st.frame_map
    if B * T > 0:
        check(lib.asr_ctc_blank_skip_compact(_p(vals), _p(ids), _p(blank_lp), _p(count), float(thr), _p(st.state) if st is not None else None, _p(reset),
                                             _p(out_vals), _p(out_ids), _p(out_blank_lp), _p(out_len), _p(frame_map), B, T, k, frame_map.shape[1],
                                             _stream()), "asr_ctc_blank_skip_compact")
    return out_vals, out_ids, out_blank_lp, out_len, frame_map


def frame_index_remap(idx, frame_map, out=None):
    """idx (B, ...) int32 -> out of its shape (a new tensor unless given; idx itself is fine): every index >= 0 becomes frame_map[b, index],
    a negative one stays (asr_frame_index_remap): frames over kept rows -> real frames."""
    B = frame_map.shape[0]
    out = torch.empty_like(idx) if out is None else out
    _chk_i32(idx, frame_map, out)
    assert idx.shape[0] == B and out.shape == idx.shape
    if idx.numel() > 0 and frame_map.shape[1] > 0:
        check(lib.asr_frame_index_remap(_p(idx), _p(frame_map), _p(out), B, idx.numel() // B, frame_map.shape[1], _stream()), "asr_frame_index_remap")
    else:
        out.copy_(idx)
    return out


# --------------------------------------------------------------------------------- independent sessions (csrc/session.hip)
def add_ln_slots_fwd(x, gamma, beta, pe, pe_off, pe_off_host, lens, slots, T, y=None, rstd=None):
    """y[b, t] = LN(x[b, t]) * gamma + beta + pe[pe_off[b] + t], rows t >= lens[b] zeroed (asr_add_ln_slots_fwd); x is overwritten with
    the normalised rows, as add_ln_fwd(xhat=x) does.  pe_off, lens: (slots) int32 on the device; pe_off_host: the same offsets as host
    ints - an offset that would leave the table raises before the launch."""
    d = x.shape[-1]
    assert x.is_contiguous() and x.numel() == slots * T * d
    _chk_f32(gamma, beta, pe, rstd)
    _chk_i32(pe_off, lens)
    assert gamma.numel() == d and beta.numel() == d and pe.dim() == 2 and pe.shape[1] == d
    assert pe_off.numel() == slots and lens.numel() == slots and len(pe_off_host) == slots
    for b, o in enumerate(pe_off_host):
        if o < 0 or o + T > pe.shape[0]:
            raise ValueError(f"add_ln_slots_fwd: slot {b} at frame offset {o} with {T} frames leaves the positional table ({pe.shape[0]} rows)")
    y = torch.empty_like(x) if y is None else y
    rstd = torch.empty(slots * T, dtype=torch.float32, device=x.device) if rstd is None else rstd
    assert y.is_contiguous() and y.shape == x.shape and y.dtype == x.dtype and y.data_ptr() != x.data_ptr() and rstd.numel() >= slots * T
    check(lib.asr_add_ln_slots_fwd(_p(x), _p(gamma), _p(beta), _p(pe), _p(pe_off), _p(lens), _p(y), _p(rstd), int(slots), int(T), d, pe.shape[0], _dt(x),
                                   _stream()), "asr_add_ln_slots_fwd")
    return y


def _slot_buffer(t, what):
    assert t.dim() == 3 and t.is_contiguous(), f"{what} must be a dense (slots, cap, cols) buffer"
    return t.shape


def slot_rows_put(src, dst, start, n, C):
    """dst[b, start[b] + t] = src[b * C + t] for t < n[b] (asr_slot_rows_put).  src: (slots * C, cols), rows may be a column slice of a
    wider matrix; dst: (slots, cap, cols) dense; start, n: (slots) int32 on the device."""
    slots, cap, cols = _slot_buffer(dst, "dst")
    assert src.dim() == 2 and src.shape == (slots * C, cols) and src.stride(1) == 1 and src.dtype == dst.dtype
    _chk_i32(start, n)
    assert start.numel() == slots and n.numel() == slots
    check(lib.asr_slot_rows_put(_p(src), _p(dst), _p(start), _p(n), slots, int(C), cap, cols, src.stride(0) if slots * C > 1 else cols, _dt(dst), _stream()),
          "asr_slot_rows_put")
    return dst


def slot_rows_slide(src, dst, frm, count, max_count):
    """dst[b, t] = src[b, frm[b] + t] for t < count[b] <= max_count (asr_slot_rows_slide); src, dst: two (slots, cap, cols) buffers."""
    slots, cap, cols = _slot_buffer(src, "src")
    assert _slot_buffer(dst, "dst") == (slots, cap, cols) and src.dtype == dst.dtype
    _chk_i32(frm, count)
    assert frm.numel() == slots and count.numel() == slots
    check(lib.asr_slot_rows_slide(_p(src), _p(dst), _p(frm), _p(count), slots, int(max_count), cap, cols, _dt(dst), _stream()), "asr_slot_rows_slide")
    return dst


def ctc_frame_best_blank(logits, in_len=None, blank=0):
    """logits (B, T, V) -> (path (B, T) int32 as ctc_frame_argmax, blank_lp (B, T) f32 as ctc_frame_topk's) in one pass per frame."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len)
    assert in_len is None or in_len.numel() == B
    path = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    blank_lp = torch.empty(B, T, dtype=torch.float32, device=logits.device)
    check(lib.asr_ctc_frame_best_blank(_p(logits), _p(in_len), _p(path), _p(blank_lp), B, T, V, ld, int(blank), _dt(logits), _stream()),
          "asr_ctc_frame_best_blank")
    return path, blank_lp


def session_ctc_step(path, blank_lp, n_valid, reset, state, C, silence_lp, blank=0, out=None):
    """One tick of the per-slot CTC bookkeeping (asr_session_ctc_step): path (slots, C) int32 or None (beam sessions), blank_lp
    (slots, C) f32, n_valid / reset (slots) int32, state (slots, 4) int32 (updated in place).  Returns out (slots, 4 + C) int32 =
    {ids emitted, trailing silent frames, frames, decoded, ids...} on the device."""
    slots = state.shape[0]
    _chk_i32(path, n_valid, reset, state)
    _chk_f32(blank_lp)
    assert state.shape == (slots, 4) and blank_lp.numel() == slots * C and (path is None or path.numel() == slots * C)
    assert n_valid.numel() == slots and reset.numel() == slots
    out = torch.empty(slots, 4 + C, dtype=torch.int32, device=state.device) if out is None else out
    check(lib.asr_session_ctc_step(_p(path), _p(blank_lp), _p(n_valid), _p(reset), _p(state), _p(out), slots, int(C), int(blank), float(silence_lp), _stream()),
          "asr_session_ctc_step")
    return out


def ctc_frame_stats(logits, in_len=None, blank=0):
    """logits (B, T, V) -> (path (B, T) int32 as ctc_frame_argmax, best_lp, blank_lp, lse, ent: (B, T) f32) in one pass per frame
    (asr_ctc_frame_stats): log p of the best class and of the blank, the log-sum-exp, and the entropy confidence 1 - H / ln V."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len)
    assert in_len is None or in_len.numel() == B
    path = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    best_lp, blank_lp, lse, ent = torch.empty(4, B, T, dtype=torch.float32, device=logits.device).unbind(0)
    check(lib.asr_ctc_frame_stats(_p(logits), _p(in_len), _p(path), _p(best_lp), _p(blank_lp), _p(lse), _p(ent), B, T, V, ld, int(blank), _dt(logits),
                                  _stream()), "asr_ctc_frame_stats")
    return path, best_lp, blank_lp, lse, ent


def ctc_token_conf(logits, labels, lab_len, spans, lse, ent):
    """The five confidence measures of every aligned token (asr_ctc_token_conf): logits (B, T, V), labels (B, Lmax) / lab_len (B,) /
    spans (B, Lmax, 2) as ctc_align takes and returns them, lse / ent (B, T) from ctc_frame_stats over the same logits.
    Returns (B, Lmax, 5) f32 = {post_max, post_min, post_mean, ent_mean, ent_min}: 0 past lab_len, NaN for a token without a span."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(labels, lab_len, spans)
    _chk_f32(lse, ent)
    Lmax = labels.shape[1]
    assert labels.shape == (B, Lmax) and lab_len.numel() == B and spans.shape == (B, Lmax, 2) and lse.shape == (B, T) and ent.shape == (B, T)
    assert lse.is_contiguous() and ent.is_contiguous()
    dev = logits.device
    if Lmax == 0:      # the entry point takes Lmax >= 1, as asr_ctc_align
        labels, spans = torch.zeros(B, 1, dtype=torch.int32, device=dev), torch.full((B, 1, 2), -1, dtype=torch.int32, device=dev)
    labels, spans = labels.contiguous(), spans.contiguous()
    La = labels.shape[1]
    out = torch.empty(B, La, 5, dtype=torch.float32, device=dev)
    check(lib.asr_ctc_token_conf(_p(logits), _p(labels), _p(lab_len), _p(spans), _p(lse), _p(ent), _p(out), B, T, V, ld, La, _dt(logits), _stream()),
          "asr_ctc_token_conf")
    return out[:, :Lmax]


STEP_TOKENS_REC = 8      # words of a run's record in session_ctc_step_tokens' buffer: id, first frame, last frame, the five measures


def session_ctc_step_tokens(path, blank_lp, best_lp, ent, n_valid, reset, state, run, C, silence_lp, blank=0):
    """session_ctc_step with the greedy path's runs (asr_session_ctc_step_tokens): best_lp, ent (slots, C) f32 from ctc_frame_stats,
    run (slots, 8) int32 = the open run between ticks (updated in place, as state).  Returns out (slots, 13 + 9 C) int32 on the
    device: session_ctc_step's 4 + C words, the count of runs closed, C records of 8 words, the open run's record (include/asr_hip.h)."""
    slots = state.shape[0]
    _chk_i32(path, n_valid, reset, state, run)
    _chk_f32(blank_lp, best_lp, ent)
    assert state.shape == (slots, 4) and run.shape == (slots, STEP_TOKENS_REC) and state.is_contiguous() and run.is_contiguous()
    assert path.numel() == slots * C and blank_lp.numel() == slots * C and best_lp.numel() == slots * C and ent.numel() == slots * C
    assert path.is_contiguous() and blank_lp.is_contiguous() and best_lp.is_contiguous() and ent.is_contiguous()
    assert n_valid.numel() == slots and reset.numel() == slots
    out = torch.empty(slots, 13 + 9 * C, dtype=torch.int32, device=state.device)
    check(lib.asr_session_ctc_step_tokens(_p(path), _p(blank_lp), _p(best_lp), _p(ent), _p(n_valid), _p(reset), _p(state), _p(run), _p(out), slots, int(C),
                                          int(blank), float(silence_lp), _stream()), "asr_session_ctc_step_tokens")
    return out


def beam_step(top_vals, top_ids, score, alive, last_tok, parent, rec_tok, rec_par, rec_end, rec_score, maxlen, alive_total, B, beam, step, eos):
    _chk_f32(top_vals, score, rec_score)
    _chk_i32(top_ids, alive, last_tok, parent, rec_tok, rec_par, rec_end, maxlen, alive_total)
    check(lib.asr_beam_step(_p(top_vals), _p(top_ids), _p(score), _p(alive), _p(last_tok), _p(parent), _p(rec_tok), _p(rec_par), _p(rec_end),
                            _p(rec_score), _p(maxlen), _p(alive_total), B, beam, int(step), int(eos), _stream()), "asr_beam_step")


def cache_gather(src, dst, parent, L, R, beam, Lcap, n_pos, row_bytes):
    _chk_i32(parent)
    check(lib.asr_cache_gather(_p(src), _p(dst), _p(parent), L, R, beam, Lcap, int(n_pos), int(row_bytes), _stream()), "asr_cache_gather")


def ctc_prefix_logprobs(logits):
    """log_softmax of the CTC head's frames, transposed (asr_ctc_prefix_logprobs): logits (B, T, V) f32 / bf16, dense or rows padded as
    the engine lays them out -> (B, V, T) f32, the per-batch input of ctc_prefix_score."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    lpT = torch.empty(B, V, T, dtype=torch.float32, device=logits.device)
    check(lib.asr_ctc_prefix_logprobs(_p(logits), _p(lpT), B, T, V, ld, _dt(logits), _stream()), "asr_ctc_prefix_logprobs")
    return lpT


def ctc_prefix_score(lpT, in_len, st_rb, st_rt, hyp_psi, last_tok, alive, att_vals, att_ids, cand_rb, cand_rt, beam, step, ctc_weight,
                     eos, blank=0, out=None):
    """One step of CTC prefix scoring (asr_ctc_prefix_score, include/asr_hip.h): lpT (B, V, T) from ctc_prefix_logprobs; state st_rb /
    st_rt (T, R) f64, hyp_psi (R) f32, last_tok / alive (R) int32 (R = B * beam; not read at step 0); candidates att_vals / att_ids
    (R, C); writes the candidates' state into cand_rb / cand_rt (T, R * C) f64.  Returns (vals, ids, att, psi, full), each (R, beam):
    per hypothesis the `beam` best candidates by joint score."""
    B, V, T = lpT.shape
    R, C = att_ids.shape
    assert R == B * beam and att_vals.shape == (R, C) and lpT.is_contiguous()
    assert cand_rb.shape == cand_rt.shape == (T, R * C) and cand_rb.dtype == cand_rt.dtype == torch.float64
    assert step == 0 or (st_rb.shape == st_rt.shape == (T, R) and st_rb.dtype == st_rt.dtype == torch.float64)
    _chk_f32(lpT, att_vals, hyp_psi)
    _chk_i32(in_len, last_tok, alive, att_ids)
    if out is None:
        dev = lpT.device
        out = (torch.empty(R, beam, dtype=torch.float32, device=dev), torch.empty(R, beam, dtype=torch.int32, device=dev),
               torch.empty(R, beam, dtype=torch.float32, device=dev), torch.empty(R, beam, dtype=torch.float32, device=dev),
               torch.empty(R, beam, dtype=torch.float32, device=dev))
    vals, ids, att, psi, full = out
    check(lib.asr_ctc_prefix_score(_p(lpT), _p(in_len), _p(st_rb), _p(st_rt), _p(hyp_psi), _p(last_tok), _p(alive), _p(att_vals), _p(att_ids),
                                   _p(cand_rb), _p(cand_rt), _p(vals), _p(ids), _p(att), _p(psi), _p(full), B, T, V, int(beam), C, int(step),
                                   float(ctc_weight), int(eos), int(blank), _stream()), "asr_ctc_prefix_score")
    return out


def ctc_prefix_gather(cand_rb, cand_rt, st_rb, st_rt, parent, last_tok, alive, att_ids, in_len, B, beam):
    """Every live slot r takes the state of its parent's candidate with token last_tok[r] (asr_ctc_prefix_gather)."""
    T, R = st_rb.shape
    C = att_ids.shape[1]
    assert R == B * beam and cand_rb.shape == cand_rt.shape == (T, R * C) and st_rt.shape == (T, R)
    _chk_i32(parent, last_tok, alive, att_ids, in_len)
    check(lib.asr_ctc_prefix_gather(_p(cand_rb), _p(cand_rt), _p(st_rb), _p(st_rt), _p(parent), _p(last_tok), _p(alive), _p(att_ids), _p(in_len),
                                    B, T, int(beam), C, _stream()), "asr_ctc_prefix_gather")


def joint_beam_step(top, score, att_score, ctc_score, alive, last_tok, parent, rec_tok, rec_par, rec_end, rec_score, rec_att, rec_ctc, maxlen,
                    alive_total, B, beam, step, eos, ctc_weight):
    """One step of the one-pass joint search (asr_joint_beam_step) on ctc_prefix_score's (vals, ids, att, psi, full)."""
    vals, ids, att, psi, full = top
    _chk_f32(vals, att, psi, full, score, att_score, ctc_score, rec_score, rec_att, rec_ctc)
    _chk_i32(ids, alive, last_tok, parent, rec_tok, rec_par, rec_end, maxlen, alive_total)
    check(lib.asr_joint_beam_step(_p(vals), _p(ids), _p(att), _p(psi), _p(full), _p(score), _p(att_score), _p(ctc_score), _p(alive), _p(last_tok),
                                  _p(parent), _p(rec_tok), _p(rec_par), _p(rec_end), _p(rec_score), _p(rec_att), _p(rec_ctc), _p(maxlen),
                                  _p(alive_total), B, beam, int(step), int(eos), float(ctc_weight), _stream()), "asr_joint_beam_step")


def xent_fwd_bwd(logits, gold, n_valid, ignore_index=0, smoothing=0.0, grad_scale=1.0, dlogits=None, want_grad=True,
                 row_nll=None, argmax=None):
    """argmax: optional (M) int32 tensor that receives every row's greedy class (first index of the maximum, ignored rows included)."""
    M, V = logits.shape
    assert logits.is_contiguous() and gold.numel() == M
    _chk_i32(gold, argmax)
    assert argmax is None or argmax.numel() == M
    _chk_f32(n_valid)
    row_nll = torch.empty(M, dtype=torch.float32, device=logits.device) if row_nll is None else row_nll
    if want_grad and dlogits is None:
        dlogits = torch.empty_like(logits)
    timed("xent", 0.0, lambda: check(
        lib.asr_xent_fwd_bwd(_p(logits), _p(gold), _p(n_valid), _p(row_nll), _p(dlogits), M, V, int(ignore_index),
                             float(smoothing), float(grad_scale), _p(argmax), _dt(logits), _stream()), "asr_xent_fwd_bwd"),
          (3.0 if dlogits is not None else 1.0) * logits.numel() * logits.element_size())                      # 3 M V e
    return row_nll, dlogits


def loss_combine(row_nll, n_valid, nll, w_ce, w_ctc, out=None):
    dev = (row_nll if row_nll is not None else nll).device
    out = torch.empty(3, dtype=torch.float32, device=dev) if out is None else out
    M = row_nll.numel() if row_nll is not None else 0
    B = nll.numel() if nll is not None else 0
    check(lib.asr_loss_combine(_p(row_nll), M, _p(n_valid), _p(nll), B, float(w_ce), float(w_ctc), _p(out), _stream()),
          "asr_loss_combine")
    return out


# --------------------------------------------------------------------------------- decoder glue
def dec_preprocess(tgt, sos=2, eos=3, lens64=()):
    """tgt (B, Lmax) int64 zero-padded -> ys_in, ys_out (B, Lmax+1) int32, labels32, dec_len, lab_len, n_valid.
    lens64: up to two (B,) int64 length vectors of the batch (wave_len, tgt_len); their int32 copies are made by the same launch and
    returned as a 7th element (a tuple)."""
    assert tgt.dtype == torch.int64 and tgt.is_contiguous() and tgt.dim() == 2
    B, Lmax = tgt.shape
    dev = tgt.device
    lens64 = tuple(lens64)
    assert len(lens64) <= 2 and all(t.dtype == torch.int64 and t.is_contiguous() and t.numel() == B and t.device == dev for t in lens64)
    lens32 = tuple(torch.empty(B, dtype=torch.int32, device=dev) for _ in lens64)
    la, lb = (list(zip(lens64, lens32)) + [(None, None), (None, None)])[:2]
    ys_in = torch.empty(B, Lmax + 1, dtype=torch.int32, device=dev)
    ys_out = torch.empty(B, Lmax + 1, dtype=torch.int32, device=dev)
    labels32 = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    dec_len = torch.empty(B, dtype=torch.int32, device=dev)
    lab_len = torch.empty(B, dtype=torch.int32, device=dev)
    n_valid = torch.empty(1, dtype=torch.float32, device=dev)
    check(lib.asr_dec_preprocess(_p(tgt), _p(ys_in), _p(ys_out), _p(labels32), _p(dec_len), _p(lab_len), _p(n_valid),
                                 B, Lmax, sos, eos, _p(la[0]), _p(la[1]), _p(lb[0]), _p(lb[1]), _stream()), "asr_dec_preprocess")
    if lens64:
        return ys_in, ys_out, labels32, dec_len, lab_len, n_valid, lens32
    return ys_in, ys_out, labels32, dec_len, lab_len, n_valid


def embed_pe_fwd(ids, emb, pe, scale, B, To, dtype, y=None, drop_p=0.0, drop_seed=0):
    V, d = emb.shape
    _chk_i32(ids)
    _chk_f32(emb, pe)
    assert ids.numel() == B * To and pe.shape[-1] == d and pe.shape[-2] >= To
    y = torch.empty(B * To, d, dtype=dtype, device=emb.device) if y is None else y
    check(lib.asr_embed_pe_fwd(_p(ids), _p(emb), _p(pe), _p(y), float(scale), B, To, d, V, float(drop_p),
                               int(drop_seed) & 0xFFFFFFFF, _dt(y), _stream()), "asr_embed_pe_fwd")
    return y


def embed_bwd(ids, dy, demb, scale, drop_p=0.0, drop_seed=0, dy2=None):
    V, d = demb.shape
    _chk_i32(ids)
    _chk_f32(demb)
    assert dy.is_contiguous() and dy.shape[-1] == d and dy.numel() == ids.numel() * d
    assert dy2 is None or (dy2.is_contiguous() and dy2.shape == dy.shape and dy2.dtype == dy.dtype)
    check(lib.asr_embed_bwd(_p(ids), _p(dy), _p(dy2), _p(demb), float(scale), ids.numel(), d, V, float(drop_p),
                            int(drop_seed) & 0xFFFFFFFF, _dt(dy), _stream()), "asr_embed_bwd")


def dropout_mask(rows, cols, drop_p, drop_seed, device="cuda"):
    """(rows, cols) uint8 keep mask of the LayerNorm / embedding dropout sites (tests)."""
    m = torch.empty(rows, cols, dtype=torch.uint8, device=device)
    check(lib.asr_dropout_mask(_p(m), rows, cols, float(drop_p), int(drop_seed) & 0xFFFFFFFF, _stream()), "asr_dropout_mask")
    return m


def sdpa_dropout_mask(B, H, Tq, Tk, drop_p, drop_seed, device="cuda"):
    m = torch.empty(B, H, Tq, Tk, dtype=torch.uint8, device=device)
    check(lib.asr_sdpa_dropout_mask(_p(m), B, H, Tq, Tk, float(drop_p), int(drop_seed) & 0xFFFFFFFF, _stream()), "asr_sdpa_dropout_mask")
    return m


# --------------------------------------------------------------------------------- elementwise
def relu_(x):
    assert x.is_contiguous()
    check(lib.asr_relu_fwd(_p(x), x.numel(), _dt(x), _stream()), "asr_relu_fwd")
    return x


def relu_bwd_(da, a, dbias, ws):
    """da *= (a > 0) in place; dbias (f32) += column sums."""
    assert da.is_contiguous() and a.is_contiguous() and da.shape == a.shape and da.dtype == a.dtype and da.dim() == 2
    _chk_f32(dbias)      # None: mask only (the bias gradient then comes from the weight-gradient GEMM)
    rows, cols = da.shape
    w = ws.get(lib.asr_colsum_workspace_bytes(rows, cols))
    check(lib.asr_relu_bwd(_p(da), _p(a), _p(dbias), _p(w), w.numel(), rows, cols, _dt(da), _stream()), "asr_relu_bwd")
    return da


def colsum(x, out, ws, accumulate=True):
    assert x.dim() == 2 and x.stride(1) == 1
    _chk_f32(out)
    rows, cols = x.shape
    assert out.numel() == cols
    w = ws.get(lib.asr_colsum_workspace_bytes(rows, cols))
    check(lib.asr_colsum(_p(x), _p(out), _p(w), w.numel(), rows, cols, x.stride(0), int(accumulate), _dt(x), _stream()),
          "asr_colsum")
    return out


def cast(src, dst):
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    check(lib.asr_cast(_p(src), _p(dst), src.numel(), _dt(src), _dt(dst), _stream()), "asr_cast")
    return dst


def rows_gather(src, B, T, Tk, out=None):
    """(B*Tk, d) = rows t < Tk of every utterance of src (B*T, d)."""
    assert src.is_contiguous() and src.dim() == 2 and src.shape[0] == B * T and 0 <= Tk <= T
    out = torch.empty(B * Tk, src.shape[1], dtype=src.dtype, device=src.device) if out is None else out
    assert out.is_contiguous() and out.shape == (B * Tk, src.shape[1]) and out.dtype == src.dtype
    check(lib.asr_rows_gather(_p(src), _p(out), B, T, Tk, src.shape[1], _dt(src), _stream()), "asr_rows_gather")
    return out


def rows_scatter_add(src, dst, B, T, Tk):
    """dst (B*T, d) rows t < Tk of every utterance += src (B*Tk, d), in place."""
    assert src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype and 0 <= Tk <= T
    assert src.shape == (B * Tk, dst.shape[1]) and dst.shape[0] == B * T
    check(lib.asr_rows_scatter_add(_p(src), _p(dst), B, T, Tk, dst.shape[1], _dt(dst), _stream()), "asr_rows_scatter_add")
    return dst


# --------------------------------------------------------------------------------- optimizer
def grad_sumsq(g, out, ws):
    _chk_f32(g, out)
    w = ws.get(lib.asr_sumsq_workspace_bytes(g.numel()))
    timed("grad_sumsq", 0.0, lambda: check(lib.asr_grad_sumsq(_p(g), g.numel(), _p(out), _p(w), w.numel(), _stream()), "asr_grad_sumsq"), 4.0 * g.numel())
    return out


def grad_sumsq_noam(g, out, ws, step, hyper, model_size, warmup, factor, lr_const, b1, b2):
    """grad_sumsq + noam_hyper with the schedule update inside the norm's finalizer (asr_grad_sumsq_noam)."""
    _chk_f32(g, out, hyper)
    _chk_i32(step)
    assert hyper.numel() >= 4
    w = ws.get(lib.asr_sumsq_workspace_bytes(g.numel()))
    timed("grad_sumsq", 0.0, lambda: check(lib.asr_grad_sumsq_noam(_p(g), g.numel(), _p(out), _p(w), w.numel(), _p(step), _p(hyper), float(model_size),
                                                                   float(warmup), float(factor), float(lr_const), float(b1), float(b2), _stream()),
                                           "asr_grad_sumsq_noam"), 4.0 * g.numel())
    return out


def noam_hyper(step, hyper, model_size, warmup, factor, lr_const, b1, b2):
    _chk_i32(step)
    _chk_f32(hyper)
    assert hyper.numel() >= 4
    check(lib.asr_noam_hyper(_p(step), _p(hyper), float(model_size), float(warmup), float(factor), float(lr_const),
                             float(b1), float(b2), _stream()), "asr_noam_hyper")


def adam_step(p, g, m, v, p_lp, hyper, sumsq, max_norm, b1, b2, eps, write_clipped=True):
    _chk_f32(p, g, m, v, hyper, sumsq)
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n
    if p_lp is not None:
        assert p_lp.dtype == torch.bfloat16 and p_lp.numel() == n and p_lp.is_contiguous()
    # p, g, m, v read + p, m, v (+ clipped g) written in fp32, bf16 shadow written: 28 (+4) (+2) B per parameter (~30)
    timed("adam", 0.0, lambda: check(
        lib.asr_adam_step(_p(p), _p(g), _p(m), _p(v), _p(p_lp), n, _p(hyper), _p(sumsq), float(max_norm), float(b1),
                          float(b2), float(eps), int(write_clipped), _stream()), "asr_adam_step"),
          (28.0 + (4.0 if write_clipped else 0.0) + (2.0 if p_lp is not None else 0.0)) * n)


def adam_ema_step(p, g, m, v, p_lp, hyper, sumsq, max_norm, b1, b2, eps, ema, decay, warmup=True, write_clipped=True):
    """adam_step and, in the same pass, ema += (1 - d) * (p - ema) on the fresh p (include/asr_hip.h: asr_adam_ema_step); the step of the
    warm-up is hyper[3].  p, g, m, v, p_lp get adam_step's bits."""
    _chk_f32(p, g, m, v, hyper, sumsq, ema)
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n and ema.numel() == n and hyper.numel() >= 4
    if p_lp is not None:
        assert p_lp.dtype == torch.bfloat16 and p_lp.numel() == n and p_lp.is_contiguous()
    # adam_step's traffic + ema read and written: 8 B per parameter more
    timed("adam", 0.0, lambda: check(
        lib.asr_adam_ema_step(_p(p), _p(g), _p(m), _p(v), _p(p_lp), n, _p(hyper), _p(sumsq), float(max_norm), float(b1), float(b2), float(eps),
                              int(write_clipped), _p(ema), float(decay), int(bool(warmup)), _stream()), "asr_adam_ema_step"),
          (36.0 + (4.0 if write_clipped else 0.0) + (2.0 if p_lp is not None else 0.0)) * n)


def ema_update(p, ema, decay, step, warmup=True):
    """ema += (1 - d) * (p - ema) as a pass of its own, d of optimizer step `step` >= 1 (asr_ema_update): 12 B per parameter."""
    _chk_f32(p, ema)
    assert p.numel() == ema.numel()
    timed("ema", 0.0, lambda: check(lib.asr_ema_update(_p(p), _p(ema), p.numel(), float(decay), int(bool(warmup)), float(step), _stream()),
                                    "asr_ema_update"), 12.0 * p.numel())
    return ema


# --------------------------------------------------------------------------------- GEMM
def gemm_nt_supported(M, N, K, lda, ldb, ldc):
    return K % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and ldc % 4 == 0


def transpose_batched(src, dst, tiles):
    """Transposed copies of the matrices listed in `tiles` (int32 (ntiles, 6), see include/asr_hip.h) from the flat
    bf16 buffer src into dst (each copy at its own offset and row stride)."""
    assert src.dtype == dst.dtype == torch.bfloat16 and tiles.dtype == torch.int32 and tiles.is_contiguous() and tiles.shape[1] == 6
    check(lib.asr_transpose_batched_bf16(_p(src), _p(dst), _p(tiles), tiles.shape[0], _stream()), "asr_transpose_batched_bf16")


def gemm_nt(a, w, bias, out, act=ACT_NONE, res=None, family="gemm_nt"):
    """out (M,N) = act(a (M,K) @ w (N,K)^T + bias) (+ res); bf16 operands, MFMA kernel.
    act = ACT_RELU_MASK: out = (a @ w^T) where res > 0 else 0 (res = the activations of a ReLU whose backward this is; no bias)."""
    assert a.dtype == w.dtype == out.dtype == torch.bfloat16
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and out.shape == (M, N) and a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1
    _chk_f32(bias)
    if res is not None:
        assert res.dtype == torch.bfloat16 and res.shape == out.shape and res.stride() == out.stride()
    timed(family, 2.0 * M * N * K, lambda: check(
        lib.asr_gemm_nt_bf16(_p(a), _p(w), _p(bias), _p(res), _p(out), M, N, K, a.stride(0), w.stride(0), out.stride(0), int(act),
                             _stream()), "asr_gemm_nt_bf16"))
    return out


_CU_LIMIT_NAME = ctypes.create_string_buffer(b"cu_limit")


def set_cu_limit(n):
    """Tuning option "cu_limit" on the launch path (no ctypes foreign call): the one-workgroup-per-CU kernels launched from now on are sized
    for n CUs (0 = the whole device).  The engine brackets the large launches that run beside the decoder's small kernels with it."""
    check(lib.asr_set_option(ctypes.addressof(_CU_LIMIT_NAME), int(n), None), "asr_set_option")


def set_option(name, value):
    """asr_set_option (include/asr_hip.h): process-wide tuning switches under which every value gives correct results; returns the previous value."""
    prev = ctypes.c_int(0)
    check(_lib.lib.asr_set_option(name.encode(), int(value), ctypes.byref(prev)), "asr_set_option")
    return prev.value


def deterministic():
    """True when the library's reductions run in a fixed order (asr_set_deterministic / ASR_DETERMINISTIC=1)."""
    return bool(lib.asr_get_deterministic())


def set_deterministic(on):
    """Process-wide switch (see include/asr_hip.h); returns the previous value.  Engines read it when they are built."""
    return bool(lib.asr_set_deterministic(int(bool(on))))


def gemm_f32(a, b, out, bias=None, trans_a=False, trans_b=False, act=ACT_NONE, mask=None, accumulate=False):
    """out (M, N) (+)= act(op(a) @ op(b) + bias) in fp32 on the matrix cores (asr_gemm_f32): a is (M, K), or (K, M) when trans_a;
    b is (K, N), or (N, K) when trans_b; mask (ACT_RELU_MASK): the activations of the ReLU whose backward this is, laid out like out."""
    assert a.dtype == b.dtype == out.dtype == torch.float32 and a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1
    M, N = out.shape
    K = a.shape[0] if trans_a else a.shape[1]
    assert a.shape == ((K, M) if trans_a else (M, K)) and b.shape == ((N, K) if trans_b else (K, N)), (a.shape, b.shape, out.shape)
    _chk_f32(bias)
    if mask is not None:
        assert mask.dtype == torch.float32 and mask.shape == out.shape and mask.stride() == out.stride()
    timed("gemm_f32", 2.0 * M * N * K, lambda: check(
        lib.asr_gemm_f32(_p(a), _p(b), _p(bias), _p(mask), _p(out), M, N, K, a.stride(0), b.stride(0), out.stride(0), int(trans_a), int(trans_b), int(act),
                         int(accumulate), _stream()), "asr_gemm_f32"))
    return out


def gemm_small(a, bm, bias, out, trans_b=False, act=ACT_NONE, mask=None):
    """Small-M projection (see include/asr_hip.h): out (M, N) = act(a (M, K) @ bm^T + bias) with bm (N, K), or a @ bm with bm (K, N) when trans_b."""
    M, K = a.shape
    N = out.shape[1]
    assert a.dtype == bm.dtype == out.dtype == torch.bfloat16 and out.shape[0] == M
    assert bm.shape == ((K, N) if trans_b else (N, K)) and a.stride(1) == 1 and bm.stride(1) == 1 and out.stride(1) == 1
    _chk_f32(bias)
    if mask is not None:
        assert mask.dtype == torch.bfloat16 and mask.shape == out.shape and mask.stride() == out.stride()
    timed("gemm_small", 2.0 * M * N * K, lambda: check(
        lib.asr_gemm_small_bf16(_p(a), _p(bm), _p(bias), _p(mask), _p(out), M, N, K, a.stride(0), bm.stride(0), out.stride(0), int(trans_b), int(act),
                                _stream()), "asr_gemm_small_bf16"))
    return out


def gemm_tn(dy, x, dw, accumulate=True, dbias=None, ws=None):
    """dw (N,K) f32 (+)= dy (M,N)^T @ x (M,K); bf16 operands, MFMA kernel.  dbias (N) f32 += column sums of dy.
    ws: a Workspace - needed in deterministic mode only (partial slabs, one per M-split)."""
    assert dy.dtype == x.dtype == torch.bfloat16 and dw.dtype == torch.float32
    M, N = dy.shape
    K = x.shape[1]
    assert x.shape[0] == M and dw.shape == (N, K) and dy.stride(1) == 1 and x.stride(1) == 1 and dw.stride(1) == 1
    _chk_f32(dbias)
    assert dbias is None or dbias.numel() == N
    need = lib.asr_gemm_tn_workspace_bytes(M, N, K)
    w = None
    if need:
        w = ws.get(need) if ws is not None else torch.empty(need, dtype=torch.uint8, device=dy.device)
    timed("gemm_tn", 2.0 * M * N * K, lambda: check(
        lib.asr_gemm_tn_bias_bf16(_p(dy), _p(x), _p(dw), _p(dbias), M, N, K, dy.stride(0), x.stride(0), dw.stride(0), int(accumulate), _p(w),
                                  w.numel() if w is not None else 0, _stream()), "asr_gemm_tn_bias_bf16"))
    return dw


_TN_SIZE = ctypes.sizeof(TnProblem)
_TN_BUF = (ctypes.c_char * (_TN_SIZE * TN_GROUP_MAX))()
_TN_ADDR = ctypes.addressof(_TN_BUF)
_TN_PACK = __import__("struct").Struct("<QQQQiiiiii").pack_into
assert _TN_SIZE == 56      # asr_tn_problem: four pointers, six ints


def gemm_tn_grouped(problems, accumulate=True):
    """problems: list of (dy (M,N) bf16, x (M,K) bf16, dw (N,K) f32, dbias (N) f32 or None);
    dw_p (+)= dy_p^T @ x_p and dbias_p += column sums of dy_p for all of them, TN_GROUP_MAX per launch."""
    for i in range(0, len(problems), TN_GROUP_MAX):
        chunk = problems[i:i + TN_GROUP_MAX]
        flops = 0.0
        for j, (dy, x, dw, dbias) in enumerate(chunk):
            assert dy.dtype == x.dtype == torch.bfloat16 and dw.dtype == torch.float32
            M, N = dy.shape
            Kd = x.shape[1]
            assert x.shape[0] == M and dw.shape == (N, Kd) and dy.stride(1) == 1 and x.stride(1) == 1 and dw.stride(1) == 1
            _chk_f32(dbias)
            assert dbias is None or dbias.numel() == N
            # one pack per problem into a reused host buffer (the launch copies the descriptors into kernel arguments before it
            # returns): field-by-field ctypes stores cost ~25 us per decoder layer, in the host-bound part of the joint step
            _TN_PACK(_TN_BUF, j * _TN_SIZE, _p(dy), _p(x), _p(dw), _p(dbias) or 0, M, N, Kd, dy.stride(0), x.stride(0), dw.stride(0))
            flops += 2.0 * M * N * Kd
        timed("gemm_tn", flops, lambda: check(lib.asr_gemm_tn_grouped_bf16(_TN_ADDR, len(chunk), int(accumulate), _stream()),
                                              "asr_gemm_tn_grouped_bf16"))


def token_table(id2token, device):
    """(tok_cp, tok_off, max_tok_len) for cer(): code points of every token string, back to back."""
    cps, off = [], [0]
    for tok in id2token:
        cps.extend(ord(c) for c in tok)
        off.append(len(cps))
    mx = max((off[i + 1] - off[i] for i in range(len(id2token))), default=0)
    return (torch.tensor(cps if cps else [0], dtype=torch.int32, device=device), torch.tensor(off, dtype=torch.int32, device=device), mx)


def cer(hyp, ref, table, pad_id, hyp_len=None, ref_len=None):
    """Per-utterance character error rate (B,) f32 on the device, reference string convention
    (score.py:4-13 over vocab.py:75-79 strings).  hyp (B, Lh), ref (B, Lr) int32 ids."""
    tok_cp, tok_off, mx = table
    _chk_i32(hyp, ref, hyp_len, ref_len)
    assert hyp.dim() == 2 and ref.dim() == 2 and hyp.shape[0] == ref.shape[0] and hyp.stride(1) == 1 and ref.stride(1) == 1
    B = hyp.shape[0]
    out = torch.empty(B, dtype=torch.float32, device=hyp.device)
    check(lib.asr_cer(_p(hyp), _p(hyp_len), hyp.shape[1], hyp.stride(0), _p(ref), _p(ref_len), ref.shape[1], ref.stride(0), _p(tok_cp), _p(tok_off),
                      tok_off.numel() - 1, mx, int(pad_id), B, _p(out), _stream()), "asr_cer")
    return out


# --------------------------------------------------------------------------------- front end
def logmel(wav, wav_len, window, melfb, Tmax, feat=None):
    _chk_f32(wav, window, melfb)
    _chk_i32(wav_len)
    B, Smax = wav.shape
    n_mels = melfb.shape[1]
    assert melfb.shape[0] == 201 and window.numel() == 400 and wav_len.numel() == B
    feat = torch.empty(B, Tmax, n_mels, dtype=torch.float32, device=wav.device) if feat is None else feat
    check(lib.asr_logmel_fwd(_p(wav), _p(wav_len), _p(window), _p(melfb), _p(feat), B, Smax, Tmax, n_mels, _stream()),
          "asr_logmel_fwd")
    return feat


def _norm_aug_lfr(entry, feat, wav_len, m, n, Tlfr_max, dtype, mean=None, istd=None, masks=None, policy=None):
    """The body of the four normalise-augment-stack calls: checks, out (B, Tlfr_max, m n_mels) and out_len (B) int32, and the library
    entry `entry`.  mean, istd: None under utterance normalisation, whose entries take none.  policy: None (the reference's masks, or
    none) or (ranges, counts)."""
    _chk_f32(feat, mean, istd)
    _chk_i32(wav_len, masks)
    B, Tmax, n_mels = feat.shape
    assert wav_len.numel() == B and (mean is None or (mean.numel() == n_mels and istd.numel() == n_mels))
    if policy is None:
        assert masks is None or tuple(masks.shape) == (B, 4)
        aug = (_p(masks),)
    else:
        aug = _specaug_ranges(policy[0], B, policy[1])
    out = torch.empty(B, Tlfr_max, m * n_mels, dtype=dtype, device=feat.device)
    out_len = torch.empty(B, dtype=torch.int32, device=feat.device)
    stats = () if mean is None else (_p(mean), _p(istd))
    check(getattr(lib, entry)(_p(feat), _p(wav_len), *aug, *stats, _p(out), _p(out_len), B, Tmax, n_mels, m, n, Tlfr_max, _dt(out), _stream()), entry)
    return out, out_len


def utt_norm_lfr(feat, wav_len, m, n, Tlfr_max, dtype=torch.float32, masks=None):
    """masks: optional (B, 4) int32 [t0, t1, f0, f1] SpecAugment ranges (see include/asr_hip.h)."""
    return _norm_aug_lfr("asr_utt_norm_augment_lfr_fwd", feat, wav_len, m, n, Tlfr_max, dtype, masks=masks)


SPEED_TILE = _lib.SPEED_TILE      # output samples per workgroup of the speed-perturbation kernel


def speed_perturb(wav, wav_len, factor, pq, taps, Smax_out, out=None, out_len=None):
    """Every utterance of wav (B, Smax) f32 resampled by the factor p/q = pq[factor[b]] with the phase table taps[factor[b]]
    (data_handler.speed.build_tables; include/asr_hip.h: asr_speed_perturb_fwd).  -> (out (B, Smax_out) f32, zero at and beyond each
    n_out, out_len (B) int32 = n_out = ceil(wav_len q / p)).  Smax_out: at least the largest n_out (data_handler.speed.perturbed_len)."""
    _chk_f32(wav, taps, out)
    _chk_i32(wav_len, factor, pq, out_len)
    B, Smax = wav.shape
    assert taps.dim() == 3 and pq.dim() == 2 and pq.shape[1] == 2 and pq.shape[0] == taps.shape[0] and wav_len.numel() == B and factor.numel() == B
    F, qmax, ntaps = taps.shape
    out = torch.empty(B, Smax_out, dtype=torch.float32, device=wav.device) if out is None else out
    out_len = torch.empty(B, dtype=torch.int32, device=wav.device) if out_len is None else out_len
    assert tuple(out.shape) == (B, Smax_out) and out_len.numel() == B and out.data_ptr() != wav.data_ptr()
    check(lib.asr_speed_perturb_fwd(_p(wav), _p(wav_len), _p(factor), _p(pq), _p(taps), _p(out), _p(out_len), B, Smax, int(Smax_out), F, qmax, ntaps,
                                    _stream()), "asr_speed_perturb_fwd")
    return out, out_len


RESAMPLE_TILE = _lib.RESAMPLE_TILE      # output samples per workgroup of the sample-rate conversion kernel


def resample(wav, rate_idx, win, pq, tap_off, taps, Smax_out, out=None, out_len=None):
    """Every utterance of wav (B, Smax) f32 converted to 16 kHz from the source rate of plan rate_idx[b] (outside [0, R): a copy), over
    the window win[b] = {in_base, n_avail, n_total, out_start, n_emit} (data_handler.resample.RateTable builds pq, tap_off, taps and the
    offline windows; include/asr_hip.h: asr_resample_fwd).  -> (out (B, Smax_out) f32, zero at and beyond each n_emit, out_len (B) int32)."""
    _chk_f32(wav, taps, out)
    _chk_i32(rate_idx, win, pq, tap_off, out_len)
    B, Smax = wav.shape
    R = pq.shape[0]
    assert pq.dim() == 2 and pq.shape[1] == 2 and tap_off.numel() == R + 1 and rate_idx.numel() == B and tuple(win.shape) == (B, 5) and taps.dim() == 1
    out = torch.empty(B, Smax_out, dtype=torch.float32, device=wav.device) if out is None else out
    out_len = torch.empty(B, dtype=torch.int32, device=wav.device) if out_len is None else out_len
    assert tuple(out.shape) == (B, Smax_out) and out_len.numel() == B and out.data_ptr() != wav.data_ptr()
    check(lib.asr_resample_fwd(_p(wav), _p(rate_idx), _p(win), _p(pq), _p(tap_off), _p(taps), _p(out), _p(out_len), B, Smax, int(Smax_out), R,
                               taps.numel(), _stream()), "asr_resample_fwd")
    return out, out_len


REVERB_TILE, REVERB_CHUNK, REVERB_MAX_TAPS = _lib.REVERB_TILE, _lib.REVERB_CHUNK, _lib.REVERB_MAX_TAPS
NOISE_MIX_TILE = _lib.NOISE_MIX_TILE


def reverb(wav, wav_len, rir_idx, rir, rir_len, rir_peak, out=None):
    """Every utterance of wav (B, Smax) f32 convolved with the response rir[rir_idx[b]] (R, Lcap) f32 of rir_len taps, its peak at
    rir_peak kept on the direct path (include/asr_hip.h: asr_reverb_fwd; data_handler.noise.RirBank builds the table).  An index
    outside [0, R) copies the utterance.  -> out (B, Smax) f32, zero at and beyond each wav_len; the lengths do not change."""
    _chk_f32(wav, rir, out)
    _chk_i32(wav_len, rir_idx, rir_len, rir_peak)
    B, Smax = wav.shape
    assert rir.dim() == 2 and wav_len.numel() == B and rir_idx.numel() == B
    R, Lcap = rir.shape
    assert rir_len.numel() == R and rir_peak.numel() == R
    out = torch.empty(B, Smax, dtype=torch.float32, device=wav.device) if out is None else out
    assert tuple(out.shape) == (B, Smax)
    check(lib.asr_reverb_fwd(_p(wav), _p(wav_len), _p(rir_idx), _p(rir), _p(rir_len), _p(rir_peak), _p(out), B, Smax, R, Lcap, _stream()), "asr_reverb_fwd")
    return out


REVERB_FFT_N, REVERB_FFT_MAX_TAPS = _lib.REVERB_FFT_N, _lib.REVERB_FFT_MAX_TAPS
_REVERB_FFT_TWIDDLE = {}      # device -> the (N, 2) f32 table, uploaded the first time that device needs it


def reverb_fft_twiddle(device):
    """(cos, -sin)(2 pi t / N), t < N = REVERB_FFT_N: computed in float64 on the host, rounded once, resident on `device`."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    tw = _REVERB_FFT_TWIDDLE.get(device)
    if tw is None:
        a = 2.0 * math.pi * torch.arange(REVERB_FFT_N, dtype=torch.float64) / REVERB_FFT_N
        tw = _REVERB_FFT_TWIDDLE[device] = torch.stack((torch.cos(a), -torch.sin(a)), dim=1).to(torch.float32).to(device)
    return tw


def reverb_fft_workspace(B, Smax, Lcap, device):
    """The window and response spectra of reverb_fft (asr_reverb_fft_workspace_bytes); need not be initialised."""
    return torch.empty((lib.asr_reverb_fft_workspace_bytes(B, Smax, Lcap) + 3) // 4, dtype=torch.float32, device=device)


def reverb_fft(wav, wav_len, rir_idx, rir, rir_len, rir_peak, out=None, ws=None):
    """reverb's result for responses of up to REVERB_FFT_MAX_TAPS taps, as a partitioned overlap-save FFT convolution whose cost is
    nearly flat in the response length (include/asr_hip.h: asr_reverb_fft_fwd).  Same arguments and semantics as reverb; ws: a
    reverb_fft_workspace(B, Smax, Lcap, device), taken here when None.  -> out (B, Smax) f32."""
    _chk_f32(wav, rir, out, ws)
    _chk_i32(wav_len, rir_idx, rir_len, rir_peak)
    B, Smax = wav.shape
    assert rir.dim() == 2 and wav_len.numel() == B and rir_idx.numel() == B
    R, Lcap = rir.shape
    assert rir_len.numel() == R and rir_peak.numel() == R
    out = torch.empty(B, Smax, dtype=torch.float32, device=wav.device) if out is None else out
    assert tuple(out.shape) == (B, Smax)
    if ws is None:
        ws = reverb_fft_workspace(B, Smax, min(Lcap, REVERB_FFT_MAX_TAPS), wav.device)
    check(lib.asr_reverb_fft_fwd(_p(wav), _p(wav_len), _p(rir_idx), _p(rir), _p(rir_len), _p(rir_peak), _p(reverb_fft_twiddle(wav.device)), _p(out), _p(ws),
                                 ws.numel() * ws.element_size(), B, Smax, R, Lcap, _stream()), "asr_reverb_fft_fwd")
    return out


def noise_mix_workspace(B, Smax, device):
    """The per-tile energy partials of noise_mix (float64; asr_noise_mix_workspace_bytes)."""
    return torch.empty((lib.asr_noise_mix_workspace_bytes(B, Smax) + 7) // 8, dtype=torch.float64, device=device)


def noise_mix(wav, wav_len, par, noise, noise_off, out=None, gain_out=None, ws=None):
    """wav (B, Smax) f32 + gain x the noise clip par[b] = {clip index, start offset, 10^(-snr_dB / 20) as fp32 bits, 0} names, wrapped
    to the utterance's length; the gain makes the mix's signal-to-noise ratio the requested one (include/asr_hip.h:
    asr_noise_mix_fwd; data_handler.noise.NoiseBank holds noise / noise_off).  A clip index outside [0, N) copies the utterance.
    -> (out (B, Smax) f32, zero at and beyond each wav_len - out may be wav itself -, gain (B) f32)."""
    _chk_f32(wav, noise, out, gain_out)
    _chk_i32(wav_len, par, noise_off)
    B, Smax = wav.shape
    N = noise_off.numel() - 1
    assert wav_len.numel() == B and tuple(par.shape) == (B, 4) and noise.dim() == 1
    out = torch.empty(B, Smax, dtype=torch.float32, device=wav.device) if out is None else out
    gain_out = torch.empty(B, dtype=torch.float32, device=wav.device) if gain_out is None else gain_out
    assert tuple(out.shape) == (B, Smax) and gain_out.numel() == B
    if ws is None:
        ws = noise_mix_workspace(B, Smax, wav.device)
    check(lib.asr_noise_mix_fwd(_p(wav), _p(wav_len), _p(par), _p(noise), _p(noise_off), _p(out), _p(gain_out), _p(ws), ws.numel() * ws.element_size(),
                                B, Smax, N, _stream()), "asr_noise_mix_fwd")
    return out, gain_out


# --------------------------------------------------------------------------------- global CMVN, streaming front end
STREAM_OPEN = _lib.STREAM_OPEN


def cmvn_accumulate(feat, wav_len, acc):
    """acc (2 n_mels + 1) float64 += per-bin sum, sum of squares and the frame count of the valid frames of feat (B, Tmax, n_mels)
    (include/asr_hip.h: asr_cmvn_accumulate)."""
    _chk_f32(feat)
    _chk_i32(wav_len)
    B, Tmax, n_mels = feat.shape
    if acc.dtype != torch.float64 or not acc.is_contiguous() or acc.numel() != 2 * n_mels + 1:
        raise ValueError(f"acc must be a contiguous float64 tensor of 2 * n_mels + 1 = {2 * n_mels + 1} elements")
    assert wav_len.numel() == B
    check(lib.asr_cmvn_accumulate(_p(feat), _p(wav_len), _p(acc), B, Tmax, n_mels, _stream()), "asr_cmvn_accumulate")
    return acc


def global_norm_lfr(feat, wav_len, mean, istd, m, n, Tlfr_max, dtype=torch.float32, masks=None):
    """utt_norm_lfr under global CMVN: (x - mean[bin]) * istd[bin]; mean, istd (n_mels) f32."""
    return _norm_aug_lfr("asr_global_norm_augment_lfr_fwd", feat, wav_len, m, n, Tlfr_max, dtype, mean, istd, masks=masks)


def _specaug_ranges(ranges, B, counts):
    """(ranges pointer, ld, n_t, n_f, n_s) of a specaug launch: ranges (B, >= width) int32 whose rows may lie ld >= width words apart."""
    n_t, n_f, n_s = (int(v) for v in counts)
    width = 2 + 2 * n_t + 2 * n_f + 3 * n_s
    if ranges.dtype != torch.int32 or ranges.dim() != 2 or ranges.shape[0] != B or ranges.shape[1] < width or (ranges.shape[1] > 1 and ranges.stride(1) != 1):
        raise ValueError(f"ranges must be (B = {B}, >= {width}) int32 with unit column stride, got {tuple(ranges.shape)} {ranges.dtype}")
    if min(n_t, n_f, n_s) < 0 or max(n_t, n_f, n_s) > _lib.SPECAUG_MAX_RANGES:
        raise ValueError(f"n_t, n_f, n_s = {n_t}, {n_f}, {n_s}: each 0 .. {_lib.SPECAUG_MAX_RANGES}")
    return _p(ranges), (ranges.stride(0) if B > 1 else ranges.shape[1]), n_t, n_f, n_s


def utt_norm_specaug_lfr(feat, wav_len, ranges, counts, m, n, Tlfr_max, dtype=torch.float32):
    """utt_norm_lfr with a SpecAugment policy (include/asr_hip.h; tests/specaug_ref.py): ranges (B, width) int32 rows
    [wc, ww | (t0, t1) x n_t | (f0, f1) x n_f | (s, e, p) x n_s], counts = (n_t, n_f, n_s)."""
    return _norm_aug_lfr("asr_utt_norm_specaug_lfr_fwd", feat, wav_len, m, n, Tlfr_max, dtype, policy=(ranges, counts))


def global_norm_specaug_lfr(feat, wav_len, ranges, counts, mean, istd, m, n, Tlfr_max, dtype=torch.float32):
    """global_norm_lfr with a SpecAugment policy: utt_norm_specaug_lfr under global CMVN, on the tiled grid of the no-mask call."""
    return _norm_aug_lfr("asr_global_norm_specaug_lfr_fwd", feat, wav_len, m, n, Tlfr_max, dtype, mean, istd, policy=(ranges, counts))


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def stream_append(pcm, par, wav_ring, pcm_off, max_new):
    """Samples pcm[b, pcm_off : pcm_off + n_new[b]] go behind the received[b] samples of ring b: par (B, 2) int32 = {received, n_new}."""
    _chk_f32(pcm, wav_ring)
    _chk_i32(par)
    B, S = pcm.shape
    assert tuple(par.shape) == (B, 2) and wav_ring.shape[0] == B and _pow2(wav_ring.shape[1]) and 0 <= pcm_off and pcm_off + max_new <= S
    check(lib.asr_stream_append(_p(pcm), _p(par), _p(wav_ring), B, S, int(pcm_off), int(max_new), wav_ring.shape[1], _stream()), "asr_stream_append")


def stream_logmel(wav_ring, par, window, melfb, feat_ring, max_new):
    """Frames t_begin .. t_begin + n_new - 1 of every utterance from its sample ring into its frame ring: par (B, 3) int32 =
    {t_begin, n_new, total samples or STREAM_OPEN}."""
    _chk_f32(wav_ring, window, melfb, feat_ring)
    _chk_i32(par)
    B, scap = wav_ring.shape
    _, fcap, n_mels = feat_ring.shape
    assert tuple(par.shape) == (B, 3) and feat_ring.shape[0] == B and melfb.shape == (201, n_mels) and window.numel() == 400
    check(lib.asr_stream_logmel(_p(wav_ring), _p(par), _p(window), _p(melfb), _p(feat_ring), B, int(max_new), scap, fcap, n_mels, _stream()),
          "asr_stream_logmel")


def fbank(wav, wav_len, window, melfb, Tmax, wav_scale, preemph, feat=None):
    """Kaldi fbank of wav (B, Smax) f32 -> (B, Tmax, n_mels) f32 (include/asr_hip.h: asr_fbank_fwd): window (400) f32, melfb (256, n_mels) f32."""
    _chk_f32(wav, window, melfb)
    _chk_i32(wav_len)
    B, Smax = wav.shape
    n_mels = melfb.shape[1]
    assert melfb.shape == (256, n_mels) and window.numel() == 400 and wav_len.numel() == B
    feat = torch.empty(B, Tmax, n_mels, dtype=torch.float32, device=wav.device) if feat is None else feat
    assert tuple(feat.shape) == (B, Tmax, n_mels)
    _chk_f32(feat)
    check(lib.asr_fbank_fwd(_p(wav), _p(wav_len), _p(window), _p(melfb), _p(feat), B, Smax, int(Tmax), n_mels, float(wav_scale), float(preemph), _stream()),
          "asr_fbank_fwd")
    return feat


def stream_fbank(wav_ring, par, window, melfb, feat_ring, max_new, wav_scale, preemph):
    """Kaldi fbank frames t_begin .. t_begin + n_new - 1 of every utterance from its sample ring into its frame ring: par (B, 2) int32 =
    {t_begin, n_new}."""
    _chk_f32(wav_ring, window, melfb, feat_ring)
    _chk_i32(par)
    B, scap = wav_ring.shape
    _, fcap, n_mels = feat_ring.shape
    assert tuple(par.shape) == (B, 2) and feat_ring.shape[0] == B and melfb.shape == (256, n_mels) and window.numel() == 400
    check(lib.asr_stream_fbank(_p(wav_ring), _p(par), _p(window), _p(melfb), _p(feat_ring), B, int(max_new), scap, fcap, n_mels, float(wav_scale),
                               float(preemph), _stream()), "asr_stream_fbank")


def stream_norm_lfr(feat_ring, par, mean, istd, m, n, C, dtype=torch.float32):
    """One encoder chunk (B, C, m n_mels) out of the frame rings under global CMVN: par (B, 3) int32 = {r_begin, n_rows, frames or STREAM_OPEN}."""
    _chk_f32(feat_ring, mean, istd)
    _chk_i32(par)
    B, fcap, n_mels = feat_ring.shape
    assert tuple(par.shape) == (B, 3) and mean.numel() == n_mels and istd.numel() == n_mels
    out = torch.empty(B, C, m * n_mels, dtype=dtype, device=feat_ring.device)
    check(lib.asr_stream_norm_lfr(_p(feat_ring), _p(par), _p(mean), _p(istd), _p(out), B, int(C), fcap, n_mels, m, n, _dt(out), _stream()),
          "asr_stream_norm_lfr")
    return out


VAD_CTX_MAX = _lib.VAD_CTX_MAX


def vad_energy(wav, wav_len, Tmax, E=None):
    """Raw log-energy of every snip_edges frame of wav (B, S) f32 -> E (B, Tmax) f32, zeros at and past each recording's frame count
    (include/asr_hip.h: asr_vad_energy)."""
    _chk_f32(wav, E)
    _chk_i32(wav_len)
    if wav.dim() != 2 or wav_len.numel() != wav.shape[0]:
        raise ValueError(f"vad_energy: wav must be (B, S) with one length per row, got {tuple(wav.shape)} and {wav_len.numel()} lengths")
    B, S = wav.shape
    E = torch.empty(B, int(Tmax), dtype=torch.float32, device=wav.device) if E is None else E
    assert tuple(E.shape) == (B, int(Tmax))
    check(lib.asr_vad_energy(_p(wav), _p(wav_len), _p(E), B, S, int(Tmax), _stream()), "asr_vad_energy")
    return E


def vad_decide(E, wav_len, params, ctx, speech=None, thr=None):
    """The speech mask (B, Tmax) uint8 and the threshold (B) f64 of the log-energies E (B, Tmax) f32: params (3) f64 on the device =
    {energy_threshold, energy_mean_scale, proportion_threshold}, ctx = frames_context (include/asr_hip.h: asr_vad_decide)."""
    _chk_f32(E)
    _chk_i32(wav_len)
    B, Tmax = E.shape
    if params.dtype != torch.float64 or params.numel() != 3 or not params.is_contiguous() or wav_len.numel() != B:
        raise ValueError("vad_decide: params must be 3 contiguous float64 values and wav_len one length per row of E")
    speech = torch.empty(B, Tmax, dtype=torch.uint8, device=E.device) if speech is None else speech
    thr = torch.empty(B, dtype=torch.float64, device=E.device) if thr is None else thr
    assert tuple(speech.shape) == (B, Tmax) and speech.dtype == torch.uint8 and speech.is_contiguous()
    assert thr.numel() == B and thr.dtype == torch.float64 and thr.is_contiguous()
    ws = torch.empty(max(lib.asr_vad_decide_workspace_bytes(B, Tmax) // 8, 1), dtype=torch.float64, device=E.device)
    check(lib.asr_vad_decide(_p(E), _p(wav_len), _p(params), _p(speech), _p(thr), _p(ws), B, Tmax, int(ctx), _stream()), "asr_vad_decide")
    return speech, thr


def segment_gather(wav, seg_rec, seg_start, seg_len, Smax, out=None):
    """N stretches of the recordings wav (B, S) f32 as a zero-padded batch (N, Smax) f32, bit for bit (include/asr_hip.h:
    asr_segment_gather).  seg_rec / seg_start / seg_len: N host integers each (lists or numpy) - checked here against the batch, since the
    kernel clamps a window to its row but cannot know how many rows there are - uploaded in one copy."""
    import numpy as np
    _chk_f32(wav, out)
    if wav.dim() != 2:
        raise ValueError(f"segment_gather: wav must be (B, S), got {tuple(wav.shape)}")
    B, S = wav.shape
    seg = np.asarray([seg_rec, seg_start, seg_len], dtype=np.int64).reshape(3, -1)
    N, Smax = seg.shape[1], int(Smax)
    if N < 1 or Smax < 1:
        raise ValueError(f"segment_gather: {N} segments into rows of {Smax} samples")
    bad = (seg[0] < 0) | (seg[0] >= B) | (seg[1] < 0) | (seg[2] < 0) | (seg[1] + seg[2] > S) | (seg[2] > Smax)
    if bad.any():
        n = int(np.argmax(bad))
        raise ValueError(f"segment_gather: segment {n} = samples [{seg[1, n]}, {seg[1, n] + seg[2, n]}) of recording {seg[0, n]} does not lie in a batch of "
                         f"{B} recordings of {S} samples, or is longer than Smax = {Smax}")
    dseg = torch.from_numpy(seg.astype(np.int32)).to(wav.device, non_blocking=True)
    out = torch.empty(N, Smax, dtype=torch.float32, device=wav.device) if out is None else out
    assert tuple(out.shape) == (N, Smax) and out.data_ptr() != wav.data_ptr()
    check(lib.asr_segment_gather(_p(wav), S, _p(dseg[0]), _p(dseg[1]), _p(dseg[2]), _p(out), N, Smax, _stream()), "asr_segment_gather")
    return out


def ctc_align_long_workspace_bytes(R, T_total, Lmax):
    """Bytes of back-pointer workspace ctc_align_long needs for R recordings of T_total frames in all and at most Lmax labels each."""
    return int(lib.asr_ctc_align_long_workspace_bytes(int(R), int(T_total), int(Lmax)))


def _ctc_align_long(name, rows, lse, row_off, labels, lab_off, blank, ws, fill=None):
    """The host checks and the launch of ctc_align_long (fill None) and ctc_align_long_filler (fill = (star, gap, gap_tail))."""
    import numpy as np
    if rows.dim() != 2 or rows.stride(1) != 1:
        raise ValueError(f"{name}: rows must be (sum T, V) with unit column stride, got {tuple(rows.shape)} / {rows.stride()}")
    Tt, V = rows.shape
    ld = rows.stride(0) if Tt > 1 else V
    if ld < V:
        raise ValueError(f"{name}: row stride {ld} below V = {V}")
    _chk_f32(lse)
    if lse.numel() != Tt:
        raise ValueError(f"{name}: lse holds {lse.numel()} values for {Tt} rows")
    ro, lo = np.asarray(row_off, dtype=np.int64).reshape(-1), np.asarray(lab_off, dtype=np.int64).reshape(-1)
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    R = ro.shape[0] - 1
    if R < 1 or lo.shape[0] != R + 1:
        raise ValueError(f"{name}: row_off holds {ro.shape[0]} and lab_off {lo.shape[0]} entries: R + 1 each, R >= 1")
    if ro[0] != 0 or lo[0] != 0 or (np.diff(ro) < 0).any() or (np.diff(lo) < 0).any() or ro[-1] != Tt or lo[-1] != lab.shape[0]:
        raise ValueError(f"{name}: offsets must ascend from 0 to the {Tt} rows and the {lab.shape[0]} labels (got {ro.tolist()}, {lo.tolist()})")
    Lmax = int(np.diff(lo).max())
    if Lmax > _lib.ALIGN_LONG_MAX_LABELS:
        r = int(np.argmax(np.diff(lo)))
        raise ValueError(f"{name}: recording {r} has {Lmax} labels, the limit is {_lib.ALIGN_LONG_MAX_LABELS}")
    if not 0 <= int(blank) < V:
        raise ValueError(f"{name}: blank = {blank} outside [0, {V})")
    bad = (lab < 0) | (lab >= V) | (lab == int(blank))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"{name}: label {i} = {int(lab[i])}: labels are classes in [0, {V}) other than the blank ({int(blank)})")
    if fill is not None:      # star (sum T) f32 without NaN, gap one flag per label, gap_tail one per recording
        star, gap, gap_tail = fill
        if not torch.is_tensor(star) or star.dtype != torch.float32 or star.dim() != 1 or star.numel() != Tt or not star.is_contiguous():
            raise ValueError(f"{name}: star must be a contiguous f32 tensor of {Tt} values, one per row (got {getattr(star, 'dtype', type(star))}, "
                             f"{tuple(getattr(star, 'shape', ()))})")
        if star.device != rows.device:
            raise ValueError(f"{name}: star lives on {star.device}, the rows on {rows.device}")
        if Tt and bool(torch.isnan(star).any()):
            raise ValueError(f"{name}: star holds NaN")
        g, gt = np.asarray(gap).reshape(-1), np.asarray(gap_tail).reshape(-1)
        if g.shape[0] != lab.shape[0]:
            raise ValueError(f"{name}: gap holds {g.shape[0]} flags for {lab.shape[0]} labels")
        if gt.shape[0] != R:
            raise ValueError(f"{name}: gap_tail holds {gt.shape[0]} flags for {R} recordings")
        g, gt = (g != 0).astype(np.uint8), (gt != 0).astype(np.uint8)
    dev = rows.device
    off = torch.from_numpy(np.concatenate((ro, lo)).astype(np.int32)).to(dev)
    dlab = torch.from_numpy(lab.astype(np.int32) if lab.shape[0] else np.zeros(1, np.int32)).to(dev)
    Ls = max(lab.shape[0], 1)
    path = torch.empty(max(Tt, 1), dtype=torch.int32, device=dev)
    spans = torch.empty(Ls, 2, dtype=torch.int32, device=dev)
    tok = torch.empty(Ls, 3, dtype=torch.float32, device=dev)
    score = torch.empty(R, dtype=torch.float64, device=dev)
    nbytes = ctc_align_long_workspace_bytes(R, Tt, Lmax)
    w = ws.get(nbytes) if ws is not None else torch.empty(max(nbytes, 64), dtype=torch.uint8, device=dev)
    if Tt == 0:      # no row to point at: the kernel reads none
        rows, lse = torch.zeros(1, V, dtype=rows.dtype, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    if fill is None:
        timed("ctc_align_long", 0.0, lambda: check(
            lib.asr_ctc_align_long(_p(rows), _p(lse), _p(off[:R + 1]), _p(dlab), _p(off[R + 1:]), _p(path), _p(spans), _p(tok), _p(score), _p(w), w.numel(),
                                   R, V, ld, _dt(rows), int(blank), _stream()), "asr_ctc_align_long"))
    else:
        flags = torch.from_numpy(np.concatenate((g if g.shape[0] else np.zeros(1, np.uint8), gt))).to(dev)
        ng = max(g.shape[0], 1)
        if Tt == 0:
            star = torch.zeros(1, dtype=torch.float32, device=dev)
        timed("ctc_align_long_filler", 0.0, lambda: check(
            lib.asr_ctc_align_long_filler(_p(rows), _p(lse), _p(star), _p(off[:R + 1]), _p(dlab), _p(off[R + 1:]), _p(flags), _p(flags[ng:]), _p(path), _p(spans),
                                          _p(tok), _p(score), _p(w), w.numel(), R, V, ld, _dt(rows), int(blank), _stream()), "asr_ctc_align_long_filler"))
    return path[:Tt], spans[:lab.shape[0]], tok[:lab.shape[0]], score


def ctc_align_long(rows, lse, row_off, labels, lab_off, blank=0, ws=None):
    """CTC forced alignment of whole recordings in one call (asr_ctc_align_long; the definition is tests/align_long_ref.py, and the kernel
    agrees with it bit for bit).  rows (sum T, V) f32 / bf16 on the device, dense or rows of a buffer padded to ld >= V elements; lse
    (sum T) f32 from ctc_frame_stats over the same rows; row_off / lab_off: R + 1 host integers (lists or numpy), recording r owns rows
    [row_off[r], row_off[r+1]) and labels [lab_off[r], lab_off[r+1]); labels: host integers (sum L).  Everything the kernel would have to
    trust is checked here, on the host: ascending offsets that end at the tables' sizes, at most ALIGN_LONG_MAX_LABELS labels per recording,
    labels in [0, V) other than the blank.  Returns device tensors (path (sum T) int32: the token's index within its recording per frame,
    -1 on blank frames; spans (sum L, 2) int32; tok (sum L, 3) f32 = the sum, the largest and the smallest log posterior over the token's
    frames; score (R) f64).  An infeasible recording has score -inf, spans -1, tok -inf and a path of -1."""
    return _ctc_align_long("ctc_align_long", rows, lse, row_off, labels, lab_off, blank, ws)


def ctc_align_long_filler(rows, lse, star, row_off, labels, lab_off, gap, gap_tail, blank=0, ws=None):
    """ctc_align_long with filler frames for audio the transcript does not cover (asr_ctc_align_long_filler; the definition is
    tests/align_filler_ref.py, and the kernel agrees with it bit for bit).  star (sum T) f32 on the device, indexed like lse: the
    log-probability of "anything" per frame; gap: host flags (sum L), gap[i] marks the blank in front of label i as wide; gap_tail: host
    flags (R), the blank behind a recording's last label.  A wide blank emits star[t] where star[t] > lp(t, blank) and the blank's value
    otherwise; path is -2 on the frames it does (filler frames), -1 on plain blank frames.  Returns what ctc_align_long returns and
    refuses what it refuses, and also (ValueError, on the host): a star that is not f32 or whose length is not the number of rows, NaN in
    star, a gap whose length is not the number of labels, a gap_tail whose length is not R."""
    return _ctc_align_long("ctc_align_long_filler", rows, lse, row_off, labels, lab_off, blank, ws, fill=(star, gap, gap_tail))


# ------------------------------------------------------------------------------------------------ keyword spotting (csrc/kws.hip)
def kws_search(logits, lse, in_len, tables, K_, cap, blank=0):
    """Every keyword of `tables` (the asr_kws_list of keywords.KeywordList.on) against logits (B, T, V), lse (B, T) from ctc_frame_stats
    (asr_kws_search).  Returns (cnt (B, K) int32: the hits per keyword, counting past cap; rec (B, K, cap, 3) int32 {start, end, score
    bits}: the first cap of each, in order of their end)."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len)
    _chk_f32(lse)
    assert lse.shape == (B, T) and (in_len is None or in_len.numel() == B)
    cnt = torch.empty(B, K_, dtype=torch.int32, device=logits.device)
    rec = torch.empty(B, K_, cap, 3, dtype=torch.int32, device=logits.device)
    check(lib.asr_kws_search(_p(logits), _p(lse), _p(in_len), ctypes.addressof(tables), _p(cnt), _p(rec), B, T, V, ld, int(blank), int(cap), _dt(logits),
                             _stream()), "asr_kws_search")
    return cnt, rec


def kws_state(slots, K_, device):
    """The state of asr_kws_chunk for `slots` sessions and K keywords, initialised (asr_kws_state_init): an int32 tensor."""
    state = torch.empty(lib.asr_kws_state_bytes(int(slots), int(K_)) // 4, dtype=torch.int32, device=device)
    check(lib.asr_kws_state_init(_p(state), int(slots), int(K_), _stream()), "asr_kws_state_init")
    return state


def kws_state_reset(state, flags, K_):
    """Slots b with flags[b] != 0 (int32, on the device) go back to the initial state (asr_kws_state_reset)."""
    _chk_i32(state, flags)
    check(lib.asr_kws_state_reset(_p(state), _p(flags), flags.numel(), int(K_), _stream()), "asr_kws_state_reset")


def kws_chunk(logits, lse, n_valid, reset, final, tables, K_, state, cap, blank=0):
    """One chunk of the resumable search (asr_kws_chunk): logits (slots, C, V), lse (slots, C), n_valid / reset / final (slots) int32,
    state from kws_state (updated in place).  Returns (cnt, rec) as kws_search, for the runs this chunk closed; frames count from the
    session's first frame."""
    slots, C, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(n_valid, reset, final, state)
    _chk_f32(lse)
    assert lse.shape == (slots, C) and n_valid.numel() == slots and reset.numel() == slots and final.numel() == slots
    assert state.numel() * 4 == lib.asr_kws_state_bytes(slots, int(K_))
    cnt = torch.empty(slots, K_, dtype=torch.int32, device=logits.device)
    rec = torch.empty(slots, K_, cap, 3, dtype=torch.int32, device=logits.device)
    check(lib.asr_kws_chunk(_p(logits), _p(lse), _p(n_valid), _p(reset), _p(final), ctypes.addressof(tables), _p(state), _p(cnt), _p(rec), slots, C, V, ld,
                            int(blank), int(cap), _dt(logits), _stream()), "asr_kws_chunk")
    return cnt, rec


def kws_compact(cnt, rec, max_hits, out=None):
    """(cnt, rec) of kws_search / kws_chunk -> (count (B), dropped (B), hits (B, max_hits, 4) int32 {keyword, start, end, score bits}) in
    the fixed order keyword ascending, then end ascending (asr_kws_compact).  The three are views of one int32 buffer of
    B * (2 + 4 max_hits) words (out, or a new one): one copy takes them to the host, kws_unpack reads them there."""
    _chk_i32(cnt, rec, out)
    B, K_, cap, _ = rec.shape
    assert cnt.shape == (B, K_)
    if out is None:
        out = torch.empty(B * (2 + 4 * int(max_hits)), dtype=torch.int32, device=cnt.device)
    count, dropped, hits = kws_unpack(out, B, max_hits)
    check(lib.asr_kws_compact(_p(cnt), _p(rec), _p(count), _p(dropped), _p(hits), B, K_, cap, int(max_hits), _stream()), "asr_kws_compact")
    return count, dropped, hits


def kws_unpack(flat, B, max_hits):
    """The views (count (B), dropped (B), hits (B, max_hits, 4)) of kws_compact's buffer, on the device or on the host."""
    assert flat.numel() == B * (2 + 4 * int(max_hits))
    return flat[:B], flat[B:2 * B], flat[2 * B:].view(B, int(max_hits), 4)


# ------------------------------------------------------------------------------------------------ token-level scoring (csrc/score.hip)
EDIT_LDS_DIR_BYTES, EDIT_MAX_REF = _lib.EDIT_LDS_DIR_BYTES, _lib.EDIT_MAX_REF
EDIT_COR, EDIT_SUB, EDIT_DEL, EDIT_INS = _lib.EDIT_COR, _lib.EDIT_SUB, _lib.EDIT_DEL, _lib.EDIT_INS


def _edit_mirrors(hyp_len, ref_len, ref_of):
    """The three small arrays as contiguous int32 numpy arrays (the launcher's host mirrors)."""
    return tuple(np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1)) for a in (hyp_len, ref_len, ref_of))


def edit_align_workspace_bytes(hyp_len, ref_len, ref_of, Lh, Lr):
    """Bytes of direction-mask workspace edit_align(ops=True) needs for these pairs (host integers): 0 when every pair's masks fit LDS
    (m * ceil(n / 64) * 16 <= EDIT_LDS_DIR_BYTES each)."""
    hl, rl, ro = _edit_mirrors(hyp_len, ref_len, ref_of)
    return int(lib.asr_edit_align_workspace_bytes(hl.ctypes.data, rl.ctypes.data, ro.ctypes.data, hl.shape[0], rl.shape[0], int(Lh), int(Lr)))


def edit_align(hyp, hyp_len, ref, ref_len, ref_of, host_hyp_len, host_ref_len, host_ref_of, ops=True, ws=None, counts=None, ops_out=None, n_ops=None):
    """Levenshtein alignment of P (hypothesis, reference) pairs in one launch (asr_edit_align; the definition is tests/score_ref.py, and
    the kernel agrees with it integer for integer).  hyp (P, Lh), ref (R, Lr) int32 id rows with unit column stride, hyp_len (P), ref_len
    (R), ref_of (P) int32 on the device: pair p is hyp row p against ref row ref_of[p].  host_*: the same three small arrays on the host
    (lists or numpy), by which the launcher checks ref_of and sizes LDS and workspace.  Returns (counts (P, 5) int32 {distance, cor, sub,
    del, ins}, ops (P, 3, ldo) int32 planes {code, ref_pos, hyp_pos} in forward order, n_ops (P)); ops=False: (counts, None, None), and
    neither direction masks nor a workspace.  counts / ops_out / n_ops: buffers to write into (views of one buffer make one copy back);
    ws: a Workspace, else the masks of pairs past the LDS budget get a fresh allocation."""
    _chk_i32(hyp_len, ref_len, ref_of, counts, ops_out, n_ops)
    for t in (hyp, ref):
        if t.dtype != torch.int32 or t.dim() != 2 or (t.shape[1] > 0 and t.stride(1) != 1):
            raise ValueError("edit_align: hyp and ref must be 2-D int32 tensors with unit column stride")
    P_, Lh = hyp.shape
    R, Lr = ref.shape
    ldh, ldr = (hyp.stride(0) if P_ > 1 and Lh > 0 else Lh), (ref.stride(0) if R > 1 and Lr > 0 else Lr)
    if hyp_len.numel() != P_ or ref_of.numel() != P_ or ref_len.numel() != R:
        raise ValueError(f"edit_align: {hyp_len.numel()} hypothesis lengths and {ref_of.numel()} ref_of for {P_} pairs, {ref_len.numel()} reference lengths for {R}")
    hl, rl, ro = _edit_mirrors(host_hyp_len, host_ref_len, host_ref_of)
    if hl.shape[0] != P_ or ro.shape[0] != P_ or rl.shape[0] != R:
        raise ValueError("edit_align: the host mirrors must have the device arrays' sizes")
    dev = hyp.device
    if counts is None:
        counts = torch.empty(P_, 5, dtype=torch.int32, device=dev)
    ldo, w, nbytes = 0, None, 0
    if ops:
        ldo = max(Lh + Lr, 1)
        if ops_out is None:
            ops_out = torch.empty(P_, 3, ldo, dtype=torch.int32, device=dev)
        if n_ops is None:
            n_ops = torch.empty(P_, dtype=torch.int32, device=dev)
        if ops_out.numel() != P_ * 3 * ldo or n_ops.numel() != P_:
            raise ValueError(f"edit_align: ops_out must hold {P_} x 3 x {ldo} words and n_ops {P_}")
        nbytes = int(lib.asr_edit_align_workspace_bytes(hl.ctypes.data, rl.ctypes.data, ro.ctypes.data, P_, R, Lh, Lr))
        if nbytes:
            w = ws.get(nbytes) if ws is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
            nbytes = w.numel()
    else:
        ops_out = n_ops = None
    if counts.numel() != P_ * 5:
        raise ValueError(f"edit_align: counts must hold {P_} x 5 words")
    # an empty tensor has no storage to point at: the kernel reads no id of a zero-length row
    one = torch.zeros(1, dtype=torch.int32, device=dev) if (hyp.numel() == 0 or ref.numel() == 0) else None
    check(lib.asr_edit_align(_p(hyp) if hyp.numel() else _p(one), _p(hyp_len), Lh, ldh, _p(ref) if ref.numel() else _p(one), _p(ref_len), Lr, ldr, _p(ref_of),
                             hl.ctypes.data, rl.ctypes.data, ro.ctypes.data, P_, R, _p(counts), _p(ops_out), _p(n_ops), ldo, _p(w), nbytes, _stream()),
          "asr_edit_align")
    return counts, ops_out, n_ops


# ------------------------------------------------------------------------------------------------ consensus of n-best lists (csrc/consensus.hip)
NBEST_MAX_N, NBEST_MAX_LEN, NBEST_MAX_ALTS, NBEST_EPS = _lib.NBEST_MAX_N, _lib.NBEST_MAX_LEN, _lib.NBEST_MAX_ALTS, _lib.NBEST_EPS
NBEST_STAGES = {"pair_dist": "asr_nbest_pair_dist", "pivot_votes": "asr_nbest_pivot_votes", "slot_vote": "asr_nbest_slot_vote", None: "asr_nbest_consensus"}


def nbest_out_words(U, N, L, alts):
    """int32 words of nbest_consensus' output buffer (asr_nbest_out_bytes / 4); raises for a shape the launcher would refuse."""
    nbytes = int(lib.asr_nbest_out_bytes(int(U), int(N), int(L), int(alts)))
    if not nbytes:
        raise ValueError(f"nbest_consensus: {_lib.last_error()}")
    return nbytes // 4


def nbest_unpack(flat, U, N, L, alts):
    """The views of nbest_consensus' buffer (an int32 tensor on the device or on the host, or a numpy array), in the order of
    include/asr_hip.h: {"risk" (U, N) int64, "d" (U, N, N), "pivot" (U), "W" (U), "extra" (U, N), "n_alts" (U, S), "pivot_w" (U, S),
    "votes" (U, N, S), "alts" (U, S, A, 2)} with S = 2 L + 1."""
    S = 2 * L + 1
    shapes = [("risk", (U, N, 2)), ("d", (U, N, N)), ("pivot", (U,)), ("W", (U,)), ("extra", (U, N)), ("n_alts", (U, S)), ("pivot_w", (U, S)),
              ("votes", (U, N, S)), ("alts", (U, S, alts, 2))]
    out, at = {}, 0
    for name, shp in shapes:
        n = int(np.prod(shp))
        out[name] = flat[at:at + n].reshape(shp)
        at += n
    if at != flat.shape[0]:
        raise ValueError(f"nbest_unpack: a buffer of {flat.shape[0]} words, the shape asks for {at}")
    out["risk"] = out["risk"].reshape(-1).view(torch.int64 if isinstance(flat, torch.Tensor) else np.int64).reshape(U, N)
    return out


def nbest_consensus(tok, ln, weights, host_len, host_weights, alts=4, out=None, stage=None):
    """Consensus decoding of U n-best lists in three launches (asr_nbest_consensus; the definition is tests/consensus_ref.py, and the
    kernels agree with it integer for integer).  tok (U, N, L) int32 ids with unit stride along L; ln (U, N) int32, -1 = absent; weights
    (U, N) int32 >= 0, at most 2**30 per utterance; host_len / host_weights: the two small arrays on the host (lists or numpy), by which
    the launcher refuses before any launch.  Returns the output buffer, an int32 tensor of nbest_out_words(U, N, L, alts) words
    (nbest_unpack gives its views); out: a buffer to write into.  stage: "pair_dist", "pivot_votes" or "slot_vote" launches that stage
    alone (the later ones read what the earlier ones wrote into `out`)."""
    _chk_i32(ln, weights, out)
    if tok.dtype != torch.int32 or tok.dim() != 3 or (tok.shape[2] > 0 and tok.stride(2) != 1):
        raise ValueError("nbest_consensus: tok must be a 3-D int32 tensor with unit stride along its last dimension")
    if stage not in NBEST_STAGES:
        raise ValueError(f"nbest_consensus: stage must be one of {[s for s in NBEST_STAGES if s]} or None (got {stage!r})")
    U, N, L = tok.shape
    if ln.shape != (U, N) or weights.shape != (U, N):
        raise ValueError(f"nbest_consensus: len {tuple(ln.shape)} and weights {tuple(weights.shape)} for {U} x {N} entries")
    hl = np.ascontiguousarray(np.asarray(host_len, dtype=np.int32).reshape(-1))
    hw = np.ascontiguousarray(np.asarray(host_weights, dtype=np.int32).reshape(-1))
    if hl.shape[0] != U * N or hw.shape[0] != U * N:
        raise ValueError("nbest_consensus: the host mirrors must have the device arrays' sizes")
    words = nbest_out_words(U, N, L, alts)
    if out is None:
        out = torch.empty(words, dtype=torch.int32, device=tok.device)
    if out.numel() != words:
        raise ValueError(f"nbest_consensus: out must hold {words} words")
    ldn = tok.stride(1) if N > 1 and L > 0 else L
    ldu = tok.stride(0) if U > 1 and L > 0 else max((N - 1) * ldn + L, 0)
    one = torch.zeros(1, dtype=torch.int32, device=tok.device) if tok.numel() == 0 else None      # an empty tensor has no storage to point at
    check(getattr(lib, NBEST_STAGES[stage])(_p(tok) if one is None else _p(one), _p(ln), _p(weights), L, ldn, ldu, hl.ctypes.data, hw.ctypes.data, U, N,
                                            int(alts), _p(out), words * 4, _stream()), NBEST_STAGES[stage])
    return out


# ------------------------------------------------------------------------------------------------ rescoring of n-best lists (csrc/rescore.hip)
RESCORE_MAX_N, RESCORE_MAX_K, RESCORE_MAX_G, RESCORE_MAX_U = _lib.RESCORE_MAX_N, _lib.RESCORE_MAX_K, _lib.RESCORE_MAX_G, _lib.RESCORE_MAX_U


def lm_score_nbest(tok, ln, host_len, lm, out=None):
    """The n-gram LM score of P finished strings in one launch (asr_lm_score_nbest; the definition is lm.NgramLM.score / walk, and the
    kernel agrees with them bit for bit).  tok (P, ld) int32 ids with unit column stride, ln (P) int32 on the device, -1 = absent; host_len:
    ln on the host (a list or numpy), by which the launcher refuses before the launch.  Returns (score (P) float64 = lm.score, bias (P)
    float64 and state (P) int32 = lm.walk, ntok (P) int32); an absent entry gives (0.0, 0.0, -1, 0).  out: a contiguous int32 buffer of
    6 P words, 8-byte aligned, to write into [score | bias | state | ntok] (one copy brings everything back)."""
    _chk_i32(ln, out)
    if tok.dtype != torch.int32 or tok.dim() != 2 or (tok.shape[1] > 0 and tok.stride(1) != 1):
        raise ValueError("lm_score_nbest: tok must be a 2-D int32 tensor with unit column stride")
    P_, L = tok.shape
    ld = tok.stride(0) if P_ > 1 and L > 0 else L
    hl = np.ascontiguousarray(np.asarray(host_len, dtype=np.int32).reshape(-1))
    if ln.numel() != P_ or hl.shape[0] != P_:
        raise ValueError(f"lm_score_nbest: {ln.numel()} lengths and {hl.shape[0]} host lengths for {P_} hypotheses")
    if P_ < 1:
        raise ValueError("lm_score_nbest: no hypotheses")
    dev = tok.device
    if out is None:
        out = torch.empty(6 * P_, dtype=torch.int32, device=dev)
    if out.numel() != 6 * P_:
        raise ValueError(f"lm_score_nbest: out must hold {6 * P_} words")
    score, bias = out[:2 * P_].view(torch.float64), out[2 * P_:4 * P_].view(torch.float64)
    state, ntok = out[4 * P_:5 * P_], out[5 * P_:]
    one = torch.zeros(1, dtype=torch.int32, device=dev) if tok.numel() == 0 else None      # an empty tensor has no storage to point at
    check(lib.asr_lm_score_nbest(_p(tok) if one is None else _p(one), _p(ln), hl.ctypes.data, P_, ld, ctypes.addressof(lm.on(dev)[1]), int(lm.has_eos),
                                 int(lm.eos), _p(score), _p(bias), _p(state), _p(ntok), _stream()), "asr_lm_score_nbest")
    return score, bias, state, ntok


def nbest_sweep_workspace_bytes(U, N, K, G):
    """Bytes of nbest_sweep's workspace (asr_nbest_sweep_workspace_bytes); raises for a shape the launcher would refuse."""
    nbytes = int(lib.asr_nbest_sweep_workspace_bytes(int(U), int(N), int(K), int(G)))
    if not nbytes:
        raise ValueError(f"nbest_sweep: {_lib.last_error()}")
    return nbytes


def nbest_sweep(feat, ln, err, grid, host_feat, host_len, host_grid, totals=False, ws=None, out_pick=None, out_tot=None, out_total=None):
    """The sweep of G weight vectors over U lists of N entries with K features (asr_nbest_sweep; the definition is tests/rescore_ref.py).
    feat (K, N, U) float64, ln (N, U) int32 (-1 = absent), err (3, N, U) int32 (sub, del, ins of every entry), grid (G, K) float64:
    contiguous device tensors; host_feat / host_len / host_grid: numpy arrays of the same layouts, by which the launcher refuses before any
    launch.  Returns (pick (G, U) int32, tot (G, 4) int64 = summed sub, del, ins and wrong utterances of the picks, total (G, U, N) float64
    with totals=True - the total of every present, scorable entry, -inf for the others - else None).  ws: a Workspace."""
    _chk_i32(ln, err, out_pick)
    for t, name in ((feat, "feat"), (grid, "grid"), (out_total, "out_total")):
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError(f"nbest_sweep: {name} must be a contiguous float64 tensor")
    if feat.dim() != 3 or grid.dim() != 2:
        raise ValueError("nbest_sweep: feat is (K, N, U) and grid (G, K)")
    K_, N, U_ = feat.shape
    G = grid.shape[0]
    if grid.shape[1] != K_ or tuple(ln.shape) != (N, U_) or tuple(err.shape) != (3, N, U_):
        raise ValueError(f"nbest_sweep: grid {tuple(grid.shape)}, len {tuple(ln.shape)} and err {tuple(err.shape)} for feat {tuple(feat.shape)}")
    hf = np.ascontiguousarray(np.asarray(host_feat, dtype=np.float64))
    hl = np.ascontiguousarray(np.asarray(host_len, dtype=np.int32))
    hg = np.ascontiguousarray(np.asarray(host_grid, dtype=np.float64))
    if hf.shape != (K_, N, U_) or hl.shape != (N, U_) or hg.shape != (G, K_):
        raise ValueError("nbest_sweep: the host mirrors must have the device arrays' shapes")
    nbytes = nbest_sweep_workspace_bytes(U_, N, K_, G)
    dev = feat.device
    w = ws.get(nbytes) if ws is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if out_pick is None:
        out_pick = torch.empty(G, U_, dtype=torch.int32, device=dev)
    if out_tot is None:
        out_tot = torch.empty(G, 4, dtype=torch.int64, device=dev)
    if totals and out_total is None:
        out_total = torch.empty(G, U_, N, dtype=torch.float64, device=dev)
    if out_pick.numel() != G * U_ or out_tot.dtype != torch.int64 or not out_tot.is_contiguous() or out_tot.numel() != G * 4 or \
            (out_total is not None and out_total.numel() != G * U_ * N):
        raise ValueError(f"nbest_sweep: out_pick holds {G} x {U_} int32, out_tot {G} x 4 int64 and out_total {G} x {U_} x {N} float64")
    check(lib.asr_nbest_sweep(_p(feat), _p(ln), _p(err), _p(grid), hf.ctypes.data, hl.ctypes.data, hg.ctypes.data, U_, N, K_, G, _p(out_pick), _p(out_tot),
                              _p(out_total), _p(w), w.numel(), _stream()), "asr_nbest_sweep")
    return out_pick, out_tot, out_total


# --------------------------------------------------------------------------------- MWER training of the CTC head (csrc/mwer.hip)
MWER_MAX_N, MWER_MAX_LEN, MWER_ABSENT, MWER_LONG = _lib.MWER_MAX_N, _lib.MWER_MAX_LEN, _lib.MWER_ABSENT, _lib.MWER_LONG


def _mwer_list(name, hyp, hyp_len):
    """(B, N, Lh, ldn, ldb) of an n-best list: hyp (B, N, Lh) int32 with unit stride along the tokens, hyp_len (B, N) int32 contiguous."""
    if hyp.dtype != torch.int32 or hyp.dim() != 3 or hyp.stride(2) != 1 and hyp.shape[2] > 1:
        raise ValueError(f"{name}: hyp is (B, N, Lh) int32 with unit stride along the tokens")
    _chk_i32(hyp_len)
    B, N, Lh = hyp.shape
    if tuple(hyp_len.shape) != (B, N):
        raise ValueError(f"{name}: hyp_len {tuple(hyp_len.shape)} for hyp {tuple(hyp.shape)}")
    ldn = hyp.stride(1) if N > 1 else Lh
    ldb = hyp.stride(0) if B > 1 else max((N - 1) * ldn + Lh, 1)
    return B, N, Lh, ldn, ldb


def ctc_mwer_workspace_bytes(B, N, T, Lh):
    """Bytes of the workspace ctc_mwer_lattice fills and ctc_mwer_grad reads (asr_ctc_mwer_workspace_bytes); raises for a shape the
    launchers would refuse."""
    nbytes = int(lib.asr_ctc_mwer_workspace_bytes(int(B), int(N), int(T), int(Lh)))
    if not nbytes:
        raise ValueError(f"ctc_mwer: {_lib.last_error()}")
    return nbytes


def mwer_errors(hyp, hyp_len, ref, ref_len, err=None, flags=None):
    """The Levenshtein distance of every entry of an n-best list to its utterance's reference (asr_mwer_errors), lengths read on the
    device only.  hyp (B, N, Lh) int32, hyp_len (B, N) int32 (-1 = absent), ref (B, Lr) int32, ref_len (B) int32.
    Returns (err (B, N) int32, flags (B, N) int32: 0, MWER_ABSENT or MWER_LONG; a flagged entry has err 0)."""
    B, N, Lh, ldn, ldb = _mwer_list("mwer_errors", hyp, hyp_len)
    _chk_i32(ref_len, err, flags)
    if ref.dtype != torch.int32 or ref.dim() != 2 or ref.shape[0] != B or (ref.stride(1) != 1 and ref.shape[1] > 1) or ref_len.numel() != B:
        raise ValueError("mwer_errors: ref is (B, Lr) int32 with unit stride along the tokens, ref_len (B) int32")
    Lr = ref.shape[1]
    ldr = ref.stride(0) if B > 1 else max(Lr, 1)
    err = torch.empty(B, N, dtype=torch.int32, device=hyp.device) if err is None else err
    flags = torch.empty(B, N, dtype=torch.int32, device=hyp.device) if flags is None else flags
    assert err.numel() == B * N and flags.numel() == B * N
    check(lib.asr_mwer_errors(_p(hyp), _p(hyp_len), _p(ref), _p(ref_len), _p(err), _p(flags), B, N, Lh, ldn, ldb, Lr, ldr, _stream()), "asr_mwer_errors")
    return err, flags


def ctc_mwer_lattice(logits, in_len, hyp, hyp_len, err, blank=0, ws=None):
    """The CTC lattices of an n-best list (asr_ctc_mwer_lattice; the definition is tests/mwer_ref.py).  logits (B, T, V) f32 / bf16, dense
    or rows padded as the engine lays them out (only read); in_len (B) int32; the list as mwer_errors takes it; err (B, N) int32.
    Returns {"ll" (B, N) float64, "post", "coef" (B, N) float32, "risk" (B) float32, "present" (B, N) int32, "ws": the uint8 buffer
    ctc_mwer_grad needs}.  ws: a Workspace to take the buffer from."""
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    Bh, N, Lh, ldn, ldb = _mwer_list("ctc_mwer_lattice", hyp, hyp_len)
    _chk_i32(in_len, err)
    if Bh != B or in_len.numel() != B or err.numel() != B * N:
        raise ValueError(f"ctc_mwer_lattice: list {tuple(hyp.shape)}, in_len {tuple(in_len.shape)}, err {tuple(err.shape)} for logits {tuple(logits.shape)}")
    dev = logits.device
    nbytes = ctc_mwer_workspace_bytes(B, N, T, Lh)
    w = ws.get(nbytes) if ws is not None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = dict(ll=torch.empty(B, N, dtype=torch.float64, device=dev), post=torch.empty(B, N, dtype=torch.float32, device=dev),
               coef=torch.empty(B, N, dtype=torch.float32, device=dev), risk=torch.empty(B, dtype=torch.float32, device=dev),
               present=torch.empty(B, N, dtype=torch.int32, device=dev), ws=w)
    timed("ctc_mwer_lattice", 0.0, lambda: check(
        lib.asr_ctc_mwer_lattice(_p(logits), _p(in_len), _p(hyp), _p(hyp_len), _p(err), _p(out["ll"]), _p(out["post"]), _p(out["coef"]), _p(out["risk"]),
                                 _p(out["present"]), B, T, V, ld, N, Lh, ldn, ldb, int(blank), _p(w), w.numel(), _dt(logits), _stream()),
        "asr_ctc_mwer_lattice"))
    return out


def ctc_mwer_grad(dlogits, in_len, hyp, hyp_len, coef, ws, blank=0, grad_scale=1.0, grad_scale_div=None, accumulate=False):
    """The sparse MWER gradient (asr_ctc_mwer_grad): reads only the workspace ctc_mwer_lattice filled, the list, in_len and coef - never the
    logits.  dlogits (B, T, V) f32 / bf16, dense or padded rows.  accumulate=False: the whole block is written (zeros where the gradient
    is zero, columns past V untouched); accumulate=True: only the touched cells are read, added to and stored.  Returns dlogits."""
    B, T, V = dlogits.shape
    ld = _frame_rows(dlogits)
    Bh, N, Lh, ldn, ldb = _mwer_list("ctc_mwer_grad", hyp, hyp_len)
    _chk_i32(in_len)
    _chk_f32(coef, grad_scale_div)
    if Bh != B or in_len.numel() != B or coef.numel() != B * N:
        raise ValueError(f"ctc_mwer_grad: list {tuple(hyp.shape)}, in_len {tuple(in_len.shape)}, coef {tuple(coef.shape)} for dlogits {tuple(dlogits.shape)}")
    if ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise ValueError("ctc_mwer_grad: ws is the uint8 buffer of ctc_mwer_lattice")
    timed("ctc_mwer_grad", 0.0, lambda: check(
        lib.asr_ctc_mwer_grad(_p(dlogits), _p(in_len), _p(hyp), _p(hyp_len), _p(coef), B, T, V, ld, N, Lh, ldn, ldb, int(blank), float(grad_scale),
                              _p(grad_scale_div), int(bool(accumulate)), _p(ws), ws.numel(), _dt(dlogits), _stream()),
        "asr_ctc_mwer_grad"))
    return dlogits


def ctc_mwer(logits, in_len, hyp, hyp_len, ref, ref_len, blank=0, grad_scale=1.0, grad_scale_div=None, dlogits=None, accumulate=False,
             want_grad=True, ws=None):
    """MWER loss and gradient of an n-best list: mwer_errors, ctc_mwer_lattice and ctc_mwer_grad in order on the current stream.
    Returns the dict of ctc_mwer_lattice plus "err", "flags" and "dlogits" (None with want_grad=False).  dlogits=None: a fresh tensor laid
    out like the logits (accumulate must then be False).  The loss of the batch is grad_scale * risk.sum()."""
    err, flags = mwer_errors(hyp, hyp_len, ref, ref_len)
    out = ctc_mwer_lattice(logits, in_len, hyp, hyp_len, err, blank=blank, ws=ws)
    out.update(err=err, flags=flags, dlogits=None)
    if want_grad:
        if dlogits is None:
            if accumulate:
                raise ValueError("ctc_mwer: accumulate=True needs the dlogits to add to")
            dlogits = torch.empty_strided(logits.shape, logits.stride(), dtype=logits.dtype, device=logits.device)
        out["dlogits"] = ctc_mwer_grad(dlogits, in_len, hyp, hyp_len, out["coef"], out["ws"], blank=blank, grad_scale=grad_scale,
                                       grad_scale_div=grad_scale_div, accumulate=accumulate)
    return out


# --------------------------------------------------------------------------------- CR-CTC: consistency between two views (csrc/cr_ctc.hip)
CR_CTC_RESIDENT_MAX_V = _lib.CR_CTC_RESIDENT_MAX_V


def cr_ctc(logits, in_len, grad_scale=1.0, grad_scale_div=None, dlogits=None, accumulate=False, want_grad=True):
    """The consistency term between the two halves of a batch and its gradient (asr_cr_ctc_fwd_bwd; the definition is tests/cr_ctc_ref.py).
    logits (2P, T, V) f32 / bf16, dense or rows padded as the engine lays them out (only read): rows p and p + P are the two views of
    utterance p; in_len (2P) int32.  Returns {"cr" (P) f32: the term of every pair, "frame" (P, T) f32: its frames (0 past
    min(in_len[p], in_len[p + P])), "dlogits": grad_scale * d cr.sum() / d logits, None with want_grad=False}.
    dlogits: a block laid out like the logits that does not overlap them; None: a fresh one (accumulate must then be False).
    accumulate=False: every cell is written, zeros past the pair's frames; accumulate=True: added to in f32, frames past them untouched.
    grad_scale_div: optional 1-element f32 device tensor; the scale is then grad_scale / grad_scale_div[0]."""
    if logits.dim() != 3 or logits.shape[0] < 2 or logits.shape[0] % 2:
        raise ValueError(f"cr_ctc: logits {tuple(logits.shape)}: (2P, T, V), the two views of P utterances")
    R, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len)
    _chk_f32(grad_scale_div)
    if in_len.numel() != R:
        raise ValueError(f"cr_ctc: in_len {tuple(in_len.shape)} for logits {tuple(logits.shape)}")
    if grad_scale_div is not None and grad_scale_div.numel() != 1:
        raise ValueError("cr_ctc: grad_scale_div is a 1-element float32 device tensor")
    if not want_grad:
        if dlogits is not None or accumulate:
            raise ValueError("cr_ctc: want_grad=False takes neither dlogits nor accumulate")
    elif dlogits is None:
        if accumulate:
            raise ValueError("cr_ctc: accumulate=True needs the dlogits to add to")
        dlogits = torch.empty_strided(logits.shape, logits.stride(), dtype=logits.dtype, device=logits.device)
    elif dlogits.shape != logits.shape or dlogits.stride() != logits.stride() or dlogits.dtype != logits.dtype:
        raise ValueError(f"cr_ctc: dlogits {tuple(dlogits.shape)} {dlogits.stride()} {dlogits.dtype} is not laid out like the logits "
                         f"{tuple(logits.shape)} {logits.stride()} {logits.dtype}")
    P_ = R // 2
    frame = torch.empty(P_, T, dtype=torch.float32, device=logits.device)
    cr = torch.empty(P_, dtype=torch.float32, device=logits.device)
    e = logits.element_size()
    timed("cr_ctc", 0.0, lambda: check(
        lib.asr_cr_ctc_fwd_bwd(_p(logits), _p(in_len), _p(dlogits), _p(frame), _p(cr), P_, T, V, ld, float(grad_scale), _p(grad_scale_div),
                               int(bool(accumulate)), _dt(logits), _stream()),
        "asr_cr_ctc_fwd_bwd"), float(R) * T * V * e * (1.0 + (0.0 if dlogits is None else 2.0 if accumulate else 1.0)))
    return {"cr": cr, "frame": frame, "dlogits": dlogits}


# --------------------------------------------------------------------------------- intermediate CTC: the conditioning's softmax (csrc/interctc.hip)
INTERCTC_RESIDENT_MAX_V = _lib.INTERCTC_RESIDENT_MAX_V


def _like_frames(name, what, t, logits):
    if t.shape != logits.shape or t.stride() != logits.stride() or t.dtype != logits.dtype or t.device != logits.device:
        raise ValueError(f"{name}: {what} {tuple(t.shape)} {t.stride()} {t.dtype} is not laid out like "
                         f"{tuple(logits.shape)} {logits.stride()} {logits.dtype}")


def softmax_rows(logits, in_len, out=None):
    """Frame posteriors (asr_softmax_rows; the definition is tests/interctc_ref.py).  logits (B, T, V) f32 / bf16, dense or rows padded
    as the engine lays them out (only read); in_len (B) int32.  Returns `out`, laid out like the logits: softmax over the V classes on
    the frames t < in_len[b], zeros on the others; padding columns are not written.  out: a block laid out like the logits that does
    not overlap them; None: a fresh one."""
    if logits.dim() != 3:
        raise ValueError(f"softmax_rows: logits {tuple(logits.shape)}: (B, T, V)")
    B, T, V = logits.shape
    ld = _frame_rows(logits)
    _chk_i32(in_len)
    if in_len.numel() != B:
        raise ValueError(f"softmax_rows: in_len {tuple(in_len.shape)} for logits {tuple(logits.shape)}")
    if out is None:
        out = torch.empty_strided(logits.shape, logits.stride(), dtype=logits.dtype, device=logits.device)
    else:
        _like_frames("softmax_rows", "out", out, logits)
    e = logits.element_size()
    timed("softmax_rows", 0.0, lambda: check(
        lib.asr_softmax_rows(_p(logits), _p(in_len), _p(out), B, T, V, ld, _dt(logits), _stream()), "asr_softmax_rows"), 2.0 * B * T * V * e)
    return out


def softmax_bwd_add(p, dp, in_len, grad, accumulate=True):
    """Backward of softmax_rows (asr_softmax_bwd_add): grad[b, t] (+)= p (dp - sum_u p[u] dp[u]) on the frames t < in_len[b]; the other
    frames are untouched under accumulate and zeroed otherwise.  p, dp, grad (B, T, V) f32 / bf16 laid out alike; grad overlaps
    neither p nor dp.  Returns grad."""
    if p.dim() != 3:
        raise ValueError(f"softmax_bwd_add: p {tuple(p.shape)}: (B, T, V)")
    B, T, V = p.shape
    ld = _frame_rows(p)
    _chk_i32(in_len)
    if in_len.numel() != B:
        raise ValueError(f"softmax_bwd_add: in_len {tuple(in_len.shape)} for p {tuple(p.shape)}")
    _like_frames("softmax_bwd_add", "dp", dp, p)
    _like_frames("softmax_bwd_add", "grad", grad, p)
    e = p.element_size()
    timed("softmax_bwd_add", 0.0, lambda: check(
        lib.asr_softmax_bwd_add(_p(p), _p(dp), _p(in_len), _p(grad), B, T, V, ld, int(bool(accumulate)), _dt(p), _stream()),
        "asr_softmax_bwd_add"), (4.0 if accumulate else 3.0) * B * T * V * e)
    return grad
