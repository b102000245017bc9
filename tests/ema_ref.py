"""The definition of the exponential moving average of the parameters, in numpy.  This file is its only statement: the kernels
(csrc/misc.hip: asr_adam_ema_step, asr_ema_update) equal it bit for bit, so no test of the average carries a tolerance.

For optimizer step s >= 1 (the value asr_noam_hyper leaves in hyper[3]), p the parameter after that step's update, e the average before it:

    d    = min(float64(float32(decay)), (1.0 + s) / (10.0 + s))   if warmup else float64(float32(decay))     # float64
    omd  = float32(1.0 - d)                                                                                  # one rounding
    t    = float32(p - e);   u = float32(omd * t);   e' = float32(e + u)                                     # three float32 roundings, no FMA

numpy rounds every float32 operation on its own (there is no contraction in numpy), and float64 division is the correctly rounded one.
"""
import numpy as np


def decay_at(decay, step, warmup=True):
    """d of optimizer step `step` as a Python float (= float64)."""
    d = float(np.float32(decay))
    if warmup:
        s = float(step)
        d = min(d, (1.0 + s) / (10.0 + s))
    return d


def one_minus_decay(decay, step, warmup=True):
    return np.float32(1.0 - decay_at(decay, step, warmup))


def ema_update(e, p, decay, step, warmup=True):
    """e' for float32 arrays e, p (any shape); returns a new float32 array."""
    e = np.asarray(e, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    omd = one_minus_decay(decay, step, warmup)
    t = np.subtract(p, e, dtype=np.float32)
    u = np.multiply(omd, t, dtype=np.float32)
    return np.add(e, u, dtype=np.float32)


def ema_fold(e0, ps, decay, first_step=1, warmup=True):
    """The average after the parameter snapshots `ps` of steps first_step, first_step + 1, ...; e0 is the average before the first."""
    e = np.asarray(e0, dtype=np.float32).copy()
    for k, p in enumerate(ps):
        e = ema_update(e, p, decay, first_step + k, warmup)
    return e
