"""The definition of the CR-CTC consistency term (include/asr_hip.h: asr_cr_ctc_fwd_bwd), torch on the CPU, float64 unless told otherwise.

A batch of R = 2 P rows holds P pairs: rows p and p + P are the two views of utterance p.  n = min(in_len[p], in_len[p + P]); for t < n,
with lp = log_softmax(z[., t]) and y = exp(lp) of each view,

    J[p, t] = 1/2 (KL(sg(y_b) || y_a) + KL(sg(y_a) || y_b)) = 1/2 sum_v (y_a - y_b)(lp_a - lp_b)        sg: the target side is a constant
    cr[p]   = sum_{t < n} J[p, t]
    d cr[p] / d z[p, t] = 1/2 (y_a - y_b),   d cr[p] / d z[p + P, t] = 1/2 (y_b - y_a),   exactly 0 for t >= n.

terms() is the expression autograd differentiates (the targets detached), explicit() the closed form; both take dtype=torch.float32
for the restatement that is the yardstick of the GPU tests' tolerances.  No device random numbers; inputs are finite logits (a -inf
logit is outside the contract)."""
import numpy as np
import torch


def _pairs(z, in_len):
    R, T, V = z.shape
    assert R >= 2 and R % 2 == 0, "rows p and p + P are the two views of utterance p"
    P = R // 2
    ln = torch.as_tensor(np.asarray(in_len, dtype=np.int64)).clamp(0, T)
    n = torch.minimum(ln[:P], ln[P:])
    live = torch.arange(T).view(1, T) < n.view(P, 1)      # (P, T): frames that take part
    return P, live


def terms(z, in_len):
    """(frame (P, T), cr (P)) of logits z (2P, T, V), in z's dtype and connected to z for autograd: the two KL terms with their targets
    detached.  Frames t >= n are 0."""
    P, live = _pairs(z, in_len)
    lp = torch.log_softmax(z, dim=-1)
    lpa, lpb = lp[:P], lp[P:]
    ya, yb = lpa.exp(), lpb.exp()
    kl_ba = (yb.detach() * (lpb.detach() - lpa)).sum(-1)      # KL(sg(y_b) || y_a)
    kl_ab = (ya.detach() * (lpa.detach() - lpb)).sum(-1)      # KL(sg(y_a) || y_b)
    frame = torch.where(live, 0.5 * (kl_ba + kl_ab), torch.zeros((), dtype=z.dtype))
    return frame, frame.sum(1)


def autograd(logits, in_len, dtype=torch.float64):
    """{"frame" (P, T), "cr" (P), "grad" (2P, T, V)} as float64 numpy arrays, computed in `dtype`: the gradient of cr.sum() by
    torch.autograd."""
    z = torch.as_tensor(logits).to(dtype).clone().requires_grad_(True)
    frame, cr = terms(z, in_len)
    g, = torch.autograd.grad(cr.sum(), z)
    return dict(frame=frame.detach().double().numpy(), cr=cr.detach().double().numpy(), grad=g.double().numpy())


def explicit(logits, in_len, dtype=torch.float64):
    """The same three arrays from the closed form: J = 1/2 sum (y_a - y_b)(lp_a - lp_b), gradient 1/2 (y_a - y_b) and its negation."""
    z = torch.as_tensor(logits).to(dtype)
    P, live = _pairs(z, in_len)
    lp = torch.log_softmax(z, dim=-1)
    y = lp.exp()
    d = y[:P] - y[P:]
    frame = torch.where(live, 0.5 * (d * (lp[:P] - lp[P:])).sum(-1), torch.zeros((), dtype=dtype))
    ga = torch.where(live.unsqueeze(-1), 0.5 * d, torch.zeros((), dtype=dtype))
    return dict(frame=frame.double().numpy(), cr=frame.sum(1).double().numpy(), grad=torch.cat([ga, -ga]).double().numpy())


def make_case(P, T, V, spread, lens=None, seed=0):
    """(logits float32 numpy (2P, T, V), in_len int32 numpy (2P)): normal draws times `spread`; lens=None: every row has T frames."""
    rng = np.random.RandomState(1000 * P + 100 * T + V + seed)
    logits = (rng.randn(2 * P, T, V) * spread).astype(np.float32)
    in_len = np.full(2 * P, T, np.int32) if lens is None else np.asarray(lens, np.int32)
    assert in_len.shape == (2 * P,)
    return logits, in_len
