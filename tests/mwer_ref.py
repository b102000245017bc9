"""MWER over an n-best list for the CTC head: the definition (include/asr_hip.h: asr_ctc_mwer_lattice), torch on the CPU.

Utterance b has frames t < T_b = in_len[b], reference r_b and a list of N entries h_i with lengths n_i (-1 = absent), rows Lh wide.
    y_t     = softmax(x_t) over the logits as stored
    ll_i    = log p(h_i | x) = -F.ctc_loss(log_softmax(x), h_i, reduction="none")
    e_i     = the Levenshtein distance of h_i and r_b (tests/score_ref.py)
    entry i TAKES PART iff 0 <= n_i <= Lh, every id is in [0, V) and is not the blank, n_i + adjacent repeats <= T_b, and T_b > 0
    P_i     = exp(ll_i - logsumexp over the entries taking part);  risk_b = sum_i P_i e_i;  loss = scale * sum_b risk_b
    G[b,t,v] = scale * sum_i c_i gamma_i(t, v),  c_i = P_i (e_i - risk_b),
    gamma_i(t, v) = sum_{s: l'_s = v} alpha_t(s) beta_t(s) / (y_t(v) p(h_i | x))      (alpha and beta both include y_t)
An utterance with T_b = 0 or no entry taking part has risk 0, posteriors 0 and gradient 0.

Two statements of the same thing: `autograd` differentiates the loss through F.ctc_loss and a softmax over the list; `explicit` builds G
from the alpha / beta recursions in the log domain.  d ll_i / d x_t = gamma_i(t, .) - y_t and sum_i c_i = 0, so the dense -y_t terms
cancel: tests/test_mwer_cpu.py holds the two against each other.  `autograd` also runs in float32 (dtype=), which is the yardstick for
how far a kernel that sums in another order may be from the float64 numbers."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import score_ref

NEG_INF = float("-inf")


def distance(hyp, ref):
    return int(score_ref.table(ref, hyp)[-1, -1])


def entry(hyp, hyp_len, b, i):
    n = int(hyp_len[b, i])
    return [int(v) for v in hyp[b, i, :max(n, 0)]] if 0 <= n <= hyp.shape[2] else []


def takes_part(hyp, hyp_len, b, i, Tb, V, blank):
    n, Lh = int(hyp_len[b, i]), hyp.shape[2]
    if n < 0 or n > Lh or Tb <= 0:
        return False
    h = entry(hyp, hyp_len, b, i)
    if any(v < 0 or v >= V or v == blank for v in h):
        return False
    return n + sum(h[j] == h[j - 1] for j in range(1, n)) <= Tb


def errors(hyp, hyp_len, ref, ref_len):
    """(err (B, N), flags (B, N)) as asr_mwer_errors writes them: a flagged entry (1 = absent, 2 = longer than the row) has err 0."""
    hyp, hyp_len, ref, ref_len = (np.asarray(a) for a in (hyp, hyp_len, ref, ref_len))
    B, N, Lh = hyp.shape
    err, flags = np.zeros((B, N), np.int32), np.zeros((B, N), np.int32)
    for b in range(B):
        r = ref[b, :min(max(int(ref_len[b]), 0), ref.shape[1])]
        for i in range(N):
            n = int(hyp_len[b, i])
            flags[b, i] = 1 if n < 0 else (2 if n > Lh else 0)
            if not flags[b, i]:
                err[b, i] = distance(hyp[b, i, :n], r)
    return err, flags


def _ll(logp, h):
    """log p(h | x) of one utterance: logp (T_b, V) log-softmax rows, h a list of ids."""
    T = logp.shape[0]
    tgt = torch.tensor(h, dtype=torch.long).view(1, -1)
    return -F.ctc_loss(logp.unsqueeze(1), tgt, torch.tensor([T]), torch.tensor([len(h)]), blank=_ll.blank, reduction="none", zero_infinity=False)[0]


def risk_terms(x, in_len, hyp, hyp_len, err, blank=0):
    """The differentiable part: x (B, T, V) a torch tensor (any float dtype, autograd allowed) -> (risk (B) tensor of x's dtype, a list per
    utterance of (entries taking part, their ll tensor, their posterior tensor))."""
    hyp, hyp_len = np.asarray(hyp), np.asarray(hyp_len)
    B, T, V = x.shape
    N = hyp.shape[1]
    _ll.blank = blank
    risks, parts = [], []
    for b in range(B):
        Tb = min(max(int(in_len[b]), 0), T)
        idx = [i for i in range(N) if takes_part(hyp, hyp_len, b, i, Tb, V, blank)]
        if not idx:
            risks.append(torch.zeros((), dtype=x.dtype))
            parts.append(([], None, None))
            continue
        logp = F.log_softmax(x[b, :Tb], dim=-1)
        lls = torch.stack([_ll(logp, entry(hyp, hyp_len, b, i)) for i in idx])
        P = torch.softmax(lls, dim=0)
        e = torch.tensor([int(err[b, i]) for i in idx], dtype=x.dtype)
        risks.append((P * e).sum())
        parts.append((idx, lls, P))
    return torch.stack(risks), parts


def autograd(logits, in_len, hyp, hyp_len, ref, ref_len, blank=0, scale=1.0, dtype=torch.float64, err=None):
    """The loss through F.ctc_loss and a softmax over the list, and its autograd gradient.  logits (B, T, V), any float dtype: the stored
    values are upcast (or, with dtype=torch.float32, the whole definition runs in float32).  Returns a dict of numpy arrays: loss, ll (B, N;
    -inf where an entry does not take part), post, coef, risk (B), err, present, grad (B, T, V)."""
    hyp, hyp_len = np.asarray(hyp), np.asarray(hyp_len)
    B, T, V = logits.shape
    N = hyp.shape[1]
    if err is None:
        err = errors(hyp, hyp_len, ref, ref_len)[0]
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    risk, parts = risk_terms(x, in_len, hyp, hyp_len, err, blank)
    loss = scale * risk.sum()
    ll = np.full((B, N), NEG_INF)
    post, coef = np.zeros((B, N)), np.zeros((B, N))
    present = np.zeros((B, N), np.int32)
    for b, (idx, lls, P) in enumerate(parts):
        for k, i in enumerate(idx):
            ll[b, i], post[b, i], present[b, i] = float(lls[k].detach()), float(P[k].detach()), 1
            coef[b, i] = float((P[k] * (float(err[b, i]) - risk[b])).detach())
    grad = torch.zeros_like(x)
    if loss.requires_grad:
        grad, = torch.autograd.grad(loss, x)
    return dict(loss=float(loss.detach()), ll=ll, post=post, coef=coef, risk=risk.detach().double().numpy(), err=np.asarray(err), present=present,
                grad=grad.double().numpy())


def _lse(*cols):
    return torch.logsumexp(torch.stack(cols), dim=0)


def lattice(logp, h, blank=0):
    """(log alpha (T, S), log beta (T, S), ll, ext) of one entry on the blank-augmented sequence ext = l' (S = 2 n + 1), float64.
    Both recursions include y_t, so the posterior of state s at frame t is exp(alpha + beta - logp[t, l'_s] - ll)."""
    T, n = logp.shape[0], len(h)
    S = 2 * n + 1
    ext = torch.full((S,), blank, dtype=torch.long)
    ext[1::2] = torch.tensor(h, dtype=torch.long)
    lp = logp[:, ext]                                                   # (T, S)
    skip = torch.zeros(S, dtype=torch.bool)                              # s - 2 -> s
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    ninf = torch.full((2,), NEG_INF, dtype=logp.dtype)
    a = torch.full((T, S), NEG_INF, dtype=logp.dtype)
    a[0, :min(2, S)] = lp[0, :min(2, S)]
    for t in range(1, T):
        p = torch.cat([ninf, a[t - 1]])
        a[t] = lp[t] + _lse(p[2:], p[1:-1], torch.where(skip, p[:-2], ninf[0]))
    ll = torch.logsumexp(a[T - 1, max(S - 2, 0):], dim=0)
    skip_b = torch.zeros(S, dtype=torch.bool)                            # s -> s + 2
    skip_b[:-2] = skip[2:]
    bt = torch.full((T, S), NEG_INF, dtype=logp.dtype)
    bt[T - 1, max(S - 2, 0):] = lp[T - 1, max(S - 2, 0):]
    for t in range(T - 2, -1, -1):
        p = torch.cat([bt[t + 1], ninf])
        bt[t] = lp[t] + _lse(p[:-2], p[1:-1], torch.where(skip_b, p[2:], ninf[0]))
    return a, bt, ll, ext


def explicit(logits, in_len, hyp, hyp_len, ref, ref_len, blank=0, scale=1.0, err=None):
    """The same quantities from the alpha / beta recursions, float64, no autograd: G = scale * sum_i c_i gamma_i."""
    hyp, hyp_len = np.asarray(hyp), np.asarray(hyp_len)
    B, T, V = logits.shape
    N = hyp.shape[1]
    if err is None:
        err = errors(hyp, hyp_len, ref, ref_len)[0]
    x = logits.detach().double()
    ll = np.full((B, N), NEG_INF)
    post, coef, risk = np.zeros((B, N)), np.zeros((B, N)), np.zeros(B)
    present = np.zeros((B, N), np.int32)
    G = torch.zeros(B, T, V, dtype=torch.float64)
    for b in range(B):
        Tb = min(max(int(in_len[b]), 0), T)
        idx = [i for i in range(N) if takes_part(hyp, hyp_len, b, i, Tb, V, blank)]
        if not idx:
            continue
        logp = F.log_softmax(x[b, :Tb], dim=-1)
        lat = [lattice(logp, entry(hyp, hyp_len, b, i), blank) for i in idx]
        lls = torch.stack([l[2] for l in lat])
        P = torch.exp(lls - torch.logsumexp(lls, dim=0))
        e = torch.tensor([float(err[b, i]) for i in idx], dtype=torch.float64)
        r = (P * e).sum()
        c = P * (e - r)
        for k, i in enumerate(idx):
            a, bt, l, ext = lat[k]
            g = torch.exp(a + bt - logp[:, ext] - l)                    # (T_b, S) state posteriors
            G[b, :Tb].index_add_(1, ext, scale * c[k] * g)
            ll[b, i], post[b, i], coef[b, i], present[b, i] = float(l), float(P[k]), float(c[k]), 1
        risk[b] = float(r)
    return dict(loss=float(scale * risk.sum()), ll=ll, post=post, coef=coef, risk=risk, err=np.asarray(err), present=present, grad=G.numpy())


def touched(hyp, hyp_len, present, in_len, T, V, blank=0):
    """(B, T, V) bool: the cells the gradient may touch - rows t < T_b, the blank and the tokens of the entries taking part."""
    hyp, hyp_len = np.asarray(hyp), np.asarray(hyp_len)
    B, N, _ = hyp.shape
    m = np.zeros((B, T, V), bool)
    for b in range(B):
        Tb = min(max(int(in_len[b]), 0), T)
        cols = set()
        for i in range(N):
            if present[b, i]:
                cols.add(blank)
                cols.update(entry(hyp, hyp_len, b, i))
        for v in cols:
            m[b, :Tb, v] = True
    return m
