"""fp64 numpy restatement of one-pass joint CTC / attention decoding (Watanabe et al. 2017, "Hybrid CTC/Attention Architecture for
End-to-End Speech Recognition", section 3.2 and algorithm 2): the CTC prefix scorer and the search built on it.  The GPU kernels
(asr_ctc_prefix_score / asr_ctc_prefix_gather / asr_joint_beam_step) and decode.one_pass_beam_search are tested against it;
tests/test_joint_prefix_cpu.py pins the scorer against brute-force enumeration of every frame path.

State of a hypothesis g over the frames: r^n_t(g), r^b_t(g) = log-probability of the paths of frames 0..t whose collapse is g and
that end in a non-blank / a blank.  [sos]: r^n = -inf, r^b_t = sum_{tau <= t} log y_tau(blank).
"""
import numpy as np

NEG = -np.inf


def log_softmax(logits):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def sos_state(logp, blank=0):
    """(r^n, r^b) of [sos] over the T frames of logp (T, V)."""
    T = logp.shape[0]
    return np.full(T, NEG), np.cumsum(logp[:, blank])


def full_logprob(state, is_sos=False):
    """log p_ctc(g): every frame path spells exactly g.  [sos] over no frames is the empty labelling with probability 1."""
    rn, rb = state
    if len(rn) == 0:
        return 0.0 if is_sos else NEG
    return float(np.logaddexp(rn[-1], rb[-1]))


def extend(logp, state, last, c, is_sos, blank=0):
    """h = g + c for a label c (not eos): returns (log psi(h), state of h).  last = last label of g (None for [sos])."""
    T = logp.shape[0]
    rn_g, rb_g = state
    rn, rb = np.full(T, NEG), np.full(T, NEG)
    if c == blank:
        return NEG, (rn, rb)
    if T == 0:
        return NEG, (rn, rb)
    x, yb = logp[:, c], logp[:, blank]
    phi = rb_g if (not is_sos and c == last) else np.logaddexp(rn_g, rb_g)
    if is_sos:
        rn[0] = x[0]
    psi = rn[0]
    for t in range(1, T):
        rn[t] = np.logaddexp(rn[t - 1], phi[t - 1]) + x[t]
        rb[t] = np.logaddexp(rb[t - 1], rn[t - 1]) + yb[t]
        psi = np.logaddexp(psi, phi[t - 1] + x[t])
    return float(psi), (rn, rb)


def prefix_state(logp, prefix, blank=0):
    """(log psi(prefix), state of prefix) by extending [sos] token by token; the empty prefix has psi = 0."""
    st, psi, last = sos_state(logp, blank), 0.0, None
    for i, c in enumerate(prefix):
        psi, st = extend(logp, st, last, int(c), i == 0, blank)
        last = int(c)
    return psi, st


def prefix_logprob(logp, prefix, blank=0):
    return prefix_state(logp, prefix, blank)[0]


def topk_stable(lp, k):
    """The k largest entries of lp, ties by ascending index (asr_logsoftmax_topk's order)."""
    lp = np.asarray(lp)
    idx = np.argsort(-lp, kind="stable")[:k]
    return [(float(lp[i]), int(i)) for i in idx]


def one_pass_search(att_logp_of, logp, beam, pre_beam, maxlen, ctc_weight, sos, eos, blank=0, nbest=1):
    """The search of decode.one_pass_beam_search for one utterance.  att_logp_of(seq) -> (V,) attention log-probabilities of the next
    token after seq (sos included); logp (T, V) CTC log-probabilities of the utterance's frames.  Returns up to nbest dicts
    {yseq, score, att_score, ctc_score}, best first."""
    lam = float(ctc_weight)
    hyps = [dict(seq=[sos], score=0.0, att=0.0, psi=0.0, state=sos_state(logp, blank), sos=True)]
    ended = []
    for i in range(maxlen):
        cands = []
        for g in hyps:
            per = []
            for j, (v, c) in enumerate(topk_stable(att_logp_of(g["seq"]), pre_beam)):
                st, full = None, NEG
                if c == eos:
                    psi = full_logprob(g["state"], g["sos"])
                else:
                    last = None if g["sos"] else g["seq"][-1]
                    psi, st = extend(logp, g["state"], last, c, g["sos"], blank)
                    if psi > NEG:
                        full = full_logprob(st)
                inc = (1.0 - lam) * v + lam * (psi - g["psi"]) if psi > NEG else NEG
                per.append((inc, j, c, v, psi, st, full))
            per = sorted(per, key=lambda p: (-p[0], p[1]))[:beam]
            for inc, j, c, v, psi, st, full in per:
                cands.append(dict(g=g, total=g["score"] + inc, c=c, v=v, psi=psi, st=st, full=full))
        keep = sorted([x for x in cands if x["total"] > NEG], key=lambda x: -x["total"])[:beam]
        nxt = []
        for x in keep:
            g = x["g"]
            seq, att = g["seq"] + [x["c"]], g["att"] + x["v"]
            if x["c"] == eos:
                ended.append(dict(yseq=seq, score=x["total"], att_score=att, ctc_score=x["psi"]))
            elif i == maxlen - 1:
                ended.append(dict(yseq=seq + [eos], score=x["total"] + lam * (x["full"] - x["psi"]), att_score=att, ctc_score=x["full"]))
            else:
                nxt.append(dict(seq=seq, score=x["total"], att=att, psi=x["psi"], state=x["st"], sos=False))
        hyps = nxt
        if not hyps:
            break
    return sorted(ended, key=lambda h: -h["score"])[:nbest]
