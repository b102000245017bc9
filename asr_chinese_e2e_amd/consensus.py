"""Consensus decoding of n-best lists (asr_nbest_consensus, csrc/consensus.hip; the definition is tests/consensus_ref.py): the list is
treated as a posterior over strings.  The entry with the least expected edit distance to the others is the minimum-Bayes-risk pick (the
pivot); every entry is aligned to it and votes per position, which gives a confusion network with the posterior mass of its
alternatives, a consensus string that may be in no entry of the list, and a token confidence from the search's own alternatives.  Lists of
several searches combine by concatenation.

The device sees integers only: nbest_weights turns scores into weights on the host (float64), so a weight cannot differ by one between
runs or machines.  consensus_ids is one upload, three launches and one copy back; consensus_packed takes and returns device tensors."""
import numpy as np

WEIGHT_ONE = 1 << 20
MAX_WEIGHT_SUM = 1 << 30
MAX_N, MAX_LEN, MAX_ALTS, EPS = 64, 256, 8, -1      # ASR_NBEST_* of include/asr_hip.h


def nbest_weights(scores, scale=1.0):
    """int32 weights of one list's scores: q_k = exp(scale * s_k - max) / sum over the finite scores in float64, w_k = floor(q_k * 2**20 +
    0.5); a score of -inf gives 0.  The weights of a list sum to 2**20 within half its length."""
    scale = float(scale)
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError(f"nbest_weights: scale must be finite and > 0 (got {scale})")
    s = np.asarray(scores, dtype=np.float64).reshape(-1) * scale
    if np.isnan(s).any() or (s == np.inf).any():
        raise ValueError("nbest_weights: a score is NaN or +inf")
    w = np.zeros(s.shape[0], dtype=np.int32)
    fin = np.isfinite(s)
    if fin.any():
        e = np.exp(s[fin] - s[fin].max())
        w[fin] = np.floor(e / e.sum() * WEIGHT_ONE + 0.5).astype(np.int32)
    return w


def _check_alts(alts):
    if not 1 <= int(alts) <= MAX_ALTS:
        raise ValueError(f"alts = {alts}: between 1 and {MAX_ALTS} alternatives per slot")
    return int(alts)


def _host_arrays(lists, weights, scores, scale):
    """(tok (U, N, L) int32, len (U, N), weights (U, N)) of U lists of id lists; a None entry is absent."""
    U = len(lists)
    if U == 0:
        raise ValueError("consensus_ids: no lists")
    if weights is not None and scores is not None:
        raise ValueError("consensus_ids: weights or scores, not both")
    for name, per in (("weights", weights), ("scores", scores)):
        if per is not None and (len(per) != U or any(len(p) != len(l) for p, l in zip(per, lists))):
            raise ValueError(f"consensus_ids: {name} must match the lists entry for entry")
    N = max(len(l) for l in lists)
    if not 1 <= N <= MAX_N:
        raise ValueError(f"consensus_ids: a list of {N} entries, between 1 and {MAX_N} are taken")
    L = max((len(h) for l in lists for h in l if h is not None), default=0)
    if L > MAX_LEN:
        raise ValueError(f"consensus_ids: a hypothesis of {L} tokens, the limit is {MAX_LEN}")
    tok, ln, w = np.zeros((U, N, L), dtype=np.int32), np.full((U, N), -1, dtype=np.int32), np.zeros((U, N), dtype=np.int32)
    for u, l in enumerate(lists):
        for k, h in enumerate(l):
            if h is None:
                continue
            ids = np.asarray(h, dtype=np.int64).reshape(-1)
            if ids.shape[0] and (ids.min() < 0 or ids.max() > 2 ** 31 - 1):
                raise ValueError(f"consensus_ids: entry {k} of list {u} has an id outside [0, 2**31)")
            ln[u, k] = ids.shape[0]
            tok[u, k, :ids.shape[0]] = ids
        if not (ln[u] >= 0).any():
            raise ValueError(f"consensus_ids: list {u} has no entry")
        if weights is not None:
            wu = np.asarray(weights[u], dtype=np.int64).reshape(-1)
        elif scores is not None:
            wu = nbest_weights(scores[u], scale).astype(np.int64)
        else:      # no posterior: every entry counts alike
            wu = np.full(len(l), WEIGHT_ONE // max(len(l), 1), dtype=np.int64)
        if (wu < 0).any() or int(wu[ln[u, :len(l)] >= 0].sum()) > MAX_WEIGHT_SUM:
            raise ValueError(f"consensus_ids: the weights of list {u} must be >= 0 and sum to at most 2**30")
        w[u, :len(l)] = wu
    return tok, ln, w


def unpack_results(host, tok, ln, w, alts, sizes=None):
    """consensus_ids' result dicts from the output buffer's host views (kernels.nbest_unpack of a numpy array) and the host inputs;
    sizes: the entries of each list (the arrays pad the shorter lists with absent ones), None = all N."""
    U, N, _ = tok.shape
    out = []
    for u in range(U):
        n = N if sizes is None else sizes[u]
        p = int(host["pivot"][u])
        m = int(ln[u, p])
        W = int(host["W"][u])
        piv = tok[u, p, :m].tolist()
        al = host["alts"][u, :2 * m + 1].tolist()
        na = host["n_alts"][u, :2 * m + 1].tolist()
        risk = host["risk"][u, :n].tolist()
        slots = [{"pivot_pos": s // 2 if s & 1 else None,
                  "alternatives": [(None if t == EPS else t, x / W if W else 0.0) for t, x in al[s][:min(na[s], alts)]],
                  "n_alternatives": na[s]} for s in range(2 * m + 1)]
        out.append({"pivot": p, "mbr": piv, "consensus": [al[s][0][0] for s in range(2 * m + 1) if al[s][0][0] != EPS], "risk": risk,
                    "expected_errors": [r / W if W else 0.0 for r in risk],
                    "confidence": [x / W if W else 0.0 for x in host["pivot_w"][u, 1:2 * m + 1:2].tolist()], "slots": slots,
                    "extra_insertions": int(host["extra"][u].sum()), "weights": w[u, :n].tolist()})
    return out


def consensus_ids(lists, weights=None, scores=None, scale=1.0, alts=4, device="cuda"):
    """lists: U n-best lists of id lists (ids >= 0), best first; a None entry is absent.  weights: int weights per entry (>= 0, at most 2**30
    per list), or scores: log-scores that nbest_weights(scores, scale) turns into weights; with neither, every entry counts alike.
    Returns per list {"pivot" (the index of the minimum-Bayes-risk entry), "mbr" (its ids), "consensus" (the top vote of every slot),
    "risk" (per entry, int), "expected_errors" (risk / W), "confidence" (per token of mbr: the posterior mass voting for it), "slots"
    [{"pivot_pos": i | None for a gap, "alternatives": [(token | None, posterior)] the top `alts`, "n_alternatives"}],
    "extra_insertions" (tokens behind the first of an insertion run: they vote nowhere), "weights"}.  One upload, one copy back."""
    import torch

    from . import kernels as K
    alts = _check_alts(alts)
    tok, ln, w = _host_arrays(lists, weights, scores, scale)
    U, N, L = tok.shape
    buf = torch.from_numpy(np.concatenate((ln.reshape(-1), w.reshape(-1), tok.reshape(-1)))).to(device)      # the one upload
    d_ln, d_w, d_tok = buf[:U * N].view(U, N), buf[U * N:2 * U * N].view(U, N), buf[2 * U * N:].view(U, N, L)
    out = K.nbest_consensus(d_tok, d_ln, d_w, ln, w, alts=alts)
    host = K.nbest_unpack(out.cpu().numpy(), U, N, L, alts)      # the one copy back
    return unpack_results(host, tok, ln, w, alts, sizes=[len(l) for l in lists])


def consensus_packed(tok, ln, weights, host_ln, host_weights, alts=4):
    """The same for lists that are on the device already, in the prefix beam search's layout: tok (U, N, L) int32, ln (U, N) int32 (-1 =
    absent), weights (U, N) int32, with host copies of the two small arrays.  Returns device tensors {"pivot" (U), "W" (U), "risk" (U, N)
    int64, "d" (U, N, N), "extra" (U, N), "votes" (U, N, 2 L + 1), "alts" (U, 2 L + 1, alts, 2) = (token, weight), "n_alts", "pivot_w"
    (U, 2 L + 1)}: views of one buffer ("buffer"), so one copy brings everything back."""
    from . import kernels as K
    alts = _check_alts(alts)
    U, N, L = tok.shape
    if not 1 <= N <= MAX_N or L > MAX_LEN:
        raise ValueError(f"consensus_packed: {N} entries of {L} tokens; at most {MAX_N} of {MAX_LEN} are taken")
    out = K.nbest_consensus(tok, ln, weights, host_ln, host_weights, alts=alts)
    views = K.nbest_unpack(out, U, N, L, alts)
    views["buffer"] = out
    return views


def _strip(seq, sos, eos):
    seq = list(seq)
    seq = seq[1:] if seq and seq[0] == sos else seq
    return seq[:-1] if seq and seq[-1] == eos else seq


def search_lists(model, input, search, beam_size, nbest, **search_kwargs):
    """(lists of id lists, scores, the search's own result) of one pack through the CTC prefix beam search or the attention beam search;
    the attention search's sos / eos are stripped as scoring.evaluate strips them."""
    from .scoring import EOS_ID, SOS_ID
    if search not in ("ctc_prefix_beam", "attention_beam"):
        raise ValueError(f"search must be 'ctc_prefix_beam' or 'attention_beam' (got {search!r})")
    if not 1 <= int(nbest) <= MAX_N:
        raise ValueError(f"nbest = {nbest}: between 1 and {MAX_N}")
    fn = model.ctc_prefix_beam_search if search == "ctc_prefix_beam" else model.beam_search
    res = fn(input, int(beam_size), int(nbest), **search_kwargs)
    lists = [[_strip(h["yseq"], SOS_ID, EOS_ID) for h in utt] or [[]] for utt in res]
    scores = [[float(h["score"]) for h in utt] or [0.0] for utt in res]
    return lists, scores, res


def model_consensus(model, input, search="ctc_prefix_beam", beam_size=5, nbest=5, posterior_scale=1.0, alts=4, **search_kwargs):
    """model.consensus: the n-best lists of one pack through consensus_ids, the weights from the search's scores."""
    import torch
    scale = float(posterior_scale)
    if not np.isfinite(scale) or scale <= 0.0:
        raise ValueError(f"posterior_scale must be finite and > 0 (got {posterior_scale})")
    alts = _check_alts(alts)
    with torch.no_grad():
        lists, scores, res = search_lists(model, input, search, beam_size, nbest, **search_kwargs)
    got = consensus_ids(lists, scores=scores, scale=scale, alts=alts, device=input.wave.device)
    id2tok = model.vocab._id2token
    return [{"text": "".join(id2tok[x] if 0 <= x < len(id2tok) else "" for x in g["consensus"]), "ids": g["consensus"], "mbr_ids": g["mbr"],
             "mbr_rank": g["pivot"], "best_ids": l[0], "confidence": g["confidence"], "slots": g["slots"], "nbest": r}
            for g, l, r in zip(got, lists, res)]
