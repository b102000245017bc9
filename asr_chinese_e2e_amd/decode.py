"""Beam search of the attention decoder on the GPU.

Same search as the reference's Decoder.recognize_beam (Predictor/Models/transformer_official.py:
331-434) - see include/asr_hip.h for the exact rules - but batched over utterances x beams, one
token per live hypothesis per step through key/value caches, instead of re-running the whole
decoder over the growing prefix for every hypothesis in a Python loop.

Device state per step: scores / alive flags / last tokens (B, beam); per layer a self-attention
K|V cache (B*beam, Lcap, 2*H*dk) in two copies (the step's survivors are gathered by parent into
the other copy); the encoder-side K|V of every layer are projected once.  The hypotheses
themselves are (token, parent) records per step; the n-best lists are rebuilt on the host by
following the parents, in the order the reference's lists would have (steps ascending, beam order
inside a step, stable sort by score).
"""
import functools
import math
import os

import torch

from . import kernels as K

# cross attention of the beam search on the training attention kernel (all beams of an utterance as Tq = beam queries against the same K / V:
# 11 us) instead of the single-query decode kernel (one wave per (hypothesis, head): ~220 us per layer and step); False: the latter (tests)
USE_SDPA = True

SOS_ID, EOS_ID = 2, 3   # transformer_official.py:53-54
BLANK_ID = 0            # CTC blank = <pad>, as in the training loss


def beam_search(model, input, beam_size=5, nbest=1, decode_max_len=0, check_every=8):
    """input: the reference's batch Pack (wave, wave_len).  Returns, per utterance, a list of at most
    `nbest` dicts {'yseq': [sos, ..., eos], 'score': float} - recognize_beam's result format."""
    if beam_size < 1 or beam_size > 8:
        raise ValueError("beam_size must be in 1..8 (asr_beam_step merges beam*beam <= 64 candidates per wave)")
    eng = model._ensure_engine(input.wave.device)
    if not eng.use_decoder:
        raise RuntimeError("this model has no attention decoder; use ctc_greedy_search")
    was_training, eng.training = eng.training, False
    try:
        with torch.no_grad():
            return _search(model, eng, input, int(beam_size), int(nbest), int(decode_max_len), int(check_every))
    finally:
        eng.training = was_training


class _DecoderSteps:
    """The batched key/value-cache decoder of the searches: the encoder, the encoder-side K|V of every layer, the two cache copies;
    logits(i, last_tok) runs decoder step i for all R = B * beam hypotheses, gather(parent, i) reorders the caches by parent."""

    def __init__(self, model, eng, input, beam, decode_max_len):
        x = input.wave.to(eng.dtype).contiguous()
        self.wave_len = input.wave_len.to(torch.int32).contiguous()
        self.B, self.T, _ = x.shape
        self.dev = x.device
        self.eng, self.beam = eng, beam
        hd = eng.H * eng.dk
        self.enc, _ = model.encode(eng, x, self.wave_len)            # (B*T, d)
        self.maxlen = self.wave_len.clone() if decode_max_len == 0 else torch.full_like(self.wave_len, decode_max_len)
        self.Lcap = int(self.maxlen.max())
        if self.Lcap > eng.pe.shape[0]:
            raise ValueError(f"decode length {self.Lcap} exceeds the positional-encoding table ({eng.pe.shape[0]})")
        self.R = R = self.B * beam
        # encoder-side keys / values of every layer, once
        self.cross_kv = [cross.kv.fwd(self.enc) for _, cross, _ in eng.dec]            # (B*T, 2hd)
        self.caches = [torch.zeros(eng.L, R, self.Lcap, 2 * hd, dtype=eng.dtype, device=self.dev) for _ in range(2)]
        self.row_bytes = 2 * hd * self.caches[0].element_size()
        self.cur = 0
        self.use_sdpa = eng.dk == 64 and eng.dtype == torch.bfloat16 and USE_SDPA
        self.o_buf = torch.empty(R, hd, dtype=eng.dtype, device=self.dev) if self.use_sdpa else None
        self.lse_buf = None

    def logits(self, i, last_tok):
        eng, R, B, T, beam = self.eng, self.R, self.B, self.T, self.beam
        d, H, dk, Lcap = eng.d, eng.H, eng.dk, self.Lcap
        hd = H * dk
        cache = self.caches[self.cur]
        y = K.embed_pe_fwd(last_tok.reshape(-1), eng.emb32, eng.pe[i:i + 1], d ** -0.5, R, 1, eng.dtype)   # :369-371
        for l, (slf, cross, ffn) in enumerate(eng.dec):
            q = slf.q.fwd(y)
            slf.kv.fwd(y, out=cache[l, :, i, :])                          # this step's key | value straight into the cache
            kv = cache[l].view(R * Lcap, 2 * hd)
            o = K.decode_attn(q, kv[:, :hd], kv[:, hd:], H, dk, Lcap, kv_div=1, k_len_uniform=i + 1)
            y, _, _ = K.add_ln_fwd(slf.fc.fwd(o), y, slf.ln.g, slf.ln.b, None, None, R, 1)
            q = cross.q.fwd(y)
            ckv = self.cross_kv[l]
            if self.use_sdpa:
                # the beams of an utterance are `beam` query rows against the SAME encoder keys / values: that is the training
                # attention kernel at Tq = beam (one workgroup per (utterance, head), K / V fetched once for all beams, MFMA) -
                # 11 us against ~220 us for the one-wave-per-(row, head) decode kernel, which was 48 of the 65 ms of a search
                o, self.lse_buf = K.sdpa_fwd(q, ckv[:, :hd], ckv[:, hd:], self.wave_len, B, H, beam, T, dk, o=self.o_buf, lse=self.lse_buf)
            else:
                o = K.decode_attn(q, ckv[:, :hd], ckv[:, hd:], H, dk, T, kv_div=beam, k_len=self.wave_len, len_div=beam)
            y, _, _ = K.add_ln_fwd(cross.fc.fwd(o), y, cross.ln.g, cross.ln.b, None, None, R, 1)
            h = ffn.w1.fwd(y, act=1)
            y, _, _ = K.add_ln_fwd(ffn.w2.fwd(h), y, ffn.ln.g, ffn.ln.b, None, None, R, 1)
        return eng.prj.fwd(y)                                             # tied projection, no bias (:379)

    def gather(self, parent, i):
        K.cache_gather(self.caches[self.cur], self.caches[self.cur ^ 1], parent.reshape(-1), self.eng.L, self.R, self.beam, self.Lcap, i + 1,
                       self.row_bytes)
        self.cur ^= 1


def _search(model, eng, input, beam, nbest, decode_max_len, check_every):
    dec = _DecoderSteps(model, eng, input, beam, decode_max_len)
    B, Lcap, dev = dec.B, dec.Lcap, dec.dev
    score = torch.zeros(B, beam, dtype=torch.float32, device=dev)
    alive = torch.zeros(B, beam, dtype=torch.int32, device=dev)
    alive[:, 0] = 1                                                       # one hypothesis [sos] per utterance
    last_tok = torch.full((B, beam), SOS_ID, dtype=torch.int32, device=dev)
    parent = torch.zeros(B, beam, dtype=torch.int32, device=dev)
    rec_tok = torch.zeros(Lcap, B, beam, dtype=torch.int32, device=dev)
    rec_par = torch.zeros_like(rec_tok)
    rec_end = torch.zeros_like(rec_tok)
    rec_score = torch.full((Lcap, B, beam), float("-inf"), dtype=torch.float32, device=dev)
    alive_total = torch.zeros(Lcap, dtype=torch.int32, device=dev)
    steps_done = 0
    for i in range(Lcap):
        logits = dec.logits(i, last_tok)
        vals, ids = K.logsoftmax_topk(logits, beam)
        K.beam_step(vals, ids, score, alive, last_tok, parent, rec_tok, rec_par, rec_end, rec_score, dec.maxlen, alive_total[i:i + 1],
                    B, beam, i, EOS_ID)
        steps_done = i + 1
        if i + 1 < Lcap:
            dec.gather(parent, i)
        if (i % check_every) == check_every - 1 and int(alive_total[i]) == 0:   # the only host sync of the loop
            break
    return _backtrace(rec_tok[:steps_done].cpu(), rec_par[:steps_done].cpu(), rec_end[:steps_done].cpu(), rec_score[:steps_done].cpu(), B, beam, nbest)


def _backtrace(rec_tok, rec_par, rec_end, rec_score, B, beam, nbest, extra=None):
    """extra: optional {name: (steps, B, beam) tensor} of per-record values that each entry carries under `name`."""
    steps = rec_tok.shape[0]
    # plain nested lists: element access on a tensor costs ~1 us each, and this walk touches ~50 k of them per batch
    # (33 of the 97 ms of a B = 32, beam 5 search before)
    rec_tok, rec_par, rec_end, rec_score = rec_tok.tolist(), rec_par.tolist(), rec_end.tolist(), rec_score.tolist()
    extra = {k: v.tolist() for k, v in (extra or {}).items()}
    out = []
    for b in range(B):
        ended = []                                           # in the order the reference appends to ended_hyps
        for i in range(steps):
            end_i = rec_end[i][b]
            for k in range(beam):
                e = end_i[k]
                if not e:
                    continue
                seq, kk = [], k
                for s in range(i, -1, -1):
                    seq.append(rec_tok[s][b][kk])
                    kk = rec_par[s][b][kk]
                seq = [SOS_ID] + seq[::-1] + ([EOS_ID] if e == 2 else [])
                ended.append((rec_score[i][b][k], seq, {n: v[i][b][k] for n, v in extra.items()}))
        ended = sorted(ended, key=lambda h: h[0], reverse=True)[: min(len(ended), nbest)]
        out.append([{"yseq": seq, "score": sc, **ex} for sc, seq, ex in ended])
    return out


# --------------------------------------------------------------------------------------------- CTC prefix beam search
def _logadd(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = a if a > b else b
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def _bias_mode(context, lm):
    """What a biased search adds to an entry, or None without a context and an LM: (the entry's key, the function (state, raw bias) ->
    the reported term).  A context reports bias - held(state): an unfinished phrase earns nothing; an LM reports lm_score = bias +
    term(</s> | state) (NgramLM.final)."""
    if context is not None:
        return "bias", lambda state, bias: bias - context.held(state)
    if lm is not None:
        return "lm_score", lm.final
    return None


def _bias_entries(key, final, tok, ln, sc, bias, state, nbest=None):
    """One utterance's result list of a biased search from its outputs in beam rank order (rows of tokens, lengths with -1 for missing
    ranks, log p, raw bias, state): entry[key] = final(state, raw bias), score = ctc_score + entry[key], ordered by score (a stable sort of
    the rank order), cut to nbest."""
    out = []
    for r in range(len(ln)):
        if ln[r] < 0:
            continue
        term = final(int(state[r]), float(bias[r]))
        out.append({"yseq": [int(x) for x in tok[r][:ln[r]]], "score": float(sc[r]) + term, "ctc_score": float(sc[r]), key: term})
    out.sort(key=lambda h: h["score"], reverse=True)
    return out if nbest is None else out[:nbest]


def context_entries(context, tok, ln, sc, bias, state, nbest=None):
    """_bias_entries under hotword biasing: 'bias' = raw bias - held(context state)."""
    return _bias_entries(*_bias_mode(context, None), tok, ln, sc, bias, state, nbest)


def lm_entries(lm, tok, ln, sc, bias, state, nbest=None):
    """_bias_entries with an n-gram LM over the LM kernels' outputs: 'lm_score' = bias + the end-of-sentence term."""
    return _bias_entries(*_bias_mode(None, lm), tok, ln, sc, bias, state, nbest)


def _check_lm(model, lm, context=None):
    from .lm import NgramLM
    if not isinstance(lm, NgramLM):
        raise TypeError(f"lm must be an lm.NgramLM (got {type(lm).__name__})")
    if context is not None:
        raise ValueError("an n-gram LM (lm=...) and a hotword context (context=...) cannot be combined: the search runs one of the two")
    lm.check_vocab(model.V)


def _check_context(model, context):
    from .context import ContextGraph
    if not isinstance(context, ContextGraph):
        raise TypeError(f"context must be a context.ContextGraph (got {type(context).__name__})")
    context.check_vocab(model.V)


def blank_skip_kept(blank_lp, n, thr):
    """The frames t < n that blank_skip keeps, in order (the definition: tests/blank_skip_ref.py): frame t is high iff blank_lp[t] > thr
    (both float32 values; a NaN is not high) and dropped iff it and frame t - 1 are high."""
    kept, prev = [], False
    for t in range(n):
        high = blank_lp[t] > thr
        if not (high and prev):
            kept.append(t)
        prev = high
    return kept


def ctc_prefix_beam_search(model, input, beam_size=5, nbest=1, frame_topk=10, on_device=None, context=None, context_ids=None, lm=None, beam_times=False,
                           confidence="post_max", blank_skip=None):
    """CTC prefix beam search (Hannun et al. 2014, algorithm 1 without a language model) over the CTC head's posteriors:
    per utterance a list of at most `nbest` dicts {'yseq': [ids], 'score': log p(yseq | x)}, best first.
    Everything runs on the GPU: encoder, CTC projection, per frame the `frame_topk` best classes with their log-softmax values
    plus the blank's (asr_ctc_frame_topk), and the prefix bookkeeping itself (asr_ctc_prefix_beam: one wave per utterance,
    prefixes as trie nodes; 2 ms per batch of 32 x 500 frames against 630 ms for the host loop below).  on_device=False (or a
    beam / top-k beyond the kernel's beam * (frame_topk + 1) <= 64) selects the host loop over the same candidates - the
    restatement the kernel is tested against, written like the reference's own search (a host loop, transformer_official.py:358-420).
    SURVEY.md 8(f) rank 1; the reference has no CTC (its greedy_search / beam_search are empty stubs, :106-110).
    context (a context.ContextGraph): hotword biasing - hypotheses that spell the graph's phrases are preferred (candidates of a frame
    are ranked by log p + bias; only tokens among the frame's `frame_topk` can be chosen).  context_ids[b] = the graph of utterance b
    (None: graph 0 for all, -1: not biased).  Entries are then {'yseq', 'score' = ctc_score + bias, 'ctc_score' = log p(yseq | x),
    'bias'}, ordered by score.  Without a context the call and its result are unchanged.
    lm (an lm.NgramLM): n-gram LM shallow fusion - candidates of a frame are ranked by log p + the hypothesis's accumulated weighted LM
    log-probability (only tokens among the frame's `frame_topk` can be chosen).  Entries are then {'yseq', 'score' = ctc_score +
    lm_score, 'ctc_score' = log p(yseq | x), 'lm_score' (the end-of-sentence term included)}, ordered by score.  Not with a context.
    beam_times=True (the device search only, not with a context or an LM): the search carries the best single alignment of every prefix
    (asr_ctc_prefix_beam_timed); entries gain 'viterbi_score' (its log-probability) and 'tokens' = per token {"id", "token", "start_frame",
    "end_frame", "start_s", "end_s", "measures": {post_max, post_min, post_mean}, "confidence"}, times as tokens() of the greedy streams;
    confidence picks the measure reported as "confidence".
    blank_skip=p in (0, 1] (every mode above, the host loop included): blank-frame skipping - a frame whose blank posterior is above p
    (log p(blank) > float32(log p), strict) and whose predecessor's is too is dropped before the search (asr_ctc_blank_skip_compact
    between the two kernels); the head of every run of such frames stays, so a doubled character keeps its separating blank.  The
    result is by definition the search on the kept frames: 'score' / 'ctc_score' sum over them only, and the frames of beam_times are
    mapped back to real frames (asr_frame_index_remap).  p = 1 keeps every frame; None (the default) launches what is launched without it."""
    if context is None and context_ids is not None:
        raise ValueError("context_ids needs a context")
    thr = None if blank_skip is None else K.blank_skip_threshold(blank_skip)
    which = None
    if beam_times:
        from .confidence import beam_times_check
        which = beam_times_check("prefix_beam", model.use_ctc, context, lm, confidence)
        if on_device is not None and not on_device:
            raise ValueError("beam_times=True runs the device search only (on_device=False is the host loop without times)")
    if lm is not None:
        _check_lm(model, lm, context)
    eng = model._ensure_engine(input.wave.device)
    if not eng.use_ctc:
        raise RuntimeError("this model has no CTC head (config.ctc_weight = 0)")
    was_training, eng.training = eng.training, False
    try:
        with torch.no_grad():
            out = model.forward(input)
    finally:
        eng.training = was_training
    logits = out.ctc_logits                                    # (B, T, V)
    B, T, V = logits.shape
    roots = None
    if context is not None:
        _check_context(model, context)
        graphs = [0] * B if context_ids is None else [int(g) for g in context_ids]
        roots = context.roots(graphs, B)
    biased = _bias_mode(context, lm)
    k = max(1, min(int(frame_topk), V))
    vals, ids, blank_lp = K.ctc_frame_topk(logits.reshape(B * T, V), k, BLANK_ID)
    fits = beam_size * (k + 1) <= 64 and beam_size <= 16 and nbest <= beam_size
    if on_device is None:
        on_device = fits or bool(beam_times)      # times come from the device search alone: a shape beyond it raises below
    if on_device:
        if not fits:
            raise ValueError(f"the device search ranks beam * (frame_topk + 1) <= 64 candidates per frame (beam {beam_size}, frame_topk {k})")
        in_len = input.wave_len.to(torch.int32).contiguous()
        frame_map = None
        if thr is not None:      # the search runs on the kept rows, with their count for its length
            vals, ids, blank_lp, in_len, frame_map = K.ctc_blank_skip_compact(vals, ids, blank_lp, in_len, thr, B, T)
        if biased is not None:      # the whole beam comes back: the reported term is settled on the host, then the order, then the cut to nbest
            res = K.ctc_prefix_beam(vals, ids, blank_lp, in_len, B, T, beam_size, beam_size, BLANK_ID, context=context, roots=roots, lm=lm)
            tok, ln, sc, bias, state = (t.cpu().tolist() for t in res)
            return [_bias_entries(*biased, tok[b], ln[b], sc[b], bias[b], state[b], nbest) for b in range(B)]
        if beam_times:
            from .confidence import beam_tokens
            res = K.ctc_prefix_beam(vals, ids, blank_lp, in_len, B, T, beam_size, nbest, BLANK_ID, times=True)
            # behind blank skipping the records count kept rows: the reported frames are the real ones, the measures stay over the kept rows
            real = None if frame_map is None else [K.frame_index_remap(res[i], frame_map).cpu().numpy() for i in (4, 5)]
            tok, ln, sc, vit, start, end, mx, mn, sm = (t.cpu().numpy() for t in res)
            d, id2tok = model.frame_seconds(), model.vocab._id2token
            return [[{"yseq": tok[b, r, :ln[b, r]].tolist(), "score": float(sc[b, r]), "viterbi_score": float(vit[b, r]),
                      "tokens": beam_tokens(tok[b, r, :ln[b, r]], *(x[b, r, :ln[b, r]] for x in (start, end, mx, mn, sm)), which, id2tok, d,
                                            real=None if real is None else [x[b, r, :ln[b, r]] for x in real])}
                     for r in range(nbest) if ln[b, r] >= 0] for b in range(B)]
        tok, ln, sc = K.ctc_prefix_beam(vals, ids, blank_lp, in_len, B, T, beam_size, nbest, BLANK_ID)
        tok, ln, sc = tok.cpu().tolist(), ln.cpu().tolist(), sc.cpu().tolist()
        return [[{"yseq": tok[b][r][:ln[b][r]], "score": sc[b][r]} for r in range(nbest) if ln[b][r] >= 0] for b in range(B)]
    vals, ids, blank_lp = vals.view(B, T, k).cpu().tolist(), ids.view(B, T, k).cpu().tolist(), blank_lp.view(B, T).cpu().tolist()
    lens = input.wave_len.cpu().tolist()
    results = []
    for b in range(B):
        if biased is not None:       # the same loop; a prefix's (state, bias) is a function of the prefix (ContextGraph.walk / NgramLM.walk)
            walk = functools.partial(context.walk, graphs[b]) if context is not None else lm.walk
            walked = {}

            def rank(kv):
                if kv[0] not in walked:
                    walked[kv[0]] = walk(kv[0])
                tot = _logadd(kv[1][0], kv[1][1])
                return tot + walked[kv[0]][1] if tot != -math.inf else tot
        else:
            rank = lambda kv: _logadd(kv[1][0], kv[1][1])      # noqa: E731
        beam = {(): (0.0, -math.inf)}                        # prefix -> (log p ending in blank, log p ending in a symbol)
        for t in (range(int(lens[b])) if thr is None else blank_skip_kept(blank_lp[b], int(lens[b]), thr)):
            lb = blank_lp[b][t]
            nxt = {}
            for prefix, (pb, pnb) in beam.items():
                tot = _logadd(pb, pnb)
                cur = nxt.setdefault(prefix, [-math.inf, -math.inf])
                cur[0] = _logadd(cur[0], tot + lb)
                last = prefix[-1] if prefix else None
                for c, lp in zip(ids[b][t], vals[b][t]):
                    if c == BLANK_ID:
                        continue
                    if c == last:
                        cur = nxt.setdefault(prefix, [-math.inf, -math.inf])
                        cur[1] = _logadd(cur[1], pnb + lp)       # repeated symbol, no blank in between: same prefix
                        new = nxt.setdefault(prefix + (c,), [-math.inf, -math.inf])
                        new[1] = _logadd(new[1], pb + lp)        # after a blank: a new symbol
                    else:
                        new = nxt.setdefault(prefix + (c,), [-math.inf, -math.inf])
                        new[1] = _logadd(new[1], tot + lp)
            ranked = sorted(nxt.items(), key=rank, reverse=True)[:beam_size]
            beam = {p: (v[0], v[1]) for p, v in ranked}
        if biased is not None:
            key, final = biased
            ents = []
            for p, v in sorted(beam.items(), key=rank, reverse=True):
                tot = _logadd(v[0], v[1])
                if tot == -math.inf:
                    continue
                x = final(*walk(p))
                ents.append({"yseq": list(p), "score": tot + x, "ctc_score": tot, key: x})
            results.append(sorted(ents, key=lambda h: h["score"], reverse=True)[:nbest])
            continue
        final = sorted(((p, _logadd(v[0], v[1])) for p, v in beam.items()), key=lambda kv: kv[1], reverse=True)[:nbest]
        results.append([{"yseq": list(p), "score": sc} for p, sc in final])
    return results


# --------------------------------------------------------------------------------------------- joint CTC / attention rescoring
def joint_beam_search(model, input, beam_size=5, nbest=1, decode_max_len=0, ctc_weight=0.3):
    """Two-pass joint decoding (Watanabe et al. 2017): the attention decoder's beam search proposes `beam_size` hypotheses per
    utterance, the CTC head scores each of them with the forward algorithm (the training kernel asr_ctc_fwd_bwd without the
    gradient, one lattice per hypothesis), and the list is re-ranked by ctc_weight * log p_ctc + (1 - ctc_weight) * log p_att.
    Returns per utterance at most `nbest` dicts {'yseq', 'score', 'att_score', 'ctc_score'}.  Hypotheses that contain the blank
    id (the attention decoder may emit <pad>) cannot be spelled by CTC: ctc_score = -inf."""
    eng = model._ensure_engine(input.wave.device)
    if not (eng.use_ctc and eng.use_decoder):
        raise RuntimeError("joint rescoring needs a model with both the attention decoder and the CTC head (0 < config.ctc_weight < 1)")
    hyps = beam_search(model, input, beam_size, beam_size, decode_max_len)
    was_training, eng.training = eng.training, False
    try:
        with torch.no_grad():
            logits = model.forward(input).ctc_logits          # (B, T, V)
    finally:
        eng.training = was_training
    B, T, V = logits.shape
    dev = logits.device
    n = beam_size
    labels, ok = [], []
    for b in range(B):
        for j in range(n):
            toks = hyps[b][j]["yseq"][1:-1] if j < len(hyps[b]) else []
            good = j < len(hyps[b]) and BLANK_ID not in toks and len(toks) <= 255
            labels.append(toks if good else [])
            ok.append(good)
    Lmax = max(1, max(len(l) for l in labels))
    lab = torch.zeros(B * n, Lmax, dtype=torch.int32)
    for r, l in enumerate(labels):
        if l:
            lab[r, : len(l)] = torch.tensor(l, dtype=torch.int32)
    lab_len = torch.tensor([len(l) for l in labels], dtype=torch.int32)
    rep = logits.repeat_interleave(n, dim=0).contiguous()     # one copy of the utterance's lattice input per hypothesis
    in_len = input.wave_len.to(torch.int32).repeat_interleave(n).contiguous()
    nll, _ = K.ctc_fwd_bwd(rep, in_len, lab.to(dev), lab_len.to(dev), eng.ws, blank=BLANK_ID, want_grad=False)
    nll = nll.cpu().tolist()
    out = []
    for b in range(B):
        cands = []
        for j, h in enumerate(hyps[b]):
            ctc = -nll[b * n + j] if ok[b * n + j] else -math.inf
            cands.append(dict(yseq=h["yseq"], att_score=h["score"], ctc_score=ctc, score=ctc_weight * ctc + (1.0 - ctc_weight) * h["score"]))
        out.append(sorted(cands, key=lambda c: c["score"], reverse=True)[:nbest])
    return out


# --------------------------------------------------------------------------------------------- attention rescoring of a CTC n-best (U2)
def attention_rescore(model, enc, wave_len, nbest_lists, ctc_weight):
    """Second pass of the U2 recipe (Zhang et al. 2020; WeNet's attention_rescoring): the decoder scores the CTC search's n-best
    teacher-forced in ONE forward pass and the list is re-ranked.  enc (B, T, d): the encoder output (offline or streamed), wave_len
    (B,): its valid frames, nbest_lists: per utterance at most n {'yseq': ids without sos / eos, 'score': the prefix beam's score}.
    Over the N = B * n hypotheses: input [sos] + y, target y + [eos], cross-attention over all T encoder rows with key length
    wave_len (the mask of beam_search / _DecoderSteps, not the ref_compat training mask); att_score = the sum of the target's
    log-probabilities (asr_xent_fwd_bwd without the gradient, summed per hypothesis).  The encoder rows are repeated per hypothesis, as
    joint_beam_search repeats its logits.  Returns per utterance the list sorted by score = ctc_weight * ctc_score + (1 - ctc_weight) *
    att_score (joint_beam_search's convention; ties keep the CTC order), entries {'yseq', 'score', 'att_score', 'ctc_score'}.  Missing
    ranks are skipped, an empty hypothesis scores log p(eos | sos), a hypothesis longer than the positional-encoding table admits gets
    att_score = score = -inf and so stays behind the others in its CTC order.
    Entries of a hotword-biased search (they carry 'bias' and a pure 'ctc_score'): score = ctc_weight * (ctc_score + bias) + (1 -
    ctc_weight) * att_score; ctc_score stays pure and 'bias' is kept.  Entries of a search with an n-gram LM (they carry 'lm_score'): score =
    ctc_weight * (ctc_score + lm_score) + (1 - ctc_weight) * att_score; ctc_score and att_score are unchanged by the LM."""
    eng = model._ensure_engine(enc.device)
    if not eng.use_decoder:
        raise RuntimeError("attention rescoring needs a model with the attention decoder")
    B, T = enc.shape[0], enc.shape[1]
    if len(nbest_lists) != B:
        raise ValueError(f"{len(nbest_lists)} n-best lists for a batch of {B}")
    n = max([len(l) for l in nbest_lists] + [0])
    if n == 0:
        return [[] for _ in range(B)]
    lam = float(ctc_weight)
    limit = eng.pe.shape[0] - 1                                # [sos] + y takes len(y) + 1 positions
    seqs = [[[int(x) for x in l[j]["yseq"]] if j < len(l) else [] for j in range(n)] for l in nbest_lists]
    # id 0 is the padding the decoder's target preparation drops: a hypothesis that holds it (no CTC search spells the blank) cannot be
    # teacher-forced as it is spelled and is treated like one that does not fit
    fits = [[len(y) <= limit and BLANK_ID not in y for y in row] for row in seqs]
    Lmax = max([len(y) for row, f in zip(seqs, fits) for y, ok in zip(row, f) if ok] + [1])
    N = B * n
    tgt = torch.zeros(N, Lmax, dtype=torch.int64)
    for b in range(B):
        for j, y in enumerate(seqs[b]):
            if y and fits[b][j]:
                tgt[b * n + j, : len(y)] = torch.tensor(y, dtype=torch.int64)
    dev = enc.device
    was_training, eng.training = eng.training, False
    try:
        with torch.no_grad():
            prep = K.dec_preprocess(tgt.to(dev), SOS_ID, EOS_ID)
            rep = enc.reshape(B, T, -1).to(eng.dtype).repeat_interleave(n, dim=0).reshape(N * T, -1).contiguous()
            cross_len = wave_len.to(torch.int32).repeat_interleave(n).contiguous()
            pred, _ = eng.decoder_fwd(prep, rep, cross_len, N, T)
            row_nll, _ = K.xent_fwd_bwd(pred.contiguous(), prep[1].reshape(-1), prep[5], BLANK_ID, smoothing=0.0, want_grad=False)
    finally:
        eng.training = was_training
    att = (-row_nll.view(N, Lmax + 1).cpu().double().sum(dim=1)).tolist()      # padded target rows (id 0) carry 0
    out = []
    for b in range(B):
        cands = []
        for j, h in enumerate(nbest_lists[b]):
            a = att[b * n + j] if fits[b][j] else -math.inf
            key = "bias" if "bias" in h else "lm_score" if "lm_score" in h else None      # a biased first pass: its term joins the CTC score
            ctc = float(h["score"] if key is None else h["ctc_score"])
            first = ctc if key is None else ctc + float(h[key])
            cand = dict(yseq=list(seqs[b][j]), score=lam * first + (1.0 - lam) * a if a != -math.inf else -math.inf, att_score=a, ctc_score=ctc)
            if key is not None:
                cand[key] = float(h[key])
            cands.append(cand)
        out.append(sorted(cands, key=lambda c: c["score"], reverse=True))
    return out


def ctc_rescore_search(model, input, beam_size=5, nbest=1, ctc_weight=0.0, frame_topk=10, context=None, context_ids=None, lm=None, blank_skip=None):
    """The U2 two-pass search offline: ctc_prefix_beam_search with n-best = beam_size, then attention_rescore of that list against the
    same encoder output (the encoder runs once).  Returns per utterance at most `nbest` {'yseq' (no sos / eos), 'score', 'att_score',
    'ctc_score'}.  context / context_ids: the first pass is hotword-biased (ctc_prefix_beam_search); entries gain 'bias'.  lm: the first
    pass runs with the n-gram LM; entries gain 'lm_score'.  blank_skip: the first pass skips blank frames (ctc_prefix_beam_search); the
    decoder pass is what it is."""
    if blank_skip is not None:
        K.blank_skip_threshold(blank_skip)      # refused before anything is launched
    if lm is not None:
        _check_lm(model, lm, context)
    eng = model._ensure_engine(input.wave.device)
    if not (eng.use_ctc and eng.use_decoder):
        raise RuntimeError("CTC n-best rescoring needs a model with both the attention decoder and the CTC head (0 < config.ctc_weight < 1)")
    was_training, eng.training = eng.training, False
    try:
        with torch.no_grad():
            enc = model.forward(input).encoder_out             # (B, T, d)
    finally:
        eng.training = was_training
    with model.given_encoder_output(enc):
        hyps = ctc_prefix_beam_search(model, input, beam_size, beam_size, frame_topk, context=context, context_ids=context_ids, lm=lm,
                                      blank_skip=blank_skip)
    res = attention_rescore(model, enc, input.wave_len, hyps, ctc_weight)
    return [r[:nbest] for r in res]


# --------------------------------------------------------------------------------------------- one-pass joint CTC / attention search
def default_pre_beam(beam_size):
    """Attention candidates per hypothesis of the one-pass search: min(16, int(1.5 * beam)), ESPnet's ratio."""
    return min(16, int(1.5 * beam_size))


def one_pass_beam_search(model, input, beam_size=5, nbest=1, decode_max_len=0, ctc_weight=0.3, pre_beam=None, check_every=8):
    """One-pass joint decoding (Watanabe et al. 2017, section 3.2 and algorithm 2): CTC shapes the beam while it is built.  At every
    step each live hypothesis g proposes its `pre_beam` best attention tokens c; each extension h = g + c is scored by
        (1 - ctc_weight) * log p_att(c | g, x) + ctc_weight * (log psi_ctc(h) - log psi_ctc(g)),
    psi_ctc the CTC prefix probability over all frames (asr_ctc_prefix_score; for c = eos the full-sequence probability of g);
    the `beam` best per hypothesis, then the `beam` best of the utterance survive (stable order), -inf extensions are dropped, eos
    ends a hypothesis, at step maxlen - 1 eos is appended to the rest, no length normalisation.
    Returns per utterance at most `nbest` dicts {'yseq', 'score', 'att_score', 'ctc_score'}, best first: att_score = the sum of the
    attention log-probabilities (plain beam_search's score of that yseq), ctc_score = log p_ctc(yseq without sos / eos), score =
    ctc_weight * ctc_score + (1 - ctc_weight) * att_score.  An utterance whose every extension is -inf gets an empty list."""
    if beam_size < 1 or beam_size > 8:
        raise ValueError("beam_size must be in 1..8 (asr_joint_beam_step merges beam*beam <= 64 candidates per wave)")
    eng = model._ensure_engine(input.wave.device)
    if not (eng.use_ctc and eng.use_decoder):
        raise RuntimeError("one-pass joint decoding needs a model with both the attention decoder and the CTC head (0 < config.ctc_weight < 1)")
    lam = float(ctc_weight)
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"one-pass joint decoding needs 0 < ctc_weight <= 1 (got {ctc_weight})")
    C = default_pre_beam(beam_size) if pre_beam is None else int(pre_beam)
    if C < beam_size or C > 16 or C > eng.V:
        raise ValueError(f"pre_beam must be in beam_size..min(16, vocabulary size) (got {C} for beam {beam_size})")
    was_training, eng.training = eng.training, False
    try:
        with torch.no_grad():
            return _one_pass(model, eng, input, int(beam_size), int(nbest), int(decode_max_len), lam, C, int(check_every))
    finally:
        eng.training = was_training


def _one_pass(model, eng, input, beam, nbest, decode_max_len, lam, C, check_every):
    dec = _DecoderSteps(model, eng, input, beam, decode_max_len)
    B, T, Lcap, R, dev = dec.B, dec.T, dec.Lcap, dec.R, dec.dev
    # the CTC head over the search's own encoder output, once: log-probabilities transposed to (B, V, T)
    lpT = K.ctc_prefix_logprobs(eng.ctc_lo.fwd(dec.enc).view(B, T, eng.V))
    st = [torch.empty(T, R, dtype=torch.float64, device=dev) for _ in range(2)]         # log r^b, log (r^n + r^b) of each hypothesis
    cand = [torch.empty(T, R * C, dtype=torch.float64, device=dev) for _ in range(2)]   # the same for every (hypothesis, candidate)
    score = torch.zeros(B, beam, dtype=torch.float32, device=dev)
    att_score = torch.zeros_like(score)
    ctc_score = torch.zeros_like(score)
    alive = torch.zeros(B, beam, dtype=torch.int32, device=dev)
    alive[:, 0] = 1                                                       # one hypothesis [sos] per utterance
    last_tok = torch.full((B, beam), SOS_ID, dtype=torch.int32, device=dev)
    parent = torch.zeros(B, beam, dtype=torch.int32, device=dev)
    rec_tok = torch.zeros(Lcap, B, beam, dtype=torch.int32, device=dev)
    rec_par = torch.zeros_like(rec_tok)
    rec_end = torch.zeros_like(rec_tok)
    rec_score = torch.full((Lcap, B, beam), float("-inf"), dtype=torch.float32, device=dev)
    rec_att = torch.full_like(rec_score, float("-inf"))
    rec_ctc = torch.full_like(rec_score, float("-inf"))
    alive_total = torch.zeros(Lcap, dtype=torch.int32, device=dev)
    top = None
    steps_done = 0
    for i in range(Lcap):
        logits = dec.logits(i, last_tok)
        att_vals, att_ids = K.logsoftmax_topk(logits, C)
        top = K.ctc_prefix_score(lpT, dec.wave_len, st[0], st[1], ctc_score.view(-1), last_tok.view(-1), alive.view(-1), att_vals, att_ids,
                                 cand[0], cand[1], beam, i, lam, EOS_ID, BLANK_ID, out=top)
        K.joint_beam_step(top, score, att_score, ctc_score, alive, last_tok, parent, rec_tok, rec_par, rec_end, rec_score, rec_att, rec_ctc,
                          dec.maxlen, alive_total[i:i + 1], B, beam, i, EOS_ID, lam)
        steps_done = i + 1
        if i + 1 < Lcap:
            K.ctc_prefix_gather(cand[0], cand[1], st[0], st[1], parent.view(-1), last_tok.view(-1), alive.view(-1), att_ids, dec.wave_len, B, beam)
            dec.gather(parent, i)
        if (i % check_every) == check_every - 1 and int(alive_total[i]) == 0:   # the only host sync of the loop
            break
    n = steps_done
    return _backtrace(rec_tok[:n].cpu(), rec_par[:n].cpu(), rec_end[:n].cpu(), rec_score[:n].cpu(), B, beam, nbest,
                      extra={"att_score": rec_att[:n].cpu(), "ctc_score": rec_ctc[:n].cpu()})
