"""Streaming encoder: the encoder under its decoding chunk mask, run one chunk of frames at a time (model.stream(batch_size)).

Under the chunk mask (asr_hip.h: asr_sdpa_chunk_fwd) every valid query of chunk n sees exactly the valid keys of chunks
n - left .. n (all of them when left = -1).  So a chunk's self-attention is the plain key-length attention of its C query rows over a
per-layer K|V cache that holds those keys at rows [0, k_len) of each utterance: K.sdpa_fwd with k_len = cached + valid-in-chunk keys.
The cache is one contiguous window per utterance: with left >= 0 it keeps the last left * C keys, copied down into a second buffer
before each chunk (ping-pong) - a ring buffer would leave the stale rows of a partial last chunk visible, as the attention masks a key
PREFIX only; with left = -1 it grows (doubling, at most to the positional-encoding table) and pushing past the table raises.

Per push: input projection, LayerNorm + positional encoding at the chunk's absolute frame offset, the L encoder layers on B * C rows,
the CTC head and its frame-wise argmax - the engine's kernels (gemm_small / NT, sdpa_fwd, add_ln_fwd, asr_ctc_frame_argmax).

push_audio takes samples instead: a StreamingFrontEnd (data_handler/stream_frontend.py) turns them into chunks, each of which is pushed.

search="prefix_beam" (the first pass of the U2 recipe): instead of the argmax, each push feeds the chunk's per-frame candidates
(asr_ctc_frame_topk) to the resumable CTC prefix beam search (asr_ctc_prefix_beam_chunk), whose beam lives on the device between
pushes.  push returns the tokens by which the STABLE prefix grew - the prefix all beam entries share, which no later chunk can retract;
partial() / nbest() give the revisable hypotheses, finish(joint="ctc_rescore") re-ranks the n-best with the decoder (second pass).

timed=True (greedy only): the frame-wise best path is the alignment, so every emitted token's first and last frame and its confidence
are known when its run of frames closes; the push then runs the two kernels of a timed sessions tick (asr_ctc_frame_stats,
asr_session_ctc_step_tokens) and tokens() lists the tokens so far, the run still open last (confidence.TokenLog).

beam_times=True (prefix beam only): the search carries the best single alignment of every prefix (asr_ctc_prefix_beam_chunk_timed), so
nbest() / partial() also give each hypothesis' tokens with frames, times and confidence, and tokens() the best hypothesis' with the
records that no later frame can change flagged final; the records travel in the push's one copy.
"""
import torch

from . import kernels as K
from .Utils import Pack

BLANK = 0      # the CTC blank (= PAD_ID of the model)
SILENCE_LP = -0.2231435513142097      # log 0.8, the sessions' default blank threshold: a timed stream's step counts silence, nothing reads it


class StreamingEncoder:
    def __init__(self, model, batch_size, parser=None, source_rate=None, search="greedy", beam_size=5, frame_topk=10, context=None, context_ids=None, lm=None,
                 timed=False, confidence="post_max", beam_times=False):
        C, left = model.decoding_chunk_size, model.decoding_left_chunks
        if C <= 0:
            raise ValueError("model.stream() needs a decoding chunk: config decoding_chunk_size > 0 (or a static chunk_size)")
        self.model, self.B, self.C, self.left = model, int(batch_size), int(C), int(left)
        if self.B < 1:
            raise ValueError("batch_size must be >= 1")
        self.eng = None
        self.offset = 0                      # absolute frame of the next chunk (the same for every utterance)
        self.valid = [0] * self.B            # valid frames pushed per utterance
        self.ended = [False] * self.B        # a chunk with fewer than C valid frames ends the utterance
        self.clen = [0] * self.B             # keys in the cache per utterance
        self.last = [BLANK] * self.B         # best class of the previous valid frame (CTC collapse across chunk boundaries)
        self.cap = 0                         # cache rows per utterance
        self.caches = None                   # [buffer][layer] -> (B * cap, 2 H dk); the second buffer only with left >= 0 (_slide)
        self.outs, self.feats = [], []
        if search not in ("greedy", "prefix_beam"):
            raise ValueError(f"search must be 'greedy' or 'prefix_beam' (got {search!r})")
        self.search, self.beam_size, self.frame_topk = search, int(beam_size), int(frame_topk)
        # timed=True (greedy streams): every emitted token's frames, times and confidence (confidence.TokenLog, tokens()), from the two
        # kernels of a timed sessions tick - asr_ctc_frame_stats and asr_session_ctc_step_tokens, the reset flag set on the first push
        self.timed, self.log, self.ctc_state, self.run_state = bool(timed), None, None, None
        if self.timed:
            if search != "greedy":
                raise ValueError("timed=True needs search='greedy': the frame-wise best path is the alignment there; times for the prefix beam's stable prefix are not supported")
            if not model.use_ctc:
                raise ValueError("timed=True needs a model with the CTC head (config.ctc_weight > 0): times and confidence come from it")
            from .confidence import TokenLog
            self.log = TokenLog(self.B, confidence, model.vocab._id2token, model.frame_seconds())
        # beam_times=True (prefix beam streams): every hypothesis' tokens with the frames and confidence of its best single alignment
        # (asr_ctc_prefix_beam_chunk_timed); tokens() lists the best hypothesis', the records no later frame can change flagged final
        self.beam_times, self.which = bool(beam_times), None
        if self.beam_times:
            from .confidence import beam_times_check
            self.which = beam_times_check(search, model.use_ctc, context, lm, confidence)
        if search == "prefix_beam":
            if not model.use_ctc:
                raise RuntimeError("search='prefix_beam' needs a model with the CTC head (config.ctc_weight > 0)")
            k = max(1, min(self.frame_topk, model.V))
            if self.beam_size < 1 or self.beam_size > 16 or self.beam_size * (k + 1) > 64:
                raise ValueError(f"the device search ranks beam * (frame_topk + 1) <= 64 candidates per frame, beam <= 16 (beam {beam_size}, frame_topk {k})")
            self.frame_topk = k
        # hotword biasing (context.ContextGraph): the streamed search ranks by log p + bias; context_ids = the graph per utterance
        self.context, self.roots = context, None
        if context is None and context_ids is not None:
            raise ValueError("context_ids needs a context")
        if context is not None:
            if search != "prefix_beam":
                raise ValueError("hotword biasing (context=...) is supported by search='prefix_beam' (the CTC prefix beam search), not by search='greedy'")
            from . import decode
            decode._check_context(model, context)
            self.graphs = [0] * self.B if context_ids is None else [int(g) for g in context_ids]
            self.roots = context.roots(self.graphs, self.B)
        # n-gram LM shallow fusion (lm.NgramLM): the streamed search ranks by log p + the hypothesis's LM bias; one LM for every utterance
        self.lm = lm
        if lm is not None:
            if search != "prefix_beam":
                raise ValueError("an n-gram LM (lm=...) is supported by search='prefix_beam' (the CTC prefix beam search), not by search='greedy'")
            from . import decode
            decode._check_lm(model, lm, context)
        self.beam = None                     # K.PrefixBeamState, allocated by the first push for the positional-encoding table's frames
        self.stable = [0] * self.B           # tokens of each utterance handed out by push so far (beam mode)
        self._hyps = None                    # the last push's (tokens, lengths, scores) as host arrays; with a context or an LM also (bias, state)
        self._times = None                   # beam_times: the last push's (vit, start, end, mx, mn, sm, final) as host arrays; dropped by finish()
        self.parser, self.frontend = parser, None      # the front end is built by the first push_audio
        # source_rate: the rate of the audio push_audio receives; other than 16 kHz it goes through a StreamResampler first (None: 16 kHz)
        self.source_rate, self.resampler = source_rate, None
        if source_rate is not None:
            from .data_handler import resample
            resample.plan(source_rate)      # an unsupported rate raises here

    def _grow(self, eng, need, dev):
        hd2 = 2 * eng.H * eng.dk
        L = len(eng.enc)
        if self.caches is None:
            if self.left >= 0:      # fixed window: two buffers, the keys slide from one to the other
                cap = self.left * self.C + self.C
                self.caches = [[torch.zeros(self.B * cap, hd2, dtype=eng.dtype, device=dev) for _ in range(L)] for _ in range(2)]
            else:                   # unlimited left context: one buffer that grows
                cap = min(max(need, 4 * self.C), eng.pe.shape[0])
                self.caches = [[torch.zeros(self.B * cap, hd2, dtype=eng.dtype, device=dev) for _ in range(L)]]
            self.cap = cap
            return
        if need <= self.cap:
            return
        cap = min(max(2 * self.cap, need), eng.pe.shape[0])      # left = -1 only: the fixed window never needs more
        new = [torch.zeros(self.B * cap, hd2, dtype=eng.dtype, device=dev) for _ in range(L)]
        for i in range(L):
            new[i].view(self.B, cap, hd2)[:, : self.cap] = self.caches[0][i].view(self.B, self.cap, hd2)
        self.caches, self.cap = [new], cap

    def _slide(self, dev):
        """left >= 0: keep the last left * C keys of each utterance at rows [0, left * C) (copied into the other buffer)."""
        keep = self.left * self.C
        if self.left < 0 or not any(c > keep for c in self.clen):
            return
        src, dst = [], []
        for b, c in enumerate(self.clen):
            s0 = c - min(c, keep)
            src += [b * self.cap + s0 + j for j in range(keep)]
            dst += [b * self.cap + j for j in range(keep)]
            self.clen[b] = min(c, keep)
        src = torch.tensor(src, dtype=torch.long, device=dev)
        dst = torch.tensor(dst, dtype=torch.long, device=dev)
        for i, cur in enumerate(self.caches[0]):
            self.caches[1][i].index_copy_(0, dst, cur.index_select(0, src))
        self.caches = [self.caches[1], self.caches[0]]

    def push(self, feats, n_valid):
        """feats (B, C, F): one chunk of encoder-rate features (after LFR and normalisation) in the model's dtype; n_valid (B,): the valid
        frames of each utterance in it (0 once an utterance has ended).  Returns per utterance the greedy CTC ids this chunk adds
        (repeats collapsed across chunk boundaries; empty lists for a model without a CTC head).  search="prefix_beam": the tokens by
        which the stable prefix of the prefix beam search grew in this chunk - append-only as well; partial() / nbest() for the rest."""
        model, B, C = self.model, self.B, self.C
        if feats.dim() != 3 or feats.shape[0] != B or feats.shape[1] != C:
            raise ValueError(f"push: feats must be (B, C, F) = ({B}, {C}, F), got {tuple(feats.shape)}")
        nv = [int(x) for x in (n_valid.tolist() if torch.is_tensor(n_valid) else n_valid)]
        if len(nv) != B or any(x < 0 or x > C for x in nv):
            raise ValueError(f"push: n_valid must hold {B} values in [0, {C}], got {nv}")
        for b in range(B):
            if self.ended[b] and nv[b] > 0:
                raise ValueError(f"push: utterance {b} has ended (an earlier chunk had fewer than {C} valid frames)")
        eng = self.eng = model._ensure_engine(feats.device)
        if self.offset + C > eng.pe.shape[0]:
            raise ValueError(f"push: frame {self.offset + C} exceeds the positional-encoding table ({eng.pe.shape[0]} frames)")
        dev = feats.device
        H, dk, hd = eng.H, eng.dk, eng.H * eng.dk
        was_training, eng.training = eng.training, False
        try:
            with torch.no_grad():
                self._slide(dev)
                self._grow(eng, max(self.clen) + C, dev)
                caches = self.caches[0]
                nv_dev = torch.tensor(nv, dtype=torch.int32, device=dev)
                # at least one key: an utterance that ended without a single frame (fewer than 400 samples under the Kaldi front end) still
                # sits in the batch; its rows are not valid and nothing reads them, and a length of 1 keeps zero-key attention off the kernels
                klen = torch.tensor([max(c + n, 1) for c, n in zip(self.clen, nv)], dtype=torch.int32, device=dev)
                rows = torch.tensor([b * self.cap + self.clen[b] + t for b in range(B) for t in range(C)], dtype=torch.long, device=dev)
                x = feats.to(eng.dtype).contiguous().reshape(B * C, -1)
                e0 = eng.lin_in.fwd(x)
                h, _, _ = K.add_ln_fwd(e0, None, eng.ln_in.g, eng.ln_in.b, eng.pe[self.offset:], None, B, C, xhat=e0)
                for i, (mha, ffn) in enumerate(eng.enc):
                    qkv = mha.qkv.fwd(h)
                    cache = caches[i]
                    cache.index_copy_(0, rows, qkv[:, hd:])
                    ctx, _ = K.sdpa_fwd(qkv[:, :hd], cache[:, :hd], cache[:, hd:], klen, B, H, C, self.cap, dk)
                    a = mha.fc.fwd(ctx)
                    h1, _, _ = K.add_ln_fwd(a, h, mha.ln.g, mha.ln.b, None, nv_dev, B, C, xhat=a)
                    h, _ = eng._ffn_block_fwd(ffn, h1, B, C, nv_dev, site=0)
                out = [[] for _ in range(B)]
                if self.search == "prefix_beam":
                    if self.beam is None:      # the trie for every frame push admits: B * 2 * (table * beam + 1) * 4 bytes
                        self.beam = K.ctc_prefix_beam_state(B, self.beam_size, eng.pe.shape[0], dev, context=self.context, roots=self.roots, lm=self.lm,
                                                            times=self.beam_times)
                    vals, ids, blank_lp = K.ctc_frame_topk(eng.ctc_lo.fwd(h), self.frame_topk, BLANK)
                    buf, Lcap = K.ctc_prefix_beam_chunk(self.beam, vals, ids, blank_lp, nv, C, self.beam_size, BLANK, packed=True)
                    # one copy: tokens, lengths, scores and stable lengths (with a context also bias and state) travel in one buffer
                    # (kept as arrays: the token rows are Lcap wide, and only the first `length` of each are ever turned into lists)
                    host = buf.cpu()
                    n_words = B * (self.beam_size * (Lcap + 2) + 1)
                    tok, ln, sc, stable = (t.numpy() for t in K.prefix_beam_unpack(host[:n_words], B, self.beam_size, Lcap))
                    self._hyps = (tok, ln, sc)
                    if self.context is not None or self.lm is not None:
                        self._hyps += tuple(t.numpy() for t in K.prefix_beam_ctx_unpack(host, B, self.beam_size, Lcap))
                    if self.beam_times:
                        self._times = tuple(t.numpy() for t in K.prefix_beam_times_unpack(host, B, self.beam_size, Lcap))
                    for b in range(B):      # every entry shares the stable prefix, so rank 0 spells it whatever the order by score
                        out[b] = tok[b, 0, self.stable[b]:int(stable[b])].tolist()
                        self.stable[b] = int(stable[b])
                elif self.timed:
                    first = self.ctc_state is None
                    if first:
                        self.ctc_state = torch.zeros(B, 4, dtype=torch.int32, device=dev)
                        self.run_state = torch.zeros(B, K.STEP_TOKENS_REC, dtype=torch.int32, device=dev)
                    reset = torch.full((B,), int(first), dtype=torch.int32, device=dev)
                    path, best_lp, blank_lp, _, ent = K.ctc_frame_stats(eng.ctc_lo.fwd(h).view(B, C, -1), nv_dev, BLANK)
                    buf = K.session_ctc_step_tokens(path, blank_lp, best_lp, ent, nv_dev, reset, self.ctc_state, self.run_state, C, SILENCE_LP, BLANK).cpu()
                    step = buf[:, :4 + C].tolist()
                    self.log.ingest(buf, C, [b for b in range(B) if nv[b] > 0])
                    for b in range(B):
                        out[b] = step[b][4:4 + step[b][0]]
                        if nv[b] < C:      # the utterance ends here: the run still open is a token like the others
                            self.log.close(b)
                elif model.use_ctc:
                    logits = eng.ctc_lo.fwd(h).view(B, C, -1)
                    path = K.ctc_frame_argmax(logits, nv_dev, BLANK).cpu().tolist()
                    for b in range(B):
                        for t in range(nv[b]):
                            s = path[b][t]
                            if s != BLANK and s != self.last[b]:
                                out[b].append(s)
                            self.last[b] = s
        finally:
            eng.training = was_training
        self.outs.append(h.view(B, C, -1))
        self.feats.append(feats)
        for b in range(B):
            self.clen[b] += nv[b]
            self.valid[b] += nv[b]
            if nv[b] < C:
                self.ended[b] = True
        self.offset += C
        return out

    def _beam_tokens(self, b, r, final=False):
        """beam_times: the tokens of the r-th hypothesis of utterance b, from the last push's records."""
        from .confidence import beam_tokens
        tok, ln = self._hyps[0], self._hyps[1]
        _, start, end, mx, mn, sm, fin = self._times
        n = max(int(ln[b, r]), 0)
        return beam_tokens(tok[b, r, :n], start[b, r, :n], end[b, r, :n], mx[b, r, :n], mn[b, r, :n], sm[b, r, :n], self.which, self.model.vocab._id2token,
                           self.model.frame_seconds(), int(fin[b]) if final else None)

    def tokens(self):
        """timed=True: per utterance its tokens so far, each {"id", "token", "start_frame", "end_frame", "start_s", "end_s", "measures",
        "confidence", "final"} (times as ctc_align's).  The run still open is the last entry, final=False: its end and measures may
        still move, the others are settled.
        beam_times=True: the tokens of the best hypothesis now, over its best single alignment; final=True for the leading records that no
        later frame can change (their count only grows), the others may still move or be replaced.  Empty after finish()."""
        if self.beam_times:
            if self._hyps is None or self._times is None:
                return [[] for _ in range(self.B)]
            return [self._beam_tokens(b, 0, final=True) if self._hyps[1][b, 0] >= 0 else [] for b in range(self.B)]
        if self.log is None:
            raise ValueError("tokens() needs model.stream(..., timed=True)")
        return [self.log.tokens(b) for b in range(self.B)]

    def _ensure_frontend(self):
        if self.parser is None:
            raise ValueError("push_audio: this stream has no front end - model.stream(B, parser=AudioParser(norm='global', cmvn=...))")
        if self.frontend is None:
            from .data_handler.stream_frontend import StreamingFrontEnd
            eng = self.model._ensure_engine(self.parser.window.device)
            self.frontend = StreamingFrontEnd(self.parser, self.B, self.C, dtype=eng.dtype)
            if self.source_rate is not None and int(self.source_rate) != 16000:
                from .data_handler.resample import StreamResampler
                self.resampler = StreamResampler(self.B, self.source_rate, self.parser.window.device)

    def push_audio(self, pcm, n_samples, final):
        """pcm (B, S) f32 on the host or the device (at model.stream's source_rate, 16 kHz by default): n_samples[b] <= S new samples of utterance b (0 is fine), final[b] closes it.  Runs
        every chunk the audio completes (StreamingFrontEnd: the utterances advance in lock-step) and returns per utterance the greedy CTC
        ids they add.  Needs model.stream(B, parser=...) with a parser of norm="global"; audio for a closed utterance raises."""
        out = [[] for _ in range(self.B)]
        for _, ids in self.push_audio_chunks(pcm, n_samples, final):
            for b in range(self.B):
                out[b] += ids[b]
        return out

    def push_audio_chunks(self, pcm, n_samples, final):
        """push_audio chunk by chunk: yields (n_valid, ids) = push()'s arguments and result for every chunk the audio completes."""
        self._ensure_frontend()
        if self.resampler is not None:      # samples at source_rate -> the 16 kHz samples they complete (bit for bit the offline conversion)
            pcm, n_samples, final = self.resampler.push(pcm, n_samples, final)
        for feats, nv in self.frontend.push_audio(pcm, n_samples, final):
            yield nv, self.push(feats, nv)

    def encoder_output(self):
        """(enc (B, T, d) with T = chunks pushed * C, lengths (B,) int32): frames past an utterance's length are not meaningful."""
        if not self.outs:
            raise ValueError("encoder_output: nothing pushed yet")
        dev = self.outs[0].device
        return torch.cat(self.outs, dim=1), torch.tensor(self.valid, dtype=torch.int32, device=dev)

    def _need_beam(self, what):
        if self.search != "prefix_beam":
            raise ValueError(f"{what} needs a stream opened with search='prefix_beam'")

    def nbest(self):
        """search="prefix_beam": per utterance the search's current list of {"yseq", "score"}, best first (at most beam_size).
        With a context: {"yseq", "score", "ctc_score", "bias"}, ordered by score = ctc_score + bias.  With an LM: {"yseq", "score",
        "ctc_score", "lm_score"}, ordered by score = ctc_score + lm_score."""
        self._need_beam("nbest()")
        if self.lm is not None:
            from .decode import lm_entries
            if self._hyps is None:      # the empty hypothesis on the start state: only the end-of-sentence term
                l = self.lm.final(self.lm.start, 0.0)
                return [[{"yseq": [], "score": 0.0 + l, "ctc_score": 0.0, "lm_score": l}] for _ in range(self.B)]
            tok, ln, sc, bias, state = self._hyps
            return [lm_entries(self.lm, tok[b], ln[b], sc[b], bias[b], state[b]) for b in range(self.B)]
        if self._hyps is None:
            if self.context is not None:
                return [[{"yseq": [], "score": 0.0, "ctc_score": 0.0, "bias": 0.0}] for _ in range(self.B)]
            return [[{"yseq": [], "score": 0.0}] for _ in range(self.B)]
        if self.context is not None:
            from .decode import context_entries
            tok, ln, sc, bias, state = self._hyps
            return [context_entries(self.context, tok[b], ln[b], sc[b], bias[b], state[b]) for b in range(self.B)]
        tok, ln, sc = self._hyps
        out = [[{"yseq": tok[b, r, :ln[b, r]].tolist(), "score": float(sc[b, r])} for r in range(self.beam_size) if ln[b, r] >= 0]
               for b in range(self.B)]
        if self.beam_times and self._times is not None:      # ranks without an entry are the last ones: list index = rank
            for b, hyps in enumerate(out):
                for r, h in enumerate(hyps):
                    h["viterbi_score"], h["tokens"] = float(self._times[0][b, r]), self._beam_tokens(b, r)
        return out

    def partial(self):
        """search="prefix_beam": per utterance {"ids": the best prefix now (revisable past stable_len), "stable_len": how many of its
        tokens are final (the concatenation of what push returned), "score": its log-probability}; with a context also "bias", with an
        LM "lm_score" (and the score includes it)."""
        out = [{"ids": h[0]["yseq"] if h else [], "stable_len": self.stable[b], "score": h[0]["score"] if h else float("-inf")}
               for b, h in enumerate(self.nbest())]
        if self.context is not None:
            for o, h in zip(out, self.nbest()):
                o["bias"] = h[0]["bias"] if h else 0.0
        if self.lm is not None:
            for o, h in zip(out, self.nbest()):
                o["lm_score"] = h[0]["lm_score"] if h else 0.0
        if self.beam_times:
            for o, h in zip(out, self.nbest()):
                o["tokens"] = h[0].get("tokens", []) if h else []
        return out

    def _live_only(self, timestamps, search, confidence=None):
        """finish() over the utterances that have a frame: search(rows) -> their result dicts, rows = their indices in the batch (every
        one of them in the common case).  An utterance without a frame gets the empty transcript and reaches no search kernel."""
        live = [b for b in range(self.B) if self.valid[b] > 0]
        res = search(live) if live else []
        out = [{"text": "", "ids": [], "score": float("-inf"), "tokens": [] if timestamps else None} for _ in range(self.B)]
        if self.context is not None:
            for o in out:
                o["bias"] = 0.0
        if self.lm is not None:
            for o in out:
                o["lm_score"] = 0.0
        if confidence is not None:
            for o in out:
                o["confidence"] = None
        for b, r in zip(live, res):
            out[b] = r
        return out

    def _finish_rescore(self, ctc_weight=None, timestamps=True, confidence=None):
        """The second pass: the decoder re-ranks the streamed search's n-best (decode.attention_rescore) against the streamed encoder
        output; a CTC-only model keeps the CTC best.  transcribe's result dicts, timestamps from the CTC head over the same output."""
        from . import decode
        self._need_beam("finish(joint='ctc_rescore')")
        model = self.model
        all_enc, all_lens = self.encoder_output()
        all_hyps = self.nbest()

        def search(rows):
            enc, lens, hyps = (all_enc, all_lens, all_hyps) if len(rows) == self.B else (all_enc[rows].contiguous(), all_lens[rows], [all_hyps[b] for b in rows])
            if model.use_decoder:
                w = float(getattr(model.config, "ctc_weight", 0.0)) if ctc_weight is None else float(ctc_weight)
                hyps = decode.attention_rescore(model, enc, lens, hyps, w)
            ids = [list(h[0]["yseq"]) if h else [] for h in hyps]
            scores = [float(h[0]["score"]) if h else float("-inf") for h in hyps]
            biases = [float(h[0]["bias"]) if h else 0.0 for h in hyps] if self.context is not None else None
            if self.lm is not None:
                biases = [float(h[0]["lm_score"]) if h else 0.0 for h in hyps]
            B, T = enc.shape[0], enc.shape[1]

            def ctc_logits():
                with torch.no_grad():
                    return self.eng.ctc_lo.fwd(enc.reshape(B * T, -1).contiguous()).view(B, T, -1)
            return model._hyp_dicts(ids, scores, timestamps, ctc_logits, lens, biases, "lm_score" if self.lm is not None else "bias", confidence=confidence)
        return self._live_only(timestamps, search, confidence)

    def finish(self, beam_size=5, **kw):
        """model.transcribe(...) of the pushed features under the same decoding chunk mask, computed from the streamed encoder output
        (the encoder does not run again).  kw: transcribe's other arguments (ctc_weight, timestamps, joint, confidence).
        joint="ctc_rescore" (a stream opened with search="prefix_beam"): no new search - the streamed prefix beam search's n-best is
        re-ranked by the decoder (_finish_rescore); beam_size does not apply, the list is the stream's."""
        from .confidence import measure
        which = measure(kw.get("confidence"))
        if which is not None and not kw.get("timestamps", True):
            raise ValueError("confidence needs timestamps=True: a token's confidence is taken over the frames of its alignment")
        self._times = None      # beam_times: the records are dropped; what follows is what it is without them
        if kw.get("joint") == "ctc_rescore":
            return self._finish_rescore(ctc_weight=kw.get("ctc_weight"), timestamps=kw.get("timestamps", True), confidence=which)
        all_enc, all_lens = self.encoder_output()
        all_wave = torch.cat(self.feats, dim=1)

        def search(rows):
            enc, lens, wave = (all_enc, all_lens, all_wave) if len(rows) == self.B else (all_enc[rows].contiguous(), all_lens[rows], all_wave[rows].contiguous())
            ctx = {}
            if self.context is not None:      # a fresh offline search over the streamed encoder output, biased as the stream is
                ctx = dict(context=self.context, context_ids=[self.graphs[b] for b in rows])
            if self.lm is not None:
                ctx = dict(lm=self.lm)
            with self.model.given_encoder_output(enc):
                return self.model.transcribe(Pack(wave=wave, wave_len=lens), beam_size=beam_size, **kw, **ctx)
        return self._live_only(kw.get("timestamps", True), search, which)
