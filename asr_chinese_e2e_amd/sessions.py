"""Streaming state and the one streaming tick of the package: independent sessions in one batch (model.sessions(slots)), and - through
the lock-step view of stream.py - model.stream(B).  Every slot of the batch holds a session that is opened, fed, closed, finished and
reopened at its own pace, and CTC endpointing tells when a slot's speaker has stopped.

The tick.  Under the chunk mask (asr_hip.h: asr_sdpa_chunk_fwd) every valid query of chunk n sees exactly the valid keys of chunks
n - left .. n (all of them when left = -1).  So a chunk's self-attention is the plain key-length attention of its C query rows over a
per-layer K|V cache that holds those keys at rows [0, k_len) of the slot: K.sdpa_fwd with k_len = cached + valid-in-chunk keys.  A tick
(push) computes slots * C encoder rows: input projection, LayerNorm + positional encoding at each slot's own frame offset, the L encoder
layers (QKV GEMM, cache append, key-length attention, fc, LayerNorm, feed-forward), the append of the output rows to the slot's rows of
self.enc, then the CTC head and its tail (greedy step, timed step or prefix beam chunk) with one copy to the host.  A slot that sits the
tick out (n_valid 0) is computed but nothing of it is kept or changed.

Capacities.  The cache is one contiguous window per slot.  left >= 0: left * C + C rows and two buffers; before a chunk for a
window that holds more than left * C keys, each slot's last left * C keys are copied down into the other buffer (asr_slot_rows_slide,
ping-pong) - a ring buffer would leave the stale rows of a partial last chunk visible, as the attention masks a key PREFIX only.
left = -1: one buffer of max(4 C, need) rows that doubles, at most to the positional-encoding table; a session that would pass the
table is refused.  The output rows double from 8 C rows in the same way.  The capacity is the Tk of the attention launch, so it
depends on the schedule only through the longest window.

Parameters.  Each slot b has its own frame offset (the positional-encoding row of its next frame), its own key cache length and its own
CTC state.  Per push the host builds ONE int32 parameter block (PAR_ROWS x slots: positional offset, cache length, n_valid, reset flag,
slide source and count, key length, output row) and uploads it once; the kernels take its rows as their per-slot arguments
(csrc/session.hip, asr_add_ln_slots_fwd, asr_ctc_prefix_beam_state_reset).  No row-index tensors, no per-row loops on the host.

Why a slot's bits do not depend on its neighbours: the GEMMs, LayerNorm and the CTC head work row by row, attention works per
(slot, head) over that slot's key prefix, and every session kernel reads only its own slot's parameters (tests/test_sessions_gpu.py).

search="prefix_beam" (the first pass of the U2 recipe): instead of the argmax, each tick feeds the chunk's per-frame candidates
(asr_ctc_frame_topk) to the resumable CTC prefix beam search (asr_ctc_prefix_beam_chunk), whose beam lives on the device between
ticks.  push returns the tokens by which the STABLE prefix grew - the prefix all beam entries share, which no later chunk can retract;
partial(b) / nbest(b) give the revisable hypotheses, results / finish(joint="ctc_rescore") re-rank the n-best with the decoder.

Endpointing (endpoint=dict(...)): WeNet's CTC endpoint rules, evaluated per slot from counters the device keeps
(asr_session_ctc_step): a frame is silent iff p(blank) > blank_threshold; trailing silence = the current run of silent frames; length
= the frames consumed; decoded = the greedy output so far is non-empty (beam sessions: the best hypothesis is).  A rule
(must_have_decoded, min_trailing_silence_ms, min_length_ms) fires when all three hold; endpoints() reports the first that does.
Endpointing only reports: the caller closes the slot (final), finishes it and opens it again for what follows.

timed=True (greedy sessions): the frame-wise best path is the alignment, so every emitted token's first and last frame and its
confidence are known when its run of frames closes.  The tick runs asr_ctc_frame_stats + asr_session_ctc_step_tokens instead of
asr_ctc_frame_best_blank + asr_session_ctc_step - the same ids and counters, and per slot the runs of the best path that closed in this
tick with their frames and confidence measures, still in one buffer and one copy; tokens(b) lists them, the run still open last
(confidence.TokenLog).  push returns what it returns.

beam_times=True (prefix beam sessions): the search carries the best single alignment of every prefix (asr_ctc_prefix_beam_chunk_timed
on a timed state) - the plain search's results and each hypothesis' token records in the same buffer; nbest(b) / partial(b) also give
each hypothesis' tokens with frames, times and confidence, and tokens(b) the best hypothesis' with the records that no later frame can
change flagged final.  The reset kernel restarts a reopened slot's lists at frame 0; results, finish, drop and open drop the slot's
records on the host.

blank_skip=p (prefix beam sessions): blank-frame skipping in front of the search (decode.ctc_prefix_beam_search describes the rule).  Per
tick asr_ctc_blank_skip_compact moves the chunk's kept rows to the front of each slot's rows and its device count takes the place of
n_valid in asr_ctc_prefix_beam_chunk*; per slot it carries one bit (the last consumed frame was high), the frames seen and kept, and the
real frame of every kept row, through which the records of beam_times go back to real frames (asr_frame_index_remap).  A slot that sits
a tick out keeps its bit, the reset flags of a reopened slot clear it with its beam, and drop / finish leave nothing behind: the state is
reset when the slot is next opened.  The host-side frame counter of the beam state keeps counting PUSHED frames - an upper bound of the
kept ones, so the refusal of a chunk past the trie's T_cap stays safe (it may come early, never late).  Endpointing and the counters
of asr_session_ctc_step read the uncompacted blank_lp: trailing silence and frame counts do not change.  After every push the
hypotheses are bit for bit those of the offline search with blank_skip on the frames so far.

keywords=KeywordList (any search): keyword spotting with the audio (keywords.py).  The tick needs each frame's log-sum-exp: the timed tick
has it, the untimed greedy tick runs asr_ctc_frame_stats in place of asr_ctc_frame_best_blank (the same path and blank_lp bits), the
prefix beam tick runs it as one more launch.  Then asr_kws_chunk advances every slot's lattice columns and open runs (one state for all
slots, reset by the tick's reset flags, its runs closed by the tick's final flags) and asr_kws_compact lists the hits the tick closed
(at most kw_rows per slot and tick, the rest counted as dropped) - behind the prefix beam's packed results in its one copy, otherwise in
one copy of their own.  keyword_hits(b) lists the session's hits so far; after final, and while nothing was dropped, they are bit for
bit model.spot_keywords' over the session's streamed encoder rows.  A final that arrives without frames for any slot runs the two kernels alone.

Out of scope: input rates other than 16 kHz for sessions (StreamResampler has no per-slot reset; the lock-step view resamples in front
of its own front end), compaction of idle slots (every tick computes slots * C rows), carrying audio across an endpoint, a varying
number of slots, capture into a hipGraph."""
import math

import torch

from . import kernels as K
from .Utils import Pack

BLANK = 0      # the CTC blank (= PAD_ID of the model)
FREE, OPEN, ENDED = "free", "open", "ended"
# rows of the per-push parameter block
P_PE_OFF, P_CLEN, P_NV, P_RESET, P_SLIDE_FROM, P_SLIDE_COUNT, P_KLEN, P_OUT_ROW, PAR_ROWS = 0, 1, 2, 3, 4, 5, 6, 7, 8
P_FINAL = PAR_ROWS      # one more row, in sessions with keywords only: the final flags of the tick
KW_ROWS = 128           # keyword hits a slot can report per tick (the rest are counted as dropped)

ENDPOINT_DEFAULTS = dict(
    blank_threshold=0.8,
    # WeNet's CtcEndpointConfig: (must_have_decoded, min_trailing_silence_ms, min_length_ms)
    rules=(("silence_start", False, 5000, 0), ("silence_after_speech", True, 1000, 0), ("max_length", False, 0, 20000)),
)


def endpoint_config(endpoint):
    """endpoint=None -> None; a dict -> the defaults overridden by it: blank_threshold, and per rule name a (must_have_decoded,
    min_trailing_silence_ms, min_length_ms) triple, or the three WeNet-style keys min_trailing_silence_ms etc. inside a dict."""
    if endpoint is None:
        return None
    cfg = dict(blank_threshold=float(endpoint.get("blank_threshold", ENDPOINT_DEFAULTS["blank_threshold"])))
    if not 0.0 < cfg["blank_threshold"] < 1.0:
        raise ValueError(f"endpoint: blank_threshold must lie in (0, 1), got {cfg['blank_threshold']}")
    known = {"blank_threshold"} | {r[0] for r in ENDPOINT_DEFAULTS["rules"]}
    if set(endpoint) - known:
        raise ValueError(f"endpoint: unknown keys {sorted(set(endpoint) - known)} (known: {sorted(known)})")
    rules = []
    for name, must, sil, length in ENDPOINT_DEFAULTS["rules"]:
        v = endpoint.get(name)
        if isinstance(v, dict):
            must, sil, length = v.get("must_have_decoded", must), v.get("min_trailing_silence_ms", sil), v.get("min_length_ms", length)
        elif v is not None:
            must, sil, length = v
        rules.append((name, bool(must), int(sil), int(length)))
    cfg["rules"] = tuple(rules)
    return cfg


def endpoint_rule(rules, frame_us, trailing, frames, decoded):
    """The first rule that fires, or None.  Times in whole microseconds (frame_us = the encoder frame's duration), so that a rule
    fires at the frame that reaches its threshold whatever the float representation of 30 ms is."""
    for name, must, sil_ms, len_ms in rules:
        if (decoded or not must) and trailing * frame_us >= sil_ms * 1000 and frames * frame_us >= len_ms * 1000:
            return name
    return None


class Sessions:
    def __init__(self, model, slots, parser=None, search="greedy", beam_size=5, frame_topk=10, endpoint=None, source_rate=None, context=None, lm=None,
                 timed=False, confidence="post_max", beam_times=False, blank_skip=None, keywords=None, _lockstep=False):
        """_lockstep: set by stream.StreamingEncoder alone - the messages name model.stream(), and a model without the CTC head is
        admitted: its tick ends once the encoder rows are stored, push returns empty lists and the results come from the attention beam."""
        who = "model.stream()" if _lockstep else "model.sessions()"
        C, left = model.decoding_chunk_size, model.decoding_left_chunks
        if C <= 0:
            raise ValueError(f"{who} needs a decoding chunk: config decoding_chunk_size > 0 (or a static chunk_size)")
        if source_rate is not None and int(source_rate) != 16000:
            raise ValueError("model.sessions(): only 16 kHz audio (StreamResampler has no per-slot reset yet)")
        self.model, self.S, self.C, self.left = model, int(slots), int(C), int(left)
        if self.S < 1:
            raise ValueError("batch_size must be >= 1" if _lockstep else "slots must be >= 1")
        if search not in ("greedy", "prefix_beam"):
            raise ValueError(f"search must be 'greedy' or 'prefix_beam' (got {search!r})")
        self.search, self.beam_size, self.frame_topk = search, int(beam_size), int(frame_topk)
        # blank_skip=p (prefix beam sessions): the float32 log threshold of the compaction in front of the search, and its per-slot state
        self.skip_thr, self.skip = None, None
        if blank_skip is not None:
            self.skip_thr = K.blank_skip_threshold(blank_skip)
            if search != "prefix_beam":
                raise ValueError("blank_skip needs search='prefix_beam': it drops frames in front of the CTC prefix beam search, the greedy path reads every frame")
        # timed=True (greedy sessions): every emitted token's frames, times and confidence (confidence.TokenLog, tokens(b))
        self.timed, self.log, self.run_state = bool(timed), None, None
        if self.timed:
            if search != "greedy":
                raise ValueError("timed=True needs search='greedy': the frame-wise best path is the alignment there; times for the prefix beam's stable prefix are not supported")
            if not model.use_ctc:
                raise ValueError("timed=True needs a model with the CTC head (config.ctc_weight > 0): times and confidence come from it")
            from .confidence import TokenLog
            self.log = TokenLog(self.S, confidence, model.vocab._id2token, model.frame_seconds())
        # beam_times=True (prefix beam sessions): every hypothesis' tokens with the frames and confidence of its best single alignment
        # (asr_ctc_prefix_beam_chunk_timed); tokens(b) lists the best hypothesis', the records no later frame can change flagged final
        self.beam_times, self.which = bool(beam_times), None
        if self.beam_times:
            from .confidence import beam_times_check
            self.which = beam_times_check(search, model.use_ctc, context, lm, confidence)
        if not model.use_ctc:
            if search == "prefix_beam":
                raise RuntimeError("search='prefix_beam' needs a model with the CTC head (config.ctc_weight > 0)")
            if not _lockstep or endpoint is not None:
                raise RuntimeError("model.sessions() needs a model with the CTC head (config.ctc_weight > 0): ids and endpointing come from it")
        if search == "prefix_beam":
            k = max(1, min(self.frame_topk, model.V))
            if self.beam_size < 1 or self.beam_size > 16 or self.beam_size * (k + 1) > 64:
                raise ValueError(f"the device search ranks beam * (frame_topk + 1) <= 64 candidates per frame, beam <= 16 (beam {beam_size}, frame_topk {k})")
            self.frame_topk = k
        # hotword biasing (context.ContextGraph): open(b, context=i) picks slot b's graph; the reset kernel applies it on the slot's first tick
        self.context = context
        if context is not None:
            if search != "prefix_beam":
                raise ValueError("hotword biasing (context=...) is supported by search='prefix_beam' (the CTC prefix beam search), not by search='greedy'")
            from . import decode
            decode._check_context(model, context)
        self.graph = [0 if context is not None else -1] * self.S      # the graph of each slot's session (-1: not biased)
        # n-gram LM shallow fusion (lm.NgramLM): one LM for all slots; the reset kernel puts a reopened slot on its start state
        self.lm = lm
        if lm is not None:
            if search != "prefix_beam":
                raise ValueError("an n-gram LM (lm=...) is supported by search='prefix_beam' (the CTC prefix beam search), not by search='greedy'")
            from . import decode
            decode._check_lm(model, lm, context)
        # keyword spotting (keywords.KeywordList): one list for all slots, one device state, the hits of each session on the host
        self.kw, self.kw_state, self.kw_rows = keywords, None, 0
        if keywords is not None:
            from .keywords import _check
            _check(model, keywords)
            if blank_skip is not None:
                raise ValueError("keywords with blank_skip is not supported: the spotter reads every frame")
            self.kw_rows = min(keywords.max_hits, KW_ROWS)
        self.kw_hits, self.kw_dropped = [[] for _ in range(self.S)], [0] * self.S
        self.endpoint = endpoint_config(endpoint)
        thr = self.endpoint["blank_threshold"] if self.endpoint else ENDPOINT_DEFAULTS["blank_threshold"]
        self.silence_lp = math.log(thr)      # the kernel compares float32(log threshold) with float32 log p(blank)
        self.frame_us = int(round(model.frame_seconds() * 1e6))
        S = self.S
        self.eng = None
        self.state = [FREE] * S
        self.frames = [0] * S                # frames consumed = the positional offset of the slot's next frame
        self.clen = [0] * S                  # keys in the slot's cache window
        self.fresh = [False] * S             # opened, and no launch has reset its device state yet
        self.trailing = [0] * S
        self.decoded = [False] * S
        self.stable = [0] * S
        self.cap = 0                         # cache rows per slot
        self.caches = None                   # [buffer][layer] -> (slots, cap, 2 H dk); two buffers with left >= 0 (the slide's ping-pong)
        self.enc = None                      # (slots, ecap, d): each slot's encoder output rows
        self.ctc_state = None                # (slots, 4) int32 {last, trailing, frames, decoded}
        self.beam = None
        self._hyps = None
        self._times = None                   # beam_times: the last tick's (vit, start, end, mx, mn, sm, final) as host arrays
        self._real = None                    # ... behind blank_skip: the records' (start, end) in real frames
        self.has_times = [False] * S         # ... and whether slot b's rows of them belong to its session (dropped by finish / drop / open)
        self.parser, self.frontend = parser, None

    # ------------------------------------------------------------------ slot life cycle
    def _slot(self, b):
        b = int(b)
        if not 0 <= b < self.S:
            raise ValueError(f"slot {b} of {self.S}")
        return b

    def open(self, b, context=None):
        """Slot b (free) starts a session at frame 0.  context (sessions with a ContextGraph): the graph that biases this session
        (default 0; -1: none) - fixed while the session is open."""
        b = self._slot(b)
        if self.state[b] != FREE:
            raise ValueError(f"open: slot {b} is {self.state[b]} (finish or drop it first)")
        if self.context is None:
            if context is not None:
                raise ValueError("open(context=...) needs model.sessions(..., context=ContextGraph(...))")
        else:
            graph = 0 if context is None else int(context)
            self.context.root(graph)      # an unknown graph raises here
            self.graph[b] = graph
        self.state[b], self.frames[b], self.clen[b], self.fresh[b] = OPEN, 0, 0, True
        self.trailing[b], self.decoded[b], self.stable[b] = 0, False, 0
        self.has_times[b] = False
        self.kw_hits[b], self.kw_dropped[b] = [], 0
        if self.log is not None:
            self.log.reset(b)
        if self.frontend is not None:
            self.frontend.reset(b)

    def drop(self, b):
        """Free slot b without a result."""
        b = self._slot(b)
        if self.state[b] == FREE:
            raise ValueError(f"drop: slot {b} is free")
        self.state[b], self.frames[b], self.clen[b], self.fresh[b] = FREE, 0, 0, False
        self.has_times[b] = False
        self.kw_hits[b], self.kw_dropped[b] = [], 0

    def status(self, b):
        b = self._slot(b)
        return {"state": self.state[b], "frames": self.frames[b], "trailing_silence_frames": self.trailing[b], "decoded": self._decoded(b)}

    def _decoded(self, b):
        if self.state[b] == FREE:
            return False
        if self.search == "prefix_beam":
            h = self.nbest(b)
            return bool(h and h[0]["yseq"])
        return self.decoded[b]

    def endpoints(self):
        """Per slot None, or the name of the first endpoint rule that fires ("silence_start", "silence_after_speech", "max_length")."""
        if self.endpoint is None:
            raise ValueError("endpoints() needs model.sessions(..., endpoint={...})")
        return [None if self.state[b] == FREE else endpoint_rule(self.endpoint["rules"], self.frame_us, self.trailing[b], self.frames[b], self._decoded(b))
                for b in range(self.S)]

    # ------------------------------------------------------------------ device buffers
    def _grow(self, eng, need, dev):
        """The cache capacity (module docstring): the fixed window's left * C + C rows, or a buffer that doubles up to the table."""
        hd2, L, S = 2 * eng.H * eng.dk, len(eng.enc), self.S
        if self.caches is None:
            if self.left >= 0:
                cap, nbuf = self.left * self.C + self.C, 2
            else:
                cap, nbuf = min(max(need, 4 * self.C), eng.pe.shape[0]), 1
            self.caches = [[torch.zeros(S, cap, hd2, dtype=eng.dtype, device=dev) for _ in range(L)] for _ in range(nbuf)]
            self.cap = cap
            return
        if self.left >= 0 or need <= self.cap:      # the fixed window never needs more: an active slot's keys were slid down first
            return
        cap = min(max(2 * self.cap, need), eng.pe.shape[0])
        new = [torch.zeros(S, cap, hd2, dtype=eng.dtype, device=dev) for _ in range(L)]
        for i in range(L):
            new[i][:, : self.cap] = self.caches[0][i]
        self.caches, self.cap = [new], cap

    def _grow_enc(self, eng, need, dev):
        d = eng.ln_in.g.numel()
        need = min(-(-need // self.C) * self.C, eng.pe.shape[0])      # whole chunks: finish() pads its batch to whole chunks
        if self.enc is None:
            self.enc = torch.zeros(self.S, min(max(need, 8 * self.C), eng.pe.shape[0]), d, dtype=eng.dtype, device=dev)
        elif need > self.enc.shape[1]:
            new = torch.zeros(self.S, min(max(2 * self.enc.shape[1], need), eng.pe.shape[0]), d, dtype=eng.dtype, device=dev)
            new[:, : self.enc.shape[1]] = self.enc
            self.enc = new

    # ------------------------------------------------------------------ one tick
    def push(self, feats, n_valid, final):
        """feats (slots, C, F): one chunk of encoder-rate features per slot; n_valid[b] = C, or 0 (the slot sits this tick out: nothing of
        it changes), or any value in [0, C] together with final[b], which ends the session's input.  Returns per slot the greedy CTC
        ids the chunk adds (repeats collapsed across chunks; empty lists for a model without the CTC head), or the growth of the stable
        prefix (search="prefix_beam").  A push that is refused (a free slot with frames, a partial chunk without final, a session that
        would pass the positional table) raises before any launch and leaves every slot as it was."""
        model, S, C = self.model, self.S, self.C
        if not torch.is_tensor(feats) or feats.dim() != 3 or feats.shape[0] != S or feats.shape[1] != C:
            raise ValueError(f"push: feats must be (slots, C, F) = ({S}, {C}, F), got {tuple(feats.shape) if torch.is_tensor(feats) else type(feats)}")
        nv = [int(x) for x in (n_valid.tolist() if torch.is_tensor(n_valid) else n_valid)]
        fin = [bool(x) for x in (final.tolist() if torch.is_tensor(final) else final)]
        if len(nv) != S or len(fin) != S or any(x < 0 or x > C for x in nv):
            raise ValueError(f"push: n_valid and final must hold {S} values, n_valid in [0, {C}], got {nv} and {fin}")
        eng = self.eng = model._ensure_engine(feats.device)
        table = eng.pe.shape[0]
        for b in range(S):
            if self.state[b] == FREE and (nv[b] > 0 or fin[b]):
                raise ValueError(f"push: slot {b} is free (open it first)")
            if self.state[b] == ENDED and nv[b] > 0:
                raise ValueError(f"push: slot {b} has ended (final was sent)")
            if 0 < nv[b] < C and not fin[b]:
                raise ValueError(f"push: slot {b} brings {nv[b]} of {C} frames without final: a partial chunk in the middle of a session would misalign the chunk mask")
            if nv[b] > 0 and self.frames[b] + C > table:
                raise ValueError(f"push: slot {b} would reach frame {self.frames[b] + C}, past the positional-encoding table ({table} frames): close the session (endpointing tells when)")
        out = [[] for _ in range(S)]
        closing = [fin[b] and self.state[b] == OPEN for b in range(S)]
        if any(nv):
            self._tick(eng, feats, nv, out, closing)
        elif self.kw is not None and any(closing):
            self._kws_close(feats.device, closing)
        for b in range(S):
            if fin[b] and self.state[b] == OPEN:
                self.state[b] = ENDED
                if self.log is not None:      # the input has ended: the run still open is a token like the others
                    self.log.close(b)
        return out

    def tokens(self, b):
        """timed=True: slot b's tokens so far, each {"id", "token", "start_frame", "end_frame", "start_s", "end_s", "measures",
        "confidence", "final"} (times as ctc_align's).  The run still open is the last entry, final=False: its end and measures may
        still move, the others are settled.  The list of a finished slot stays until the slot is opened again.
        beam_times=True: the tokens of the best hypothesis now, over its best single alignment; final=True for the leading records that no
        later frame can change (their count only grows), the others may still move or be replaced.  Empty after results() / finish()."""
        if self.beam_times:
            b = self._slot(b)
            if not self.has_times[b] or self.fresh[b] or self._hyps[1][b, 0] < 0:
                return []
            return self._beam_tokens(b, 0, final=True)
        if self.log is None:
            raise ValueError("tokens() needs model.sessions(..., timed=True)")
        return self.log.tokens(self._slot(b))

    def _beam_tokens(self, b, r, final=False):
        """beam_times: the tokens of the r-th hypothesis of slot b, from the last tick's records."""
        from .confidence import beam_tokens
        tok, ln = self._hyps[0], self._hyps[1]
        _, start, end, mx, mn, sm, fin = self._times
        n = max(int(ln[b, r]), 0)
        real = None if self._real is None else [x[b, r, :n] for x in self._real]
        return beam_tokens(tok[b, r, :n], start[b, r, :n], end[b, r, :n], mx[b, r, :n], mn[b, r, :n], sm[b, r, :n], self.which, self.model.vocab._id2token,
                           self.model.frame_seconds(), int(fin[b]) if final else None, real=real)

    def _tick(self, eng, feats, nv, out, closing):
        S, C, dev = self.S, self.C, feats.device
        H, dk, hd = eng.H, eng.dk, eng.H * eng.dk
        keep = self.left * C
        # ---- the parameter block (host ints only), then one upload
        slide = self.left > 0 and any(nv[b] > 0 and self.clen[b] > keep for b in range(S))
        if self.left == 0:      # no key is kept: every chunk starts on an empty window, nothing to move
            self.clen = [0 if nv[b] > 0 else self.clen[b] for b in range(S)]
        par = [[0] * S for _ in range(PAR_ROWS + (self.kw is not None))]
        if self.kw is not None:
            par[P_FINAL] = [int(c) for c in closing]
        for b in range(S):
            c = self.clen[b]
            if slide:      # every slot moves to the other buffer: its last `keep` keys, or all it has
                par[P_SLIDE_FROM][b], par[P_SLIDE_COUNT][b] = c - min(c, keep), min(c, keep)
                c = self.clen[b] = min(c, keep)
            par[P_PE_OFF][b] = self.frames[b] if nv[b] > 0 else 0
            par[P_CLEN][b], par[P_NV][b], par[P_RESET][b] = c, nv[b], int(self.fresh[b])
            # at least one key: a slot without a frame (idle, or ended with fewer than 400 samples under the Kaldi front end) still sits in
            # the batch; its rows are not valid and nothing reads them, and a length of 1 keeps zero-key attention off the kernels
            par[P_KLEN][b] = max(c + nv[b], 1)
            par[P_OUT_ROW][b] = self.frames[b]
        reset_slots = [b for b in range(S) if self.fresh[b]]
        was_training, eng.training = eng.training, False
        try:
            with torch.no_grad():
                self._grow(eng, max(self.clen) + C, dev)
                self._grow_enc(eng, max(f + n for f, n in zip(self.frames, nv)), dev)
                pd = torch.tensor(par, dtype=torch.int32, device=dev)
                if slide:
                    for i, cur in enumerate(self.caches[0]):
                        K.slot_rows_slide(cur, self.caches[1][i], pd[P_SLIDE_FROM], pd[P_SLIDE_COUNT], keep)
                    self.caches = [self.caches[1], self.caches[0]]
                caches, cap = self.caches[0], self.cap
                nv_dev = pd[P_NV]
                # ---- the encoder chunk body, with per-slot offsets and appends
                x = feats.to(eng.dtype).contiguous().reshape(S * C, -1)
                e0 = eng.lin_in.fwd(x)
                h = K.add_ln_slots_fwd(e0, eng.ln_in.g, eng.ln_in.b, eng.pe, pd[P_PE_OFF], par[P_PE_OFF], nv_dev, S, C)
                for i, (mha, ffn) in enumerate(eng.enc):
                    qkv = mha.qkv.fwd(h)
                    cache = caches[i]
                    K.slot_rows_put(qkv[:, hd:], cache, pd[P_CLEN], nv_dev, C)
                    flat = cache.view(S * cap, 2 * hd)
                    ctx, _ = K.sdpa_fwd(qkv[:, :hd], flat[:, :hd], flat[:, hd:], pd[P_KLEN], S, H, C, cap, dk)
                    a = mha.fc.fwd(ctx)
                    h1, _, _ = K.add_ln_fwd(a, h, mha.ln.g, mha.ln.b, None, nv_dev, S, C, xhat=a)
                    h, _ = eng._ffn_block_fwd(ffn, h1, S, C, nv_dev, site=0)
                K.slot_rows_put(h, self.enc, pd[P_OUT_ROW], nv_dev, C)
                # a model without the CTC head (the lock-step view alone admits one): the tick ends here
                step = self._ctc_tail(eng, h, pd, nv, reset_slots, out) if self.model.use_ctc else None
        finally:
            eng.training = was_training
        for b in range(S):
            self.fresh[b] = False
            if step is not None and (nv[b] > 0 or b in reset_slots):
                self.trailing[b], self.decoded[b] = step[b][1], bool(step[b][3])
            self.clen[b] += nv[b]
            self.frames[b] += nv[b]

    def _ctc_tail(self, eng, h, pd, nv, reset_slots, out):
        """The CTC end of a tick over its encoder rows h: the ids (or the stable prefix's growth) of the slots with frames into `out`, the
        hypotheses and records onto the host in one copy; returns per slot the step words {n_ids, trailing, frames, decoded, ids ...}."""
        S, C, dev = self.S, self.C, h.device
        nv_dev = pd[P_NV]
        n_kw = S * (2 + 4 * self.kw_rows)      # the words of the tick's keyword hits (0 without keywords)
        if self.ctc_state is None:
            self.ctc_state = torch.zeros(S, 4, dtype=torch.int32, device=dev)
        logits = eng.ctc_lo.fwd(h)
        if self.search == "prefix_beam":
            roots = None if self.context is None else self.context.roots(self.graph, S)
            if self.beam is None:
                self.beam = K.ctc_prefix_beam_state(S, self.beam_size, eng.pe.shape[0], dev, context=self.context, roots=roots, lm=self.lm,
                                                    times=self.beam_times)
            elif reset_slots:
                K.ctc_prefix_beam_state_reset(self.beam, pd[P_RESET], reset_slots, roots=roots)
            vals, ids, blank_lp = K.ctc_frame_topk(logits, self.frame_topk, BLANK)
            cand, n_dev = (vals, ids, blank_lp), nv_dev
            if self.skip_thr is not None:      # the search sees the kept rows and their count; nv stays the host's upper bound of it
                if self.skip is None:
                    self.skip = K.BlankSkipState(S, eng.pe.shape[0], dev)
                *cand, n_dev, _ = K.ctc_blank_skip_compact(vals, ids, blank_lp, nv_dev, self.skip_thr, S, C, self.skip, pd[P_RESET])
            # behind blank skipping the records of beam_times count kept rows: their real frames travel behind the step words in the same copy
            Lcap = max(1, max(f + n for f, n in zip(self.beam.frames, nv)))      # ctc_prefix_beam_chunk's own default
            n_real = S * self.beam_size * Lcap if self.skip is not None and self.beam_times else 0
            buf, Lcap = K.ctc_prefix_beam_chunk(self.beam, *cand, nv, C, self.beam_size, BLANK, max_len=Lcap, packed=True, nv_dev=n_dev,
                                                extra_words=S * (4 + C) + 2 * n_real + n_kw)
            n_words = buf.numel() - S * (4 + C) - 2 * n_real - n_kw      # the search's words (with a context: bias and state included)
            n_step = n_words + S * (4 + C)
            if n_real:
                views = K.prefix_beam_unpack(buf[:n_words], S, self.beam_size, Lcap, "timed")
                for i, v in enumerate(views[5:7]):      # start, end
                    K.frame_index_remap(v, self.skip.frame_map, out=buf[n_step + i * n_real:n_step + (i + 1) * n_real].view(v.shape))
            K.session_ctc_step(None, blank_lp, nv_dev, pd[P_RESET], self.ctc_state, C, self.silence_lp, BLANK, out=buf[n_words:n_step].view(S, 4 + C))
            if self.kw is not None:      # the hits ride behind everything else in the same copy
                lse = K.ctc_frame_stats(logits.view(S, C, -1), nv_dev, BLANK)[3]
                self._kws_launch(logits.view(S, C, -1), lse, nv_dev, pd[P_RESET], pd[P_FINAL], buf[buf.numel() - n_kw:])
            host = buf.cpu()
            if self.kw is not None:
                self._kws_ingest(host[host.numel() - n_kw:])
            tok, ln, sc, stable, *extra = (t.numpy() for t in K.prefix_beam_unpack(host[:n_words], S, self.beam_size, Lcap, self.beam.mode))
            self._hyps = (tok, ln, sc)
            if self.beam_times:
                self._times = tuple(extra)
                self._real = tuple(host[n_step + i * n_real:n_step + (i + 1) * n_real].view(S, self.beam_size, Lcap).numpy() for i in (0, 1)) if n_real else None
                for b in range(S):
                    if self.state[b] != FREE:
                        self.has_times[b] = True
            else:
                self._hyps += tuple(extra)      # with a context / an LM: bias and state
            step = host[n_words:n_step].view(S, 4 + C).tolist()
            for b in reset_slots:
                self.stable[b] = 0
            for b in range(S):
                if nv[b] > 0:
                    out[b] = tok[b, 0, self.stable[b]:int(stable[b])].tolist()
                    self.stable[b] = int(stable[b])
        elif self.timed:
            if self.run_state is None:
                self.run_state = torch.zeros(S, K.STEP_TOKENS_REC, dtype=torch.int32, device=dev)
            path, best_lp, blank_lp, lse, ent = K.ctc_frame_stats(logits.view(S, C, -1), nv_dev, BLANK)
            buf = K.session_ctc_step_tokens(path, blank_lp, best_lp, ent, nv_dev, pd[P_RESET], self.ctc_state, self.run_state, C, self.silence_lp,
                                            BLANK).cpu()
            step = buf[:, :4 + C].tolist()
            self.log.ingest(buf, C, [b for b in range(S) if nv[b] > 0 or b in reset_slots])
        else:
            if self.kw is not None:      # the same path and blank_lp bits, and the frames' log-sum-exp
                path, _, blank_lp, lse, _ = K.ctc_frame_stats(logits.view(S, C, -1), nv_dev, BLANK)
            else:
                path, blank_lp = K.ctc_frame_best_blank(logits.view(S, C, -1), nv_dev, BLANK)
            step = K.session_ctc_step(path, blank_lp, nv_dev, pd[P_RESET], self.ctc_state, C, self.silence_lp, BLANK).cpu().tolist()
        if self.kw is not None and self.search != "prefix_beam":      # no packed buffer to ride in: one copy of their own
            self._kws_ingest(self._kws_launch(logits.view(S, C, -1), lse, nv_dev, pd[P_RESET], pd[P_FINAL]).cpu())
        if self.search != "prefix_beam":
            for b in range(S):
                if nv[b] > 0:
                    out[b] = step[b][4:4 + step[b][0]]
        # this tick's frame-wise log p(blank) (slots * C) f32 and best path (slots, C) int32 (None: beam sessions), on the device: diagnostics
        self.last_blank_lp, self.last_path = blank_lp, (None if self.search == "prefix_beam" else path)
        return step

    # ------------------------------------------------------------------ keyword spotting
    def _kws_launch(self, logits, lse, nv_dev, reset, final, out=None):
        """asr_kws_chunk + asr_kws_compact of one tick; the hits the tick closed, in `out` (or a new buffer) on the device."""
        kw, S = self.kw, self.S
        if self.kw_state is None:
            self.kw_state = K.kws_state(S, kw.K, logits.device)
        if out is None:
            out = torch.empty(S * (2 + 4 * self.kw_rows), dtype=torch.int32, device=logits.device)
        tabs = kw.on(logits.device, self.model.frame_seconds())
        cnt, rec = K.kws_chunk(logits, lse, nv_dev, reset, final, tabs, kw.K, self.kw_state, kw.hits_per_keyword, BLANK)
        K.kws_compact(cnt, rec, self.kw_rows, out=out)
        return out

    def _kws_ingest(self, flat):
        for b, r in enumerate(self.kw.decode(flat, self.S, self.kw_rows, self.model.frame_seconds(), self.model.vocab._id2token)):
            if self.state[b] != FREE:
                self.kw_hits[b] += r["hits"]
                self.kw_dropped[b] += r["dropped"]

    def _kws_close(self, dev, closing):
        """final without a frame for any slot: no tick runs, the open runs of the closing slots are closed by the two kernels alone (a
        slot opened and never fed is reset here as in its first tick - the tick's own reset still follows)."""
        S = self.S
        par = torch.tensor([[0] * S, [int(f) for f in self.fresh], [int(c) for c in closing]], dtype=torch.int32, device=dev)
        eng = self.model._ensure_engine(dev)
        logits = torch.zeros(S, 1, self.model.V, dtype=eng.dtype, device=dev)      # n_valid = 0 everywhere: never read
        lse = torch.zeros(S, 1, dtype=torch.float32, device=dev)
        self._kws_ingest(self._kws_launch(logits, lse, par[0], par[1], par[2]).cpu())

    def keyword_hits(self, b):
        """keywords=...: slot b's hits so far, sorted by (end_frame, keyword), each as model.spot_keywords reports it with frames and
        times counted from the session's first frame; a run still open is reported once it closes (final closes it).  The list of a
        finished slot stays until the slot is opened again."""
        if self.kw is None:
            raise ValueError("keyword_hits() needs model.sessions(..., keywords=KeywordList(...))")
        return sorted(self.kw_hits[self._slot(b)], key=lambda h: (h["end_frame"], h["keyword"]))

    def keywords_dropped(self, b):
        """keywords=...: the hits of slot b's session that were found and not reported (past hits_per_keyword or kw_rows in a tick)."""
        if self.kw is None:
            raise ValueError("keywords_dropped() needs model.sessions(..., keywords=KeywordList(...))")
        return self.kw_dropped[self._slot(b)]

    # ------------------------------------------------------------------ audio in
    def _ensure_frontend(self):
        if self.parser is None:
            raise ValueError("push_audio: these sessions have no front end - model.sessions(slots, parser=AudioParser(norm='global', cmvn=...))")
        if self.frontend is None:
            from .data_handler.stream_frontend import StreamingFrontEnd
            eng = self.model._ensure_engine(self.parser.window.device)
            self.frontend = StreamingFrontEnd(self.parser, self.S, self.C, dtype=eng.dtype, independent=True)

    def push_audio(self, pcm, n_samples, final):
        """pcm (slots, S) f32 at 16 kHz: n_samples[b] <= S new samples of slot b's session (0 is fine), final[b] closes its audio.  Runs a
        chunk whenever one slot has C rows ready or is closed with rows left - no slot waits for another - and returns per slot the ids
        the chunks add.  A slot whose audio is closed and whose rows are all out becomes ended."""
        out = [[] for _ in range(self.S)]
        for _, ids in self.push_audio_chunks(pcm, n_samples, final):
            for b in range(self.S):
                out[b] += ids[b]
        return out

    def push_audio_chunks(self, pcm, n_samples, final):
        """push_audio chunk by chunk: yields (n_valid, ids) for every chunk the audio completes."""
        self._ensure_frontend()
        ns = [int(x) for x in (n_samples.tolist() if torch.is_tensor(n_samples) else n_samples)]
        fin = [bool(x) for x in (final.tolist() if torch.is_tensor(final) else final)]
        if len(ns) != self.S or len(fin) != self.S:
            raise ValueError(f"push_audio: n_samples and final must hold {self.S} values")
        for b in range(self.S):
            if self.state[b] != OPEN and (ns[b] > 0 or fin[b]):
                raise ValueError(f"push_audio: slot {b} is {self.state[b]}")
        table = self.model._ensure_engine(self.parser.window.device).pe.shape[0]
        acts, _ = self.frontend.plan(ns, fin)      # refuse a call that would pass the table before the front end takes its samples
        rows = list(self.frames)
        for act in acts:
            if act[0] == "chunk":
                for b, n in enumerate(act[2]):
                    if n > 0 and rows[b] + self.C > table:
                        raise ValueError(f"push_audio: slot {b} would reach frame {rows[b] + self.C}, past the positional-encoding table ({table} frames)")
                    rows[b] += n
        for feats, nv, done in self.frontend.push_audio(pcm, ns, fin):
            if feats is None:      # only ends
                feats = torch.empty(self.S, self.C, 0, device=self.parser.window.device)
            yield nv, self.push(feats, nv, done)

    # ------------------------------------------------------------------ hypotheses and results
    def _need_beam(self, what):
        if self.search != "prefix_beam":
            raise ValueError(f"{what} needs sessions opened with search='prefix_beam'")

    def nbest(self, b):
        """search="prefix_beam": slot b's current list of {"yseq", "score"}, best first (at most beam_size).  With a context:
        {"yseq", "score", "ctc_score", "bias"}, ordered by score = ctc_score + bias.  With an LM: {"yseq", "score", "ctc_score",
        "lm_score"}, ordered by score = ctc_score + lm_score."""
        self._need_beam("nbest()")
        b = self._slot(b)
        if self.state[b] == FREE:
            raise ValueError(f"nbest: slot {b} is free")
        from .decode import _bias_entries, _bias_mode
        biased = _bias_mode(self.context, self.lm)
        if self._hyps is None or self.fresh[b]:      # the empty hypothesis: an LM's start state (only the end-of-sentence term), a context's -1 (nothing held)
            if biased is None:
                return [{"yseq": [], "score": 0.0}]
            x = biased[1](self.lm.start if self.lm is not None else -1, 0.0)
            return [{"yseq": [], "score": 0.0 + x, "ctc_score": 0.0, biased[0]: x}]
        if biased is not None:
            tok, ln, sc, bias, state = self._hyps
            return _bias_entries(*biased, tok[b], ln[b], sc[b], bias[b], state[b])
        tok, ln, sc = self._hyps
        out = [{"yseq": tok[b, r, :ln[b, r]].tolist(), "score": float(sc[b, r])} for r in range(self.beam_size) if ln[b, r] >= 0]
        if self.beam_times and self.has_times[b]:      # ranks without an entry are the last ones: list index = rank
            for r, h in enumerate(out):
                h["viterbi_score"], h["tokens"] = float(self._times[0][b, r]), self._beam_tokens(b, r)
        return out

    def partial(self, b):
        """search="prefix_beam": {"ids": slot b's best prefix now (revisable past stable_len), "stable_len": how many of its tokens are
        final (the concatenation of what push returned), "score": its log-probability}; with a context also "bias", with an LM "lm_score"
        (and the score includes it), with beam_times "tokens"."""
        h = self.nbest(b)
        out = {"ids": h[0]["yseq"] if h else [], "stable_len": self.stable[self._slot(b)], "score": h[0]["score"] if h else float("-inf")}
        if self.context is not None:
            out["bias"] = h[0]["bias"] if h else 0.0
        if self.lm is not None:
            out["lm_score"] = h[0]["lm_score"] if h else 0.0
        if self.beam_times:
            out["tokens"] = h[0].get("tokens", []) if h else []
        return out

    def encoder_output(self, slots):
        """(enc (n, T, d), lengths (n,) int32) of the listed slots: T = the longest, rounded up to whole chunks; rows past a slot's
        length are zero."""
        if self.eng is None:
            raise ValueError("encoder_output: nothing pushed yet")
        self._grow_enc(self.eng, self.C, self.eng.pe.device)      # pushes without a single frame so far: one chunk of zero rows
        slots = [self._slot(b) for b in slots]
        lens = [self.frames[b] for b in slots]
        T = min(max(self.C, -(-max(lens) // self.C) * self.C), self.enc.shape[1])
        dev = self.enc.device
        rows = self.enc[:, :T] if slots == list(range(self.S)) else torch.stack([self.enc[b, :T] for b in slots])
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
        live = (torch.arange(T, device=dev)[None, :] < lens_dev[:, None])[:, :, None]
        return torch.where(live, rows, torch.zeros((), dtype=rows.dtype, device=dev)).contiguous(), lens_dev

    def _empty_result(self, timestamps, which):
        """The result dict of a session without a frame: the empty transcript, with the keys the others of its call carry."""
        r = {"text": "", "ids": [], "score": float("-inf"), "tokens": [] if timestamps else None}
        if self.context is not None:
            r["bias"] = 0.0
        if self.lm is not None:
            r["lm_score"] = 0.0
        if which is not None:
            r["confidence"] = None
        return r

    def results(self, slots, beam_size=5, **kw):
        """model.transcribe(...)'s result dicts for the session of each listed slot (one slot: one dict) under the same decoding chunk
        mask, computed from the slot's own streamed encoder rows (the encoder does not run again) as one batch padded to the longest.
        kw: transcribe's other arguments (ctc_weight, timestamps, joint, confidence).  joint="ctc_rescore" (search="prefix_beam"): no new
        search - the decoder re-ranks the streamed prefix beam search's n-best (decode.attention_rescore; a CTC-only model keeps the CTC
        best), beam_size does not apply.  A session without a frame gets the empty transcript and reaches no search kernel.  The sessions
        stay as they are, open ones included - only their beam-time records are dropped - so the call may be repeated."""
        single = not isinstance(slots, (list, tuple))
        slots = [self._slot(b) for b in ([slots] if single else slots)]
        if len(set(slots)) != len(slots):
            raise ValueError(f"finish: slots listed twice in {slots}")
        for b in slots:
            if self.state[b] == FREE:
                raise ValueError(f"finish: slot {b} is free")
        model, timestamps = self.model, kw.get("timestamps", True)
        from .confidence import measure
        which = measure(kw.get("confidence"))
        if which is not None and not timestamps:
            raise ValueError("confidence needs timestamps=True: a token's confidence is taken over the frames of its alignment")
        rescore = kw.get("joint") == "ctc_rescore"
        if rescore:
            self._need_beam("finish(joint='ctc_rescore')")
        for b in slots:      # beam_times: the records are dropped; what follows is what it is without them
            self.has_times[b] = False
        res = [self._empty_result(timestamps, which) for _ in slots]
        live = [i for i, b in enumerate(slots) if self.frames[b] > 0]
        if live:
            rows = [slots[i] for i in live]
            enc, lens = self.encoder_output(rows)
            n, T = enc.shape[0], enc.shape[1]
            if rescore:
                from . import decode
                hyps = [self.nbest(b) for b in rows]
                if model.use_decoder:
                    w = float(getattr(model.config, "ctc_weight", 0.0)) if kw.get("ctc_weight") is None else float(kw["ctc_weight"])
                    hyps = decode.attention_rescore(model, enc, lens, hyps, w)
                ids = [list(h[0]["yseq"]) if h else [] for h in hyps]
                scores = [float(h[0]["score"]) if h else float("-inf") for h in hyps]
                biases = [float(h[0]["bias"]) if h else 0.0 for h in hyps] if self.context is not None else None
                if self.lm is not None:
                    biases = [float(h[0]["lm_score"]) if h else 0.0 for h in hyps]

                def ctc_logits():
                    with torch.no_grad():
                        return self.eng.ctc_lo.fwd(enc.reshape(n * T, -1).contiguous()).view(n, T, -1)
                got = model._hyp_dicts(ids, scores, timestamps, ctc_logits, lens, biases, "lm_score" if self.lm is not None else "bias", confidence=which)
            else:
                # under given_encoder_output the searches take the batch's features for their (B, T) only: none are kept
                wave = torch.zeros(n, T, 1, dtype=enc.dtype, device=enc.device)
                ctx = dict(context=self.context, context_ids=[self.graph[b] for b in rows]) if self.context is not None else {}
                if self.lm is not None:
                    ctx = dict(lm=self.lm)
                with model.given_encoder_output(enc):
                    got = model.transcribe(Pack(wave=wave, wave_len=lens), beam_size=beam_size, **kw, **ctx)
            for i, r in zip(live, got):
                res[i] = r
        return res[0] if single else res

    def finish(self, slots, beam_size=5, **kw):
        """results(slots, ...), after which the slots become free."""
        res = self.results(slots, beam_size=beam_size, **kw)
        for b in (slots if isinstance(slots, (list, tuple)) else [slots]):
            b = self._slot(b)
            self.state[b], self.frames[b], self.clen[b], self.fresh[b] = FREE, 0, 0, False
        return res
