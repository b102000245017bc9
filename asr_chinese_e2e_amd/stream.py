"""model.stream(batch_size): the lock-step view of sessions.Sessions.  A lock-step stream of B utterances is B sessions that are opened
together, fed at one cadence and never reopened; the caches, the tick, the searches, the hypotheses and the results are Sessions'
(sessions.py describes them), and this file holds what the lock-step form adds: n_valid < C ends an utterance, the batch-list forms of
the per-slot accessors, a finish() that may be repeated, and audio in through the lock-step front end (push_audio: a StreamingFrontEnd
of data_handler/stream_frontend.py turns samples into chunks, a StreamResampler in front of it converts another source_rate)."""
import torch

from .sessions import ENDED, Sessions


class StreamingEncoder:
    def __init__(self, model, batch_size, parser=None, source_rate=None, search="greedy", beam_size=5, frame_topk=10, context=None, context_ids=None, lm=None,
                 timed=False, confidence="post_max", beam_times=False, blank_skip=None, keywords=None):
        self.core = Sessions(model, batch_size, search=search, beam_size=beam_size, frame_topk=frame_topk, context=context, lm=lm, timed=timed,
                             confidence=confidence, beam_times=beam_times, blank_skip=blank_skip, keywords=keywords, _lockstep=True)
        self.model, self.B, self.C = model, self.core.S, self.core.C
        if context is None and context_ids is not None:
            raise ValueError("context_ids needs a context")
        # hotword biasing: context_ids = the graph per utterance (None: graph 0 for all, the default of open)
        graphs = [None] * self.B if context is None or context_ids is None else list(context_ids)
        if len(graphs) != self.B:
            raise ValueError(f"context_ids must hold {self.B} graph indices, got {len(graphs)}")
        for b in range(self.B):
            self.core.open(b, context=graphs[b])
        self.pushes = 0
        self.parser, self.frontend = parser, None      # the front end is built by the first push_audio
        # source_rate: the rate of the audio push_audio receives; other than 16 kHz it goes through a StreamResampler first (None: 16 kHz)
        self.source_rate, self.resampler = source_rate, None
        if source_rate is not None:
            from .data_handler import resample
            resample.plan(source_rate)      # an unsupported rate raises here

    # what callers read of the stream: the core's, or the core's per-slot state in lock-step terms
    left = property(lambda self: self.core.left)
    search = property(lambda self: self.core.search)
    timed = property(lambda self: self.core.timed)
    beam_times = property(lambda self: self.core.beam_times)
    which = property(lambda self: self.core.which)
    log = property(lambda self: self.core.log)
    cap = property(lambda self: self.core.cap, doc="cache rows per utterance")
    offset = property(lambda self: self.C * self.pushes, doc="absolute frame of the next chunk (the same for every utterance)")
    valid = property(lambda self: list(self.core.frames), doc="valid frames pushed per utterance")
    ended = property(lambda self: [s == ENDED for s in self.core.state], doc="a chunk with fewer than C valid frames ends the utterance")

    def push(self, feats, n_valid):
        """feats (B, C, F): one chunk of encoder-rate features (after LFR and normalisation) in the model's dtype; n_valid (B,): the valid
        frames of each utterance in it (0 once an utterance has ended).  Returns per utterance the greedy CTC ids this chunk adds
        (repeats collapsed across chunk boundaries; empty lists for a model without a CTC head).  search="prefix_beam": the tokens by
        which the stable prefix of the prefix beam search grew in this chunk - append-only as well; partial() / nbest() for the rest."""
        B, C = self.B, self.C
        if not torch.is_tensor(feats) or feats.dim() != 3 or feats.shape[0] != B or feats.shape[1] != C:
            raise ValueError(f"push: feats must be (B, C, F) = ({B}, {C}, F), got {tuple(feats.shape) if torch.is_tensor(feats) else type(feats)}")
        nv = [int(x) for x in (n_valid.tolist() if torch.is_tensor(n_valid) else n_valid)]
        if len(nv) != B or any(x < 0 or x > C for x in nv):
            raise ValueError(f"push: n_valid must hold {B} values in [0, {C}], got {nv}")
        for b, ended in enumerate(self.ended):
            if ended and nv[b] > 0:
                raise ValueError(f"push: utterance {b} has ended (an earlier chunk had fewer than {C} valid frames)")
        out = self.core.push(feats, nv, [n < C for n in nv])      # a live utterance that would pass the positional-encoding table raises here
        self.pushes += 1
        return out

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
        """pcm (B, S) f32 on the host or the device (at model.stream's source_rate, 16 kHz by default): n_samples[b] <= S new samples of
        utterance b (0 is fine), final[b] closes it.  Runs every chunk the audio completes (StreamingFrontEnd: the utterances advance in
        lock-step) and returns per utterance the ids they add.  Needs model.stream(B, parser=...) with a parser of norm="global"; audio
        for a closed utterance raises."""
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

    # ------------------------------------------------------------------ the core's per-slot methods over the batch
    def nbest(self):
        """Per utterance Sessions.nbest (search="prefix_beam")."""
        return [self.core.nbest(b) for b in range(self.B)]

    def partial(self):
        """Per utterance Sessions.partial (search="prefix_beam")."""
        return [self.core.partial(b) for b in range(self.B)]

    def tokens(self):
        """Per utterance Sessions.tokens (timed=True or beam_times=True).  beam_times: empty after finish()."""
        return [self.core.tokens(b) for b in range(self.B)]

    def keyword_hits(self):
        """Per utterance Sessions.keyword_hits (keywords=...)."""
        return [self.core.keyword_hits(b) for b in range(self.B)]

    def encoder_output(self):
        """(enc (B, T, d), lengths (B,) int32): T = the longest utterance rounded up to whole chunks; rows past an utterance's length are zero."""
        return self.core.encoder_output(range(self.B))

    def finish(self, beam_size=5, **kw):
        """Sessions.results of every utterance: model.transcribe(...) of the pushed features under the same decoding chunk mask, from the
        streamed encoder output.  Nothing is freed: the stream stays readable and finish may be called again with other arguments."""
        return self.core.results(list(range(self.B)), beam_size=beam_size, **kw)
