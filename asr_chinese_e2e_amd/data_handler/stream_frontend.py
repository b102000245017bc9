"""Streaming waveform front end: blocks of samples in, encoder chunks out (StreamingFrontEnd), for a parser with global CMVN.

What may leave, and when, is decided by four pure functions of the sample counts (the availability rules; tests check them against
brute force).  A log-mel frame t is the 400-sample window centred on sample 160 t, reflected at the start of the utterance: it is
emitted as soon as every sample it touches has arrived, so frame 0 needs 201 samples, frame 1 needs 360 and frame t >= 2 needs
160 t + 200.  Once the utterance is closed its length is known and every frame t < 1 + len // 160 is emitted with the offline
kernel's reflection and clamping at the end.  LFR row r stacks frames r n .. r n + m - 1: it is emitted when the last of them exists,
and after the close every row r < ceil(frames / n) is, the tail repeating the last frame.

The four functions are the rules of the reference front end.  The class asks its parser how many frames are ready
(AudioParser.frames_ready), so a parser with frontend="kaldi" streams by its own rule: frame t is samples 160 t .. 160 t + 399 and
nothing else, it is emitted once sample 160 t + 399 has arrived, and the close adds no frame - only the LFR tail rows, which repeat the
last frame.  What keeps a live sample in the ring is the same for both front ends: once every frame that can leave has left, fewer than
400 received samples are still needed (the `piece` of __init__).

State: per utterance a ring of samples and a ring of log-mel frames on the device (kernels.stream_append / stream_logmel /
stream_norm_lfr; include/asr_hip.h), and the counters below on the host - n_samples is host data, so nothing is read back."""
import torch

from .. import kernels as K

HOP, N_FFT = 160, 400


def total_frames(length):
    """Log-mel frames of an utterance of `length` samples (the offline kernel's Tb)."""
    return 1 + length // HOP if length > 0 else 0


def samples_needed(t):
    """Samples that must have arrived before frame t can be computed without knowing the length."""
    return N_FFT // 2 + 1 if t == 0 else HOP * t + N_FFT // 2


def frames_ready(received, closed=False):
    """Frames that can be emitted after `received` samples; closed: `received` is the whole utterance."""
    if closed:
        return total_frames(received)
    return 0 if received < samples_needed(0) else (received - N_FFT // 2) // HOP + 1


def rows_ready(frames, m, n, closed=False):
    """LFR rows that can be emitted once `frames` frames exist; closed: `frames` is the utterance's frame count."""
    if closed:
        return (frames + n - 1) // n
    return 0 if frames < m else (frames - m) // n + 1


def oldest_sample(t):
    """The first sample frame t (and so any later frame) touches: history before it can go."""
    return max(0, HOP * t - N_FFT // 2)


def _pow2_at_least(v):
    p = 1
    while p < v:
        p *= 2
    return p


class StreamingFrontEnd:
    """push_audio(pcm (B, S), n_samples, final) -> list of (feats (B, C, lfr_m * n_mels) in `dtype`, n_valid list of B ints): the encoder
    chunks that became complete.  The B utterances advance in lock-step (one chunk index for all, as StreamingEncoder.push takes one chunk
    of every utterance): a chunk leaves when every utterance that is still open has C rows ready; a closed utterance contributes what it has left
    (n_valid < C, then 0).  independent=True (sessions.py) lifts the lock-step: a chunk leaves whenever one utterance has C rows ready or
    is closed with rows left, the others ride along with n_valid 0 and keep their rows - per utterance the chunks of a B = 1 front
    end - and reset(b) starts utterance b again; push_audio then returns (feats, n_valid, done) with done[b] = utterance b's last row
    left with this chunk (feats None for an empty chunk that only carries an end).  sample_cap: samples per ring (a power of two); longer blocks are worked
    through in pieces.  An utterance that runs ahead of one that stalls the chunk keeps its log-mel frames (the frame rings are re-laid
    at a larger size), up to max_frames of them (163 s by default): past that push_audio raises before it takes anything of the call.

    push_audio first plans the whole call on the host (plan(): which pieces, frames and chunks, from the counters alone), then
    launches what the plan lists and commits the counters - so a refused call leaves the front end as it was."""

    def __init__(self, parser, B, C, dtype=torch.float32, sample_cap=16384, max_frames=16384, independent=False):
        if getattr(parser, "norm", None) != "global":
            raise ValueError("streaming needs a parser with norm='global': per-utterance normalisation needs the whole utterance "
                             "before its first frame (AudioParser(norm='global', cmvn=...))")
        if B < 1 or C < 1:
            raise ValueError(f"B and C must be at least 1, got {B} and {C}")
        if sample_cap < 1024 or sample_cap & (sample_cap - 1):
            raise ValueError(f"sample_cap must be a power of two of at least 1024, got {sample_cap}")
        self.parser, self.B, self.C, self.dtype = parser, int(B), int(C), dtype
        self.independent = bool(independent)      # independent sessions (sessions.py): every utterance leaves at its own cadence
        self.m, self.n, self.n_mels = parser.lfr_m, parser.lfr_n, parser.n_mels
        self.dev = parser.window.device
        self.scap = int(sample_cap)
        self.kaldi = getattr(parser, "frontend", "reference") == "kaldi"
        self.piece = self.scap - 512      # fewer than 400 samples of history are ever live (every frame that can leave has left)
        self.fcap = _pow2_at_least(self.C * self.n + self.m + self.piece // HOP + 34)
        self.max_frames = max(int(max_frames), self.fcap)
        self.wav_ring = torch.zeros(self.B, self.scap, dtype=torch.float32, device=self.dev)
        self.feat_ring = torch.zeros(self.B, self.fcap, self.n_mels, dtype=torch.float32, device=self.dev)
        self.received = [0] * self.B      # samples so far
        self.closed = [False] * self.B
        self.next_frame = [0] * self.B    # log-mel frames computed so far
        self.next_row = [0] * self.B      # LFR rows emitted so far

    def _par(self, rows):
        return torch.tensor(rows, dtype=torch.int32, device=self.dev)

    def plan(self, ns, fin):
        """The launches push_audio makes for n_samples = ns and final = fin, from the counters alone (nothing is launched or changed):
        -> (actions, counters after the call).  Actions, in order: ("append", pcm offset, [[received, n_new]], max n_new),
        ("grow", new frame capacity, [(first live frame, end)] per utterance), ("logmel", [[t_begin, n_new, total or OPEN]], max n_new)
        (the frames of the parser's front end; a Kaldi parser's kernel reads the first two columns only),
        ("chunk", [[r_begin, n_rows, frames or OPEN]], n_valid)."""
        B, C, m, n = self.B, self.C, self.m, self.n
        received, closed, next_frame, next_row, fcap = list(self.received), list(self.closed), list(self.next_frame), list(self.next_row), self.fcap
        acts = []
        for off in range(0, max(max(ns), 1), self.piece):
            take = [max(0, min(self.piece, x - off)) for x in ns]
            if max(take) > 0:
                acts.append(("append", off, [[received[b], take[b]] for b in range(B)], max(take)))
            for b in range(B):
                received[b] += take[b]
                if fin[b] and off + take[b] >= ns[b]:
                    closed[b] = True
            new = [self.parser.frames_ready(received[b], closed[b]) - next_frame[b] for b in range(B)]
            if max(new) > 0:
                # live frames of an utterance: from the first one its next row stacks (none once every row has left) to its last
                live = [(min(next_row[b] * n, next_frame[b] + new[b]), next_frame[b] + new[b]) for b in range(B)]
                need = max(hi - lo for lo, hi in live)
                if need > self.max_frames:
                    b = max(range(B), key=lambda k: live[k][1] - live[k][0])
                    raise ValueError(f"push_audio: utterance {b} would hold {need} log-mel frames that no chunk has taken (limit {self.max_frames}): "
                                     f"the utterances of one stream advance in lock-step and another one is short of audio")
                if need > fcap:
                    fcap = _pow2_at_least(need)
                    acts.append(("grow", fcap, [(lo, next_frame[b]) for b, (lo, _) in enumerate(live)]))
                acts.append(("logmel", [[next_frame[b], new[b], received[b] if closed[b] else K.STREAM_OPEN] for b in range(B)], max(new)))
                for b in range(B):
                    next_frame[b] += new[b]
            while True:
                ready = [rows_ready(next_frame[b], m, n, closed[b]) - next_row[b] for b in range(B)]
                if self.independent:
                    # a chunk runs whenever one utterance has C rows, or is closed with rows left; the others ride along with no row and
                    # keep theirs: per utterance this is the cadence of a front end that serves it alone.  done: the utterances whose
                    # last row leaves with this chunk (they are closed and nothing is left).
                    nv = [min(C, r) if (r >= C or (closed[b] and r > 0)) else 0 for b, r in enumerate(ready)]
                    if not any(nv):
                        break
                    done = [closed[b] and nv[b] > 0 and nv[b] == ready[b] for b in range(B)]
                    acts.append(("chunk", [[next_row[b], nv[b], next_frame[b] if closed[b] else K.STREAM_OPEN] for b in range(B)], nv, done))
                    for b in range(B):
                        next_row[b] += nv[b]
                    continue
                if not any(r > 0 for r in ready) or not all(closed[b] or ready[b] >= C for b in range(B)):
                    break
                nv = [min(C, r) for r in ready]
                acts.append(("chunk", [[next_row[b], nv[b], next_frame[b] if closed[b] else K.STREAM_OPEN] for b in range(B)], nv))
                for b in range(B):
                    next_row[b] += nv[b]
        if self.independent:
            # an utterance this call closes whose rows were all out before the close (it added none), or that never had one: an empty
            # chunk carries its end to the consumer
            done = [closed[b] and not self.closed[b] and not any(a[0] == "chunk" and a[3][b] for a in acts) for b in range(B)]
            if any(done):
                acts.append(("chunk", [[next_row[b], 0, next_frame[b] if closed[b] else K.STREAM_OPEN] for b in range(B)], [0] * B, done))
            return acts, (received, closed, next_frame, next_row)
        # Kaldi: utterances of fewer than 400 samples have no frame.  When this call closes the last of them and no row has ever left,
        # one empty chunk tells the consumer that every utterance has ended (a reference utterance of any sample has a frame).
        if self.kaldi and all(closed) and not all(self.closed) and not any(next_row) and not any(a[0] == "chunk" for a in acts):
            acts.append(("chunk", [[0, 0, 0] for _ in range(B)], [0] * B))
        return acts, (received, closed, next_frame, next_row)

    def reset(self, b):
        """Utterance b starts again at sample 0 (independent sessions: its slot is reopened).  Only the host counters: after it every
        sample and frame a kernel reads for b was written after the reset - stream_append writes [received, received + n), the
        log-mel / fbank tile reads the samples of the frames it is asked for (all received; reflected at sample 0 and at the closed
        end, never past them), and a tile row that is not asked for is computed from whatever its ring positions hold but never
        stored; stream_norm_lfr reads frames [r n, r n + m) clamped to the closed utterance's last frame.  So no stale ring content
        can reach a result, and the rings are not cleared."""
        if not 0 <= b < self.B:
            raise ValueError(f"reset: utterance {b} of {self.B}")
        self.received[b], self.closed[b], self.next_frame[b], self.next_row[b] = 0, False, 0, 0

    def _grow_frames(self, cap, live):
        """The frame rings re-laid at capacity `cap`: frame t of [lo, hi) moves from slot t mod the old capacity to t mod cap."""
        new = torch.zeros(self.B, cap, self.n_mels, dtype=torch.float32, device=self.dev)
        for b, (lo, hi) in enumerate(live):
            if hi > lo:
                t = torch.arange(lo, hi, device=self.dev)
                new[b, t % cap] = self.feat_ring[b, t % self.fcap]
        self.feat_ring, self.fcap = new, cap

    def push_audio(self, pcm, n_samples, final):
        B = self.B
        if pcm.dim() != 2 or pcm.shape[0] != B or pcm.dtype != torch.float32:
            raise ValueError(f"push_audio: pcm must be ({B}, S) float32, got {tuple(pcm.shape)} {pcm.dtype}")
        ns = [int(x) for x in (n_samples.tolist() if torch.is_tensor(n_samples) else n_samples)]
        fin = [bool(x) for x in (final.tolist() if torch.is_tensor(final) else final)]
        S = pcm.shape[1]
        if len(ns) != B or len(fin) != B or any(x < 0 or x > S for x in ns):
            raise ValueError(f"push_audio: n_samples and final must hold {B} values, n_samples in [0, {S}], got {ns} and {fin}")
        for b in range(B):
            if self.closed[b] and ns[b] > 0:
                raise ValueError(f"push_audio: utterance {b} is closed (final was sent), yet {ns[b]} more samples arrive")
            if self.received[b] + ns[b] >= K.STREAM_OPEN:
                raise ValueError(f"push_audio: utterance {b} would pass {K.STREAM_OPEN} samples")
        acts, after = self.plan(ns, fin)
        if max(ns) > 0:
            pcm = pcm.to(self.dev).contiguous()
        out = []
        for act in acts:
            if act[0] == "append":
                K.stream_append(pcm, self._par(act[2]), self.wav_ring, act[1], act[3])
            elif act[0] == "grow":
                self._grow_frames(act[1], act[2])
            elif act[0] == "logmel" and self.kaldi:
                par = self._par([row[:2] for row in act[1]])
                K.stream_fbank(self.wav_ring, par, self.parser.window, self.parser.melfb, self.feat_ring, act[2], self.parser.wav_scale, self.parser.preemph)
            elif act[0] == "logmel":
                K.stream_logmel(self.wav_ring, self._par(act[1]), self.parser.window, self.parser.melfb, self.feat_ring, act[2])
            elif any(act[2]) or not self.independent:
                out.append((K.stream_norm_lfr(self.feat_ring, self._par(act[1]), self.parser.mean, self.parser.istd, self.m, self.n, self.C,
                                              self.dtype),) + tuple(act[2:]))
            else:      # independent: an empty chunk that only carries the end of some utterance - no features, no launch
                out.append((None,) + tuple(act[2:]))
        self.received, self.closed, self.next_frame, self.next_row = after
        return out
