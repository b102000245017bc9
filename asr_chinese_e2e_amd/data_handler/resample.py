"""Host side of the sample-rate conversion to 16 kHz (the reference has no resampler: parity unpinned by the reference).  For a source
rate fs and the target 16000, p/q = fs/16000 in lowest terms; an utterance x of n_in samples becomes n_out = ceil(n_in q / p) samples
(speed.perturbed_len: THE length formula),
    y[n] = sum_k x[k] h(n p / q - k),   h(t) = c sinc(c t) w(t c / Z),   c = ROLLOFF min(1, q / p),
    w(u) = I0(BETA sqrt(1 - u^2)) / I0(BETA) for |u| < 1, else 0,
a Kaiser-windowed sinc of Z = 64 zero crossings with the constants of the common "kaiser_best" resamplers.  The knee of the filter lies at
c times the lower of the two Nyquist frequencies, so tones beyond about 0.93 of it are already attenuated: a 7.4 kHz tone from a source of
at least 22.05 kHz, and a 3.7 kHz tone from 8 kHz, each come out with an error of 0.11; tones at 1, 3.4 and 7 kHz come out within 5e-8,
tones at 8.5 and 10 kHz below 5e-8 (float64 evaluation, tests/test_resample_cpu.py).  The kernel (csrc/resample.hip) evaluates the
polyphase form with the tables built here, in one fixed order of fp32 multiply-adds, so that StreamResampler reproduces the offline call
bit for bit; tests/resample_ref.py restates the definition in float64."""
import math

import numpy as np

from .speed import perturbed_len

TARGET = 16000
Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
Q_MAX, NTAPS_MAX, PLANS_MAX = 640, 1023, 16      # ASR_RESAMPLE_* of include/asr_hip.h
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)      # the usual ones; plan() decides, not this list


class Plan:
    """fs -> p / q = fs / 16000 in lowest terms, W = ceil(Z / c), ntaps = 2 W + 1."""

    def __init__(self, fs, p, q, W):
        self.fs, self.p, self.q, self.W, self.ntaps = fs, p, q, W, 2 * W + 1

    def n_out(self, n_in):
        return perturbed_len(n_in, self.p, self.q)


def cutoff(p, q):
    return ROLLOFF * min(1.0, q / p)


def plan(fs):
    """The plan of source rate fs; a rate whose reduced q passes 640 or whose filter passes 1023 taps raises ValueError here, never later."""
    if isinstance(fs, bool) or int(fs) != fs or int(fs) < 1:
        raise ValueError(f"sample rate {fs!r} is not a positive integer")
    fs = int(fs)
    g = math.gcd(fs, TARGET)
    p, q = fs // g, TARGET // g
    W = 0 if p == q else math.ceil(Z / cutoff(p, q))
    if q > Q_MAX or 2 * W + 1 > NTAPS_MAX:
        raise ValueError(f"sample rate {fs} = {p}/{q} x {TARGET}: the resampler takes rates whose reduced denominator is at most {Q_MAX} and "
                         f"whose filter has at most {NTAPS_MAX} taps (this one: q = {q}, {2 * W + 1} taps)")
    return Plan(fs, p, q, W)


def h(t, p, q):
    c = cutoff(p, q)
    u = np.asarray(t, dtype=np.float64) * (c / Z)
    inside = np.abs(u) < 1.0
    w = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(BETA)
    return np.where(inside, c * np.sinc(c * np.asarray(t, dtype=np.float64)) * w, 0.0)


def phase_table(pl):
    """H (q, ntaps) float64: H[r][j + W] = h(r/q - j)."""
    t = np.arange(pl.q, dtype=np.float64)[:, None] / pl.q - np.arange(-pl.W, pl.W + 1, dtype=np.float64)[None, :]
    return h(t, pl.p, pl.q)


def kernel_table(pl):
    """T (ntaps, q) float32 in the order the kernel reads it: T[j][n mod q] = H[(n p) mod q][j], computed in float64 and rounded once -
    lanes of consecutive outputs read consecutive words."""
    H = phase_table(pl).astype(np.float32)
    return np.ascontiguousarray(H[(np.arange(pl.q) * pl.p) % pl.q].T)


class RateTable:
    """The plans of up to 16 source rates as the kernel takes them: pq (R, 2) int32, tap_off (R + 1) int32 (plan r's taps are
    taps[tap_off[r] : tap_off[r + 1]] = kernel_table, ntaps x q words; nothing for 16 kHz), taps f32.  index(fs) is the utterance's
    rate index; 16 kHz has index -1, which the kernel copies.  device=None keeps the arrays on the host (numpy)."""

    def __init__(self, rates, device=None):
        self.plans = [plan(fs) for fs in sorted(set(rates) - {TARGET})]
        if len(self.plans) > PLANS_MAX:
            raise ValueError(f"{len(self.plans)} source rates other than {TARGET}: one table holds at most {PLANS_MAX}")
        tabs = [kernel_table(pl).reshape(-1) for pl in self.plans]
        self.pq = np.asarray([(pl.p, pl.q) for pl in self.plans] or [(1, 1)], dtype=np.int32).reshape(-1, 2)
        self.tap_off = np.concatenate([[0], np.cumsum([t.size for t in tabs] or [0])]).astype(np.int32)
        self.taps = np.concatenate(tabs) if tabs else np.zeros(1, dtype=np.float32)
        self._index = {pl.fs: r for r, pl in enumerate(self.plans)}
        self._index[TARGET] = -1
        self.by_rate = {pl.fs: pl for pl in self.plans}
        self.by_rate[TARGET] = plan(TARGET)
        self.dev = None
        if device is not None:
            import torch
            self.dev = tuple(torch.from_numpy(a).to(device) for a in (self.pq, self.tap_off, self.taps))

    def index(self, fs):
        try:
            return self._index[int(fs)]
        except KeyError:
            raise ValueError(f"sample rate {fs}: not among the rates this table was built for ({sorted(self._index)})") from None

    def n_out(self, n_in, fs):
        return self.by_rate[int(fs)].n_out(n_in)

    def windows(self, n_in, rates):
        """Offline windows (B, 5) int32 {in_base, n_avail, n_total, out_start, n_emit} and rate indices (B) int32."""
        win = np.asarray([(0, n, n, 0, self.n_out(n, fs)) for n, fs in zip(n_in, rates)], dtype=np.int32).reshape(-1, 5)
        return win, np.asarray([self.index(fs) for fs in rates], dtype=np.int32)


def resample_batch(wav, lens, rates, Smax_out=None, table=None):
    """wav (B, Smax) f32 on the device, lens / rates: B host ints -> (out (B, Smax_out) f32 at 16 kHz, out_len (B) int32, n_out list):
    one asr_resample_fwd launch for the batch, whatever rates it mixes."""
    import torch
    from .. import kernels as K
    table = table or RateTable(rates, wav.device)
    win, ridx = table.windows(lens, rates)
    n_out = [int(v) for v in win[:, 4]]
    put = lambda a: torch.from_numpy(a).to(wav.device)
    out, out_len = K.resample(wav, put(ridx), put(win), *table.dev, max(max(n_out), 1) if Smax_out is None else Smax_out)
    return out, out_len, n_out


class StreamPlan:
    """The counters of StreamResampler and the integers of each call, on the host alone (no device buffers).  Per utterance: received
    (source samples so far), emitted (outputs so far), closed.  The device row of a call is [tail | new block] with the tail holding the
    last `tail` = 2 W + p source samples, i.e. samples [received - tail, received + new).  Output n is emitted as soon as
    floor(n p / q) + W < received; at final everything up to n_out.  The oldest sample output `emitted` needs, floor(emitted p / q) - W,
    is at least received - 2 W, so it is always still in the tail."""

    def __init__(self, B, source_rate):
        self.pl = plan(source_rate)
        self.B, self.tail = int(B), 2 * self.pl.W + self.pl.p
        self.received, self.emitted, self.closed = [0] * self.B, [0] * self.B, [False] * self.B

    def ready(self, received, closed):
        """Outputs that can be emitted with `received` samples held."""
        return self.pl.n_out(received) if closed else self.pl.n_out(max(received - self.pl.W, 0))

    def step(self, ns, fin):
        """Advance by ns[b] new samples (fin[b]: the utterance ends with them) -> windows (B, 5) int32 of this call."""
        if len(ns) != self.B or len(fin) != self.B:
            raise ValueError(f"StreamResampler.push: n_samples and final must hold {self.B} values, got {list(ns)} and {list(fin)}")
        win = np.zeros((self.B, 5), dtype=np.int32)
        for b in range(self.B):
            n = int(ns[b])
            if n < 0:
                raise ValueError(f"StreamResampler.push: utterance {b}: n_samples = {n}")
            if self.closed[b] and n:
                raise ValueError(f"StreamResampler.push: utterance {b} is closed (final was sent), yet {n} more samples arrive")
            if self.received[b] + n >= 2 ** 31 - self.tail:
                raise ValueError(f"StreamResampler.push: utterance {b} would pass 2^31 source samples")
            base = self.received[b] - self.tail
            if self.closed[b]:
                win[b] = (base, self.tail, self.received[b], self.emitted[b], 0)
                continue
            self.received[b] += n
            self.closed[b] = bool(fin[b])
            upto = self.ready(self.received[b], self.closed[b])
            assert upto == self.emitted[b] or (self.emitted[b] * self.pl.p) // self.pl.q - self.pl.W >= base      # still in the tail
            win[b] = (base, self.tail + n, self.received[b], self.emitted[b], upto - self.emitted[b])
            self.emitted[b] = upto
        return win


class StreamResampler:
    """push(pcm (B, S) f32 at source_rate, n_samples, final) -> (pcm16k (B, S') f32 on the device, n16k list, final list), ready for
    push_audio unchanged.  Each call is one asr_resample_fwd launch on [tail | new block] with the window integers of StreamPlan; since the
    kernel's arithmetic per output is fixed (ascending taps, one accumulator), the concatenated output equals the offline call bit for
    bit under every cutting.  No internal buffer bounds a block: the row is built per call, so blocks of 0 samples and blocks far longer
    than the tail both work.  16 kHz is a pass-through."""

    def __init__(self, B, source_rate, device="cuda"):
        import torch
        self.plan, self.device = StreamPlan(B, source_rate), torch.device(device)
        self.copy = self.plan.pl.p == self.plan.pl.q
        if not self.copy:
            self.table = RateTable([source_rate], self.device)
            self.tail = torch.zeros(B, self.plan.tail, dtype=torch.float32, device=self.device)
            self.ridx = torch.zeros(B, dtype=torch.int32, device=self.device)
            self.cols = torch.arange(self.plan.tail, device=self.device)[None, :]

    def push(self, pcm, n_samples, final):
        import torch
        from .. import kernels as K
        B = self.plan.B
        if pcm.dim() != 2 or pcm.shape[0] != B or pcm.dtype != torch.float32:
            raise ValueError(f"StreamResampler.push: pcm must be ({B}, S) float32, got {tuple(pcm.shape)} {pcm.dtype}")
        ns, fin = [int(v) for v in n_samples], [bool(v) for v in final]
        if any(n > pcm.shape[1] for n in ns):
            raise ValueError(f"StreamResampler.push: n_samples {ns} pass the block's {pcm.shape[1]} samples")
        pcm = pcm.to(self.device, non_blocking=True)
        if self.copy:
            self.plan.step(ns, fin)
            return pcm, ns, fin
        win = self.plan.step(ns, fin)
        n16 = [int(v) for v in win[:, 4]]
        row = torch.cat((self.tail, pcm), dim=1)
        dwin = torch.from_numpy(win).to(self.device, non_blocking=True)
        out, _ = K.resample(row, self.ridx, dwin, *self.table.dev, max(max(n16), 1))
        # the new tail: the last `tail` samples of [tail | the n new ones] of every utterance (n differs from row to row)
        new = torch.tensor(ns, dtype=torch.int64, device=self.device)[:, None]
        self.tail = torch.gather(row, 1, self.cols + new)
        return out, n16, fin
