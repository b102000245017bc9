"""Waveform dataset + length-bucketed loader with the feature front end on the GPU
(SURVEY.md 8(f) rank 2).

The reference's input pipeline (data/data_loader/ai_shell_1.py:12-104) computes the features on
the CPU per utterance (torchaudio), pads whole batches of FEATURES on the host, is unshuffled,
unbucketed, single-process, and moves the batch to the GPU inside collate.  Here the host only
decodes PCM and pads WAVEFORMS into a pinned buffer; the copy runs on its own stream, log-mel /
normalisation / SpecAugment / frame stacking run on the GPU (data_handler.processor.AudioParser),
and the next batch is prepared while the model trains on the current one.  Batches are drawn
from length buckets so that padding stays small.

The yielded Pack has the reference's batch contract (collat, ai_shell_1.py:75-88): wave (B, T, F),
wave_len, tgt_for_input, tgt_for_metric (0-padded, int64), tgt_len.
"""
import collections
import contextlib
import random
import threading
import wave as wave_module
import weakref

import numpy as np
import torch

from ..Utils import Pack
from .padder import Padder
from .processor import AudioParser
from . import speed as speed_mod
from . import noise as noise_mod
from . import resample as resample_mod
from . import specaug as specaug_mod


def read_pcm(path):
    """16-bit PCM WAV -> (interleaved int16 samples AS THE FILE HOLDS THEM, channels, sample_rate): the one reader of load_wav and
    WaveDataset.wave_into.  A data chunk shorter than its header says is a truncated recording, not an error: fewer samples come back."""
    with wave_module.open(path, "rb") as f:
        if f.getsampwidth() != 2:
            raise ValueError(f"{path}: only 16-bit PCM is supported (sample width {f.getsampwidth()})")
        sr, ch = f.getframerate(), f.getnchannels()
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2"), ch, sr


def pcm_to_float(pcm, ch, out):
    """The first out.size frames of interleaved int16 `pcm` -> out (float32, in [-1, 1)): scale in float32, then average the channels.
    Mono goes int16 -> float32 in one pass (no intermediate array); numpy releases the GIL for it."""
    if ch > 1:
        out[:] = (pcm[:out.size * ch].astype(np.float32) / np.float32(32768.0)).reshape(-1, ch).mean(axis=1)
    else:
        np.multiply(pcm[:out.size], np.float32(1.0 / 32768.0), out=out, casting="unsafe")


def load_wav(path):
    """16-bit PCM WAV -> (float32 mono waveform in [-1, 1), sample_rate); channels are averaged
    (loader.py:5-17 of the reference did the same through torchaudio with normalization=True)."""
    pcm, ch, sr = read_pcm(path)
    out = np.empty(pcm.size // ch, dtype=np.float32)
    pcm_to_float(pcm, ch, out)
    return out, sr


class WaveDataset:
    """items: list of (waveform, text) where waveform is a 1-D float array / tensor or a path to a
    16-bit WAV file, and text is a string (converted by `vocab.convert_str(..., use_bos=False,
    use_eos=False)` as ai_shell_1.py:53-54) or a list of ids.
    resample=True: a file at another rate the resampler takes (resample.plan) is accepted and handed on at ITS rate - wave(), wave_into()
    and num_samples() stay in source samples, rate(i) tells the rate, and the consumer (BucketedWaveLoader(resample=True), transcribe.py)
    converts on the GPU; an array in memory carries its rate as a third element (waveform, text, rate).  False: today's ValueError."""

    def __init__(self, items, vocab=None, sample_rate=16000, resample=False):
        self.items, self.vocab, self.sample_rate, self.resample = items, vocab, sample_rate, bool(resample)
        self._len = [None] * len(items)
        self._rate = [None] * len(items)

    def _check_rate(self, name, sr):
        if sr != self.sample_rate:
            if not self.resample:
                raise ValueError(f"{name}: sample rate {sr}, expected {self.sample_rate}")
            resample_mod.plan(sr)      # an unsupported rate raises here, naming it

    def rate(self, i):
        """Source rate of utterance i: a file's header, an array's third element, else sample_rate; cached."""
        if self._rate[i] is None:
            it = self.items[i]
            if isinstance(it[0], str):
                with wave_module.open(it[0], "rb") as f:
                    sr = f.getframerate()
            else:
                sr = int(it[2]) if len(it) > 2 else self.sample_rate
            self._check_rate(it[0] if isinstance(it[0], str) else f"utterance {i}", sr)
            self._rate[i] = sr
        return self._rate[i]

    def __len__(self):
        return len(self.items)

    def wave(self, i):
        w = self.items[i][0]
        if isinstance(w, str):
            w, sr = load_wav(w)
            self._check_rate(self.items[i][0], sr)
        return np.asarray(w, dtype=np.float32).reshape(-1)

    def wave_into(self, i, row):
        """Utterance i decoded straight into `row` (a float32 numpy view of the loader's pinned staging buffer), the rest of the row zeroed;
        returns the sample count (read_pcm, pcm_to_float)."""
        w = self.items[i][0]
        if isinstance(w, str):
            pcm, ch, sr = read_pcm(w)
            self._check_rate(w, sr)
            n = min(pcm.size // ch, row.size)      # what the file really holds, never more than the row the loader sized from the header
            pcm_to_float(pcm, ch, row[:n])
        else:
            a = np.asarray(w, dtype=np.float32).reshape(-1)
            n = a.size
            row[:n] = a
        row[n:] = 0.0
        return n

    def num_samples(self, i):
        if self._len[i] is None:
            w = self.items[i][0]
            if isinstance(w, str):
                with wave_module.open(w, "rb") as f:
                    self._len[i] = f.getnframes()
            else:
                self._len[i] = int(np.asarray(w).size)
        return self._len[i]

    def ids(self, i):
        t = self.items[i][1]
        if isinstance(t, str):
            return self.vocab.convert_str(t, use_bos=False, use_eos=False)
        return [int(x) for x in t]


def bucket_batches(lengths, batch_size, bucket_size=None, shuffle=True, drop_last=False, rng=None):
    """Index batches drawn from length buckets: indices sorted by length are cut into buckets of
    `bucket_size` (default 8 batches), each bucket is shuffled and cut into batches, the batches
    are shuffled.  Every index appears exactly once (or is dropped with a short last batch)."""
    rng = rng or random
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    bucket_size = bucket_size or 8 * batch_size
    batches = []
    for s in range(0, len(order), bucket_size):
        b = order[s:s + bucket_size]
        if shuffle:
            rng.shuffle(b)
        for t in range(0, len(b), batch_size):
            batches.append(b[t:t + batch_size])
    if drop_last:
        batches = [b for b in batches if len(b) == batch_size]
    if shuffle:
        rng.shuffle(batches)
    return batches


def shard_batches(batches, rank, world):
    """Data-parallel shard of a batch list that every rank builds identically: the ragged tail of len % world is
    dropped (every rank must take the same number of steps) and rank r takes batches[r::world]."""
    if world <= 1:
        return batches
    return batches[: len(batches) // world * world][rank::world]


class BatchPlan:
    """The batch list of every epoch, host logic only (no GPU): what BucketedWaveLoader iterates over.  `rng` drives the batch order (and,
    in the loader, the SpecAugment masks); with speed perturbation (`speed_pq`: list of (p, q)) each epoch first draws a factor index per
    utterance - speed.draw_factors, a pure function of (seed, epoch, utterance index) that never touches `rng` - and forms the buckets on
    the PERTURBED lengths, so padding stays small.  The epoch is the number of next_epoch() calls so far.  Every data-parallel rank
    builds the same full list and takes its shard."""

    def __init__(self, lengths, batch_size, bucket_size=None, shuffle=True, drop_last=False, seed=0, rank=0, world=1, speed_pq=None):
        self.lengths, self.batch_size, self.bucket_size, self.shuffle = list(lengths), batch_size, bucket_size, shuffle
        self.rank, self.world = int(rank), int(world)
        assert 0 <= self.rank < self.world
        self.drop_last = True if self.world > 1 else drop_last
        self.seed, self.rng, self.epoch = seed, random.Random(seed), 0
        self.speed_pq = [tuple(x) for x in speed_pq] if speed_pq else None

    def batches(self, rng, lengths=None):
        full = bucket_batches(self.lengths if lengths is None else lengths, self.batch_size, self.bucket_size, self.shuffle, self.drop_last, rng)
        return shard_batches(full, self.rank, self.world), full

    def next_epoch(self):
        """-> (this rank's batches, the full batch list, factor index per utterance of the data set or None)."""
        epoch, self.epoch = self.epoch, self.epoch + 1
        if self.speed_pq is None:
            return self.batches(self.rng) + (None,)
        fidx = speed_mod.draw_factors(self.seed, epoch, len(self.lengths), len(self.speed_pq))
        lengths = [speed_mod.perturbed_len(n, *self.speed_pq[f]) for n, f in zip(self.lengths, fidx)]
        return self.batches(self.rng, lengths) + (fidx,)


def source_rates(dataset, lengths):
    """-> (rate of every utterance, or None when all are at 16 kHz; lengths at 16 kHz), host logic only.  The converted lengths are what
    BatchPlan forms its buckets on (and what a speed factor then perturbs); `lengths` stay source samples."""
    rates = [dataset.rate(i) for i in range(len(dataset))]
    if all(r == resample_mod.TARGET for r in rates):
        return None, lengths
    return rates, [resample_mod.plan(r).n_out(n) for n, r in zip(lengths, rates)]


class MetaLayout:
    """THE layout of the one int32 buffer that carries every integer of a batch to the device, stated once: a field's offset exists
    here and nowhere else, and field() slices the numpy view of the pinned buffer and its device copy alike.  A feature that is off
    contributes no words (all off: 2 B + B lmax words, the copy the first loader made)."""

    def __init__(self, B, lmax, factor=False, rate=False, aug=False, spec=0, views=1):
        fields = [("n_samples", (B,)), ("tgt_len", (B,)), ("tgt", (B, lmax))]
        if factor:
            fields += [("factor", (B,))]                               # speed-factor index per utterance
        if rate:
            fields += [("rate_idx", (B,)), ("win", (B, 5))]            # {in_base, n_avail, n_total, out_start, n_emit}
        if aug:
            fields += [("rir_idx", (B,)), ("noise_par", (B, 4))]       # {clip, offset, scale as float bits, 0}
        if spec:
            fields += [("spec", (B, int(spec)))]                       # SpecAugment policy rows, spec = the policy's width (specaug.resolve)
            if views == 2:
                fields += [("spec1", (B, int(spec)))]                  # ... of the second view of the same B utterances (views=2)
        self.B, self.lmax, self.at, self.size = B, lmax, {}, 0
        for name, shape in fields:
            words = B * (shape[1] if len(shape) > 1 else 1)
            self.at[name] = (self.size, self.size + words, shape)
            self.size += words

    def __contains__(self, name):
        return name in self.at

    def field(self, buf, name):
        """Field `name` of `buf` (1-D, numpy or torch, at least `size` words) as a view of its shape."""
        lo, hi, shape = self.at[name]
        return buf[lo:hi].reshape(shape)


# BucketedWaveLoader.speed: the (p, q) list on the host, pq (F, 2) int32 and taps (F, qmax, ntaps) f32 on the device (speed.build_tables)
SpeedTables = collections.namedtuple("SpeedTables", "pq_host pq taps")

# what pack_meta decides: the lengths at 16 kHz and after the speed perturbation (each the one before it where its stage does not run), the
# row widths of the two length-changing stages (0: the batch does not launch that stage) and whether any utterance drew a response / a clip
BatchMeta = collections.namedtuple("BatchMeta", "len16 len_out smax16 smax_out any_rir any_noise")


def pack_meta(lay, meta, sizes, tgt, fs=None, pq=None, rates=None, rate_table=None, aug=None, *, spec=None, spec1=None):
    """The host half of a batch, no GPU: fills `meta` (numpy int32, lay.size words) field by field and decides what the batch launches.
    sizes: sample counts, tgt: label lists; fs, pq: the batch's speed-factor indices and the (p, q) list; rates, rate_table: the batch's
    source rates and a resample.RateTable (one built with device=None does); aug: noise.draw_augment's four lists, the batch's rows;
    spec: the batch's SpecAugment policy rows (B, width), or a function that makes them from the batch's final lengths (len_out, which are
    decided here); spec1: the same for the second view's rows (a layout built with views=2).  Each group is read only when `lay` has its
    fields.  -> BatchMeta."""
    assert meta.shape == (lay.size,) and meta.dtype == np.int32 and len(sizes) == len(tgt) == lay.B
    lay.field(meta, "n_samples")[:] = sizes
    lay.field(meta, "tgt_len")[:] = [len(t) for t in tgt]
    tg = lay.field(meta, "tgt")
    for r, t in enumerate(tgt):
        tg[r, :len(t)] = t
        tg[r, len(t):] = 0
    len16, smax16 = sizes, 0          # smax16 > 0: at least one utterance of the batch is at another rate than 16 kHz
    if "rate_idx" in lay:
        win, ridx = rate_table.windows(sizes, rates)
        lay.field(meta, "rate_idx")[:], lay.field(meta, "win")[:] = ridx, win
        if any(r >= 0 for r in ridx):
            len16 = [int(v) for v in win[:, 4]]      # from here on the lengths are those at 16 kHz
            smax16 = max(1, max(len16))
    len_out, smax_out = len16, 0      # smax_out > 0: at least one utterance of the batch is speed-perturbed
    if "factor" in lay:
        lay.field(meta, "factor")[:] = fs
        if any(pq[f][0] != pq[f][1] for f in fs):
            len_out = [speed_mod.perturbed_len(n, *pq[f]) for n, f in zip(len16, fs)]
            smax_out = max(1, max(len_out))
    any_rir = any_noise = False
    if "rir_idx" in lay:
        nidx, noff, snr, ridx = aug
        lay.field(meta, "rir_idx")[:] = ridx
        par = lay.field(meta, "noise_par")
        for r in range(lay.B):
            par[r] = (nidx[r], noff[r], noise_mod.snr_scale_bits(snr[r]), 0)
        any_rir, any_noise = any(v >= 0 for v in ridx), any(v >= 0 for v in nidx)
    if "spec" in lay:
        lay.field(meta, "spec")[:] = spec(len_out) if callable(spec) else spec
    if "spec1" in lay:
        lay.field(meta, "spec1")[:] = spec1(len_out) if callable(spec1) else spec1
    return BatchMeta(len16, len_out, smax16, smax_out, any_rir, any_noise)


_LOADERS = weakref.WeakSet()      # loaders of this process (paused() holds every one's gate)


@contextlib.contextmanager
def paused():
    """No loader's helper thread touches the GPU runtime inside this block: each helper takes its loader's gate around the preparation of a
    batch (pinned allocations, copies, front-end kernels, event calls), and this context holds all the gates.  graph.GraphedStep wraps its
    warm-up and capture in it: under torch.cuda.graph's default capture mode an allocation or an event synchronisation on ANOTHER thread
    invalidates the capture (round-4 ADVICE).  Work a helper has already queued on its stream keeps running - only API calls matter."""
    gates = [l._gate for l in list(_LOADERS)]
    for g in gates:
        g.acquire()
    try:
        yield
    finally:
        for g in reversed(gates):
            g.release()


class BucketedWaveLoader:
    """Iterating yields Packs on `device`; batches are prepared ahead on the loader's stream by a helper thread.
    A yielded Pack (and every tensor in it) is valid until the NEXT one is requested: its memory belongs to a staging slot that the helper
    reuses SLOTS batches later, ordered behind an event the consumer's stream records when it asks for the next batch (copy what must live
    longer)."""

    def __init__(self, dataset, batch_size, parser=None, augment=False, shuffle=True, drop_last=False, seed=0, bucket_size=None,
                 device="cuda", dtype=torch.bfloat16, rank=0, world=1, speed_perturb=None, noise=None, noise_prob=0.5, snr_db=(5, 20), rir=None,
                 rir_prob=0.5, rir_method="direct", rir_max_taps=noise_mod.MAX_TAPS, resample=False, spec_augment=None, views=1):
        """rank / world: data-parallel sharding.  Every rank draws the SAME batch list (same seed), keeps only the full
        batches when world > 1 (dist.DataParallel normalises by world x local batch and every rank must take the same
        number of steps), drops the ragged tail of len(batches) % world and takes batches[rank::world].
        speed_perturb: sequence of speed factors such as (0.9, 1.0, 1.1) (speed.parse_factor); every epoch each utterance draws one of
        them (BatchPlan) and is resampled on the loader's stream in front of the log-mel kernel, so lengths and frame counts change
        from epoch to epoch.  None / empty: no perturbation, nothing of it is called.
        noise / rir: a noise.NoiseBank / noise.RirBank, or a list of wav paths (or arrays) from which one is built.  Every epoch each
        utterance draws (noise.draw_augment) a response with probability rir_prob and a noise clip, a start offset in it and a
        signal-to-noise ratio uniform in snr_db = (lo, hi) dB with probability noise_prob; on the loader's stream the utterance is then
        speed-perturbed, reverberated, mixed with the noise - the room first, as Kaldi does - and only then parsed.  Lengths, buckets
        and labels do not change.  Both None: nothing of it is called.
        rir_method, rir_max_taps: for a bank built here from paths - "direct" (asr_reverb_fwd, responses cut to at most 8192 taps), "fft"
        (asr_reverb_fft_fwd, at most 65536 taps, cost nearly flat in the length) or "auto" (decided once from the bank's longest response:
        noise.RirBank).  A ready-made RirBank decides by its own method.  Draws, lengths and buckets do not depend on the method.
        resample: True = utterances at another rate than 16 kHz (dataset.rate(i); WaveDataset(resample=True)) are converted on the loader's
        stream in front of everything else - one asr_resample_fwd launch per batch, whatever rates it mixes; a batch that is all 16 kHz
        launches nothing.  Buckets, and the speed perturbation's lengths, are formed on the converted lengths; the staging slot holds
        source samples.  False: nothing of it is called.
        spec_augment: a specaug.SpecAugmentPolicy or its string ("wenet", "espnet", "w5,t2x50,f2x10,s3x30,r200"): several time and mel masks
        with zero fill, time warp and substitution on the normalised frames (tests/specaug_ref.py), in place of - never together with -
        augment=True, the reference's one-mask variant.  Every epoch each utterance draws its numbers (specaug.draw: a function of seed,
        epoch and utterance index that leaves `rng` alone); the ranges are resolved on the host from the lengths pack_meta decides and
        travel in the one meta buffer, so nothing is read back from the device.  None / empty: nothing of it is called.
        views: 2 = two views of every utterance for CR-CTC training (config.cr_ctc_weight): a batch then has 2 * batch_size rows, [view 0
        of the B utterances | view 1 of the same B], with the targets and lengths repeated.  The waveform chain (resample, speed,
        reverberation, noise) runs once per utterance; only parse_batch, which applies the masks, runs per view - view 0 with the table of
        a one-view loader (its rows are that loader's batch, bit for bit), view 1 with specaug.draw(..., view=1).  Without a policy the two
        views are equal and differ by the model's dropout only.  Not with augment=True (masks from `rng`, not reproducible per view)."""
        if isinstance(views, bool) or views not in (1, 2):
            raise ValueError(f"views={views!r}: 1, or 2 (two views of every utterance, CR-CTC training)")
        if views == 2 and augment:
            raise ValueError("views=2 draws every view's masks per utterance (spec_augment=...): not with augment=True, whose masks come from the loader's rng")
        self.views = views
        self.spec = specaug_mod.as_policy(spec_augment)
        if self.spec is not None and augment:
            raise ValueError("spec_augment replaces the reference's SpecAugment: pass it or augment=True, not both")
        self.ds, self.batch_size, self.augment = dataset, batch_size, augment
        self.device, self.dtype = torch.device(device), dtype
        if self.device.type != "cuda":
            raise RuntimeError("the feature front end runs on the GPU only (no CPU fallback)")
        self.parser = parser or AudioParser(device=self.device)
        if self.spec is not None:
            self.spec.check_mels(self.parser.n_mels)
        self.stream = self._copy_stream()
        self.lengths = [dataset.num_samples(i) for i in range(len(dataset))]      # source samples: what the staging slot holds
        # per-utterance source rates (None: all 16 kHz, or resample off) and the lengths at 16 kHz the buckets are formed on
        self.rates, lengths16 = source_rates(dataset, self.lengths) if resample else (None, self.lengths)
        self.rate_table = resample_mod.RateTable(self.rates, self.device) if self.rates is not None else None      # resident on the device
        self.speed = None      # built once, resident on the device
        if speed_perturb is not None and len(speed_perturb) > 0:
            pq, taps = speed_mod.build_tables(speed_perturb)
            self.speed = SpeedTables([tuple(int(v) for v in r) for r in pq], torch.from_numpy(pq).to(self.device), torch.from_numpy(taps).to(self.device))
        bank = lambda v, cls, **kw: None if v is None else v if isinstance(v, cls) else cls(v, self.device, **kw) if len(v) > 0 else None
        if rir_method not in noise_mod.METHODS + ("auto",):
            raise ValueError(f"rir_method={rir_method!r}: one of 'direct', 'fft', 'auto'")
        self.noise, self.rir = bank(noise, noise_mod.NoiseBank, resample=resample), bank(rir, noise_mod.RirBank, max_taps=rir_max_taps, method=rir_method, resample=resample)
        self.noise_prob, self.rir_prob, self.snr_db = float(noise_prob), float(rir_prob), snr_db
        self.plan = BatchPlan(lengths16, batch_size, bucket_size, shuffle, drop_last, seed, rank, world, self.speed.pq_host if self.speed else None)
        self.rank, self.world, self.shuffle, self.drop_last, self.bucket_size = self.plan.rank, self.plan.world, shuffle, self.plan.drop_last, bucket_size
        self.rng = self.plan.rng                # batch order AND SpecAugment masks (the reference uses the global `random`)
        self._gate = threading.Lock()      # held by the helper thread around _prepare; paused() takes it
        _LOADERS.add(self)

    def _copy_stream(self):
        """The stream of the host-to-device copies and the feature front end of the NEXT batch: ONE per device and process, on a hardware
        queue other than the training stream's and the engine's weight-gradient / auxiliary streams' - whichever of the two is built first
        (engine.shared_stream keeps the registry: a stream chosen later avoids every stream chosen before it)."""
        from .. import engine as E
        return E.shared_stream(self.device, "loader")

    def __len__(self):
        n = len(self.ds)
        if self.world > 1:      # full batches only (per bucket), the same count on every rank
            return len(self.plan.batches(random.Random(0))[0])
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _batches(self, rng):      # this rank's batch list for `rng` (tests/test_train_loop_gpu.py reads the order through it)
        return self.plan.batches(rng)[0]

    # ---- staging: pinned host buffers that are REUSED (a fresh pageable tensor + pin_memory() + 32 tensor-slice assignments + six small
    # pageable host-to-device copies cost 25 ms of host time per batch of 32 x 5 s - the training step takes 3 ms), filled through
    # numpy views (plain memcpy, the GIL released), one buffer for the samples and ONE for every integer of the batch
    SLOTS = 4

    def _slot(self, k, n_wave, n_meta):
        """Staging slot k, free for a new batch.  A slot owns the pinned host buffers AND the device tensors of the batch it staged last
        (`keep`): those go back to the loader stream's pool only here, SLOTS batches later, after the loader's stream has been made to wait
        for `consumed` - the event the consumer's stream recorded when it asked for the batch after that one.  (Round 4 marked every tensor
        of a pack with Tensor.record_stream instead: the mechanism that made the caching allocator regrow by hipMalloc in the engine.)"""
        slots = self.__dict__.setdefault("_slots", [None] * self.SLOTS)
        s = slots[k]
        if s is not None:
            s["copied"].synchronize()      # the copy out of this slot (SLOTS batches ago) has run: the host may overwrite the pinned buffers
            if s["handed"]:
                self.stream.wait_event(s["consumed"])      # recorded before the consumer took the batch after this slot's (see __iter__)
            s["keep"], s["handed"] = None, False
        if s is None or s["wave"].numel() < n_wave or s["meta"].numel() < n_meta:
            cap_w = max(n_wave, s["wave"].numel() if s else 0) * 5 // 4
            cap_m = max(n_meta, s["meta"].numel() if s else 0) * 2
            s = dict(wave=torch.empty(cap_w, dtype=torch.float32, pin_memory=True), meta=torch.empty(cap_m, dtype=torch.int32, pin_memory=True),
                     copied=torch.cuda.Event(), consumed=torch.cuda.Event(), keep=None, handed=False)
            s["wave_np"], s["meta_np"] = s["wave"].numpy(), s["meta"].numpy()
            slots[k] = s
        return s

    def _prepare(self, idx, k=0, fidx=None, aug=None, spec=None, spec1=None):
        """fidx: speed-factor index per utterance of the data set (BatchPlan.next_epoch), None = no perturbation.
        aug: noise.draw_augment's four lists for the data set, None = neither noise nor reverberation.
        spec: specaug.draw's table for the data set, None = no SpecAugment policy; spec1: the second view's table (views=2 with a policy).
        The integers of the batch travel in one buffer whose layout is MetaLayout; pack_meta fills it and decides what is launched."""
        tgt = [self.ds.ids(i) for i in idx]
        B = len(idx)
        lay = MetaLayout(B, max(1, max(len(t) for t in tgt)), factor=fidx is not None, rate=self.rates is not None, aug=aug is not None,
                         spec=self.spec.width if spec is not None else 0, views=2 if spec1 is not None else 1)
        into = getattr(self.ds, "wave_into", None)
        waves = None if into is not None else [self.ds.wave(i) for i in idx]
        smax = max(self.lengths[i] for i in idx) if waves is None else max(w.size for w in waves)
        slot = self._slot(k % self.SLOTS, B * smax, lay.size)
        buf = slot["wave_np"][:B * smax].reshape(B, smax)
        items = getattr(self.ds, "items", None)
        if waves is None and items is not None and any(isinstance(items[i][0], str) for i in idx):
            # files: read / decode the rows in parallel (file reads and numpy loops run without the GIL); 3.4 - 3.8 ms/step against 4 - 6 serially
            pool = self.__dict__.get("_pool")
            if pool is None:
                import concurrent.futures
                pool = self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=4, thread_name_prefix="asr-decode")
            sizes = list(pool.map(lambda r: into(idx[r], buf[r]), range(B)))
        elif waves is None:      # arrays in memory: 32 memcpys are cheaper than handing them to a pool (3.24 vs 3.35 ms/step)
            sizes = [into(idx[r], buf[r]) for r in range(B)]
        else:
            sizes = []
            for r, w in enumerate(waves):
                buf[r, :w.size] = w
                buf[r, w.size:] = 0.0
                sizes.append(w.size)
        take = lambda per_utt: [per_utt[i] for i in idx]
        m = pack_meta(lay, slot["meta_np"][:lay.size], sizes, tgt, fs=take(fidx) if fidx is not None else None,
                      pq=self.speed.pq_host if self.speed else None, rates=take(self.rates) if self.rates is not None else None,
                      rate_table=self.rate_table, aug=[take(a) for a in aug] if aug is not None else None,
                      spec=(lambda lens: self.parser.spec_ranges(self.spec, spec[idx], lens)) if spec is not None else None,
                      spec1=(lambda lens: self.parser.spec_ranges(self.spec, spec1[idx], lens)) if spec1 is not None else None)
        from .. import kernels as K
        with torch.cuda.stream(self.stream):
            dev_wav = slot["wave"][:B * smax].view(B, smax).to(self.device, non_blocking=True)
            dev_meta = slot["meta"][:lay.size].to(self.device, non_blocking=True)
            slot["copied"].record()
            field = lambda name: lay.field(dev_meta, name)
            wav, wav_len = dev_wav, field("n_samples")
            # the chain: each stage takes (wav, wav_len) and gives (wav, wav_len), launched or skipped by pack_meta's flags.  `keep` is what
            # the slot holds until it is reused: the copies, then everything a stage makes (outputs and workspaces) - a stage's input is
            # the output of the one before it - so nothing a kernel queued on this stream touches goes back to the pool early.
            keep = [dev_wav, dev_meta]
            if m.smax16:
                wav, wav_len = K.resample(wav, field("rate_idx"), field("win"), *self.rate_table.dev, m.smax16)
                keep += [wav, wav_len]
            if m.smax_out:
                wav, wav_len = K.speed_perturb(wav, wav_len, field("factor"), self.speed.pq, self.speed.taps, m.smax_out)
                keep += [wav, wav_len]
            if m.any_rir:      # a batch in which no utterance drew a response launches nothing
                rir = (wav, wav_len, field("rir_idx"), self.rir.table, self.rir.lens, self.rir.peaks)
                if self.rir.method == "fft":
                    ws = K.reverb_fft_workspace(B, wav.shape[1], self.rir.table.shape[1], self.device)
                    wav = K.reverb_fft(*rir, ws=ws)
                    keep += [wav, ws]
                else:
                    wav = K.reverb(*rir)
                    keep += [wav]
            if m.any_noise:      # in place
                ws = K.noise_mix_workspace(B, wav.shape[1], self.device)
                keep += [ws, *K.noise_mix(wav, wav_len, field("noise_par"), self.noise.noise, self.noise.noise_off, out=wav, ws=ws)]
            if spec is not None:
                feat, feat_len = self.parser.parse_batch(wav, wav_len, self.dtype, spec_ranges=field("spec"), spec_policy=self.spec)
            else:
                feat, feat_len = self.parser.parse_batch(wav, wav_len, self.dtype, augment=self.augment, rng=self.rng)
            tgt_dev, tgt_len, feat_len = field("tgt").long(), field("tgt_len").long(), feat_len.long()
            if self.views == 2:      # [view 0 of the B utterances | view 1 of the same B]: the same waveforms, targets and lengths
                feat1 = feat
                if spec1 is not None:
                    feat1, _ = self.parser.parse_batch(wav, wav_len, self.dtype, spec_ranges=field("spec1"), spec_policy=self.spec)
                feat = torch.cat([feat, feat1])
                tgt_dev, tgt_len, feat_len = tgt_dev.repeat(2, 1), tgt_len.repeat(2), feat_len.repeat(2)
            pack = Pack()
            pack.add(wave=feat, wave_len=feat_len, tgt_for_input=tgt_dev, tgt_for_metric=tgt_dev.clone(), tgt_len=tgt_len)
            done = torch.cuda.Event()
            done.record()
        slot["keep"] = tuple(keep) + (feat, feat_len) + tuple(v for v in pack.values() if torch.is_tensor(v))
        return pack, done, slot

    PREFETCH = 2      # batches prepared ahead by the helper thread

    def __iter__(self):
        """Batches are prepared by a helper thread, PREFETCH ahead: decoding / padding into the pinned slot (memcpy: no GIL), the two
        host-to-device copies and the feature kernels on the loader's stream.  The consumer's stream waits for the batch's event."""
        import queue
        from .. import kernels as K
        epoch = self.plan.epoch
        batches, _, fidx = self.plan.next_epoch()
        aug = None
        if self.noise is not None or self.rir is not None:
            aug = noise_mod.draw_augment(self.plan.seed, epoch, len(self.ds), self.noise_prob, len(self.noise) if self.noise else 0,
                                         self.noise.lens if self.noise else (), self.snr_db, self.rir_prob, len(self.rir) if self.rir else 0)
        spec = specaug_mod.draw(self.plan.seed, epoch, len(self.ds), self.spec) if self.spec is not None else None
        spec1 = specaug_mod.draw(self.plan.seed, epoch, len(self.ds), self.spec, view=1) if (self.spec is not None and self.views == 2) else None
        q = queue.Queue(maxsize=self.PREFETCH)
        stop = threading.Event()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()      # the consumer's device

        def hand_over(item):      # False: the consumer is gone
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    continue
            return False

        def work():
            K._TLS.own_stream = True      # never follow the training thread's stream override (kernels._stream)
            try:
                torch.cuda.set_device(dev_index)
                for k, idx in enumerate(batches):
                    with self._gate:      # paused() (a hipGraph capture on the consumer thread) keeps this thread off the GPU runtime
                        item = self._prepare(idx, k, fidx, aug, spec, spec1)
                    if not hand_over(item):
                        return
                hand_over(None)
            except BaseException as e:      # noqa: BLE001 - handed to the consumer
                hand_over(e)

        th = threading.Thread(target=work, name="asr-loader", daemon=True)
        th.start()
        last = None      # slot of the batch the consumer is working on
        try:
            while True:
                if last is not None:
                    # the consumer is back for the next batch: everything it queued on its stream with the previous one is in front of this
                    # event, and the helper makes the loader's stream wait for it before that slot's device memory is reused (SLOTS batches
                    # later; the queue's depth guarantees the record happens before the helper gets there, see _slot)
                    last["consumed"].record(torch.cuda.current_stream())
                    last["handed"] = True
                    last = None
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                pack, done, last = item
                torch.cuda.current_stream().wait_event(done)
                yield pack
        finally:
            stop.set()
            th.join(timeout=5.0)
            if last is not None:      # the consumer left in the middle of an epoch
                last["consumed"].record(torch.cuda.current_stream())
                last["handed"] = True

def parser_norm(cmvn):
    """AudioParser's normalisation arguments for the value of a cmvn flag: a path selects global CMVN, None / empty today's."""
    return dict(norm="global", cmvn=str(cmvn)) if cmvn else {}


def build_dataloader(collector_path, vocab, batch_size, part="test", use_cuda=True, sample_rate=16000, window_size=400, n_mels=40,
                     augment=False, predump=False, use_old=False, lfr_m=4, lfr_n=3, dtype=torch.bfloat16, shuffle=None, seed=0,
                     rank=0, world=1, speed_perturb=None, cmvn=None, noise=None, noise_prob=0.5, snr_db=(5, 20), rir=None, rir_prob=0.5,
                     rir_method="direct", rir_max_taps=noise_mod.MAX_TAPS, resample=False, frontend="reference", spec_augment=None, views=1):
    """build_dataloader of the reference (data/data_loader/ai_shell_1.py:91-104), same arguments: reads the manifest
    `<collector_path>_<part>.json` written by the reference's collector (one JSON object {"wave": path, "tgt": text}
    per line, data_collector/ai_shell_1.py:73-79) and returns an iterable of Packs.  The reference computes features
    on the CPU per utterance and can cache them as .t files (predump / use_old); here they are computed on the GPU
    per batch, so both flags are accepted and ignored.  drop_last=True as in the reference (:103).
    speed_perturb: speed factors such as (0.9, 1.0, 1.1) for BucketedWaveLoader (the reference has none); None = off.
    noise / rir, noise_prob, snr_db, rir_prob: BucketedWaveLoader's noise and reverberation augmentation, applied to part="train" only
    (the reference has none); None = off.  rir_method, rir_max_taps: BucketedWaveLoader's, for the same part.
    cmvn: path of a global-CMVN statistics file (tools/compute_cmvn.py): the features of this part are normalised per mel bin by
    the corpus statistics (AudioParser norm="global"); None / empty = the reference's per-utterance normalisation.
    resample: True = files (and noise / response files of a bank built here) at another rate than 16 kHz are converted on the GPU
    (WaveDataset / BucketedWaveLoader / noise banks, every part); False = they raise, as before.
    frontend: "reference" (the reference's log-mel) or "kaldi" (Kaldi fbank): AudioParser's.
    spec_augment: BucketedWaveLoader's SpecAugment policy (a specaug.SpecAugmentPolicy or its string), applied to part="train" only and never
    together with augment=True; None / empty = off.
    views: BucketedWaveLoader's, for part="train" only (2: two views of every utterance, CR-CTC training); every other part has one view."""
    import json
    spec = specaug_mod.as_policy(spec_augment)      # a malformed string, or both augmentations, is refused before anything is built
    if spec is not None:
        spec.check_mels(n_mels)
        if augment:
            raise ValueError("spec_augment replaces the reference's SpecAugment: pass it or augment=True, not both")
    if not use_cuda:
        raise RuntimeError("the feature front end runs on the GPU only (no CPU fallback)")
    if window_size != 400:
        raise ValueError("the log-mel kernel is built for the reference's window of 400 samples (data_config.py:13)")
    items = []
    with open(collector_path + "_" + part + ".json", encoding="utf-8") as reader:
        for line in reader:
            if line.strip():
                rec = json.loads(line)
                items.append((rec["wave"], rec["tgt"]))
    ds = WaveDataset(items, vocab, sample_rate=sample_rate, resample=resample)
    parser = AudioParser(sample_rate=sample_rate, n_mels=n_mels, lfr_m=lfr_m, lfr_n=lfr_n, device="cuda", frontend=frontend, **parser_norm(cmvn))
    wave_aug = dict(noise=noise, noise_prob=noise_prob, snr_db=snr_db, rir=rir, rir_prob=rir_prob, rir_method=rir_method,
                    rir_max_taps=rir_max_taps, spec_augment=spec, views=views) if part == "train" else {}
    return BucketedWaveLoader(ds, batch_size, parser=parser, augment=augment, shuffle=(part == "train") if shuffle is None else shuffle,
                              drop_last=True, seed=seed, dtype=dtype, rank=rank, world=world, speed_perturb=speed_perturb, resample=resample, **wave_aug)
