"""Training from WAVEFORMS: in-memory 5-s utterances -> BucketedWaveLoader (pinned copy + log-mel / normalisation / SpecAugment on a side stream) ->
model.iterate, against the same model fed one resident batch (what bench.py times).  python tools/loader_bench.py [joint]
python tools/loader_bench.py --speed_perturb[=0.9,1.0,1.1] [--out=profiles/speed_perturb_bench.json]: the speed-perturbation kernel alone
(B = 32 x 5 s, factors mixed in thirds) beside a device-to-device copy of the same input plus output bytes, and the waveform-fed joint
step with the perturbation off and on, alternated in one process; the figures go to the JSON file.
python tools/loader_bench.py --noise_reverb [--out=profiles/noise_reverb_bench.json]: asr_reverb_fwd at 1024, 4096 and 8192 taps with every
utterance of B = 32 x 5 s reverberated (achieved fp32 FLOP/s against the vector peak) beside the same convolution through torch.fft,
asr_noise_mix_fwd beside a device-to-device copy of its bytes, and the waveform-fed joint step with the augmentation off, at the default
probabilities and with both probabilities 1, alternated in one process.
python tools/loader_bench.py --reverb_fft [--out=profiles/reverb_fft_bench.json]: asr_reverb_fft_fwd, asr_reverb_fwd (up to its 8192 taps) and
the torch.fft stand-in at 256 .. 65536 taps, same protocol, and the waveform-fed joint step with rir_method direct and fft at 4096 taps.
python tools/loader_bench.py --resample [--out=profiles/resample_bench.json]: asr_resample_fwd on B = 32 x 5 s at 8, 44.1 and 48 kHz beside a
device-to-device copy of its bytes and the strided conv1d polyphase form in torch, the waveform-fed joint step from a 16 kHz corpus (resample
off and on) and from a 48 kHz one, alternated, and the host time of StreamResampler.push for one 480 ms block.
python tools/loader_bench.py --fbank [--out=profiles/fbank_bench.json]: asr_fbank_fwd (Kaldi fbank) beside asr_logmel_fwd on the same batch of
B = 32 x 5 s at 80 bins, a device-to-device copy of the same bytes, and a torch stand-in (unfold, the frame arithmetic, torch.fft.rfft,
matmul, log); then push_audio of one 480 ms block with each front end (tools/stream_frontend_bench.py).
python tools/loader_bench.py --spec_augment [--out=profiles/spec_augment_bench.json]: per normalisation the no-mask call, the reference-mask call
and asr_*_norm_specaug_lfr_fwd under `wenet`, `espnet` and `w5,t2x50,f2x10,s3x30` (B = 32 x 5 s, 80 bins, LFR 4/3, bf16), the host time of
_prepare with augment=True and with spec_augment, and the waveform-fed joint step off, with augment=True and with `wenet`, alternated."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from asr_chinese_e2e_amd import Models
from asr_chinese_e2e_amd.data_handler import AudioParser, BucketedWaveLoader, Vocab, WaveDataset
from asr_chinese_e2e_amd.Trainer import FusedAdam, NoamOpt

SPEED = next((a for a in sys.argv[1:] if a.startswith("--speed_perturb")), None)
NOISE_REVERB = any(a == "--noise_reverb" for a in sys.argv[1:])
REVERB_FFT = any(a == "--reverb_fft" for a in sys.argv[1:])
RESAMPLE = any(a == "--resample" for a in sys.argv[1:])
FBANK = any(a == "--fbank" for a in sys.argv[1:])
SPEC_AUGMENT = any(a == "--spec_augment" for a in sys.argv[1:])
JOINT = SPEED is not None or NOISE_REVERB or REVERB_FFT or RESAMPLE or FBANK or SPEC_AUGMENT or (len(sys.argv) > 1 and sys.argv[1] == "joint")
B, S, NB = 32, 16000 * 5, 40
rng = np.random.RandomState(0)
vocab = Vocab.synthetic(4232)
items = [((rng.randn(S) * 0.1).astype(np.float32), [int(t) for t in rng.randint(4, 4232, size=16)]) for _ in range(B * NB)]
if os.environ.get("FILES") == "1":      # the same utterances as 16-bit WAV files (decoded by the loader)
    import tempfile, wave
    d = tempfile.mkdtemp(prefix="asr_wav_")
    for i, (w, t) in enumerate(items):
        path = os.path.join(d, f"u{i}.wav")
        with wave.open(path, "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((np.clip(w, -1, 1) * 32767).astype("<i2").tobytes())
        items[i] = (path, t)
    print(f"{len(items)} WAV files under {d}")
ds = WaveDataset(items, vocab)
parser = AudioParser(n_mels=80, lfr_m=1, lfr_n=1, device="cuda")
M = Models.TransformerOffical if JOINT else Models.TransformerCTC
cfg = M.get_default_config()(); cfg.fn_build(dict(n_mels=80, lfr_m=1, dropout=0.0, ctc_weight=0.3 if JOINT else 1.0))
model = M(cfg, vocab).cuda()
opt = NoamOpt(512, 1, 4000, FusedAdam(model.parameters(), lr=3e-4, betas=(0.9, 0.98), eps=1e-9))
loader = BucketedWaveLoader(ds, B, parser=parser, augment=True, shuffle=True, seed=1, dtype=torch.bfloat16)


def speed_bench():
    import json
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.data_handler import speed
    factors = tuple(SPEED.split("=", 1)[1].split(",")) if "=" in SPEED else ("0.9", "1.0", "1.1")
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), "profiles/speed_perturb_bench.json")
    pq, taps = speed.build_tables(factors)
    fac = [i % len(factors) for i in range(B)]                                   # mixed in thirds
    n_out = [speed.perturbed_len(S, int(pq[f][0]), int(pq[f][1])) for f in fac]
    smax_out = max(n_out)
    wav = torch.from_numpy(np.stack([items[i][0] for i in range(B)])).cuda() if not isinstance(items[0][0], str) else torch.randn(B, S, device="cuda") * 0.1
    wl = torch.full((B,), S, dtype=torch.int32, device="cuda")
    args = (wav, wl, torch.tensor(fac, dtype=torch.int32, device="cuda"), torch.from_numpy(pq).cuda(), torch.from_numpy(taps).cuda(), smax_out)
    out, out_len = K.speed_perturb(*args)
    assert out_len.tolist() == n_out
    half = (B * S + B * smax_out) // 2                                            # a copy of `half` floats reads and writes the kernel's bytes in all
    src, dst = torch.randn(half, device="cuda"), torch.empty(half, device="cuda")

    def timed(fn, reps=200):
        for _ in range(20): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    kern, copy = [], []
    for _ in range(5):                                                            # alternated
        kern.append(timed(lambda: K.speed_perturb(*args, out=out, out_len=out_len)))
        copy.append(timed(lambda: dst.copy_(src)))
    algo_bytes = 4 * (B * S + B * smax_out)                                      # every input sample read once, every output sample (padding included) written once
    res = dict(device=torch.cuda.get_device_name(0), factors=list(factors), B=B, samples=S, Smax_out=smax_out, ntaps=int(taps.shape[2]), phases=int(taps.shape[1]),
               kernel_us=kern, kernel_us_median=float(np.median(kern)), bytes_read_plus_written=algo_bytes,
               kernel_GBps=algo_bytes / float(np.median(kern)) / 1e3,
               d2d_copy_same_bytes_us=copy, d2d_copy_us_median=float(np.median(copy)), d2d_copy_GBps=8 * half / float(np.median(copy)) / 1e3,
               timing="HIP events around 200 back-to-back launches after 20 warm-up launches, 5 rounds alternating kernel and copy")
    print(json.dumps({k: res[k] for k in ("kernel_us_median", "d2d_copy_us_median", "kernel_GBps", "d2d_copy_GBps")}), flush=True)
    # the waveform-fed joint step, perturbation off and on, alternated; same model, same data set, SpecAugment on
    mk = lambda sp: BucketedWaveLoader(ds, B, parser=parser, augment=True, shuffle=True, seed=1, dtype=torch.bfloat16, speed_perturb=sp)
    loaders = dict(off=mk(None), on=mk(factors))

    def run(ld):
        n = 0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for pack in ld:
            model.iterate(pack, optimizer=opt)
            n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for ld in loaders.values(): run(ld)                                           # warm-up epoch each (new shapes: allocator, code objects)
    step = dict(off=[], on=[])
    for _ in range(4):
        for name, ld in loaders.items():
            step[name].append(run(ld))
            print(f"joint step from waveforms, speed perturbation {name}: {step[name][-1]:.3f} ms/step", flush=True)
    prep = {}
    for name, ld in loaders.items():                                              # host time of preparing a batch alone
        _, _, fidx = ld.plan.next_epoch()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for k in range(20): ld._prepare(list(range(B)), k, fidx)
        prep[name] = (time.perf_counter() - t0) / 20 * 1e3
        torch.cuda.synchronize()
    res.update(joint_step_ms_off=step["off"], joint_step_ms_on=step["on"], joint_step_ms_off_median=float(np.median(step["off"])),
               joint_step_ms_on_median=float(np.median(step["on"])), prepare_host_ms_off=prep["off"], prepare_host_ms_on=prep["on"],
               joint_config=f"{NB} batches of {B} x 5 s per epoch in host memory, SpecAugment on, bf16 joint model at the default width; 1 warm-up epoch each, "
                            "then 4 epochs each, alternating off / on; host clock around an epoch that ends in a device synchronise")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def noise_reverb_bench():
    import json
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.data_handler import noise
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), "profiles/noise_reverb_bench.json")
    PEAK = 157.3e12                                                               # fp32 vector peak of the MI355X, FLOP/s
    wav = torch.from_numpy(np.stack([items[i][0] for i in range(B)])).cuda() if not isinstance(items[0][0], str) else torch.randn(B, S, device="cuda") * 0.1
    wl = torch.full((B,), S, dtype=torch.int32, device="cuda")
    r = np.random.RandomState(5)

    def timed(fn, reps, warm=3):
        for _ in range(warm): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    def responses(n, L):                                                          # exponentially decaying noise behind a direct path at sample 64
        hs = []
        for _ in range(n):
            h = r.randn(L + 40) * np.exp(-np.arange(L + 40) / (L / 6.0)) * 0.1
            h[:104] *= 0.01
            h[104] = 1.0
            hs.append(h)
        return hs
    res = dict(device=torch.cuda.get_device_name(0), B=B, samples=S, fp32_vector_peak_TFLOPs=PEAK / 1e12, reverb=[])
    out = torch.empty_like(wav)
    for L in (1024, 4096, 8192):
        bank = noise.RirBank(responses(8, L), "cuda", max_taps=L)
        assert bank.lens.tolist() == [L] * 8 and bank.peaks.tolist() == [64] * 8
        ridx = torch.tensor([i % 8 for i in range(B)], dtype=torch.int32, device="cuda")
        args = (wav, wl, ridx, bank.table, bank.lens, bank.peaks)
        nfft = 1 << int(np.ceil(np.log2(S + L - 1)))

        def fft_conv():
            X, H = torch.fft.rfft(wav, nfft), torch.fft.rfft(bank.table[ridx.long()], nfft)
            return torch.fft.irfft(X * H, nfft)[:, 64:64 + S]
        K.reverb(*args, out=out)
        ref = fft_conv()
        diff = float((out - ref).abs().max())                                     # the two computations agree (fp32 FFT round-off)
        kern, fft = [], []
        for _ in range(3):                                                        # alternated
            kern.append(timed(lambda: K.reverb(*args, out=out), reps=20))
            fft.append(timed(fft_conv, reps=20))
        flops = 2.0 * B * S * L
        k, f = float(np.median(kern)), float(np.median(fft))
        res["reverb"].append(dict(taps=L, kernel_us=kern, kernel_us_median=k, multiply_adds=B * S * L, lower_bound_us=flops / PEAK * 1e6,
                                  achieved_TFLOPs=flops / k / 1e6, share_of_vector_peak=flops / k / 1e6 / (PEAK / 1e12),
                                  torch_fft_us=fft, torch_fft_us_median=f, nfft=nfft, max_abs_diff_vs_torch_fft=diff))
        print(json.dumps(res["reverb"][-1]), flush=True)
    res["reverb_timing"] = ("HIP events around 20 back-to-back launches after 3 warm-up launches, 3 rounds alternating the kernel and torch.fft (rfft of the "
                            "batch and of the gathered responses at the next power of two, product, irfft, slice); lower bound = B S L multiply-adds = "
                            "2 B S L FLOP at the fp32 vector peak; edge tiles skip the taps that fall in front of the utterance, so slightly fewer are executed")
    # noise mix beside a copy of the same bytes: x and v read twice (energies, then the mix), out written once = 5 floats per sample
    nb = noise.NoiseBank([(r.randn(n) * 0.05).astype(np.float32) for n in (16000, 50000, 160000, 400000)], "cuda")
    par = torch.tensor([[i % 4, (7919 * i) % nb.lens[i % 4], noise.snr_scale_bits(5 + i % 16), 0] for i in range(B)], dtype=torch.int32, device="cuda")
    ws, gain = K.noise_mix_workspace(B, S, "cuda"), torch.empty(B, device="cuda")
    src, dst = torch.randn(B * S * 5 // 2, device="cuda"), torch.empty(B * S * 5 // 2, device="cuda")
    mix, copy = [], []
    for _ in range(5):
        mix.append(timed(lambda: K.noise_mix(wav, wl, par, nb.noise, nb.noise_off, out=out, gain_out=gain, ws=ws), reps=200, warm=20))
        copy.append(timed(lambda: dst.copy_(src), reps=200, warm=20))
    res["noise_mix"] = dict(kernel_us=mix, kernel_us_median=float(np.median(mix)), bytes_read_plus_written=4 * 5 * B * S, d2d_copy_same_bytes_us=copy,
                            d2d_copy_us_median=float(np.median(copy)), launches=2,
                            timing="HIP events around 200 back-to-back calls (two launches each) after 20 warm-up calls, 5 rounds alternating mix and copy")
    print(json.dumps({k: res["noise_mix"][k] for k in ("kernel_us_median", "d2d_copy_us_median")}), flush=True)
    # the waveform-fed joint step: augmentation off, default probabilities, both probabilities 1; responses of 4096 taps (0.25 s)
    rb = noise.RirBank(responses(8, 4096), "cuda", max_taps=4096)
    mk = lambda **kw: BucketedWaveLoader(ds, B, parser=parser, augment=True, shuffle=True, seed=1, dtype=torch.bfloat16, **kw)
    loaders = dict(off=mk(), default=mk(noise=nb, rir=rb), all=mk(noise=nb, rir=rb, noise_prob=1.0, rir_prob=1.0))

    def run(ld):
        n = 0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for pack in ld:
            model.iterate(pack, optimizer=opt)
            n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for ld in loaders.values(): run(ld)                                           # warm-up epoch each
    step = {name: [] for name in loaders}
    for _ in range(4):
        for name, ld in loaders.items():
            step[name].append(run(ld))
            print(f"joint step from waveforms, noise and reverberation {name}: {step[name][-1]:.3f} ms/step", flush=True)
    res["joint_step_ms"] = step
    res["joint_step_ms_median"] = {name: float(np.median(v)) for name, v in step.items()}
    res["joint_config"] = (f"{NB} batches of {B} x 5 s per epoch in host memory, SpecAugment on, bf16 joint model at the default width, 8 responses of 4096 taps, "
                           "4 noise clips of 1 - 25 s, SNR 5 - 20 dB; off = no banks, default = both probabilities 0.5, all = both 1.0; 1 warm-up epoch each, "
                           "then 4 epochs each, alternating; host clock around an epoch that ends in a device synchronise")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def reverb_fft_bench():
    import json
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.data_handler import noise
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), "profiles/reverb_fft_bench.json")
    wav = torch.from_numpy(np.stack([items[i][0] for i in range(B)])).cuda() if not isinstance(items[0][0], str) else torch.randn(B, S, device="cuda") * 0.1
    wl = torch.full((B,), S, dtype=torch.int32, device="cuda")
    r = np.random.RandomState(5)

    def timed(fn, reps=20, warm=3):
        for _ in range(warm): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    def responses(n, L):                                                          # exponentially decaying noise behind a direct path at sample 64
        hs = []
        for _ in range(n):
            h = r.randn(L + 40) * np.exp(-np.arange(L + 40) / (L / 6.0)) * 0.1
            h[:104] *= 0.01
            h[104] = 1.0
            hs.append(h)
        return hs
    res = dict(device=torch.cuda.get_device_name(0), B=B, samples=S, fft_points=K.REVERB_FFT_N, reverb=[])
    out = torch.empty_like(wav)
    ridx = torch.tensor([i % 8 for i in range(B)], dtype=torch.int32, device="cuda")
    for L in (256, 1024, 4096, 8192, 16384, 32768, 65536):
        bank = noise.RirBank(responses(8, L), "cuda", max_taps=L, method="fft")
        assert bank.lens.tolist() == [L] * 8 and bank.peaks.tolist() == [64] * 8
        args = (wav, wl, ridx, bank.table, bank.lens, bank.peaks)
        ws = K.reverb_fft_workspace(B, S, L, "cuda")
        nfft = 1 << int(np.ceil(np.log2(S + L - 1)))

        def fft_conv():
            X, H = torch.fft.rfft(wav, nfft), torch.fft.rfft(bank.table[ridx.long()], nfft)
            return torch.fft.irfft(X * H, nfft)[:, 64:64 + S]
        contenders = dict(fft_kernel=lambda: K.reverb_fft(*args, out=out, ws=ws), torch_fft=fft_conv)
        if L <= K.REVERB_MAX_TAPS:
            contenders["direct_kernel"] = lambda: K.reverb(*args, out=out)
        K.reverb_fft(*args, out=out, ws=ws)
        diff = float((out - fft_conv()).abs().max())                              # the two computations agree (fp32 FFT round-off)
        us = {name: [] for name in contenders}
        for _ in range(3):                                                        # alternated
            for name, fn in contenders.items():
                us[name].append(timed(fn))
        row = dict(taps=L, partitions=-(-L // (K.REVERB_FFT_N // 2)), workspace_MB=ws.numel() * 4 / 1e6, nfft_torch=nfft, max_abs_diff_vs_torch_fft=diff)
        for name, v in us.items():
            row[name + "_us"], row[name + "_us_median"] = v, float(np.median(v))
        res["reverb"].append(row)
        print(json.dumps(row), flush=True)
        del ws, bank
    res["reverb_timing"] = ("every utterance of the batch reverberated, 8 responses; HIP events around 20 back-to-back calls after 3 warm-up calls, 3 rounds "
                            "alternating the contenders in one process; asr_reverb_fft_fwd = two launches per call; torch.fft = rfft of the batch and of the "
                            "gathered responses at the next power of two, product, irfft, slice")
    wins = [row["taps"] for row in res["reverb"] if "direct_kernel_us_median" in row and row["fft_kernel_us_median"] < row["direct_kernel_us_median"]]
    res["smallest_measured_taps_where_fft_kernel_beats_direct"] = min(wins) if wins else None
    # the waveform-fed joint step, every utterance reverberated with a response of 4096 taps, by either kernel
    hs = responses(8, 4096)
    mk = lambda **kw: BucketedWaveLoader(ds, B, parser=parser, augment=True, shuffle=True, seed=1, dtype=torch.bfloat16, **kw)
    loaders = dict(off=mk(), direct=mk(rir=noise.RirBank(hs, "cuda", max_taps=4096, method="direct"), rir_prob=1.0),
                   fft=mk(rir=noise.RirBank(hs, "cuda", max_taps=4096, method="fft"), rir_prob=1.0))

    def run(ld):
        n = 0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for pack in ld:
            model.iterate(pack, optimizer=opt)
            n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for ld in loaders.values(): run(ld)                                           # warm-up epoch each
    step = {name: [] for name in loaders}
    for _ in range(3):
        for name, ld in loaders.items():
            step[name].append(run(ld))
            print(f"joint step from waveforms, reverberation {name}: {step[name][-1]:.3f} ms/step", flush=True)
    res["joint_step_ms"] = step
    res["joint_step_ms_median"] = {name: float(np.median(v)) for name, v in step.items()}
    res["joint_config"] = (f"{NB} batches of {B} x 5 s per epoch in host memory, SpecAugment on, bf16 joint model at the default width, 8 responses of 4096 taps, "
                           "rir_prob 1; off = no bank; 1 warm-up epoch each, then 3 epochs each, alternating; host clock around an epoch that ends in a "
                           "device synchronise")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def resample_bench():
    import json
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.data_handler import resample as R
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), "profiles/resample_bench.json")
    PEAK = 157.3e12                                                               # fp32 vector peak of one MI355X, FLOP/s
    res = dict(device=torch.cuda.get_device_name(0), B=B, seconds=5, rates=[])

    def timed(fn, reps=20, warm=3):
        for _ in range(warm): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    for fs in (8000, 44100, 48000):
        pl = R.plan(fs)
        n_in = 5 * fs
        n_out = pl.n_out(n_in)
        table = R.RateTable([fs], "cuda")
        wav = torch.randn(B, n_in, device="cuda") * 0.1
        win, ridx = table.windows([n_in] * B, [fs] * B)
        args = (wav, torch.from_numpy(ridx).cuda(), torch.from_numpy(win).cuda()) + table.dev + (n_out,)
        out, out_len = K.resample(*args)
        assert out_len.tolist() == [n_out] * B
        half = (B * n_in + B * n_out) // 2                                        # a copy of `half` floats reads and writes the kernel's bytes in all
        src, dst = torch.randn(half, device="cuda"), torch.empty(half, device="cuda")
        # the stand-in: the polyphase filter as ONE strided conv1d, a channel per phase, as the common toolkits do it - channel i holds
        # H[(i p) mod q] shifted by floor(i p / q), so every channel is wider than the filter by up to p taps (those products are wasted)
        H = R.phase_table(pl).astype(np.float32)
        shift = (np.arange(pl.q) * pl.p) // pl.q
        wt = np.zeros((pl.q, 1, pl.ntaps + int(shift.max())), dtype=np.float32)
        for i in range(pl.q):
            wt[i, 0, shift[i]:shift[i] + pl.ntaps] = H[(i * pl.p) % pl.q]
        wt = torch.from_numpy(wt).cuda()
        M = -(-n_out // pl.q)
        need = (M - 1) * pl.p + wt.shape[2]
        xp = torch.nn.functional.pad(wav, (pl.W, max(need - pl.W - n_in, 0)))[:, None]

        def stand_in():
            return torch.nn.functional.conv1d(xp, wt, stride=pl.p).transpose(1, 2).reshape(B, -1)[:, :n_out]
        diff = float((stand_in() - out).abs().max())
        kern, copy, conv = [], [], []
        for _ in range(3):                                                        # alternated
            kern.append(timed(lambda: K.resample(*args, out=out, out_len=out_len)))
            copy.append(timed(lambda: dst.copy_(src)))
            conv.append(timed(stand_in))
        flop = 2.0 * B * n_out * pl.ntaps
        k, c, t = float(np.median(kern)), float(np.median(copy)), float(np.median(conv))
        row = dict(source_rate=fs, p=pl.p, q=pl.q, ntaps=pl.ntaps, samples_in=n_in, samples_out=n_out, table_KB=table.taps.size * 4 / 1024,
                   kernel_us=kern, kernel_us_median=k, flop=flop, kernel_TFLOPs=flop / k / 1e6, share_of_vector_peak=flop / k / 1e6 / (PEAK / 1e12),
                   bytes_read_plus_written=8 * half, d2d_copy_same_bytes_us=copy, d2d_copy_us_median=c, torch_conv1d_us=conv, torch_conv1d_us_median=t,
                   torch_conv1d_taps_per_channel=int(wt.shape[2]), max_abs_diff_vs_torch_conv1d=diff)
        res["rates"].append(row)
        print(json.dumps({a: row[a] for a in ("source_rate", "kernel_us_median", "d2d_copy_us_median", "torch_conv1d_us_median", "kernel_TFLOPs",
                                              "max_abs_diff_vs_torch_conv1d")}), flush=True)
        del wav, out, src, dst, xp, wt
    res["timing"] = ("every utterance at the one source rate; HIP events around 20 back-to-back calls after 3 warm-up calls, 3 rounds alternating the "
                     "contenders in one process; FLOP = 2 B n_out ntaps; peak = 157.3 TFLOP/s fp32 vector")
    # StreamResampler.push: host time of one 480 ms block at 48 kHz
    res["stream_push"] = {}
    for Bs in (1, 32):
        sr = R.StreamResampler(Bs, 48000, "cuda")
        blk = torch.randn(Bs, 23040, device="cuda") * 0.1
        host, wall = [], []
        for i in range(40):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sr.push(blk, [23040] * Bs, [False] * Bs)
            t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
            host.append((t1 - t0) * 1e3); wall.append((t2 - t0) * 1e3)
        res["stream_push"][f"B={Bs}"] = dict(block_samples=23040, block_ms=480, host_ms_median=float(np.median(host[5:])), with_sync_ms_median=float(np.median(wall[5:])))
    print(json.dumps(res["stream_push"]), flush=True)
    # the waveform-fed joint step: the 16 kHz corpus with resample off (the code path of before) and on (nothing launched), and a corpus of
    # as many 5-s utterances stored at 48 kHz
    nb = 10
    sub = items[:B * nb]
    r48 = np.random.RandomState(1)
    items48 = [((r48.randn(5 * 48000) * 0.1).astype(np.float32), t, 48000) for _, t in sub]
    mk = lambda it, **kw: BucketedWaveLoader(WaveDataset(it, vocab, resample=bool(kw.get("resample"))), B, parser=parser, augment=True, shuffle=True, seed=1,
                                             dtype=torch.bfloat16, **kw)
    loaders = {"16k_off": mk(sub), "16k_on": mk(sub, resample=True), "48k_on": mk(items48, resample=True)}
    assert loaders["16k_on"].rate_table is None and loaders["48k_on"].rate_table is not None

    def run(ld):
        n = 0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for pack in ld:
            model.iterate(pack, optimizer=opt)
            n += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for ld in loaders.values(): run(ld)                                           # warm-up epoch each
    step = {name: [] for name in loaders}
    for _ in range(4):
        for name, ld in loaders.items():
            step[name].append(run(ld))
            print(f"joint step from waveforms, {name}: {step[name][-1]:.3f} ms/step", flush=True)
    res["joint_step_ms"] = step
    res["joint_step_ms_median"] = {name: float(np.median(v)) for name, v in step.items()}
    res["joint_config"] = (f"{nb} batches of {B} x 5 s per epoch in host memory, SpecAugment on, bf16 joint model at the default width; 16k_off = resample=False "
                           "(the loader of before), 16k_on = resample=True on the same 16 kHz corpus (no launch), 48k_on = as many 5-s utterances stored at "
                           "48 kHz; 1 warm-up epoch each, then 4 epochs each, alternating; host clock around an epoch that ends in a device synchronise")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def fbank_bench():
    import json
    from asr_chinese_e2e_amd import kernels as K
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), "profiles/fbank_bench.json")
    B, S, n_mels = 32, 16000 * 5, 80
    wav = torch.from_numpy((np.random.RandomState(0).randn(B, S) * 0.1).astype(np.float32)).cuda()
    wl = torch.full((B,), S, dtype=torch.int32, device="cuda")
    ref, kal = AudioParser(n_mels=n_mels, lfr_m=1, lfr_n=1, device="cuda"), AudioParser(n_mels=n_mels, lfr_m=1, lfr_n=1, device="cuda", frontend="kaldi")
    T_ref, T_kal = ref.max_frames(S), kal.max_frames(S)
    f_ref, f_kal = torch.empty(B, T_ref, n_mels, device="cuda"), torch.empty(B, T_kal, n_mels, device="cuda")
    half = (B * S + B * T_kal * n_mels) // 2                                      # a copy of `half` floats reads and writes the fbank kernel's bytes in all
    src, dst = torch.randn(half, device="cuda"), torch.empty(half, device="cuda")
    win64, fb64 = kal.window.double(), kal.melfb.double()

    def stand_in(dtype=torch.float32):
        w, fb = (win64, fb64) if dtype == torch.float64 else (kal.window, kal.melfb)
        x = (wav.to(dtype) * 32768.0).unfold(1, 400, 160)                         # (B, T, 400) frames, snip_edges
        x = x - x.mean(dim=2, keepdim=True)
        x = (x - 0.97 * torch.cat([x[:, :, :1], x[:, :, :-1]], dim=2)) * w
        p = torch.fft.rfft(x, n=512, dim=2)[:, :, :256].abs() ** 2
        return torch.log(torch.clamp(p @ fb, min=2.0 ** -23))

    def timed(fn, reps=20, warm=3):
        for _ in range(warm): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    contenders = dict(fbank_kernel=lambda: kal.features(wav, wl, T_kal, feat=f_kal), logmel_kernel=lambda: ref.features(wav, wl, T_ref, feat=f_ref),
                      d2d_copy_same_bytes=lambda: dst.copy_(src), torch_stand_in=stand_in)
    contenders["fbank_kernel"]()
    diff = float((f_kal.double() - stand_in(torch.float64)).abs().max())           # the two computations agree (log domain)
    us = {name: [] for name in contenders}
    for _ in range(3):                                                            # alternated
        for name, fn in contenders.items():
            us[name].append(timed(fn))
    res = dict(device=torch.cuda.get_device_name(0), B=B, samples=S, n_mels=n_mels, frames_fbank=T_kal, frames_logmel=T_ref,
               bytes_read_plus_written=8 * half, max_abs_log_diff_vs_torch_float64=diff)
    for name, v in us.items():
        res[name + "_us"], res[name + "_us_median"] = v, float(np.median(v))
    res["fbank_over_logmel"] = res["fbank_kernel_us_median"] / res["logmel_kernel_us_median"]
    res["timing"] = ("HIP events around 20 back-to-back calls after 3 warm-up calls, 3 rounds alternating the contenders in one process; torch stand-in = "
                     "unfold, mean removal, pre-emphasis, window, torch.fft.rfft at 512 points, |.|^2, matmul with the banks, clamp, log, in fp32")
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_median") or k in ("fbank_over_logmel", "max_abs_log_diff_vs_torch_float64")}), flush=True)
    from tools import stream_frontend_bench as SB
    res["push_audio"] = {f: SB.run(50, f) for f in ("reference", "kaldi")}
    print(json.dumps({f: {b: r[b]["frontend_ms"] for b in ("B=1", "B=32")} for f, r in res["push_audio"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def spec_augment_bench():
    import json
    from asr_chinese_e2e_amd import kernels as K
    from asr_chinese_e2e_amd.data_handler import specaug
    from asr_chinese_e2e_amd.data_handler.processor import sample_spec_augment
    import random
    out_path = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")), "profiles/spec_augment_bench.json")
    n_mels, m, n = 80, 4, 3
    ref = AudioParser(n_mels=n_mels, lfr_m=m, lfr_n=n, device="cuda")
    wav = torch.from_numpy((np.random.RandomState(0).randn(B, S) * 0.1).astype(np.float32)).cuda()
    wl = torch.full((B,), S, dtype=torch.int32, device="cuda")
    Tmax = ref.max_frames(S)
    Tl = (Tmax + n - 1) // n
    feat = ref.features(wav, wl, Tmax)
    g = np.random.RandomState(1)
    mean, istd = torch.from_numpy((g.randn(n_mels) - 9.0).astype(np.float32)).cuda(), torch.from_numpy(g.uniform(0.2, 0.5, n_mels).astype(np.float32)).cuda()
    r = random.Random(0)
    masks = torch.tensor([sample_spec_augment(n_mels, Tmax, r) for _ in range(B)], dtype=torch.int32).cuda()
    policies = {"wenet": "wenet", "espnet": "espnet", "w5_t2x50_f2x10_s3x30": "w5,t2x50,f2x10,s3x30"}
    ranges = {}
    for name, text in policies.items():
        pol = specaug.SpecAugmentPolicy.from_string(text)
        ranges[name] = (torch.from_numpy(ref.spec_ranges(pol, specaug.draw(0, 0, B, pol), [S] * B, S)).cuda(), (pol.n_t, pol.n_f, pol.n_s))

    def timed(fn, reps=20, warm=3):
        for _ in range(warm): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    bf = torch.bfloat16
    contenders = {
        "global": dict(no_mask=lambda: K.global_norm_lfr(feat, wl, mean, istd, m, n, Tl, bf),
                       reference_mask=lambda: K.global_norm_lfr(feat, wl, mean, istd, m, n, Tl, bf, masks=masks),
                       **{name: (lambda rg=rg, c=c: K.global_norm_specaug_lfr(feat, wl, rg, c, mean, istd, m, n, Tl, bf)) for name, (rg, c) in ranges.items()}),
        "utterance": dict(no_mask=lambda: K.utt_norm_lfr(feat, wl, m, n, Tl, bf),
                          reference_mask=lambda: K.utt_norm_lfr(feat, wl, m, n, Tl, bf, masks=masks),
                          **{name: (lambda rg=rg, c=c: K.utt_norm_specaug_lfr(feat, wl, rg, c, m, n, Tl, bf)) for name, (rg, c) in ranges.items()}),
    }
    res = dict(device=torch.cuda.get_device_name(0), B=B, samples=S, n_mels=n_mels, lfr=[m, n], frames=Tmax, dtype="bf16", policies=policies,
               timing="HIP events around 20 back-to-back calls (output allocation included) after 3 warm-up calls, 3 rounds alternating the contenders in one process")
    for norm, cs in contenders.items():
        us = {name: [] for name in cs}
        for _ in range(3):                                                        # alternated
            for name, fn in cs.items():
                us[name].append(timed(fn))
        res[norm + "_norm_us"] = us
        res[norm + "_norm_us_median"] = {name: float(np.median(v)) for name, v in us.items()}
        print(json.dumps({norm: res[norm + "_norm_us_median"]}), flush=True)
    # host time of preparing a batch: the reference's SpecAugment reads wav_len back for its masks, a policy resolves its rows from host lengths
    mk = lambda **kw: BucketedWaveLoader(ds, B, parser=parser, shuffle=True, seed=1, dtype=torch.bfloat16, **kw)
    loaders = {"off": mk(), "augment_true": mk(augment=True), "wenet": mk(spec_augment="wenet")}
    prep = {name: [] for name in loaders}
    table = specaug.draw(1, 0, len(ds), loaders["wenet"].spec)
    for _ in range(3):
        for name, ld in loaders.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for k in range(20): ld._prepare(list(range(B)), k, spec=table if name == "wenet" else None)
            prep[name].append((time.perf_counter() - t0) / 20 * 1e3)
            torch.cuda.synchronize()
    res["prepare_host_ms"] = prep
    res["prepare_host_ms_median"] = {name: float(np.median(v)) for name, v in prep.items()}
    print(json.dumps({"prepare_host_ms_median": res["prepare_host_ms_median"]}), flush=True)

    def run(ld):
        k = 0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for pack in ld:
            model.iterate(pack, optimizer=opt)
            k += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3
    for ld in loaders.values(): run(ld)                                           # warm-up epoch each
    step = {name: [] for name in loaders}
    for _ in range(3):
        for name, ld in loaders.items():
            step[name].append(run(ld))
            print(f"joint step from waveforms, {name}: {step[name][-1]:.3f} ms/step", flush=True)
    res["joint_step_ms"] = step
    res["joint_step_ms_median"] = {name: float(np.median(v)) for name, v in step.items()}
    res["joint_config"] = (f"{NB} batches of {B} x 5 s per epoch in host memory, 80 bins, LFR 1/1 (the model of this tool), bf16 joint model at the default width; "
                           "off = no SpecAugment, augment_true = the reference's, wenet = spec_augment='wenet'; prepare_host_ms = host clock around 20 _prepare "
                           "calls; joint step = 1 warm-up epoch each, then 3 epochs each, alternating; host clock around an epoch that ends in a device synchronise")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if SPEED is not None:
    speed_bench()
    sys.exit(0)
if SPEC_AUGMENT:
    spec_augment_bench()
    sys.exit(0)
if RESAMPLE:
    resample_bench()
    sys.exit(0)
if REVERB_FFT:
    reverb_fft_bench()
    sys.exit(0)
if NOISE_REVERB:
    noise_reverb_bench()
    sys.exit(0)
if FBANK:
    fbank_bench()
    sys.exit(0)


def epoch():
    n = 0
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for pack in loader:
        model.iterate(pack, optimizer=opt)
        n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, pack
epoch()
for _ in range(3):
    ms, pack = epoch()
    print(f"from waveforms ({NB} batches of {B} x 5 s, SpecAugment on): {ms:.3f} ms/step", flush=True)
# host cost of preparing a batch alone
idx = list(range(B))
torch.cuda.synchronize(); t0 = time.perf_counter()
for _k in range(20): loader._prepare(idx, _k)
t1 = time.perf_counter(); torch.cuda.synchronize()
print(f"_prepare alone: {(t1 - t0) / 20 * 1e3:.3f} ms of host time per batch")
for _ in range(10): model.iterate(pack, optimizer=opt)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(100): model.iterate(pack, optimizer=opt)
torch.cuda.synchronize()
print(f"one resident batch: {(time.perf_counter() - t0) / 100 * 1e3:.3f} ms/step")
