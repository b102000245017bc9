"""Inputs shared by tests/test_vad_cpu.py and tests/test_vad_gpu.py: bursts of uniform noise at amplitude 0.1 in noise at 1e-4, fixed seeds.
The CPU test checks on the float32 restatement of the kernel that no frame of these inputs lies near its threshold and that the
end-to-end recording yields the segments the GPU test counts on, so the seeds are vetted before the GPU sees them."""
import numpy as np

SR = 16000
AMP, FLOOR = 0.1, 1e-4
MARGIN = 1e-6                 # no frame's |E - thr| may be below this


def bursts(n_samples, spans, seed):
    """(n_samples,) float32: uniform noise of amplitude FLOOR, of amplitude AMP inside every [a, b) of spans (samples)."""
    rng = np.random.RandomState(seed)
    x = FLOOR * rng.uniform(-1.0, 1.0, n_samples)
    for a, b in spans:
        x[a:b] = AMP * rng.uniform(-1.0, 1.0, b - a)
    return x.astype(np.float32)


# the decision test: T = 257, 3, 8 and 0 frames - 3 < 2 ctx + 1 for ctx 2 and 5, 8 < 11 for ctx 5
DECIDE_LENS = [41360, 720, 1520, 300]
DECIDE_SPANS = [[(3000, 9000), (15000, 16000), (22000, 38000)], [(0, 300)], [(500, 1100)], []]
DECIDE_SEED = 7
DECIDE_OPTIONS = [dict(), dict(energy_threshold=6.0, energy_mean_scale=0.4, proportion_threshold=0.3)]      # EnergyVad's keywords


def decide_case():
    """-> wav (4, 41360) float32 (zeros behind each recording), lengths."""
    wav = np.zeros((len(DECIDE_LENS), max(DECIDE_LENS)), dtype=np.float32)
    for b, (n, spans) in enumerate(zip(DECIDE_LENS, DECIDE_SPANS)):
        wav[b, :n] = bursts(n, spans, DECIDE_SEED + b)
    return wav, list(DECIDE_LENS)


# the end-to-end test: 12 s, five bursts with pauses of 0.2, 0.3, 0.5 and 1.0 s.  With min_silence_s = 0.25 the 0.2 s pause (18 frames
# without a burst sample) is bridged and the others (28, 48, 98 frames) cut: four runs; the first, 3.2 s plus padding, passes
# max_segment_s = 3.0 and is split at the 0.2 s pause: five segments, batches of 2, 2 and 1.
LONG_SECONDS = 12.0
LONG_BURSTS_S = [(0.5, 2.0), (2.2, 3.7), (4.0, 5.0), (5.5, 7.5), (8.5, 10.5)]
LONG_SEED = 3
LONG_OPTS = dict(min_silence_s=0.25, min_speech_s=0.1, pad_s=0.1, max_segment_s=3.0)
LONG_SEGMENTS = 5


def long_case():
    """-> wav (192000,) float32."""
    return bursts(int(LONG_SECONDS * SR), [(int(a * SR), int(b * SR)) for a, b in LONG_BURSTS_S], LONG_SEED)
