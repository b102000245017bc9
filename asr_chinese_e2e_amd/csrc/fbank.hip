// Kaldi-compatible fbank front end on device (compute-fbank-feats / torchaudio.compliance.kaldi.fbank / kaldi-native-fbank with
// WeNet's defaults, dither 0): snip_edges framing (frame t = samples 160 t .. 160 t + 399, no padding), input scale, DC removal,
// pre-emphasis, Povey window, 512-point power spectrum (bins 0 .. 255), mel filterbank, log(max(., FLT_EPSILON)).
// The float64 definition is tests/fbank_ref.py; logmel.hip (the reference's own log-mel) is a separate front end.  The two share the
// frame tile of dft_mel_tile.h; what is here is the frame preparation, the floor and the entry points.
#include "dft_mel_tile.h"

#include <cfloat>

namespace {

using dmt::FLEN;
using dmt::FR;
constexpr int HOP = 160;          // frame shift
// The tile: the padded transform and its bins (no Nyquist) - 512 DFT columns are exactly 16 column tiles; frame rows and C rows both at the
// odd stride 513; 128 filterbank steps in 4 chunks.
struct Plan {
    static constexpr int NFFT = 512, NBIN = NFFT / 2, XS = NFFT + 1, CHUNK = 32;
};

// The 32 prepared rows of the tile at t0: fetch(idx) is the sample at absolute index idx (only indices 160 t .. 160 t + 399 of frames
// t < Tb are asked for).  A frame's bits depend on its own 400 samples only: one wave prepares a frame at a time, lane l holding taps
// l, l + 64, .. l + 384 (< 400); the mean is the lane's sum in that order, then a xor butterfly over the 64 lanes (32, 16, .. 1) - a
// fixed tree over the tap index, the same in every lane; contraction is off so that the tree is what is written.
struct PoveyFrames {
    const float* __restrict__ window;
    int Tb;
    float wav_scale, preemph;
    template <typename Fetch>
    __device__ __forceinline__ void operator()(float* buf, int t0, Fetch fetch) const {
#pragma clang fp contract(off)
        constexpr int RS = Plan::XS, NT = (FLEN + 63) / 64;      // 7 taps per lane, the last for lanes 0 .. 15 only
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        float win[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) win[j] = lane + 64 * j < FLEN ? window[lane + 64 * j] : 0.f;
        for (int f = w; f < FR; f += 4) {
            float* xr = buf + f * RS;
            if (t0 + f >= Tb) {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (lane + 64 * j < FLEN) xr[lane + 64 * j] = 0.f;
                continue;
            }
            const int base = (t0 + f) * HOP;
            float x[NT], p[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = lane + 64 * j;
                x[j] = n < FLEN ? fetch(base + n) * wav_scale : 0.f;
                p[j] = n < FLEN ? fetch(base + (n > 0 ? n - 1 : 0)) * wav_scale : 0.f;      // tap 0 is its own predecessor (Kaldi)
            }
            float s = x[0];
#pragma unroll
            for (int j = 1; j < NT; ++j) s = s + x[j];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m, 64);
            const float mean = s / (float)FLEN;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = lane + 64 * j;
                const float d = x[j] - mean, dp = p[j] - mean;
                const float y = d - preemph * dp;
                if (n < FLEN) xr[n] = y * win[j];
            }
        }
    }
};

struct EpsilonFloorLog {
    __device__ __forceinline__ float operator()(float x) const { return logf(fmaxf(x, FLT_EPSILON)); }
};

__global__ __launch_bounds__(256, 2) void fbank_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const float* __restrict__ window,
                                                    const float* __restrict__ melfb, float* __restrict__ feat, int Smax, int Tmax, int n_mels, float wav_scale,
                                                    float preemph) {
    const int len = min(max(wav_len[blockIdx.y], 0), Smax);     // a length past the row would read the next row (or past the tensor)
    const int Tb = len >= FLEN ? min(1 + (len - FLEN) / HOP, Tmax) : 0;
    dmt::offline<Plan>(PoveyFrames{window, Tb, wav_scale, preemph}, EpsilonFloorLog{}, wav, melfb, feat, Smax, Tb, Tmax, n_mels);
}

// Streaming (dmt::streamed): par[b] = {t_begin, n_new}.  No length: frame t touches samples 160 t .. 160 t + 399 and nothing else, and
// the host asks for a frame only once they have arrived.
__global__ __launch_bounds__(256, 2) void stream_fbank_kernel(const float* __restrict__ wav_ring, const int32_t* __restrict__ par, const float* __restrict__ window,
                                                           const float* __restrict__ melfb, float* __restrict__ feat_ring, int scap, int fcap, int n_mels,
                                                           float wav_scale, float preemph) {
    const int t_begin = par[2 * blockIdx.y], n_new = par[2 * blockIdx.y + 1];
    dmt::streamed<Plan>(PoveyFrames{window, t_begin + n_new, wav_scale, preemph}, EpsilonFloorLog{}, wav_ring, melfb, feat_ring, t_begin, n_new,
                              t_begin + n_new, scap, fcap, n_mels);
}

}  // namespace

extern "C" int asr_fbank_fwd(const float* wav, const int32_t* wav_len, const float* window, const float* melfb, float* feat, int B, int Smax, int Tmax,
                             int n_mels, float wav_scale, float preemph, void* stream) {
    if (!wav || !wav_len || !window || !melfb || !feat) ASR_FAIL(ASR_EINVAL, "asr_fbank_fwd: null pointer");
    if (B <= 0 || Smax <= 0 || Tmax <= 0 || n_mels <= 0 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_fbank_fwd: bad shape B=%d Smax=%d Tmax=%d n_mels=%d", B, Smax, Tmax, n_mels);
    dim3 grid(ceil_div(Tmax, FR), B);
    fbank_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav, wav_len, window, melfb, feat, Smax, Tmax, n_mels, wav_scale, preemph);
    ASR_CHECK_LAUNCH("asr_fbank_fwd");
    return ASR_OK;
}

extern "C" int asr_stream_fbank(const float* wav_ring, const int32_t* par, const float* window, const float* melfb, float* feat_ring, int B, int max_new, int scap,
                                int fcap, int n_mels, float wav_scale, float preemph, void* stream) {
    dim3 grid;
    if (const int rc = dmt::stream_check("asr_stream_fbank", wav_ring, par, window, melfb, feat_ring, B, max_new, scap, fcap, n_mels, &grid)) return rc;
    stream_fbank_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav_ring, par, window, melfb, feat_ring, scap, fcap, n_mels, wav_scale, preemph);
    ASR_CHECK_LAUNCH("asr_stream_fbank");
    return ASR_OK;
}
