// Kaldi-compatible fbank front end on device (compute-fbank-feats / torchaudio.compliance.kaldi.fbank / kaldi-native-fbank with
// WeNet's defaults, dither 0): snip_edges framing (frame t = samples 160 t .. 160 t + 399, no padding), input scale, DC removal,
// pre-emphasis, Povey window, 512-point power spectrum (bins 0 .. 255), mel filterbank, log(max(., FLT_EPSILON)).
// The float64 definition is tests/fbank_ref.py; logmel.hip (the reference's own log-mel) is a separate front end.
#include "asr_common.h"

#include <cfloat>

namespace {

constexpr int FLEN = 400, HOP = 160, NFFT = 512, NBIN = NFFT / 2;      // frame length, shift, padded transform, bins used (no Nyquist)

// The tile plan of logmel_tile: one workgroup = 32 consecutive frames of one utterance; the DFT is a GEMM on the fp32 matrix pipe,
//   C[32 frames][512] = X[32][400] (prepared frames, LDS)  x  D[400][512],
//   D[n][c] = cos(2 pi n c / 512) for c < 256,  -sin(2 pi n (c - 256) / 512) for c >= 256   (taps 400 .. 511 are the zero padding),
// D never stored: the lane that owns column c rotates cos / sin of its angle by 2 theta per step, 200 steps from exact start
// values.  The 512 columns are exactly 16 column tiles, four per wave (waves 0, 1: cosines, waves 2, 3: sines).  Then
// power[32][256] x melfb[256][n_mels] on the matrix pipe, floor, log, store.
constexpr int FR = 32;            // frames per workgroup
constexpr int RS = NFFT + 1;      // LDS row stride of the frame tile and of C (odd: rows hit distinct banks)

// 32 frames t0 .. t0 + 31 of one utterance of Tb frames.  fetch(idx) is the sample at absolute index idx (how the samples are stored is
// the caller's business; only indices 160 t .. 160 t + 399 of frames t < Tb are asked for); row(frame) is where frame t0 + frame goes,
// or nullptr for a row that is not written.
// A frame's bits depend on its own 400 samples only.  Preparation: one wave prepares a frame at a time, lane l holding taps
// l, l + 64, .. l + 384 (< 400); the mean is the lane's sum in that order, then a xor butterfly over the 64 lanes (32, 16, .. 1) - a
// fixed tree over the tap index, the same in every lane; contraction is off so that the tree is what is written.  After that every
// MFMA accumulator row is the sum over its own A row and the recurrence runs along the columns, as in logmel_tile.
template <typename Fetch, typename Row>
__device__ __forceinline__ void fbank_tile(Fetch fetch, Row row, const float* __restrict__ window, const float* __restrict__ melfb, int Tb, int t0, int n_mels,
                                           float wav_scale, float preemph) {
    __shared__ float buf[FR * RS];            // frames (32 x 400 of 513), later C (32 x 512 of 513)
    __shared__ float tw_c[NFFT], tw_s[NFFT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    {
#pragma clang fp contract(off)
        constexpr int NT = (FLEN + 63) / 64;           // 7 taps per lane, the last for lanes 0 .. 15 only
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
    for (int n = tid; n < NFFT; n += 256) {            // exact cos / sin(2 pi n / 512): start values and rotation steps
        float sv, cv;
        sincospif(2.f * (float)n / (float)NFFT, &sv, &cv);
        tw_c[n] = cv;
        tw_s[n] = sv;
    }
    __syncthreads();
    // ---- DFT: wave w owns the four column tiles 4w .. 4w+3; the lane that owns column c rotates its twiddle by 2 theta per step
    const int r = lane & 31, kh = lane >> 5;
    const bool is_im = w >= 2;                         // columns 256 .. 511
    f32x16 acc[4];
    float tc[4], ts[4], rc[4], rs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
        const int bin = ((4 * w + q) * 32 + r) & (NBIN - 1);
        const int j2 = (2 * bin) & (NFFT - 1), j0 = (kh * bin) & (NFFT - 1);
        rc[q] = tw_c[j2];                              // rotation by 2 theta
        rs[q] = tw_s[j2];
        tc[q] = tw_c[j0];                              // k = kh
        ts[q] = tw_s[j0];
    }
    const float* xrow = buf + r * RS + kh;
#pragma unroll 4
    for (int kk = 0; kk < FLEN / 2; ++kk) {
        const float a = xrow[2 * kk];                  // X[frame r][k = 2 kk + kh]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float d = is_im ? -ts[q] : tc[q];
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, d, acc[q], 0, 0, 0);   // A rows = frames, B cols = DFT columns
            const float nc = fmaf(tc[q], rc[q], -ts[q] * rs[q]);
            ts[q] = fmaf(ts[q], rc[q], tc[q] * rs[q]);
            tc[q] = nc;
        }
    }
    __syncthreads();                                   // everyone is done with the frames: the buffer becomes C
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = (4 * w + q) * 32 + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int frame = (i & 3) + 8 * (i >> 2) + 4 * kh;        // accumulator row
            buf[frame * RS + c] = acc[q][i];
        }
    }
    __syncthreads();
    // ---- mel: out[32][n_mels] = power[32][256] x melfb[256][n_mels]; wave w owns mel columns 32 w .. 32 w + 31
    for (int mt = w; mt * 32 < n_mels; mt += 4) {
        const int m = mt * 32 + r;
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
        const float* crow = buf + r * RS;
        // the filterbank column of this lane is fetched a quarter at a time into registers BEFORE the MFMAs that use it
        constexpr int KSTEPS = NBIN / 2, CHUNK = 32;           // 128 steps in 4 chunks
#pragma unroll 1
        for (int k0 = 0; k0 < KSTEPS; k0 += CHUNK) {
            float mbv[CHUNK];
#pragma unroll
            for (int i = 0; i < CHUNK; ++i) {
                const int k = 2 * (k0 + i) + kh;
                mbv[i] = m < n_mels ? melfb[(size_t)k * n_mels + m] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < CHUNK; ++i) {
                const int k = 2 * (k0 + i) + kh;
                const float re = crow[k], im = crow[NBIN + k];
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(re * re + im * im, mbv[i], o, 0, 0, 0);
            }
        }
        if (m < n_mels) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int frame = (i & 3) + 8 * (i >> 2) + 4 * kh;
                float* dst = row(frame);
                if (dst) dst[m] = (t0 + frame < Tb) ? logf(fmaxf(o[i], FLT_EPSILON)) : 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void fbank_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const float* __restrict__ window,
                                                    const float* __restrict__ melfb, float* __restrict__ feat, int Smax, int Tmax, int n_mels, float wav_scale,
                                                    float preemph) {
    const int t0 = blockIdx.x * FR, b = blockIdx.y, tid = threadIdx.x;
    const int len = min(max(wav_len[b], 0), Smax);     // a length past the row would read the next row (or past the tensor)
    const int Tb = len >= FLEN ? min(1 + (len - FLEN) / HOP, Tmax) : 0;
    float* out = feat + ((size_t)b * Tmax + t0) * n_mels;
    const int rows_here = min(FR, Tmax - t0);
    if (t0 >= Tb) {                            // nothing but padding: zeros
        for (int i = tid; i < rows_here * n_mels; i += 256) out[i] = 0.f;
        return;
    }
    const float* wv = wav + (size_t)b * Smax;
    fbank_tile([=](int idx) { return wv[idx]; }, [=](int frame) { return frame < rows_here ? out + (size_t)frame * n_mels : nullptr; }, window, melfb, Tb, t0,
               n_mels, wav_scale, preemph);
}

// Streaming: frames [t_begin, t_begin + n_new) of each utterance from a ring of its most recent samples into a ring of its most
// recent frames.  par[b] = {t_begin, n_new}.  No length: frame t touches samples 160 t .. 160 t + 399 and nothing else, and the host asks
// for a frame only once they have arrived.
__global__ __launch_bounds__(256, 2) void stream_fbank_kernel(const float* __restrict__ wav_ring, const int32_t* __restrict__ par, const float* __restrict__ window,
                                                           const float* __restrict__ melfb, float* __restrict__ feat_ring, int scap, int fcap, int n_mels,
                                                           float wav_scale, float preemph) {
    const int b = blockIdx.y;
    const int t_begin = par[2 * b], n_new = par[2 * b + 1];
    const int f0 = blockIdx.x * FR;
    if (f0 >= n_new) return;
    const int t0 = t_begin + f0;
    const float* wv = wav_ring + (size_t)b * scap;
    float* fr = feat_ring + (size_t)b * fcap * n_mels;
    const int smask = scap - 1, fmask = fcap - 1, rows_here = n_new - f0;
    fbank_tile([=](int idx) { return wv[idx & smask]; }, [=](int frame) { return frame < rows_here ? fr + (size_t)((t0 + frame) & fmask) * n_mels : nullptr; },
               window, melfb, t_begin + n_new, t0, n_mels, wav_scale, preemph);
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

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
    if (!wav_ring || !par || !window || !melfb || !feat_ring) ASR_FAIL(ASR_EINVAL, "asr_stream_fbank: null pointer");
    if (B <= 0 || B > 65535 || max_new <= 0 || n_mels <= 0 || !pow2(scap) || scap < 1024 || !pow2(fcap) || max_new > fcap)
        ASR_FAIL(ASR_EINVAL, "asr_stream_fbank: bad shape B=%d max_new=%d scap=%d fcap=%d n_mels=%d (scap >= 1024 and fcap powers of two, max_new <= fcap)", B,
                 max_new, scap, fcap, n_mels);
    dim3 grid(ceil_div(max_new, FR), B);
    stream_fbank_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav_ring, par, window, melfb, feat_ring, scap, fcap, n_mels, wav_scale, preemph);
    ASR_CHECK_LAUNCH("asr_stream_fbank");
    return ASR_OK;
}
