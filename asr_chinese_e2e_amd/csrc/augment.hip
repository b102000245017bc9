// Reverberation and additive noise for a waveform batch on device, between the speed perturbation and the log-mel kernel
// (the other two waveform-side augmentations of the Kaldi / WeNet / ESPnet recipes).  The reference has no waveform-side
// augmentation: parity unpinned by the reference; the definitions are in include/asr_hip.h and, in float64, in tests/noise_ref.py.
//   reverb:  out[b, n] = sum_{k < L} rir[r][k] x[n + p - k]      (p = the response's peak: the direct path stays where it was)
//   mix:     out[b, n] = x[n] + g v[n],   g = scale sqrt(sum x^2 / sum v^2),   v = the noise clip from its offset, wrapped
#include "asr_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ reverberation
// One workgroup = REVERB_TILE consecutive outputs of one utterance, RUN consecutive outputs per lane in registers.  The taps are
// taken KC at a time; the input span of a chunk, x[n0 + p - k0 - KC + 1 .. n0 + p - k0 + TILE), is staged in LDS (zeros outside
// [0, len)).  A lane walks the taps of the chunk upwards, 8 at a time: the 8 + 7 inputs its 8 outputs see under 8 taps are two
// aligned blocks of 8 LDS words, of which one is new per step (two 16-byte reads feed 64 multiply-adds) and the other is the
// previous step's - the two blocks swap roles from step to step (as compiled: 7 register moves per 128 multiply-adds).  The taps are the same for
// the whole workgroup: they are read from global memory at wave-uniform addresses (scalar loads, one per 8 taps) and enter the
// multiply-adds as scalar operands, which leaves LDS to the samples.  The work is B S L multiply-adds on the vector ALU; on this chip
// the fp32 matrix rate equals the fp32 vector rate, so a matrix form of the FIR has nothing to gain.  Measured (profiles/noise_reverb_bench.json,
// B = 32 x 5 s): 112 / 419 / 817 us at 1024 / 4096 / 8192 taps, 30 - 33 % of the vector peak; an FFT convolution through torch.fft takes 158 us
// at every one of these lengths, so from a few thousand taps on this direct form is the slower one.
constexpr int RTILE = ASR_REVERB_TILE;    // outputs per workgroup
constexpr int RNT = 128;                  // threads
constexpr int RUN = 8;                    // consecutive outputs per lane
constexpr int KC = ASR_REVERB_CHUNK;      // taps per staged chunk
static_assert(RTILE == RNT * RUN, "one run of RUN outputs per lane");
static_assert(KC % 16 == 0 && RUN == 8, "the tap loop takes two steps of 8 taps per iteration");

__device__ __forceinline__ void load8_lds(const float* p, float (&r)[8]) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[i] = a[i]; r[4 + i] = b[i]; }
}

// taps k .. k + 7 of the response at h (wave-uniform), 0 at and beyond L
__device__ __forceinline__ void taps8(const float* __restrict__ h, int k, int L, float (&hv)[8]) {
    if (k + 8 <= L) {
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[e] = h[k + e];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[e] = k + e < L ? h[k + e] : 0.f;
    }
}

// acc[j] += sum_e hv[e] w[j + 7 - e], w = lo (words 0 .. 7) followed by hi (words 8 .. 15, the last one unused)
__device__ __forceinline__ void fir8(float (&acc)[8], const float (&lo)[8], const float (&hi)[8], const float (&hv)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = j + 7 - e;
            acc[j] = fmaf(hv[e], i < 8 ? lo[i] : hi[i - 8], acc[j]);
        }
}

__global__ __launch_bounds__(RNT) void reverb_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ rir_idx,
                                                     const float* __restrict__ rir, const int32_t* __restrict__ rir_len, const int32_t* __restrict__ rir_peak,
                                                     float* __restrict__ out, int Smax, int R, int Lcap, int vec) {
    __shared__ __attribute__((aligned(16))) float xs[RTILE + KC];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n0 = blockIdx.x * RTILE;                  // first output of the tile; n0 < Smax
    const int tcount = min(RTILE, Smax - n0);
    const int len = min(max(wav_len[b], 0), Smax);
    const int tlive = min(tcount, len - n0);            // outputs of this tile below len (<= 0: the tile is padding only)
    const long long row = (long long)b * Smax;
    const int r = rir_idx[b];
    if (r < 0 || r >= R || tlive <= 0) {                // no response drawn (or nothing to filter): copy, zeros from len on; the bank is not read
        const float* src = wav + row + n0;
        float* dst = out + row + n0;
        if (vec && ((row + n0) & 3) == 0) {
            for (int t = 4 * tid; t < tcount; t += 4 * RNT) {
                if (t + 4 <= tlive) {
                    *(f32x4*)(dst + t) = *(const f32x4*)(src + t);
                } else {
                    for (int e = 0; e < 4 && t + e < tcount; ++e) dst[t + e] = t + e < tlive ? src[t + e] : 0.f;
                }
            }
        } else {
            for (int t = tid; t < tcount; t += RNT) dst[t] = t < tlive ? src[t] : 0.f;
        }
        return;
    }
    const int L = min(max(rir_len[r], 1), Lcap);
    const int p = min(max(rir_peak[r], 0), L - 1);
    const float* __restrict__ h = rir + (size_t)r * Lcap;
    float acc[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) acc[j] = 0.f;
    for (int k0 = 0; k0 < L; k0 += KC) {
        // xs[i] = x[g0 + i]; output n0 + t under tap k0 + kk reads xs[t + KC - 1 - kk]
        const int g0 = n0 + p - k0 - KC + 1;
        if (g0 >= len || g0 + RTILE + KC - 1 <= 0) continue;      // the whole span of the chunk lies outside the utterance (workgroup-uniform)
        __syncthreads();                                          // the previous chunk is done with xs
        for (int i = tid; i < RTILE + KC; i += RNT) {
            const int g = g0 + i;
            xs[i] = g >= 0 && g < len ? wav[row + g] : 0.f;
        }
        __syncthreads();
        const int nt = min(KC, L - k0);                           // this utterance's taps, not the bank's width
        const float* xw = xs + RUN * tid + KC;
        float A[8], Bv[8], hv[8];
        load8_lds(xw, A);
        for (int m = 0; m < nt; m += 16) {                        // taps at and beyond L are 0: the second step of the last pair may be idle
            load8_lds(xw - 8 - m, Bv);
            taps8(h, k0 + m, L, hv);
            fir8(acc, Bv, A, hv);
            load8_lds(xw - 16 - m, A);
            taps8(h, k0 + m + 8, L, hv);
            fir8(acc, A, Bv, hv);
        }
    }
    __syncthreads();
    // through LDS so that neighbouring lanes store neighbouring words
#pragma unroll
    for (int j = 0; j < RUN; ++j) xs[RUN * tid + j] = acc[j];
    __syncthreads();
    float* dst = out + row + n0;
    for (int t = tid; t < tcount; t += RNT) dst[t] = t < tlive ? xs[t] : 0.f;
}

// ------------------------------------------------------------------------------------------------ additive noise
// Two launches.  noise_energy_kernel: one workgroup per MIX_TILE samples of one utterance sums x^2 and v^2 in fp64 (lane-strided
// partial sums, then a fixed tree in LDS) into ws[b][tile] - no atomics, so the same input gives the same bits.  noise_mix_kernel:
// every workgroup adds the partials of its utterance in tile order, forms the gain in fp64, rounds it once and writes x + g v.
constexpr int MTILE = ASR_NOISE_MIX_TILE;
constexpr int MNT = 256;

struct NoiseClip {
    const float* v;      // start of the clip, NULL: nothing to mix
    uint32_t nlen, first, step;      // clip length, (o + n0 + tid) mod nlen, MNT mod nlen
    float scale;
};

__device__ __forceinline__ NoiseClip noise_clip(const int32_t* __restrict__ par, const float* __restrict__ noise, const int32_t* __restrict__ noise_off, int b,
                                                int N, int n0, int tid) {
    NoiseClip c;
    c.v = nullptr;
    c.nlen = c.first = c.step = 0;
    c.scale = __int_as_float(par[4 * b + 2]);
    const int j = par[4 * b];
    if (j < 0 || j >= N) return c;
    const int beg = noise_off[j], nlen = noise_off[j + 1] - beg;
    if (nlen <= 0 || beg < 0) return c;
    // exact for o + n up to 2^31 and beyond: 64 bits once per lane, then additions below 2^32
    const long long o = ((long long)par[4 * b + 1] % nlen + nlen) % nlen;
    c.v = noise + beg;
    c.nlen = (uint32_t)nlen;
    c.first = (uint32_t)((o + n0 + tid) % nlen);
    c.step = (uint32_t)(MNT % nlen);
    return c;
}

__global__ __launch_bounds__(MNT) void noise_energy_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ par,
                                                           const float* __restrict__ noise, const int32_t* __restrict__ noise_off, double* __restrict__ ws,
                                                           int Smax, int N) {
    __shared__ double red[2][MNT];
    const int b = blockIdx.y, tid = threadIdx.x, n0 = blockIdx.x * MTILE;
    const int len = min(max(wav_len[b], 0), Smax);
    const int n1 = min(n0 + MTILE, len);
    const NoiseClip c = noise_clip(par, noise, noise_off, b, N, n0, tid);
    double ex = 0.0, ev = 0.0;
    if (c.v) {
        const float* x = wav + (long long)b * Smax;
        uint32_t i = c.first;
        for (int n = n0 + tid; n < n1; n += MNT) {
            const double xv = (double)x[n], vv = (double)c.v[i];
            ex += xv * xv;
            ev += vv * vv;
            i += c.step;
            if (i >= c.nlen) i -= c.nlen;
        }
    }
    red[0][tid] = ex;
    red[1][tid] = ev;
    __syncthreads();
    for (int s = MNT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* w = ws + 2 * ((size_t)b * gridDim.x + blockIdx.x);
        w[0] = red[0][0];
        w[1] = red[1][0];
    }
}

// wav and out may be the same buffer: every sample is read and written by the same lane
__global__ __launch_bounds__(MNT) void noise_mix_kernel(const float* wav, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ par,
                                                        const float* __restrict__ noise, const int32_t* __restrict__ noise_off, float* out,
                                                        float* __restrict__ gain_out, const double* __restrict__ ws, int Smax, int N) {
    const int b = blockIdx.y, tid = threadIdx.x, n0 = blockIdx.x * MTILE;
    const int len = min(max(wav_len[b], 0), Smax);
    const int n1 = min(n0 + MTILE, Smax);
    const NoiseClip c = noise_clip(par, noise, noise_off, b, N, n0, tid);
    double ex = 0.0, ev = 0.0;
    const double* w = ws + 2 * (size_t)b * gridDim.x;
    for (int t = 0; t < (int)gridDim.x; ++t) {      // tile order: the same sum in every workgroup and every run
        ex += w[2 * t];
        ev += w[2 * t + 1];
    }
    const bool mix = c.v && len > 0 && ex > 0.0 && ev > 0.0;
    const float g = mix ? (float)((double)c.scale * sqrt(ex / ev)) : 0.f;
    if (gain_out && blockIdx.x == 0 && tid == 0) gain_out[b] = g;
    const float* x = wav + (long long)b * Smax;
    float* y = out + (long long)b * Smax;
    uint32_t i = c.first;
    for (int n = n0 + tid; n < n1; n += MNT) {
        float o = 0.f;
        if (n < len) {
            o = x[n];
            if (mix) o = fmaf(g, c.v[i], o);
        }
        y[n] = o;
        i += c.step;
        if (mix && i >= c.nlen) i -= c.nlen;
    }
}

}  // namespace

extern "C" int asr_reverb_fwd(const float* wav, const int32_t* wav_len, const int32_t* rir_idx, const float* rir, const int32_t* rir_len,
                              const int32_t* rir_peak, float* out, int B, int Smax, int R, int Lcap, void* stream) {
    if (!wav || !wav_len || !rir_idx || !rir || !rir_len || !rir_peak || !out) ASR_FAIL(ASR_EINVAL, "asr_reverb_fwd: null pointer");
    if (B < 1 || Smax < 1 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_reverb_fwd: bad shape B=%d Smax=%d", B, Smax);
    if (R < 1 || Lcap < 1 || Lcap > ASR_REVERB_MAX_TAPS) ASR_FAIL(ASR_EINVAL, "asr_reverb_fwd: R=%d Lcap=%d (1 .. %d)", R, Lcap, ASR_REVERB_MAX_TAPS);
    if (out == wav) ASR_FAIL(ASR_EINVAL, "asr_reverb_fwd: out must not alias wav");
    dim3 grid(ceil_div(Smax, RTILE), B);
    const int vec = (((uintptr_t)wav | (uintptr_t)out) & 15) == 0;
    reverb_kernel<<<grid, RNT, 0, (hipStream_t)stream>>>(wav, wav_len, rir_idx, rir, rir_len, rir_peak, out, Smax, R, Lcap, vec);
    ASR_CHECK_LAUNCH("asr_reverb_fwd");
    return ASR_OK;
}

extern "C" size_t asr_noise_mix_workspace_bytes(int B, int Smax) {
    if (B < 1 || Smax < 1) return 0;
    return (size_t)B * ceil_div(Smax, MTILE) * 2 * sizeof(double);
}

extern "C" int asr_noise_mix_fwd(const float* wav, const int32_t* wav_len, const int32_t* par, const float* noise, const int32_t* noise_off, float* out,
                                 float* gain_out, void* ws, size_t ws_bytes, int B, int Smax, int N, void* stream) {
    if (!wav || !wav_len || !par || !noise || !noise_off || !out || !ws) ASR_FAIL(ASR_EINVAL, "asr_noise_mix_fwd: null pointer");
    if (B < 1 || Smax < 1 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_noise_mix_fwd: bad shape B=%d Smax=%d", B, Smax);
    if (N < 1) ASR_FAIL(ASR_EINVAL, "asr_noise_mix_fwd: N=%d clips", N);
    const size_t need = asr_noise_mix_workspace_bytes(B, Smax);
    if (ws_bytes < need) ASR_FAIL(ASR_EWORKSPACE, "asr_noise_mix_fwd: workspace %zu < %zu bytes", ws_bytes, need);
    if (((uintptr_t)ws & 7) != 0) ASR_FAIL(ASR_EINVAL, "asr_noise_mix_fwd: workspace not 8-byte aligned");
    dim3 grid(ceil_div(Smax, MTILE), B);
    noise_energy_kernel<<<grid, MNT, 0, (hipStream_t)stream>>>(wav, wav_len, par, noise, noise_off, (double*)ws, Smax, N);
    ASR_CHECK_LAUNCH("asr_noise_mix_fwd (energies)");
    noise_mix_kernel<<<grid, MNT, 0, (hipStream_t)stream>>>(wav, wav_len, par, noise, noise_off, out, gain_out, (const double*)ws, Smax, N);
    ASR_CHECK_LAUNCH("asr_noise_mix_fwd");
    return ASR_OK;
}
