// Energy voice-activity detection over waveforms (Kaldi's compute-vad-energy, restated in float64 in tests/vad_ref.py) and the gather
// of the segments it yields into a batch: what model.transcribe_long runs in front of the searches.  Three entry points:
//   asr_vad_energy      raw log-energy of every snip_edges frame (frame t = samples 160 t .. 160 t + 399, scaled by 32768, mean removed)
//   asr_vad_decide      threshold from the recording's mean log-energy in fp64, the context-window vote, the speech mask
//   asr_segment_gather  N stretches of the recordings into a zero-padded (N, Smax) batch, bit for bit
#include "asr_common.h"

#include <cfloat>

namespace {

constexpr int FLEN = 400, HOP = 160;
constexpr float WAV_SCALE = 32768.f;

// ---- energy ------------------------------------------------------------------------------------------------------------------------
// One workgroup = 64 consecutive frames of one recording: their 63 * 160 + 400 = 10480 samples (41 KiB) come into LDS once - every
// sample lies in two or three frames - by 16-byte loads where the row stride allows (the tile starts at sample 160 t0, a multiple of
// four).  A wave takes a frame at a time; lane l reads taps l, l + 64, .. l + 384 (< 400): consecutive words, no bank conflict.
// THE SUMMATION ORDER (tests/vad_ref.py emulate32 restates it): the lane adds its taps in ascending order, the 64 lane sums are added as
// a pairwise tree over the lane index - partners at distance 1, 2, 4, 8, 16, 32 (wave_sum: each level adds two values that are
// themselves sums of the same shape, so the order of the two operands does not matter and every lane holds the same bits).  The mean is
// that sum divided by 400.  Then d = x - mean; the lane's q = d0 * d0, q = fma(d_j, d_j, q) in ascending tap order; the same tree.
// Contraction is off so that nothing but the fma written here is fused.  A frame's bits therefore depend on its own 400 samples only: not
// on the tile, the row of the batch or the recording's length.
constexpr int FR = 64;                                 // frames per workgroup
constexpr int NS = (FR - 1) * HOP + FLEN;              // samples per workgroup

__global__ __launch_bounds__(256) void vad_energy_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, float* __restrict__ E, int S, int Tmax,
                                                         int vec) {
    __shared__ __attribute__((aligned(16))) float smp[NS];
    ASR_FULL_WAVES(256);
    const int t0 = blockIdx.x * FR, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int len = min(max(wav_len[b], 0), S);        // a length past the row would read the next row (or past the tensor)
    const int Tb = len >= FLEN ? min(1 + (len - FLEN) / HOP, Tmax) : 0;
    float* out = E + (size_t)b * Tmax + t0;
    const int rows_here = min(FR, Tmax - t0);
    if (t0 >= Tb) {                                    // nothing but padding: zeros
        for (int i = tid; i < rows_here; i += 256) out[i] = 0.f;
        return;
    }
    const int nf = min(FR, Tb - t0), n = (nf - 1) * HOP + FLEN;      // the last sample touched is 160 (t0 + nf - 1) + 399 < len <= S
    const float* src = wav + (size_t)b * S + (size_t)t0 * HOP;
    if (vec) {
        for (int i = tid; i < n / 4; i += 256) ((f32x4*)smp)[i] = ((const f32x4*)src)[i];      // n is a multiple of 4
    } else {
        for (int i = tid; i < n; i += 256) smp[i] = src[i];
    }
    __syncthreads();
    {
#pragma clang fp contract(off)
        constexpr int NT = (FLEN + 63) / 64;           // 7 taps per lane, the last for lanes 0 .. 15 only
        for (int f = w; f < rows_here; f += 4) {       // wave-uniform: wave_sum needs the whole wave
            if (f >= nf) {
                if (lane == 0) out[f] = 0.f;
                continue;
            }
            const float* xr = smp + f * HOP;
            float x[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) x[j] = lane + 64 * j < FLEN ? xr[lane + 64 * j] * WAV_SCALE : 0.f;
            float s = x[0];
#pragma unroll
            for (int j = 1; j < NT; ++j) s = s + x[j];
            const float mean = wave_sum(s) / (float)FLEN;
            float d[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) d[j] = lane + 64 * j < FLEN ? x[j] - mean : 0.f;
            float q = d[0] * d[0];
#pragma unroll
            for (int j = 1; j < NT; ++j) q = fmaf(d[j], d[j], q);
            q = wave_sum(q);
            if (lane == 0) out[f] = logf(fmaxf(q, FLT_EPSILON));
        }
    }
}

// ---- decision ----------------------------------------------------------------------------------------------------------------------
// The sum of a recording's log-energies in fp64, without atomics: workgroup j of the first launch adds frames 1024 j .. 1024 j + 1023 -
// thread i its frames i, i + 256, i + 512, i + 768 in that order, then the 256 values as a tree (i += i + 128, 64, .. 1) - into
// ws[b][j]; every workgroup of the second launch adds the partials the same way (thread i: partials i, i + 256, .. in that order, the
// same tree).  One order whatever the grid: the threshold is bit-reproducible.
constexpr int CH = 1024;                               // frames per partial
constexpr int CTX_MAX = ASR_VAD_CTX_MAX;

__device__ __forceinline__ double tree_sum_256(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ int vad_frames(int len, int Tmax) { return len >= FLEN ? min(1 + (len - FLEN) / HOP, Tmax) : 0; }

__global__ __launch_bounds__(256) void vad_partial_kernel(const float* __restrict__ E, const int32_t* __restrict__ wav_len, double* __restrict__ ws, int Tmax, int nblk) {
    __shared__ double red[256];
    const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    const int T = vad_frames(wav_len[b], Tmax);
    const float* e = E + (size_t)b * Tmax;
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < CH / 256; ++k) {
        const int t = j * CH + tid + 256 * k;
        v = v + (t < T ? (double)e[t] : 0.0);
    }
    v = tree_sum_256(v, red);
    if (tid == 0) ws[(size_t)b * nblk + j] = v;
}

__global__ __launch_bounds__(256) void vad_decide_kernel(const float* __restrict__ E, const int32_t* __restrict__ wav_len, const double* __restrict__ params,
                                                         const double* __restrict__ ws, uint8_t* __restrict__ speech, double* __restrict__ thr_out, int Tmax,
                                                         int nblk, int ctx) {
    __shared__ double red[256];
    __shared__ uint8_t above[256 + 2 * CTX_MAX];
    const int b = blockIdx.y, tid = threadIdx.x, tb = blockIdx.x * 256;
    const int T = vad_frames(wav_len[b], Tmax);
    double v = 0.0;
    for (int p = tid; p < nblk; p += 256) v = v + ws[(size_t)b * nblk + p];
    const double total = tree_sum_256(v, red);
    const double thr = T > 0 ? params[0] + params[1] * total / (double)T : params[0];      // no frame: no mean term, nothing divided
    if (blockIdx.x == 0 && tid == 0) thr_out[b] = thr;
    const float* e = E + (size_t)b * Tmax;
    for (int i = tid; i < 256 + 2 * ctx; i += 256) {
        const int t2 = tb - ctx + i;
        above[i] = (t2 >= 0 && t2 < T && (double)e[t2] > thr) ? 1 : 0;
    }
    __syncthreads();
    const int t = tb + tid;
    if (t >= Tmax) return;
    uint8_t is_speech = 0;
    if (t < T) {
        int num = 0;
        for (int i = 0; i <= 2 * ctx; ++i) num += above[tid + i];
        const int den = min(t + ctx, T - 1) - max(t - ctx, 0) + 1;
        is_speech = (double)num >= (double)den * params[2] ? 1 : 0;
    }
    speech[(size_t)b * Tmax + t] = is_speech;
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------
// Segment n = samples [start, start + len) of recording rec -> out[n][0 .. len), zeros behind.  The window is clamped to the row
// (start in [0, S), len <= min(Smax, S - start)); rec is the caller's to keep inside the batch (kernels.segment_gather checks it on the
// host).  16-byte pieces when every row base is 16-byte aligned (vec: S and Smax multiples of four, aligned tensors) and start is a
// multiple of four, as the starts of VAD segments (multiples of 160) are.
__global__ __launch_bounds__(256) void segment_gather_kernel(const float* __restrict__ wav, const int32_t* __restrict__ seg_rec, const int32_t* __restrict__ seg_start,
                                                             const int32_t* __restrict__ seg_len, float* __restrict__ out, int S, int Smax, int vec) {
    const int n = blockIdx.y, tid = threadIdx.x;
    const int r = seg_rec[n], st = seg_start[n];
    int ln = seg_len[n];
    const bool ok = r >= 0 && st >= 0 && st < S;
    ln = ok ? max(0, min(ln, min(Smax, S - st))) : 0;
    const float* src = wav + (ok ? (size_t)r * S + st : 0);
    float* dst = out + (size_t)n * Smax;
    const int stride = gridDim.x * 256;
    if (vec && (st & 3) == 0) {
        for (int c4 = blockIdx.x * 256 + tid; c4 < Smax / 4; c4 += stride) {
            const int c = 4 * c4;
            f32x4 x;
            if (c + 4 <= ln) {
                x = *(const f32x4*)(src + c);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = c + k < ln ? src[c + k] : 0.f;
            }
            *(f32x4*)(dst + c) = x;
        }
    } else {
        for (int c = blockIdx.x * 256 + tid; c < Smax; c += stride) dst[c] = c < ln ? src[c] : 0.f;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int asr_vad_energy(const float* wav, const int32_t* wav_len, float* E, int B, int S, int Tmax, void* stream) {
    if (!wav || !wav_len || !E) ASR_FAIL(ASR_EINVAL, "asr_vad_energy: null pointer");
    if (B <= 0 || S <= 0 || Tmax <= 0 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_vad_energy: bad shape B=%d S=%d Tmax=%d", B, S, Tmax);
    const int vec = (S % 4 == 0 && aligned16(wav)) ? 1 : 0;
    dim3 grid(ceil_div(Tmax, FR), B);
    vad_energy_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav, wav_len, E, S, Tmax, vec);
    ASR_CHECK_LAUNCH("asr_vad_energy");
    return ASR_OK;
}

extern "C" size_t asr_vad_decide_workspace_bytes(int B, int Tmax) {
    if (B <= 0 || Tmax <= 0) return 0;
    return (size_t)B * ceil_div(Tmax, CH) * sizeof(double);
}

extern "C" int asr_vad_decide(const float* E, const int32_t* wav_len, const double* params, uint8_t* speech, double* thr_out, void* ws, int B, int Tmax, int ctx,
                              void* stream) {
    if (!E || !wav_len || !params || !speech || !thr_out || !ws) ASR_FAIL(ASR_EINVAL, "asr_vad_decide: null pointer");
    if (B <= 0 || Tmax <= 0 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_vad_decide: bad shape B=%d Tmax=%d", B, Tmax);
    if (ctx < 0 || ctx > CTX_MAX) ASR_FAIL(ASR_EINVAL, "asr_vad_decide: ctx=%d (frames_context must lie in 0 .. %d)", ctx, CTX_MAX);
    if (((uintptr_t)ws & 7) || ((uintptr_t)params & 7) || ((uintptr_t)thr_out & 7)) ASR_FAIL(ASR_EINVAL, "asr_vad_decide: params, thr_out and ws hold doubles: 8-byte alignment");
    const int nblk = ceil_div(Tmax, CH);
    vad_partial_kernel<<<dim3(nblk, B), 256, 0, (hipStream_t)stream>>>(E, wav_len, (double*)ws, Tmax, nblk);
    ASR_CHECK_LAUNCH("asr_vad_decide (partials)");
    vad_decide_kernel<<<dim3(ceil_div(Tmax, 256), B), 256, 0, (hipStream_t)stream>>>(E, wav_len, params, (const double*)ws, speech, thr_out, Tmax, nblk, ctx);
    ASR_CHECK_LAUNCH("asr_vad_decide");
    return ASR_OK;
}

extern "C" int asr_segment_gather(const float* wav, int S, const int32_t* seg_rec, const int32_t* seg_start, const int32_t* seg_len, float* out, int N, int Smax,
                                  void* stream) {
    if (!wav || !seg_rec || !seg_start || !seg_len || !out) ASR_FAIL(ASR_EINVAL, "asr_segment_gather: null pointer");
    if (S <= 0 || N <= 0 || Smax <= 0 || N > 65535) ASR_FAIL(ASR_EINVAL, "asr_segment_gather: bad shape S=%d N=%d Smax=%d", S, N, Smax);
    const int vec = (S % 4 == 0 && Smax % 4 == 0 && aligned16(wav) && aligned16(out)) ? 1 : 0;
    const int per = vec ? 4 * 256 * 4 : 256 * 4;       // about four pieces per thread
    dim3 grid(ceil_div(Smax, per), N);
    segment_gather_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav, seg_rec, seg_start, seg_len, out, S, Smax, vec);
    ASR_CHECK_LAUNCH("asr_segment_gather");
    return ASR_OK;
}
