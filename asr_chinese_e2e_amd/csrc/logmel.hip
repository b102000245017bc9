// Log-mel front end on device: framing (centred, reflect padding) -> Hann window -> 400-point
// real DFT power spectrum -> mel filterbank -> log, then normalisation, SpecAugment and
// low-frame-rate stacking.  Replaces the CPU/torchaudio path of
// Predictor/data_handler/processor.py:33-46, 74-100.  The frame tile (DFT, power, filterbank, log) is dft_mel_tile.h, shared with
// fbank.hip; the normalise-augment-stack kernel, the CMVN statistics and the streaming rings below serve both front ends.
#include "dft_mel_tile.h"

namespace {

using dmt::FR;
constexpr int HOP = 160;          // frame shift
// The tile: a 400-point transform, bins 0 .. 200 - 402 DFT columns (re | im) on 13 column tiles of the 16; frame rows at the odd stride
// 401, C rows at 417; 101 filterbank steps in 4 chunks.
struct Plan {
    static constexpr int NFFT = 400, NBIN = NFFT / 2 + 1, XS = NFFT + 1, CHUNK = 26;
};
static_assert(Plan::NFFT == dmt::FLEN, "the transform is the frame: no zero padding");

// The 32 prepared rows of the tile at t0: centred frames of an utterance of len samples, reflected at both ends, times the Hann window.
// fetch(idx) is the sample at absolute index idx of [0, len).
struct HannFrames {
    const float* __restrict__ window;
    int len, Tb;
    template <typename Fetch>
    __device__ __forceinline__ void operator()(float* buf, int t0, Fetch fetch) const {
        constexpr int NFFT = Plan::NFFT;
        for (int i = threadIdx.x; i < FR * NFFT; i += 256) {
            const int f = i / NFFT, n = i - f * NFFT;
            int idx = (t0 + f) * HOP - NFFT / 2 + n;
            if (idx < 0) idx = -idx;                       // reflect (no edge repeat)
            if (idx >= len) idx = 2 * (len - 1) - idx;
            idx = idx < 0 ? 0 : (idx >= len ? len - 1 : idx);
            buf[f * Plan::XS + n] = (t0 + f < Tb) ? fetch(idx) * window[n] : 0.f;
        }
    }
};

struct TinyFloorLog {
    __device__ __forceinline__ float operator()(float x) const { return logf(x + 1e-20f); }
};

__global__ __launch_bounds__(256, 2) void logmel_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const float* __restrict__ window,
                                                     const float* __restrict__ melfb, float* __restrict__ feat, int Smax, int Tmax, int n_mels) {
    const int len = min(max(wav_len[blockIdx.y], 0), Smax);     // a length past the row would read the next row (or past the tensor)
    const int Tb = len > 0 ? min(1 + len / HOP, Tmax) : 0;
    dmt::offline<Plan>(HannFrames{window, len, Tb}, TinyFloorLog{}, wav, melfb, feat, Smax, Tb, Tmax, n_mels);
}

// Streaming (dmt::streamed): par[b] = {t_begin, n_new, total}: total = the utterance's length in samples once it is closed (the end is
// then reflected and clamped as above, and the last frame is 1 + total / 160 - 1), ASR_STREAM_OPEN while it is open (no frame the
// host asks for touches the end then).
__global__ __launch_bounds__(256, 2) void stream_logmel_kernel(const float* __restrict__ wav_ring, const int32_t* __restrict__ par, const float* __restrict__ window,
                                                            const float* __restrict__ melfb, float* __restrict__ feat_ring, int scap, int fcap, int n_mels) {
    const int b = blockIdx.y;
    const int t_begin = par[3 * b], n_new = par[3 * b + 1], len = par[3 * b + 2];
    const int Tb = 1 + len / HOP;              // closed: the host never asks for a frame of an empty utterance
    dmt::streamed<Plan>(HannFrames{window, len, Tb}, TinyFloorLog{}, wav_ring, melfb, feat_ring, t_begin, n_new, Tb, scap, fcap, n_mels);
}

// ---- global CMVN: corpus statistics ------------------------------------------------------------------------------------------------------------------
// Corpus statistics: per mel bin sum x, sum x^2 over every valid frame (t < Tb), and the frame count, added to float64 accumulators
// acc[0 .. n_mels) | acc[n_mels .. 2 n_mels) | acc[2 n_mels] that persist across launches.  One workgroup = CMVN_ROWS frames of
// one utterance; thread (g, c) sums rows g, g + G, .. of column c in float64 (consecutive threads read consecutive bins), the
// G partial sums of a column meet in LDS, and one float64 vector atomic per column and workgroup reaches memory.
constexpr int CMVN_ROWS = 64, CMVN_MAX_MELS = 256;

__global__ __launch_bounds__(256) void cmvn_stats_kernel(const float* __restrict__ feat, const int32_t* __restrict__ wav_len, double* __restrict__ acc, int Tmax,
                                                         int n_mels) {
    __shared__ double red[2][256];
    const int b = blockIdx.y, t0 = blockIdx.x * CMVN_ROWS, tid = threadIdx.x;
    const int len = wav_len[b];
    const int Tb = len > 0 ? min(1 + len / HOP, Tmax) : 0;
    const int rows = min(CMVN_ROWS, Tb - t0);
    if (rows <= 0) return;
    const int G = 256 / n_mels, g = tid / n_mels, c = tid - g * n_mels;
    double s = 0., q = 0.;
    if (g < G) {
        const float* f = feat + ((size_t)b * Tmax + t0) * n_mels + c;
        for (int r = g; r < rows; r += G) {
            const double x = (double)f[(size_t)r * n_mels];
            s += x;
            q += x * x;
        }
    }
    red[0][tid] = s;
    red[1][tid] = q;
    __syncthreads();
    if (tid < n_mels) {
        for (int k = 1; k < G; ++k) {
            s += red[0][tid + k * n_mels];
            q += red[1][tid + k * n_mels];
        }
        atomicAdd(acc + tid, s);
        atomicAdd(acc + n_mels + tid, q);
    }
    if (tid == 0) atomicAdd(acc + 2 * n_mels, (double)rows);
}

// ---- SpecAugment policies: several masks with zero fill, linear time warp, substitution (the definition: tests/specaug_ref.py) -----
// An utterance's row is [wc, ww | (t0, t1) x n_t | (f0, f1) x n_f | (s, e, p) x n_s], resolved on the host (data_handler/specaug.py).
constexpr int SPEC_MAX = ASR_SPECAUG_MAX_RANGES, SPEC_ROW = 2 + 7 * SPEC_MAX;

// The row of one utterance of T frames and F bins, clamped, into LDS: thread 0 takes the warp, the next n_t + n_f + n_s threads one range
// each.  After it every range lies in [0, T] (or [0, F]), p <= s, and wc = ww = 0 unless 0 < wc < T and 0 < ww < T - whatever the row held.
__device__ __forceinline__ void specaug_load_row(int* row, const int32_t* __restrict__ in, int n_t, int n_f, int n_s, int T, int F) {
    const int k = threadIdx.x;
    if (k == 0) {
        const int wc = in[0], ww = in[1];
        const bool on = wc > 0 && wc < T && ww > 0 && ww < T;
        row[0] = on ? wc : 0;
        row[1] = on ? ww : 0;
    } else if (k <= n_t + n_f) {
        const int at = 2 * k, lim = k <= n_t ? T : F;
        const int lo = min(max(in[at], 0), lim);
        row[at] = lo;
        row[at + 1] = min(max(in[at + 1], lo), lim);
    } else if (k <= n_t + n_f + n_s) {
        const int at = 2 + 2 * (n_t + n_f) + 3 * (k - 1 - n_t - n_f);
        const int s = min(max(in[at], 0), T);
        row[at] = s;
        row[at + 1] = min(max(in[at + 1], s), T);
        row[at + 2] = min(max(in[at + 2], 0), s);
    }
    __syncthreads();
}

// Output cell (frame t, bin f) of an utterance of T frames, pulled through substitution source, masks and warp.  val_t = the normalised
// x[t][f] (what the sibling kernel stores), norm(u) = the normalised x[u][f] for any 0 <= u < T.  The row is wave-uniform LDS, so every
// range test is a broadcast read.  Frame indices: u = t - p lies in [0, t] as p <= s <= t; with the warp on, o < n_out gives
// num < 2 n_out n_in, so i0 <= n_in - 1 and base + i1 <= T - 1 - no index is formed from anything but the clamped row.
template <typename Norm>
__device__ __forceinline__ float specaug_pull(const int* row, int n_t, int n_f, int n_s, int t, int f, int T, float val_t, Norm norm) {
    const int* tm = row + 2;
    const int* fm = tm + 2 * n_t;
    const int* sb = fm + 2 * n_f;
    int u = t;
    for (int i = 0; i < n_s; ++i)                       // the last substitution that covers t wins; it reads augmented frames, never chains
        if (t >= sb[3 * i] && t < sb[3 * i + 1]) u = t - sb[3 * i + 2];
    bool masked = false;
    for (int i = 0; i < n_t; ++i) masked |= u >= tm[2 * i] && u < tm[2 * i + 1];
    for (int i = 0; i < n_f; ++i) masked |= f >= fm[2 * i] && f < fm[2 * i + 1];
    if (masked) return 0.f;
    const int wc = row[0], ww = row[1];
    if (ww == 0) return u == t ? val_t : norm(u);
    // linear warp: output frames [0, ww) resample input frames [0, wc), output frames [ww, T) input frames [wc, T), sample centres aligned
    const bool left = u < ww;
    const int o = left ? u : u - ww, n_out = left ? ww : T - ww, base = left ? 0 : wc, n_in = left ? wc : T - wc;
    const long long num = max((2ll * o + 1) * n_in - n_out, 0ll);
    const unsigned den = 2u * (unsigned)n_out;
    unsigned q, rem;
    if ((num >> 32) == 0) {                             // every utterance of fewer than 32768 frames: one 32-bit division
        q = (unsigned)num / den;
        rem = (unsigned)num - q * den;
    } else {
        q = (unsigned)((unsigned long long)num / den);
        rem = (unsigned)((unsigned long long)num - (unsigned long long)q * den);
    }
    const int i0 = min((int)q, n_in - 1), i1 = min(i0 + 1, n_in - 1);
    const float v0 = norm(base + i0), v1 = norm(base + i1);
    {
        // One division, subtraction, multiplication and addition, each rounded on its own.  The operators are written out under the pragma
        // because that is what keeps them apart: the build contracts a * b + c into an fma wherever both operations allow it, and the
        // header's __fmul_rn / __fadd_rn are plain inline operators that allow it (they came out as one v_fmac_f32 here).  There is no
        // fast-math, so nothing is reassociated, and the division is the correctly rounded one.
        #pragma clang fp contract(off)
        const float w = (float)rem / (float)den;
        const float d = v1 - v0;
        const float wd = w * d;
        return v0 + wd;
    }
}

// ---- normalise, augment, stack -------------------------------------------------------------------------------------------------------
// Element (LFR row r, column c) of an utterance of Tb frames is bin mm of frame src: row r stacks the frames r n .. r n + m - 1, and tail
// rows repeat the last frame.  The one place the rule is written: the offline and the streaming kernel both call it.
__device__ __forceinline__ void lfr_source(int r, int c, int n_mels, int n, int Tb, int* src, int* mm) {
    const int j = c / n_mels;
    *mm = c - j * n_mels;
    *src = min(r * n + j, Tb - 1);
}

// The one place the global normalisation is written: one subtraction and one multiplication in fp32.  With lfr_source it is what makes
// streamed rows equal offline rows bit for bit.
__device__ __forceinline__ float global_norm(float x, int mm, const float* __restrict__ mean, const float* __restrict__ istd) {
    return (x - mean[mm]) * istd[mm];
}

// Normalisation + SpecAugment + LFR of feat (B, Tmax, n_mels) into out (B, Tlfr_max, m n_mels), rows past an utterance's Tl zero.
//   GLOBAL: (x - mean[bin]) * istd[bin]; otherwise the utterance's own scalar mean and unbiased deviation, from two passes over it.
//   POLICY: aug holds a SpecAugment policy row per utterance, ld words apart (specaug_pull); otherwise aug is the reference's masks
//           (B, 4) = [t0, t1, f0, f1], or null for none.
// SpecAugment of the reference (augments.py:4-42 via processor.py:52-58): a time mask [t0, t1) filled with the mean of the normalised
// feature, THEN a mel mask [f0, f1) filled with the mean of the time-masked feature (cloned.mean() at each call).  The ranges come from
// the host's RNG.  A policy fills with zero, the mean under both normalisations, so it reduces nothing.
// Workgroup (x, b) stores elements 1024 x + tid, + 1024 gridDim.x, .. of utterance b.  Whatever reduces over the utterance - its
// statistics, the reference's fill values - needs gridDim.x == 1; the rest is elementwise and the launcher tiles it.
template <typename T, bool GLOBAL, bool POLICY>
__global__ __launch_bounds__(1024) void norm_aug_lfr_kernel(const float* __restrict__ feat, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ aug, int ld,
                                                            int n_t, int n_f, int n_s, const float* __restrict__ mean, const float* __restrict__ istd,
                                                            T* __restrict__ out, int32_t* __restrict__ out_len, int Tmax, int n_mels, int m, int n, int Tlfr_max) {
    __shared__ float red[16];
    __shared__ int row[SPEC_ROW];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int len = wav_len[b];
    const int Tb = len > 0 ? min(1 + len / HOP, Tmax) : 0;
    const int Tl = min((Tb + n - 1) / n, Tlfr_max);
    const float* f = feat + (size_t)b * Tmax * n_mels;
    const int cnt = Tb * n_mels;
    float mean_u = 0.f, rstd_u = 1.f;
    if constexpr (!GLOBAL) {
        float s = 0.f;
        for (int i = tid; i < cnt; i += 1024) s += f[i];
        mean_u = cnt > 0 ? block_sum(s, red) / (float)cnt : 0.f;
        float q = 0.f;
        for (int i = tid; i < cnt; i += 1024) { const float d = f[i] - mean_u; q += d * d; }
        const float var = cnt > 1 ? block_sum(q, red) / (float)(cnt - 1) : 1.f;  // unbiased (torch .std())
        rstd_u = rsqrtf(var);
    }
    const auto norm = [=](float x, int mm) {
        if constexpr (GLOBAL) return global_norm(x, mm, mean, istd);
        else return (x - mean_u) * rstd_u;
    };
    int t0 = 0, t1 = 0, f0 = 0, f1 = 0;
    float fill_t = 0.f, fill_f = 0.f;
    if constexpr (POLICY) {
        specaug_load_row(row, aug + (size_t)b * ld, n_t, n_f, n_s, Tb, n_mels);
    } else if (aug) {
        t0 = min(max(aug[4 * b + 0], 0), Tb);
        t1 = min(max(aug[4 * b + 1], t0), Tb);
        f0 = min(max(aug[4 * b + 2], 0), n_mels);
        f1 = min(max(aug[4 * b + 3], f0), n_mels);
        float sa = 0.f, sm = 0.f;
        for (int i = tid; i < cnt; i += 1024) {
            const int t = i / n_mels, mm = i - t * n_mels;
            const float v = norm(f[i], mm);
            sa += v;
            if (t >= t0 && t < t1) sm += v;
        }
        const float sum_all = block_sum(sa, red), sum_masked = block_sum(sm, red);
        fill_t = cnt > 0 ? sum_all / (float)cnt : 0.f;
        fill_f = cnt > 0 ? (sum_all - sum_masked + (float)((t1 - t0) * n_mels) * fill_t) / (float)cnt : 0.f;
    }
    const int W = m * n_mels;
    T* o = out + (size_t)b * Tlfr_max * W;
    const int total = Tlfr_max * W;
    // the utterance statistics are never tiled: their store loop gets gridDim.x = 1 at compile time
    for (int i = GLOBAL ? blockIdx.x * 1024 + tid : tid; i < total; i += GLOBAL ? gridDim.x * 1024 : 1024) {
        const int r = i / W, c = i - r * W;
        float val = 0.f;
        if (r < Tl) {
            int src, mm;
            lfr_source(r, c, n_mels, n, Tb, &src, &mm);
            val = norm(f[(size_t)src * n_mels + mm], mm);
            if constexpr (POLICY) val = specaug_pull(row, n_t, n_f, n_s, src, mm, Tb, val, [=](int u) { return norm(f[(size_t)u * n_mels + mm], mm); });
            else if (mm >= f0 && mm < f1) val = fill_f;
            else if (src >= t0 && src < t1) val = fill_t;
        }
        o[i] = from_f32<T>(val);
    }
    if (tid == 0 && (!GLOBAL || blockIdx.x == 0)) out_len[b] = Tl;
}

// Streaming: LFR rows [r_begin, r_begin + n_rows) of each utterance out of its frame ring into one encoder chunk (B, C, m n_mels),
// rows past n_rows zero.  par[b] = {r_begin, n_rows, Tb}: Tb = the utterance's frame count once it is closed, ASR_STREAM_OPEN before.
template <typename T>
__global__ __launch_bounds__(256) void stream_norm_lfr_kernel(const float* __restrict__ feat_ring, const int32_t* __restrict__ par, const float* __restrict__ mean,
                                                              const float* __restrict__ istd, T* __restrict__ out, int fcap, int n_mels, int m, int n, int C) {
    const int b = blockIdx.y;
    const int r_begin = par[3 * b], n_rows = par[3 * b + 1], Tb = par[3 * b + 2];
    const float* f = feat_ring + (size_t)b * fcap * n_mels;
    const int fmask = fcap - 1, W = m * n_mels, total = C * W;
    T* o = out + (size_t)b * total;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int r = i / W, c = i - r * W;
        float val = 0.f;
        if (r < n_rows) {
            int src, mm;
            lfr_source(r_begin + r, c, n_mels, n, Tb, &src, &mm);
            val = global_norm(f[(size_t)(src & fmask) * n_mels + mm], mm, mean, istd);
        }
        o[i] = from_f32<T>(val);
    }
}

// Streaming: n_new[b] new samples of pcm (B, S) go behind the received[b] samples each utterance's ring has seen: par[b] = {received, n_new}.
__global__ __launch_bounds__(256) void stream_append_kernel(const float* __restrict__ pcm, const int32_t* __restrict__ par, float* __restrict__ wav_ring, int S,
                                                            int pcm_off, int max_new, int scap) {
    const int b = blockIdx.y;
    const int received = par[2 * b], n_new = min(par[2 * b + 1], max_new);      // never past the row of pcm
    const float* src = pcm + (size_t)b * S + pcm_off;
    float* ring = wav_ring + (size_t)b * scap;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_new; i += gridDim.x * 256) ring[(received + i) & (scap - 1)] = src[i];
}

}  // namespace

extern "C" int asr_logmel_fwd(const float* wav, const int32_t* wav_len, const float* window, const float* melfb, float* feat, int B, int Smax, int Tmax,
                              int n_mels, void* stream) {
    if (!wav || !wav_len || !window || !melfb || !feat) ASR_FAIL(ASR_EINVAL, "asr_logmel_fwd: null pointer");
    if (B <= 0 || Smax <= Plan::NFFT / 2 || Tmax <= 0 || n_mels <= 0 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_logmel_fwd: bad shape B=%d Smax=%d Tmax=%d n_mels=%d", B, Smax, Tmax, n_mels);
    dim3 grid(ceil_div(Tmax, FR), B);
    logmel_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav, wav_len, window, melfb, feat, Smax, Tmax, n_mels);
    ASR_CHECK_LAUNCH("asr_logmel_fwd");
    return ASR_OK;
}

// ---- normalise, augment, stack: the one launcher of norm_aug_lfr_kernel -------------------------------------------------------------------
// aug: the policy rows (POLICY; required) or the reference's masks (may be null).  Geometry: one 1024-thread workgroup per utterance
// wherever it reduces (utterance statistics, reference masks); otherwise 4 elements per thread on up to 256 workgroups per utterance.
template <bool GLOBAL, bool POLICY>
static int norm_aug_lfr_fwd(const char* name, const float* feat, const int32_t* wav_len, const int32_t* aug, int ld, int n_t, int n_f, int n_s, const float* mean,
                            const float* istd, void* out, int32_t* out_len, int B, int Tmax, int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream) {
    if (!feat || !wav_len || !out || !out_len || (GLOBAL && (!mean || !istd))) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if (B <= 0 || B > 65535 || Tmax <= 0 || n_mels <= 0 || m <= 0 || n <= 0 || Tlfr_max <= 0)
        ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d Tmax=%d n_mels=%d m=%d n=%d Tlfr_max=%d", name, B, Tmax, n_mels, m, n, Tlfr_max);
    if ((long long)Tlfr_max * m * n_mels > INT32_MAX) ASR_FAIL(ASR_EINVAL, "%s: Tlfr_max * m * n_mels does not fit an int", name);
    if (POLICY) {
        if (!aug) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
        if (n_t < 0 || n_f < 0 || n_s < 0 || n_t > SPEC_MAX || n_f > SPEC_MAX || n_s > SPEC_MAX)
            ASR_FAIL(ASR_EINVAL, "%s: n_t=%d n_f=%d n_s=%d (each 0 .. %d)", name, n_t, n_f, n_s, SPEC_MAX);
        if (ld < 2 + 2 * n_t + 2 * n_f + 3 * n_s) ASR_FAIL(ASR_EINVAL, "%s: ld=%d, a row has %d words", name, ld, 2 + 2 * n_t + 2 * n_f + 3 * n_s);
    }
    const bool tiled = GLOBAL && (POLICY || !aug);
    const dim3 grid(tiled ? max(1, min(ceil_div(Tlfr_max * m * n_mels, 4096), 256)) : 1, B);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ASR_F32)
        norm_aug_lfr_kernel<float, GLOBAL, POLICY><<<grid, 1024, 0, st>>>(feat, wav_len, aug, ld, n_t, n_f, n_s, mean, istd, (float*)out, out_len, Tmax, n_mels, m, n, Tlfr_max);
    else if (dtype == ASR_BF16)
        norm_aug_lfr_kernel<bf16_t, GLOBAL, POLICY><<<grid, 1024, 0, st>>>(feat, wav_len, aug, ld, n_t, n_f, n_s, mean, istd, (bf16_t*)out, out_len, Tmax, n_mels, m, n, Tlfr_max);
    else ASR_FAIL(ASR_EDTYPE, "%s: dtype %d", name, dtype);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}

extern "C" int asr_utt_norm_augment_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* masks, void* out, int32_t* out_len, int B, int Tmax,
                                            int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream) {
    return norm_aug_lfr_fwd<false, false>("asr_utt_norm_augment_lfr_fwd", feat, wav_len, masks, 0, 0, 0, 0, nullptr, nullptr, out, out_len, B, Tmax, n_mels, m, n,
                                          Tlfr_max, dtype, stream);
}

extern "C" int asr_utt_norm_lfr_fwd(const float* feat, const int32_t* wav_len, void* out, int32_t* out_len, int B, int Tmax, int n_mels, int m, int n,
                                    int Tlfr_max, int dtype, void* stream) {
    return norm_aug_lfr_fwd<false, false>("asr_utt_norm_lfr_fwd", feat, wav_len, nullptr, 0, 0, 0, 0, nullptr, nullptr, out, out_len, B, Tmax, n_mels, m, n, Tlfr_max,
                                          dtype, stream);
}

extern "C" int asr_global_norm_augment_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* masks, const float* mean, const float* istd, void* out,
                                               int32_t* out_len, int B, int Tmax, int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream) {
    return norm_aug_lfr_fwd<true, false>("asr_global_norm_augment_lfr_fwd", feat, wav_len, masks, 0, 0, 0, 0, mean, istd, out, out_len, B, Tmax, n_mels, m, n, Tlfr_max,
                                         dtype, stream);
}

extern "C" int asr_utt_norm_specaug_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* ranges, int ld, int n_t, int n_f, int n_s, void* out,
                                            int32_t* out_len, int B, int Tmax, int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream) {
    return norm_aug_lfr_fwd<false, true>("asr_utt_norm_specaug_lfr_fwd", feat, wav_len, ranges, ld, n_t, n_f, n_s, nullptr, nullptr, out, out_len, B, Tmax, n_mels, m, n,
                                         Tlfr_max, dtype, stream);
}

extern "C" int asr_global_norm_specaug_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* ranges, int ld, int n_t, int n_f, int n_s,
                                               const float* mean, const float* istd, void* out, int32_t* out_len, int B, int Tmax, int n_mels, int m, int n,
                                               int Tlfr_max, int dtype, void* stream) {
    return norm_aug_lfr_fwd<true, true>("asr_global_norm_specaug_lfr_fwd", feat, wav_len, ranges, ld, n_t, n_f, n_s, mean, istd, out, out_len, B, Tmax, n_mels, m, n,
                                        Tlfr_max, dtype, stream);
}

// ---- global CMVN statistics and the streaming front end ------------------------------------------------------------------------------
extern "C" int asr_cmvn_accumulate(const float* feat, const int32_t* wav_len, double* acc, int B, int Tmax, int n_mels, void* stream) {
    if (!feat || !wav_len || !acc) ASR_FAIL(ASR_EINVAL, "asr_cmvn_accumulate: null pointer");
    if (B <= 0 || B > 65535 || Tmax <= 0 || n_mels <= 0 || n_mels > CMVN_MAX_MELS)
        ASR_FAIL(ASR_EINVAL, "asr_cmvn_accumulate: bad shape B=%d Tmax=%d n_mels=%d (n_mels at most %d)", B, Tmax, n_mels, CMVN_MAX_MELS);
    dim3 grid(ceil_div(Tmax, CMVN_ROWS), B);
    cmvn_stats_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(feat, wav_len, acc, Tmax, n_mels);
    ASR_CHECK_LAUNCH("asr_cmvn_accumulate");
    return ASR_OK;
}

extern "C" int asr_stream_append(const float* pcm, const int32_t* par, float* wav_ring, int B, int S, int pcm_off, int max_new, int scap, void* stream) {
    if (!pcm || !par || !wav_ring) ASR_FAIL(ASR_EINVAL, "asr_stream_append: null pointer");
    if (B <= 0 || B > 65535 || S <= 0 || pcm_off < 0 || max_new <= 0 || pcm_off > S - max_new || !pow2(scap) || max_new > scap)
        ASR_FAIL(ASR_EINVAL, "asr_stream_append: bad shape B=%d S=%d pcm_off=%d max_new=%d scap=%d (scap a power of two, pcm_off + max_new <= S, max_new <= scap)",
                 B, S, pcm_off, max_new, scap);
    dim3 grid(min(ceil_div(max_new, 1024), 64), B);
    stream_append_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pcm, par, wav_ring, S, pcm_off, max_new, scap);
    ASR_CHECK_LAUNCH("asr_stream_append");
    return ASR_OK;
}

extern "C" int asr_stream_logmel(const float* wav_ring, const int32_t* par, const float* window, const float* melfb, float* feat_ring, int B, int max_new, int scap,
                                 int fcap, int n_mels, void* stream) {
    dim3 grid;
    if (const int rc = dmt::stream_check("asr_stream_logmel", wav_ring, par, window, melfb, feat_ring, B, max_new, scap, fcap, n_mels, &grid)) return rc;
    stream_logmel_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav_ring, par, window, melfb, feat_ring, scap, fcap, n_mels);
    ASR_CHECK_LAUNCH("asr_stream_logmel");
    return ASR_OK;
}

// Its own launcher: another kernel with another launch shape (256 threads, ring fetch, a chunk instead of an utterance).
extern "C" int asr_stream_norm_lfr(const float* feat_ring, const int32_t* par, const float* mean, const float* istd, void* out, int B, int C, int fcap, int n_mels,
                                   int m, int n, int dtype, void* stream) {
    if (!feat_ring || !par || !mean || !istd || !out) ASR_FAIL(ASR_EINVAL, "asr_stream_norm_lfr: null pointer");
    if (B <= 0 || B > 65535 || C <= 0 || n_mels <= 0 || m <= 0 || n <= 0 || !pow2(fcap) || (long long)C * m * n_mels > INT32_MAX)
        ASR_FAIL(ASR_EINVAL, "asr_stream_norm_lfr: bad shape B=%d C=%d fcap=%d n_mels=%d m=%d n=%d (fcap a power of two)", B, C, fcap, n_mels, m, n);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(max(1, min(ceil_div(C * m * n_mels, 1024), 64)), B);
    if (dtype == ASR_F32) stream_norm_lfr_kernel<float><<<grid, 256, 0, st>>>(feat_ring, par, mean, istd, (float*)out, fcap, n_mels, m, n, C);
    else if (dtype == ASR_BF16) stream_norm_lfr_kernel<bf16_t><<<grid, 256, 0, st>>>(feat_ring, par, mean, istd, (bf16_t*)out, fcap, n_mels, m, n, C);
    else ASR_FAIL(ASR_EDTYPE, "asr_stream_norm_lfr: dtype %d", dtype);
    ASR_CHECK_LAUNCH("asr_stream_norm_lfr");
    return ASR_OK;
}
