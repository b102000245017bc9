// Log-mel front end on device: framing (centred, reflect padding) -> Hann window -> 400-point
// real DFT power spectrum -> mel filterbank -> log, then per-utterance scalar normalisation and
// low-frame-rate stacking.  Replaces the CPU/torchaudio path of
// Predictor/data_handler/processor.py:33-46, 74-100.
#include "asr_common.h"

namespace {

constexpr int NFFT = 400, HOP = 160, NBIN = NFFT / 2 + 1;

// One workgroup = 32 consecutive frames of one utterance; the DFT is a GEMM on the fp32 matrix pipe:
//   C[32 frames][402] = X[32][400] (windowed frames, LDS)  x  D[400][402],
//   D[n][c] = cos(2 pi n c / 400) for c < 201,  -sin(2 pi n (c-201) / 400) for 201 <= c < 402,
// with D never stored: the lane that owns column c keeps cos / sin of its angle in registers and
// rotates them by 2 theta per step: 200 steps of an fp32 recurrence from exact start values, never restarted (its drift is the
// larger part of the error budget that tests/logmel_emul.py states and tests/test_logmel_gpu.py measures; DESIGN.md has the
// table).  v_mfma_f32_32x32x2_f32 is exact fp32 multiply-accumulate, so the rest is the error of the direct sum.  Then power = re^2 + im^2 (from C, kept in LDS) times the mel
// filterbank, again on the matrix pipe, log, store.  (The first version gave one DFT bin to each
// thread and one frame to each workgroup: 80 k scalar MACs per frame through LDS reads, 0.6 ms for
// 32 x 5 s of audio = 17 % of a training step.)
constexpr int FR = 32;            // frames per workgroup
constexpr int XS = 401;           // LDS row stride of the frame tile (odd: rows hit distinct banks)
constexpr int NC = 2 * NBIN;      // 402 DFT output columns (re | im)
constexpr int CS = 417;           // LDS row stride of C (13 column tiles of 32 = 416, +1)
constexpr int CT = 13;            // column tiles

// The tile body shared by the offline and the streaming kernel: 32 frames t0 .. t0 + 31 of one utterance.  fetch(idx) is the sample at
// absolute index idx of [0, len) (how the samples are stored is the caller's business); row(frame) is where frame t0 + frame goes, or
// nullptr for a row that is not written.  A frame's value depends on its own samples only: every MFMA accumulator row is the
// sum over its own A row, and the rotation recurrence runs along the columns - so a frame has the same bits in whichever tile
// and row it is computed, which is what lets streamed frames equal offline ones.
template <typename Fetch, typename Row>
__device__ __forceinline__ void logmel_tile(Fetch fetch, Row row, const float* __restrict__ window, const float* __restrict__ melfb, int len, int Tb, int t0,
                                            int n_mels) {
    __shared__ float buf[FR * CS];            // frames (32 x 401), later C (32 x 417)
    __shared__ float tw_c[NFFT], tw_s[NFFT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < FR * NFFT; i += 256) {
        const int f = i / NFFT, n = i - f * NFFT;
        int idx = (t0 + f) * HOP - NFFT / 2 + n;
        if (idx < 0) idx = -idx;                       // reflect (no edge repeat)
        if (idx >= len) idx = 2 * (len - 1) - idx;
        idx = idx < 0 ? 0 : (idx >= len ? len - 1 : idx);
        buf[f * XS + n] = (t0 + f < Tb) ? fetch(idx) * window[n] : 0.f;
    }
    for (int n = tid; n < NFFT; n += 256) {            // exact cos / sin(2 pi n / 400): start values and rotation steps
        float sv, cv;
        sincospif(2.f * (float)n / (float)NFFT, &sv, &cv);
        tw_c[n] = cv;
        tw_s[n] = sv;
    }
    __syncthreads();
    // ---- DFT: wave w owns the four column tiles 4w .. 4w+3 (16 tiles cover 512 >= 402 columns; the
    // three all-zero ones keep the code branch-free and the four waves equally loaded).  The lane
    // that owns column c needs cos / sin(2 pi k bin / 400) for k = kh, kh+2, ...: a rotation by
    // 2 theta per step in registers (a table in LDS would be read at stride k*bin: up to 32-way bank
    // conflicts).  200 steps of the fp32 recurrence drift by ~2e-5 relative: 1e-5 in the log domain.
    const int r = lane & 31, kh = lane >> 5;
    f32x16 acc[4];
    float tc[4], ts[4], rc[4], rs[4], sgn_c[4], sgn_s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
        const int c = (4 * w + q) * 32 + r;
        const bool live = c < NC, is_im = c >= NBIN;
        const int bin = is_im ? c - NBIN : c;
        sgn_c[q] = live && !is_im ? 1.f : 0.f;         // operand = sgn_c * cos + sgn_s * sin
        sgn_s[q] = live && is_im ? -1.f : 0.f;
        const int j2 = (2 * bin) % NFFT, j0 = (kh * bin) % NFFT;
        rc[q] = tw_c[j2];                              // rotation by 2 theta
        rs[q] = tw_s[j2];
        tc[q] = tw_c[j0];                              // k = kh
        ts[q] = tw_s[j0];
    }
    const float* xrow = buf + r * XS + kh;
#pragma unroll 4
    for (int kk = 0; kk < NFFT / 2; ++kk) {
        const float a = xrow[2 * kk];                  // X[frame r][k = 2 kk + kh]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float d = fmaf(sgn_c[q], tc[q], sgn_s[q] * ts[q]);
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
        if (c >= CT * 32) continue;                    // columns past the C row (all zero anyway)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int frame = (i & 3) + 8 * (i >> 2) + 4 * kh;        // accumulator row
            buf[frame * CS + c] = acc[q][i];
        }
    }
    __syncthreads();
    // ---- mel: out[32][n_mels] = power[32][201] x melfb[201][n_mels]; wave w owns mel columns 32 w .. 32 w + 31
    for (int mt = w; mt * 32 < n_mels; mt += 4) {
        const int m = mt * 32 + r;
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
        const float* crow = buf + r * CS;
        // the filterbank column of this lane is fetched a quarter at a time into registers BEFORE the
        // MFMAs that use it: issued one by one between MFMAs, each L2 round trip would be exposed
        constexpr int KSTEPS = (NBIN + 1) / 2, CHUNK = 26;     // 101 steps in 4 chunks
#pragma unroll 1
        for (int k0 = 0; k0 < KSTEPS; k0 += CHUNK) {
            float mbv[CHUNK];
#pragma unroll
            for (int i = 0; i < CHUNK; ++i) {
                const int k = 2 * (k0 + i) + kh;
                mbv[i] = (k0 + i < KSTEPS && k < NBIN && m < n_mels) ? melfb[(size_t)k * n_mels + m] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < CHUNK; ++i) {
                const int k = 2 * (k0 + i) + kh;
                float pa = 0.f;
                if (k0 + i < KSTEPS && k < NBIN) {
                    const float re = crow[k], im = crow[NBIN + k];
                    pa = re * re + im * im;
                }
                o = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, mbv[i], o, 0, 0, 0);
            }
        }
        if (m < n_mels) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int frame = (i & 3) + 8 * (i >> 2) + 4 * kh;
                float* dst = row(frame);
                if (dst) dst[m] = (t0 + frame < Tb) ? logf(o[i] + 1e-20f) : 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void logmel_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const float* __restrict__ window,
                                                     const float* __restrict__ melfb, float* __restrict__ feat, int Smax, int Tmax, int n_mels) {
    const int t0 = blockIdx.x * FR, b = blockIdx.y, tid = threadIdx.x;
    const int len = min(max(wav_len[b], 0), Smax);     // a length past the row would read the next row (or past the tensor)
    const int Tb = len > 0 ? min(1 + len / HOP, Tmax) : 0;
    float* out = feat + ((size_t)b * Tmax + t0) * n_mels;
    const int rows_here = min(FR, Tmax - t0);
    if (t0 >= Tb) {                            // nothing but padding: zeros
        for (int i = tid; i < rows_here * n_mels; i += 256) out[i] = 0.f;
        return;
    }
    const float* wv = wav + (size_t)b * Smax;
    logmel_tile([=](int idx) { return wv[idx]; }, [=](int frame) { return frame < rows_here ? out + (size_t)frame * n_mels : nullptr; }, window, melfb, len, Tb,
                t0, n_mels);
}

// Streaming: frames [t_begin, t_begin + n_new) of each utterance from a ring of its most recent samples, into a ring of its most
// recent frames.  par[b] = {t_begin, n_new, total}: total = the utterance's length in samples once it is closed (the end is then
// reflected and clamped as above, and the last frame is 1 + total / 160 - 1), ASR_STREAM_OPEN while it is open (no frame the
// host asks for touches the end then).  Sample s lives at wav_ring[b][s & (scap - 1)], frame t at feat_ring[b][t & (fcap - 1)].
__global__ __launch_bounds__(256, 2) void stream_logmel_kernel(const float* __restrict__ wav_ring, const int32_t* __restrict__ par, const float* __restrict__ window,
                                                            const float* __restrict__ melfb, float* __restrict__ feat_ring, int scap, int fcap, int n_mels) {
    const int b = blockIdx.y;
    const int t_begin = par[3 * b], n_new = par[3 * b + 1], len = par[3 * b + 2];
    const int f0 = blockIdx.x * FR;
    if (f0 >= n_new) return;
    const int t0 = t_begin + f0;
    const int Tb = 1 + len / HOP;              // closed: the host never asks for a frame of an empty utterance
    const float* wv = wav_ring + (size_t)b * scap;
    float* fr = feat_ring + (size_t)b * fcap * n_mels;
    const int smask = scap - 1, fmask = fcap - 1, rows_here = n_new - f0;
    logmel_tile([=](int idx) { return wv[idx & smask]; },
                [=](int frame) { return frame < rows_here ? fr + (size_t)((t0 + frame) & fmask) * n_mels : nullptr; }, window, melfb, len, Tb, t0, n_mels);
}

template <typename T>
__global__ __launch_bounds__(1024) void utt_norm_lfr_kernel(const float* __restrict__ feat, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ masks,
                                                            T* __restrict__ out, int32_t* __restrict__ out_len, int Tmax, int n_mels, int m, int n, int Tlfr_max) {
    __shared__ float red[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = wav_len[b];
    const int Tb = len > 0 ? min(1 + len / HOP, Tmax) : 0;
    const int Tl = min((Tb + n - 1) / n, Tlfr_max);
    const float* f = feat + (size_t)b * Tmax * n_mels;
    const int cnt = Tb * n_mels;
    float s = 0.f;
    for (int i = tid; i < cnt; i += 1024) s += f[i];
    const float mean = cnt > 0 ? block_sum(s, red) / (float)cnt : 0.f;
    float q = 0.f;
    for (int i = tid; i < cnt; i += 1024) { const float d = f[i] - mean; q += d * d; }
    const float var = cnt > 1 ? block_sum(q, red) / (float)(cnt - 1) : 1.f;  // unbiased (torch .std())
    const float rstd = rsqrtf(var);
    // SpecAugment of the reference (augments.py:4-42 via processor.py:52-58): a time mask [t0, t1)
    // filled with the mean of the normalised feature, THEN a mel mask [f0, f1) filled with the mean of
    // the time-masked feature (cloned.mean() at each call).  The ranges come from the host's RNG.
    int t0 = 0, t1 = 0, f0 = 0, f1 = 0;
    float fill_t = 0.f, fill_f = 0.f;
    if (masks) {
        t0 = min(max(masks[4 * b + 0], 0), Tb);
        t1 = min(max(masks[4 * b + 1], t0), Tb);
        f0 = min(max(masks[4 * b + 2], 0), n_mels);
        f1 = min(max(masks[4 * b + 3], f0), n_mels);
        float sa = 0.f, sm = 0.f;
        for (int i = tid; i < cnt; i += 1024) {
            const float v = (f[i] - mean) * rstd;
            const int t = i / n_mels;
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
    for (int i = tid; i < total; i += 1024) {
        const int r = i / W, c = i - r * W;
        float val = 0.f;
        if (r < Tl) {
            const int j = c / n_mels, mm = c - j * n_mels;
            const int src = min(r * n + j, Tb - 1);   // tail frames repeat the last input frame
            val = (f[(size_t)src * n_mels + mm] - mean) * rstd;
            if (mm >= f0 && mm < f1) val = fill_f;
            else if (src >= t0 && src < t1) val = fill_t;
        }
        o[i] = from_f32<T>(val);
    }
    if (tid == 0) out_len[b] = Tl;
}

// ---- global CMVN ------------------------------------------------------------------------------------------------------------------
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

// The one place the global normalisation is written: element (LFR row r, column c) of an utterance of Tb frames, frame_at(t) = the
// log-mel row of frame t.  src = min(r n + j, Tb - 1) (tail rows repeat the last frame), then one subtraction and one
// multiplication in fp32.  The offline and the streaming kernel both call it, so their rows agree bit for bit.
template <typename FrameAt>
__device__ __forceinline__ float cmvn_lfr_elem(FrameAt frame_at, int r, int c, int n_mels, int n, int Tb, const float* __restrict__ mean,
                                               const float* __restrict__ istd, int* src_out, int* mm_out) {
    const int j = c / n_mels, mm = c - j * n_mels;
    const int src = min(r * n + j, Tb - 1);
    *src_out = src;
    *mm_out = mm;
    return (frame_at(src)[mm] - mean[mm]) * istd[mm];
}

// Global normalisation + SpecAugment + LFR: utt_norm_lfr_kernel without its two statistics passes.  Without masks it is elementwise
// and the grid's x dimension tiles the output; with masks one workgroup per utterance first reduces the two fill values.
template <typename T>
__global__ __launch_bounds__(1024) void global_norm_lfr_kernel(const float* __restrict__ feat, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ masks,
                                                               const float* __restrict__ mean, const float* __restrict__ istd, T* __restrict__ out,
                                                               int32_t* __restrict__ out_len, int Tmax, int n_mels, int m, int n, int Tlfr_max) {
    __shared__ float red[16];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int len = wav_len[b];
    const int Tb = len > 0 ? min(1 + len / HOP, Tmax) : 0;
    const int Tl = min((Tb + n - 1) / n, Tlfr_max);
    const float* f = feat + (size_t)b * Tmax * n_mels;
    const int cnt = Tb * n_mels;
    int t0 = 0, t1 = 0, f0 = 0, f1 = 0;
    float fill_t = 0.f, fill_f = 0.f;
    if (masks) {                               // the semantics of utt_norm_lfr_kernel's masks (gridDim.x == 1 here)
        t0 = min(max(masks[4 * b + 0], 0), Tb);
        t1 = min(max(masks[4 * b + 1], t0), Tb);
        f0 = min(max(masks[4 * b + 2], 0), n_mels);
        f1 = min(max(masks[4 * b + 3], f0), n_mels);
        float sa = 0.f, sm = 0.f;
        for (int i = tid; i < cnt; i += 1024) {
            const int t = i / n_mels, mm = i - t * n_mels;
            const float v = (f[i] - mean[mm]) * istd[mm];
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
    for (int i = blockIdx.x * 1024 + tid; i < total; i += gridDim.x * 1024) {
        const int r = i / W, c = i - r * W;
        float val = 0.f;
        if (r < Tl) {
            int src, mm;
            val = cmvn_lfr_elem([=](int t) { return f + (size_t)t * n_mels; }, r, c, n_mels, n, Tb, mean, istd, &src, &mm);
            if (mm >= f0 && mm < f1) val = fill_f;
            else if (src >= t0 && src < t1) val = fill_t;
        }
        o[i] = from_f32<T>(val);
    }
    if (tid == 0 && blockIdx.x == 0) out_len[b] = Tl;
}

// ---- SpecAugment policies: several masks with zero fill, linear time warp, substitution (the definition: tests/specaug_ref.py) -----
// An utterance's row is [wc, ww | (t0, t1) x n_t | (f0, f1) x n_f | (s, e, p) x n_s], resolved on the host (data_handler/specaug.py).
// Zero is the mean under both normalisations, so nothing is reduced: the two kernels below are their siblings with another store loop.
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

// utt_norm_lfr_kernel with the policies' store loop: the same two statistics passes over the un-augmented frames.
template <typename T>
__global__ __launch_bounds__(1024) void utt_norm_specaug_lfr_kernel(const float* __restrict__ feat, const int32_t* __restrict__ wav_len,
                                                                    const int32_t* __restrict__ ranges, int ld, int n_t, int n_f, int n_s, T* __restrict__ out,
                                                                    int32_t* __restrict__ out_len, int Tmax, int n_mels, int m, int n, int Tlfr_max) {
    __shared__ float red[16];
    __shared__ int row[SPEC_ROW];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = wav_len[b];
    const int Tb = len > 0 ? min(1 + len / HOP, Tmax) : 0;
    const int Tl = min((Tb + n - 1) / n, Tlfr_max);
    const float* f = feat + (size_t)b * Tmax * n_mels;
    const int cnt = Tb * n_mels;
    float s = 0.f;
    for (int i = tid; i < cnt; i += 1024) s += f[i];
    const float mean = cnt > 0 ? block_sum(s, red) / (float)cnt : 0.f;
    float q = 0.f;
    for (int i = tid; i < cnt; i += 1024) { const float d = f[i] - mean; q += d * d; }
    const float var = cnt > 1 ? block_sum(q, red) / (float)(cnt - 1) : 1.f;  // unbiased (torch .std())
    const float rstd = rsqrtf(var);
    specaug_load_row(row, ranges + (size_t)b * ld, n_t, n_f, n_s, Tb, n_mels);
    const int W = m * n_mels;
    T* o = out + (size_t)b * Tlfr_max * W;
    const int total = Tlfr_max * W;
    for (int i = tid; i < total; i += 1024) {
        const int r = i / W, c = i - r * W;
        float val = 0.f;
        if (r < Tl) {
            const int j = c / n_mels, mm = c - j * n_mels;
            const int src = min(r * n + j, Tb - 1);   // tail frames repeat the last input frame
            val = (f[(size_t)src * n_mels + mm] - mean) * rstd;
            val = specaug_pull(row, n_t, n_f, n_s, src, mm, Tb, val, [=](int u) { return (f[(size_t)u * n_mels + mm] - mean) * rstd; });
        }
        o[i] = from_f32<T>(val);
    }
    if (tid == 0) out_len[b] = Tl;
}

// global_norm_lfr_kernel's tiled no-mask path with the policies' store loop; every workgroup of an utterance loads its row.
template <typename T>
__global__ __launch_bounds__(1024) void global_norm_specaug_lfr_kernel(const float* __restrict__ feat, const int32_t* __restrict__ wav_len,
                                                                       const int32_t* __restrict__ ranges, int ld, int n_t, int n_f, int n_s,
                                                                       const float* __restrict__ mean, const float* __restrict__ istd, T* __restrict__ out,
                                                                       int32_t* __restrict__ out_len, int Tmax, int n_mels, int m, int n, int Tlfr_max) {
    __shared__ int row[SPEC_ROW];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int len = wav_len[b];
    const int Tb = len > 0 ? min(1 + len / HOP, Tmax) : 0;
    const int Tl = min((Tb + n - 1) / n, Tlfr_max);
    const float* f = feat + (size_t)b * Tmax * n_mels;
    specaug_load_row(row, ranges + (size_t)b * ld, n_t, n_f, n_s, Tb, n_mels);
    const int W = m * n_mels;
    T* o = out + (size_t)b * Tlfr_max * W;
    const int total = Tlfr_max * W;
    const auto frame_at = [=](int t) { return f + (size_t)t * n_mels; };
    for (int i = blockIdx.x * 1024 + tid; i < total; i += gridDim.x * 1024) {
        const int r = i / W, c = i - r * W;
        float val = 0.f;
        if (r < Tl) {
            int src, mm;
            val = cmvn_lfr_elem(frame_at, r, c, n_mels, n, Tb, mean, istd, &src, &mm);
            // frame u, bin mm through the same function: stacking factor 1, row u, column mm
            val = specaug_pull(row, n_t, n_f, n_s, src, mm, Tb, val, [=](int u) {
                int s2, m2;
                return cmvn_lfr_elem(frame_at, u, mm, n_mels, 1, Tb, mean, istd, &s2, &m2);
            });
        }
        o[i] = from_f32<T>(val);
    }
    if (tid == 0 && blockIdx.x == 0) out_len[b] = Tl;
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
            val = cmvn_lfr_elem([=](int t) { return f + (size_t)(t & fmask) * n_mels; }, r_begin + r, c, n_mels, n, Tb, mean, istd, &src, &mm);
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
    if (B <= 0 || Smax <= NFFT / 2 || Tmax <= 0 || n_mels <= 0 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_logmel_fwd: bad shape B=%d Smax=%d Tmax=%d n_mels=%d", B, Smax, Tmax, n_mels);
    dim3 grid(ceil_div(Tmax, FR), B);
    logmel_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav, wav_len, window, melfb, feat, Smax, Tmax, n_mels);
    ASR_CHECK_LAUNCH("asr_logmel_fwd");
    return ASR_OK;
}

extern "C" int asr_utt_norm_augment_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* masks, void* out, int32_t* out_len, int B, int Tmax,
                                            int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream) {
    if (!feat || !wav_len || !out || !out_len) ASR_FAIL(ASR_EINVAL, "asr_utt_norm_augment_lfr_fwd: null pointer");
    if (B <= 0 || Tmax <= 0 || n_mels <= 0 || m <= 0 || n <= 0 || Tlfr_max <= 0) ASR_FAIL(ASR_EINVAL, "asr_utt_norm_augment_lfr_fwd: bad shape");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ASR_F32) utt_norm_lfr_kernel<float><<<B, 1024, 0, st>>>(feat, wav_len, masks, (float*)out, out_len, Tmax, n_mels, m, n, Tlfr_max);
    else if (dtype == ASR_BF16) utt_norm_lfr_kernel<bf16_t><<<B, 1024, 0, st>>>(feat, wav_len, masks, (bf16_t*)out, out_len, Tmax, n_mels, m, n, Tlfr_max);
    else ASR_FAIL(ASR_EDTYPE, "asr_utt_norm_augment_lfr_fwd: dtype %d", dtype);
    ASR_CHECK_LAUNCH("asr_utt_norm_augment_lfr_fwd");
    return ASR_OK;
}

extern "C" int asr_utt_norm_lfr_fwd(const float* feat, const int32_t* wav_len, void* out, int32_t* out_len, int B, int Tmax, int n_mels, int m, int n,
                                    int Tlfr_max, int dtype, void* stream) {
    return asr_utt_norm_augment_lfr_fwd(feat, wav_len, nullptr, out, out_len, B, Tmax, n_mels, m, n, Tlfr_max, dtype, stream);
}

// ---- global CMVN and the streaming front end -----------------------------------------------------------------------------------------
extern "C" int asr_cmvn_accumulate(const float* feat, const int32_t* wav_len, double* acc, int B, int Tmax, int n_mels, void* stream) {
    if (!feat || !wav_len || !acc) ASR_FAIL(ASR_EINVAL, "asr_cmvn_accumulate: null pointer");
    if (B <= 0 || B > 65535 || Tmax <= 0 || n_mels <= 0 || n_mels > CMVN_MAX_MELS)
        ASR_FAIL(ASR_EINVAL, "asr_cmvn_accumulate: bad shape B=%d Tmax=%d n_mels=%d (n_mels at most %d)", B, Tmax, n_mels, CMVN_MAX_MELS);
    dim3 grid(ceil_div(Tmax, CMVN_ROWS), B);
    cmvn_stats_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(feat, wav_len, acc, Tmax, n_mels);
    ASR_CHECK_LAUNCH("asr_cmvn_accumulate");
    return ASR_OK;
}

extern "C" int asr_global_norm_augment_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* masks, const float* mean, const float* istd, void* out,
                                               int32_t* out_len, int B, int Tmax, int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream) {
    if (!feat || !wav_len || !mean || !istd || !out || !out_len) ASR_FAIL(ASR_EINVAL, "asr_global_norm_augment_lfr_fwd: null pointer");
    if (B <= 0 || B > 65535 || Tmax <= 0 || n_mels <= 0 || m <= 0 || n <= 0 || Tlfr_max <= 0)
        ASR_FAIL(ASR_EINVAL, "asr_global_norm_augment_lfr_fwd: bad shape B=%d Tmax=%d n_mels=%d m=%d n=%d Tlfr_max=%d", B, Tmax, n_mels, m, n, Tlfr_max);
    if ((long long)Tlfr_max * m * n_mels > INT32_MAX) ASR_FAIL(ASR_EINVAL, "asr_global_norm_augment_lfr_fwd: Tlfr_max * m * n_mels does not fit an int");
    hipStream_t st = (hipStream_t)stream;
    // 4 elements per thread without masks; with masks one workgroup per utterance owns the fill reductions
    dim3 grid(masks ? 1 : max(1, min(ceil_div(Tlfr_max * m * n_mels, 4096), 256)), B);
    if (dtype == ASR_F32) global_norm_lfr_kernel<float><<<grid, 1024, 0, st>>>(feat, wav_len, masks, mean, istd, (float*)out, out_len, Tmax, n_mels, m, n, Tlfr_max);
    else if (dtype == ASR_BF16) global_norm_lfr_kernel<bf16_t><<<grid, 1024, 0, st>>>(feat, wav_len, masks, mean, istd, (bf16_t*)out, out_len, Tmax, n_mels, m, n, Tlfr_max);
    else ASR_FAIL(ASR_EDTYPE, "asr_global_norm_augment_lfr_fwd: dtype %d", dtype);
    ASR_CHECK_LAUNCH("asr_global_norm_augment_lfr_fwd");
    return ASR_OK;
}

// ---- SpecAugment policies ---------------------------------------------------------------------------------------------------------------
static int specaug_check(const char* name, const int32_t* ranges, int ld, int n_t, int n_f, int n_s) {
    if (!ranges) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if (n_t < 0 || n_f < 0 || n_s < 0 || n_t > SPEC_MAX || n_f > SPEC_MAX || n_s > SPEC_MAX)
        ASR_FAIL(ASR_EINVAL, "%s: n_t=%d n_f=%d n_s=%d (each 0 .. %d)", name, n_t, n_f, n_s, SPEC_MAX);
    if (ld < 2 + 2 * n_t + 2 * n_f + 3 * n_s) ASR_FAIL(ASR_EINVAL, "%s: ld=%d, a row has %d words", name, ld, 2 + 2 * n_t + 2 * n_f + 3 * n_s);
    return ASR_OK;
}

extern "C" int asr_utt_norm_specaug_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* ranges, int ld, int n_t, int n_f, int n_s, void* out,
                                            int32_t* out_len, int B, int Tmax, int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream) {
    if (!feat || !wav_len || !out || !out_len) ASR_FAIL(ASR_EINVAL, "asr_utt_norm_specaug_lfr_fwd: null pointer");
    if (B <= 0 || Tmax <= 0 || n_mels <= 0 || m <= 0 || n <= 0 || Tlfr_max <= 0)
        ASR_FAIL(ASR_EINVAL, "asr_utt_norm_specaug_lfr_fwd: bad shape B=%d Tmax=%d n_mels=%d m=%d n=%d Tlfr_max=%d", B, Tmax, n_mels, m, n, Tlfr_max);
    if (const int rc = specaug_check("asr_utt_norm_specaug_lfr_fwd", ranges, ld, n_t, n_f, n_s)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ASR_F32)
        utt_norm_specaug_lfr_kernel<float><<<B, 1024, 0, st>>>(feat, wav_len, ranges, ld, n_t, n_f, n_s, (float*)out, out_len, Tmax, n_mels, m, n, Tlfr_max);
    else if (dtype == ASR_BF16)
        utt_norm_specaug_lfr_kernel<bf16_t><<<B, 1024, 0, st>>>(feat, wav_len, ranges, ld, n_t, n_f, n_s, (bf16_t*)out, out_len, Tmax, n_mels, m, n, Tlfr_max);
    else ASR_FAIL(ASR_EDTYPE, "asr_utt_norm_specaug_lfr_fwd: dtype %d", dtype);
    ASR_CHECK_LAUNCH("asr_utt_norm_specaug_lfr_fwd");
    return ASR_OK;
}

extern "C" int asr_global_norm_specaug_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* ranges, int ld, int n_t, int n_f, int n_s,
                                               const float* mean, const float* istd, void* out, int32_t* out_len, int B, int Tmax, int n_mels, int m, int n,
                                               int Tlfr_max, int dtype, void* stream) {
    if (!feat || !wav_len || !mean || !istd || !out || !out_len) ASR_FAIL(ASR_EINVAL, "asr_global_norm_specaug_lfr_fwd: null pointer");
    if (B <= 0 || B > 65535 || Tmax <= 0 || n_mels <= 0 || m <= 0 || n <= 0 || Tlfr_max <= 0)
        ASR_FAIL(ASR_EINVAL, "asr_global_norm_specaug_lfr_fwd: bad shape B=%d Tmax=%d n_mels=%d m=%d n=%d Tlfr_max=%d", B, Tmax, n_mels, m, n, Tlfr_max);
    if ((long long)Tlfr_max * m * n_mels > INT32_MAX) ASR_FAIL(ASR_EINVAL, "asr_global_norm_specaug_lfr_fwd: Tlfr_max * m * n_mels does not fit an int");
    if (const int rc = specaug_check("asr_global_norm_specaug_lfr_fwd", ranges, ld, n_t, n_f, n_s)) return rc;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(max(1, min(ceil_div(Tlfr_max * m * n_mels, 4096), 256)), B);      // the tiling of the sibling's no-mask path: 4 elements per thread
    if (dtype == ASR_F32)
        global_norm_specaug_lfr_kernel<float><<<grid, 1024, 0, st>>>(feat, wav_len, ranges, ld, n_t, n_f, n_s, mean, istd, (float*)out, out_len, Tmax, n_mels, m,
                                                                     n, Tlfr_max);
    else if (dtype == ASR_BF16)
        global_norm_specaug_lfr_kernel<bf16_t><<<grid, 1024, 0, st>>>(feat, wav_len, ranges, ld, n_t, n_f, n_s, mean, istd, (bf16_t*)out, out_len, Tmax, n_mels,
                                                                      m, n, Tlfr_max);
    else ASR_FAIL(ASR_EDTYPE, "asr_global_norm_specaug_lfr_fwd: dtype %d", dtype);
    ASR_CHECK_LAUNCH("asr_global_norm_specaug_lfr_fwd");
    return ASR_OK;
}

static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

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
    if (!wav_ring || !par || !window || !melfb || !feat_ring) ASR_FAIL(ASR_EINVAL, "asr_stream_logmel: null pointer");
    if (B <= 0 || B > 65535 || max_new <= 0 || n_mels <= 0 || !pow2(scap) || scap < 1024 || !pow2(fcap) || max_new > fcap)
        ASR_FAIL(ASR_EINVAL, "asr_stream_logmel: bad shape B=%d max_new=%d scap=%d fcap=%d n_mels=%d (scap >= 1024 and fcap powers of two, max_new <= fcap)", B,
                 max_new, scap, fcap, n_mels);
    dim3 grid(ceil_div(max_new, FR), B);
    stream_logmel_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(wav_ring, par, window, melfb, feat_ring, scap, fcap, n_mels);
    ASR_CHECK_LAUNCH("asr_stream_logmel");
    return ASR_OK;
}

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
