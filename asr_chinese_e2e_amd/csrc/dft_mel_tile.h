// The frame tile the two spectral front ends (logmel.hip, fbank.hip) share: everything after the 32 prepared frames of a workgroup lie in
// LDS - twiddle table, DFT, power, mel filterbank, floor, log, store - and the offline and streaming kernels' way to that tile.  How a
// frame is prepared (padding, DC removal, pre-emphasis, window) and the floor under the logarithm stay with the front ends.
//
// One workgroup of 256 threads = 32 consecutive frames of one utterance; the DFT is a GEMM on the fp32 matrix pipe:
//   C[32 frames][2 NBIN] = X[32][400] (prepared frames, LDS)  x  D[400][2 NBIN],
//   D[n][c] = cos(2 pi n c / NFFT) for c < NBIN,  -sin(2 pi n (c - NBIN) / NFFT) for NBIN <= c < 2 NBIN
// (taps 400 .. NFFT - 1 of a longer transform are its zero padding), with D never stored: the lane that owns column c keeps cos / sin
// of its angle in registers and rotates them by 2 theta per step: 200 steps of an fp32 recurrence from exact start values, never
// restarted.  Its drift is the larger part of the error budget that tests/logmel_emul.py states and tests/test_logmel_gpu.py measures
// (DESIGN.md has the table); v_mfma_f32_32x32x2_f32 is exact fp32 multiply-accumulate, so the rest is the error of the direct sum.  Then
// power = re^2 + im^2 (from C, kept in LDS) times the mel filterbank, again on the matrix pipe, floor, log, store.  (The first version
// gave one DFT bin to each thread and one frame to each workgroup: 80 k scalar MACs per frame through LDS reads, 0.6 ms for 32 x 5 s of
// audio = 17 % of a training step.)
//
// A frame's value depends on its own prepared row only: every MFMA accumulator row is the sum over its own A row, and the rotation
// recurrence runs along the columns - so a frame has the same bits in whichever tile and row it is computed, which is what lets streamed
// frames equal offline ones.
#pragma once
#include "asr_common.h"

namespace dmt {

constexpr int FR = 32;            // frames per workgroup
constexpr int FLEN = 400;         // samples of a frame = DFT taps that are not zero padding

// 32 frames t0 .. t0 + 31 of one utterance of Tb frames.  Plan holds the front end's constants: NFFT = transform size, NBIN = bins used
// (re | im = 2 NBIN DFT columns), XS = LDS row stride of the prepared frames (odd: rows hit distinct banks), CHUNK = filterbank rows a lane
// prefetches at a time.
// prepare(buf) fills row f (stride XS) of buf with the FLEN prepared samples of frame t0 + f, zeros for t0 + f >= Tb; row(frame) is
// where frame t0 + frame goes, or nullptr for a row that is not written; floor_log(x) is the logarithm of the floored mel energy.
template <typename Plan, typename Prepare, typename Row, typename FloorLog>
__device__ __forceinline__ void tile(Prepare prepare, Row row, FloorLog floor_log, const float* __restrict__ melfb, int Tb, int t0, int n_mels) {
    constexpr int NFFT = Plan::NFFT, NBIN = Plan::NBIN, XS = Plan::XS, CHUNK = Plan::CHUNK;
    constexpr int NC = 2 * NBIN;              // DFT output columns
    constexpr int CT = (NC + 31) / 32;        // column tiles that hold one
    constexpr int CS = CT * 32 + 1;           // LDS row stride of C
    // 16 column tiles, four per wave, cover 512 columns.  ALIGNED: they are exactly the 2 NBIN columns, waves 0, 1 own the cosines and
    // waves 2, 3 the sines.  Otherwise the re | im boundary and the end fall inside a tile: each lane selects its operand, and the tiles
    // past CT are all zero (they keep the code branch-free and the four waves equally loaded).
    constexpr bool ALIGNED = NC == 512;
    static_assert(NC <= 512 && FLEN <= NFFT && FLEN % 2 == 0 && XS >= FLEN, "16 column tiles, taps in pairs");
    __shared__ float buf[FR * (XS > CS ? XS : CS)];      // the prepared frames, later C
    __shared__ float tw_c[NFFT], tw_s[NFFT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    prepare(buf);
    for (int n = tid; n < NFFT; n += 256) {            // exact cos / sin(2 pi n / NFFT): start values and rotation steps
        float sv, cv;
        sincospif(2.f * (float)n / (float)NFFT, &sv, &cv);
        tw_c[n] = cv;
        tw_s[n] = sv;
    }
    __syncthreads();
    // ---- DFT: wave w owns the four column tiles 4w .. 4w+3.  The lane that owns column c needs cos / sin(2 pi k bin / NFFT) for
    // k = kh, kh+2, ...: a rotation by 2 theta per step in registers (a table in LDS would be read at stride k*bin: up to 32-way bank
    // conflicts).  200 steps of the fp32 recurrence drift by ~2e-5 relative: 1e-5 in the log domain.
    const int r = lane & 31, kh = lane >> 5;
    f32x16 acc[4];
    float tc[4], ts[4], rc[4], rs[4], sgn_c[4], sgn_s[4];      // sgn_*: unaligned only, operand = sgn_c * cos + sgn_s * sin
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
        const unsigned c = (4 * w + q) * 32 + r;
        const bool live = c < NC, is_im = c >= NBIN;
        const unsigned bin = c % NBIN;                 // of a live column
        sgn_c[q] = live && !is_im ? 1.f : 0.f;
        sgn_s[q] = live && is_im ? -1.f : 0.f;
        const unsigned j2 = (2 * bin) % NFFT, j0 = (kh * bin) % NFFT;
        rc[q] = tw_c[j2];                              // rotation by 2 theta
        rs[q] = tw_s[j2];
        tc[q] = tw_c[j0];                              // k = kh
        ts[q] = tw_s[j0];
    }
    const float* xrow = buf + r * XS + kh;
#pragma unroll 4
    for (int kk = 0; kk < FLEN / 2; ++kk) {
        const float a = xrow[2 * kk];                  // X[frame r][k = 2 kk + kh]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float d;
            if constexpr (ALIGNED) d = w >= 2 ? -ts[q] : tc[q];      // wave-uniform
            else d = fmaf(sgn_c[q], tc[q], sgn_s[q] * ts[q]);        // the same values: fmaf(1, c, 0 s) = c, fmaf(0, c, -1 s) = -s
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
        if constexpr (!ALIGNED)
            if (c >= CT * 32) continue;                // columns past the C row (all zero anyway)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int frame = (i & 3) + 8 * (i >> 2) + 4 * kh;        // accumulator row
            buf[frame * CS + c] = acc[q][i];
        }
    }
    __syncthreads();
    // ---- mel: out[32][n_mels] = power[32][NBIN] x melfb[NBIN][n_mels]; wave w owns mel columns 32 w .. 32 w + 31
    for (int mt = w; mt * 32 < n_mels; mt += 4) {
        const int m = mt * 32 + r;
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
        const float* crow = buf + r * CS;
        // the filterbank column of this lane is fetched a quarter at a time into registers BEFORE the
        // MFMAs that use it: issued one by one between MFMAs, each L2 round trip would be exposed
        constexpr int KSTEPS = (NBIN + 1) / 2;                 // two bins per MFMA: 101 steps in 4 chunks of 26, 128 in 4 of 32
        constexpr bool WHOLE = KSTEPS % CHUNK == 0 && NBIN % 2 == 0;      // no step past the end, no bin past the last
#pragma unroll 1
        for (int k0 = 0; k0 < KSTEPS; k0 += CHUNK) {
            float mbv[CHUNK];
#pragma unroll
            for (int i = 0; i < CHUNK; ++i) {
                const int k = 2 * (k0 + i) + kh;
                mbv[i] = ((WHOLE || (k0 + i < KSTEPS && k < NBIN)) && m < n_mels) ? melfb[(size_t)k * n_mels + m] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < CHUNK; ++i) {
                const int k = 2 * (k0 + i) + kh;
                float pa = 0.f;
                if (WHOLE || (k0 + i < KSTEPS && k < NBIN)) {
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
                if (dst) dst[m] = (t0 + frame < Tb) ? floor_log(o[i]) : 0.f;
            }
        }
    }
}

// Offline: workgroup (x, b) computes frames 32 x .. 32 x + 31 of utterance b, Tb of whose Tmax rows of feat (B, Tmax, n_mels) are frames
// and the rest zeros.  frames(buf, t0, fetch) prepares the tile at t0 from fetch(idx) = the sample at absolute index idx of the utterance.
template <typename Plan, typename Frames, typename FloorLog>
__device__ __forceinline__ void offline(Frames frames, FloorLog floor_log, const float* __restrict__ wav, const float* __restrict__ melfb,
                                        float* __restrict__ feat, int Smax, int Tb, int Tmax, int n_mels) {
    const int t0 = blockIdx.x * FR, b = blockIdx.y, tid = threadIdx.x;
    float* out = feat + ((size_t)b * Tmax + t0) * n_mels;
    const int rows_here = min(FR, Tmax - t0);
    if (t0 >= Tb) {                            // nothing but padding: zeros
        for (int i = tid; i < rows_here * n_mels; i += 256) out[i] = 0.f;
        return;
    }
    const float* wv = wav + (size_t)b * Smax;
    tile<Plan>([=](float* buf) { frames(buf, t0, [=](int idx) { return wv[idx]; }); },
                                [=](int frame) { return frame < rows_here ? out + (size_t)frame * n_mels : nullptr; }, floor_log, melfb, Tb, t0, n_mels);
}

// Streaming: frames [t_begin, t_begin + n_new) of utterance b = blockIdx.y from a ring of its most recent samples into a ring of its
// most recent frames: sample s lives at wav_ring[b][s & (scap - 1)], frame t at feat_ring[b][t & (fcap - 1)].  Tb: the utterance's frame
// count as far as the tile is concerned (frames at and past it are neither prepared nor stored).
template <typename Plan, typename Frames, typename FloorLog>
__device__ __forceinline__ void streamed(Frames frames, FloorLog floor_log, const float* __restrict__ wav_ring, const float* __restrict__ melfb,
                                         float* __restrict__ feat_ring, int t_begin, int n_new, int Tb, int scap, int fcap, int n_mels) {
    const int b = blockIdx.y, f0 = blockIdx.x * FR;
    if (f0 >= n_new) return;
    const int t0 = t_begin + f0;
    const float* wv = wav_ring + (size_t)b * scap;
    float* fr = feat_ring + (size_t)b * fcap * n_mels;
    const int smask = scap - 1, fmask = fcap - 1, rows_here = n_new - f0;
    tile<Plan>([=](float* buf) { frames(buf, t0, [=](int idx) { return wv[idx & smask]; }); },
                                [=](int frame) { return frame < rows_here ? fr + (size_t)((t0 + frame) & fmask) * n_mels : nullptr; }, floor_log, melfb, Tb,
                                t0, n_mels);
}

// The host check of the two streaming entries (asr_stream_logmel, asr_stream_fbank); on success the grid of their launch.
static inline int stream_check(const char* name, const void* wav_ring, const void* par, const void* window, const void* melfb, const void* feat_ring, int B,
                               int max_new, int scap, int fcap, int n_mels, dim3* grid) {
    if (!wav_ring || !par || !window || !melfb || !feat_ring) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if (B <= 0 || B > 65535 || max_new <= 0 || n_mels <= 0 || !pow2(scap) || scap < 1024 || !pow2(fcap) || max_new > fcap)
        ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d max_new=%d scap=%d fcap=%d n_mels=%d (scap >= 1024 and fcap powers of two, max_new <= fcap)", name, B, max_new,
                 scap, fcap, n_mels);
    *grid = dim3(ceil_div(max_new, FR), B);
    return ASR_OK;
}

}  // namespace dmt
