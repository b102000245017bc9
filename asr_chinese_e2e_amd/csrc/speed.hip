// Speed perturbation of a waveform batch on device: every utterance is resampled by its own rational factor p/q with a Hann-windowed sinc
// in polyphase form,
//   y[n] = sum_{j=-W..W} x[(n p) / q + j] * H[(n p) % q][j + W],      n < n_out = ceil(n_in q / p),      x = 0 outside [0, n_in),
// and handed to the log-mel kernel as if it had been recorded that way (sox / Kaldi `speed`: pitch and tempo change together).  The
// reference has no waveform-side augmentation: parity unpinned by the reference; the definition and its float64 restatement are in
// tests/speed_ref.py.  Factor 1 (p == q) is a copy, bit for bit, inside the same launch.
#include "asr_common.h"
#include "polyphase_tile.h"

namespace {

// One workgroup = SPEED_TILE consecutive output samples of one utterance.  The input span of the tile (plus W samples of halo on each side)
// is staged in LDS with 16-byte loads, the utterance's phase table sits beside it; neighbouring lanes compute neighbouring outputs
// (they read neighbouring LDS words: at most 2-way bank conflicts up to p/q = 2, where four consecutive outputs per lane would be
// 4-way), each lane at one phase of the filter, into an LDS row from which every lane stores 4 consecutive outputs with one 16-byte store.  The kernel moves 8 bytes
// per output and does 2 W + 1 multiply-adds from LDS for it: at the 15 taps of 9/10 and 11/10 it takes 10.6 us for 32 x 5 s, three times a
// device-to-device copy of the same bytes (profiles/speed_perturb_bench.json) - the LDS reads, not memory, set its time.
constexpr int TILE = ASR_SPEED_TILE;      // output samples per workgroup
constexpr int NT = ptile::NT;             // threads
constexpr int SPAN = 2048;                // staged input samples per pass: a whole tile up to p/q ~ 1.9, several passes beyond
constexpr int PQ_MAX = 20, NTAPS_MAX = 255, F_MAX = 64;

constexpr int NTAPS_FAST = 15;            // 2 W + 1 of every factor in [1/2, 1): the taps of a lane's phase live in registers

__global__ __launch_bounds__(NT) void speed_perturb_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ factor,
                                                           const int32_t* __restrict__ pq, const float* __restrict__ taps, float* __restrict__ out,
                                                           int32_t* __restrict__ out_len, int Smax, int Smax_out, int F, int qmax, int ntaps, int vec_in, int vec_out) {
    __shared__ __attribute__((aligned(16))) float xs[SPAN];
    __shared__ __attribute__((aligned(16))) float ys[TILE + 4];
    extern __shared__ float tab[];                      // (q, ntaps) phase table of this utterance
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n0 = blockIdx.x * TILE;                   // first output of the tile; n0 < Smax_out
    const int tcount = min(TILE, Smax_out - n0);
    const int len = min(max(wav_len[b], 0), Smax);
    const int f = min(max(factor[b], 0), F - 1);
    int p = pq[2 * f], q = pq[2 * f + 1];
    if (p < 1 || p > PQ_MAX || q < 1 || q > qmax) p = q = 1;      // a table entry the host did not validate: factor 1
    const bool copy = p == q;
    if (copy) p = q = 1;
    const int n_out = (int)min(((long long)len * q + p - 1) / p, (long long)Smax_out);
    if (blockIdx.x == 0 && tid == 0) out_len[b] = n_out;
    const long long row_in = (long long)b * Smax, row_out = (long long)b * Smax_out;
    const int tlive = min(tcount, n_out - n0);          // outputs of this tile below n_out (<= 0: the tile is padding only)
    const int opad = ptile::begin_tile(ys, row_out + n0, tlive, tcount, tid);      // ys[opad + t] = output n0 + t
    if (tlive > 0) {
        const int W = copy ? 0 : (ntaps - 1) >> 1;
        if (!copy) {
            const float* src = taps + (size_t)f * qmax * ntaps;
            for (int i = tid; i < q * ntaps; i += NT) tab[i] = src[i];
        }
        // exact index arithmetic: 64 bits once per workgroup, then (r0 + t p) < 2^15 per output
        const long long np0 = (long long)n0 * p;
        const int base0 = (int)(np0 / q), r0 = (int)(np0 % q);
        const int sub = min(TILE, ((SPAN - 2 * W - 8) * q) / p);      // outputs per pass: their span, halo and alignment pads fit xs
        for (int t0 = 0; t0 < tlive; t0 += sub) {
            const int t1 = min(t0 + sub, tlive);
            const int lo = base0 + (r0 + t0 * p) / q - W;
            const int count = base0 + (r0 + (t1 - 1) * p) / q + W - lo + 1;
            if (t0 > 0) __syncthreads();                // the previous pass is done with xs
            const int ipad = ptile::stage(xs, wav, row_in, lo, count, 0, len, vec_in != 0, tid);      // valid samples: [0, len)
            __syncthreads();
            // lane l takes outputs t0 + l, t0 + l + stride, ... with stride = q floor(NT / q): all of them at ONE phase r (its taps are
            // fetched once) and dstep input samples apart, so the one division per lane and pass is all the index arithmetic there is
            const int stride = q * (NT / q), dstep = (NT / q) * p;
            int t = t0 + tid;
            if (tid < stride && t < t1) {
                const int u = r0 + t * p, d = u / q, r = u - d * q;
                const float* x = xs + ipad + (base0 + d - W - lo);
                if (copy) {
                    for (; t < t1; t += stride, x += dstep) ys[opad + t] = x[0];
                } else if (ntaps == NTAPS_FAST) {
                    float h[NTAPS_FAST];
#pragma unroll
                    for (int j = 0; j < NTAPS_FAST; ++j) h[j] = tab[r * NTAPS_FAST + j];
                    for (; t < t1; t += stride, x += dstep) {
                        float acc = 0.f;
#pragma unroll
                        for (int j = 0; j < NTAPS_FAST; ++j) acc = fmaf(x[j], h[j], acc);
                        ys[opad + t] = acc;
                    }
                } else {
                    const float* h = tab + r * ntaps;
                    for (; t < t1; t += stride, x += dstep) {
                        float acc = 0.f;
                        for (int j = 0; j < ntaps; ++j) acc = fmaf(x[j], h[j], acc);
                        ys[opad + t] = acc;
                    }
                }
            }
        }
    }
    ptile::store_tile(out + row_out + n0, ys, opad, tcount, vec_out != 0, tid);
}

}  // namespace

extern "C" int asr_speed_perturb_fwd(const float* wav, const int32_t* wav_len, const int32_t* factor, const int32_t* pq, const float* taps, float* out,
                                     int32_t* out_len, int B, int Smax, int Smax_out, int F, int qmax, int ntaps, void* stream) {
    if (!wav || !wav_len || !factor || !pq || !taps || !out || !out_len) ASR_FAIL(ASR_EINVAL, "asr_speed_perturb_fwd: null pointer");
    if (B < 1 || Smax < 1 || Smax_out < 1 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_speed_perturb_fwd: bad shape B=%d Smax=%d Smax_out=%d", B, Smax, Smax_out);
    if (ntaps < 1 || ntaps > NTAPS_MAX || (ntaps & 1) == 0) ASR_FAIL(ASR_EINVAL, "asr_speed_perturb_fwd: ntaps=%d (odd, 1 .. %d)", ntaps, NTAPS_MAX);
    if (F < 1 || F > F_MAX || qmax < 1 || qmax > PQ_MAX) ASR_FAIL(ASR_EINVAL, "asr_speed_perturb_fwd: F=%d (1 .. %d) qmax=%d (1 .. %d)", F, F_MAX, qmax, PQ_MAX);
    dim3 grid(ceil_div(Smax_out, TILE), B);
    const int vec_in = ((uintptr_t)wav & 15) == 0, vec_out = ((uintptr_t)out & 15) == 0;
    speed_perturb_kernel<<<grid, NT, (size_t)qmax * ntaps * sizeof(float), (hipStream_t)stream>>>(wav, wav_len, factor, pq, taps, out, out_len, Smax, Smax_out, F,
                                                                                                 qmax, ntaps, vec_in, vec_out);
    ASR_CHECK_LAUNCH("asr_speed_perturb_fwd");
    return ASR_OK;
}
