// Sample-rate conversion of a waveform batch to 16 kHz on device: every utterance is resampled from its own source rate fs = 16000 p/q with a
// Kaiser-windowed sinc of 64 zero crossings in polyphase form,
//   y[n] = sum_{j=-W..W} x[(n p) / q + j] * H[(n p) % q][j + W],      x = 0 outside [0, n_total),
// in front of everything else the waveform loader does.  The reference has no resampler: parity unpinned by the reference; the definition
// and its float64 restatement are in data_handler/resample.py and tests/resample_ref.py.  The arithmetic of one output is part of the
// definition - acc = 0, then acc = fmaf(x, h, acc) over j ascending, one accumulator - so that a stream cut anywhere (the window form:
// a row that holds only part of the utterance, an output range that starts anywhere) gives the bits of the offline call.
#include "asr_common.h"
#include "polyphase_tile.h"

namespace {

// One workgroup = TILE consecutive outputs of one utterance.  The input span of the tile (up to 7.6 samples per output plus 2 W of halo) is
// staged in LDS once, with 16-byte loads; the taps stay in global memory (up to 350 KB per rate: resident in L2, not in LDS) in the order
// T[j][n mod q], so lanes of consecutive outputs read consecutive words.  A lane owns NR outputs `stride` apart; for q <= NT the stride
// is a multiple of q, the NR outputs share one phase and every tap is loaded once for NR multiply-adds; for q == 1 (48, 32, 96 kHz) every
// output of the workgroup shares it and the taps are scalar operands.  Each multiply-add still takes one 4-byte LDS read: the LDS
// (32 lanes per clock against the VALU's 64) bounds the kernel at half the vector rate.
constexpr int TILE = ASR_RESAMPLE_TILE;
constexpr int NT = ptile::NT, NR = 4;
constexpr int Q_MAX = ASR_RESAMPLE_Q_MAX, NTAPS_MAX = ASR_RESAMPLE_NTAPS_MAX, R_MAX = ASR_RESAMPLE_PLANS_MAX;
constexpr int XS = 8832;                  // staged samples: (TILE - 1) p/q + 1 + 2 W + 1 + alignment pads at the largest p/q (7.56) 1023 taps admit

// MODE 0: q == 1, one phase for the workgroup (uniform tap address: scalar loads); 1: the lane's NR outputs share the phase m[0];
// 2: q > NT, a phase per output.  THE summation order: j ascending, one accumulator per output.
template <int MODE>
__device__ __forceinline__ void fir(const float* xs, const float* __restrict__ T, int q, int ntaps, const int (&xo)[NR], const int (&m)[NR], float (&acc)[NR]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) acc[i] = 0.f;
#pragma unroll 4
    for (int j = 0; j < ntaps; ++j) {
        const float* row = T + j * q;
        if (MODE == 2) {
#pragma unroll
            for (int i = 0; i < NR; ++i) acc[i] = fmaf(xs[xo[i] + j], row[m[i]], acc[i]);
        } else {
            const float h = MODE == 0 ? row[0] : row[m[0]];
#pragma unroll
            for (int i = 0; i < NR; ++i) acc[i] = fmaf(xs[xo[i] + j], h, acc[i]);
        }
    }
}

__global__ __launch_bounds__(NT) void resample_kernel(const float* __restrict__ wav, const int32_t* __restrict__ rate_idx, const int32_t* __restrict__ win,
                                                      const int32_t* __restrict__ pq, const int32_t* __restrict__ tap_off, const float* __restrict__ taps,
                                                      float* __restrict__ out, int32_t* __restrict__ out_len, int Smax, int Smax_out, int R, int taps_len,
                                                      int vec_in, int vec_out) {
    __shared__ __attribute__((aligned(16))) float xs[XS];
    __shared__ __attribute__((aligned(16))) float ys[TILE + 4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n0 = blockIdx.x * TILE;                   // first output of the tile, counted from out_start; n0 < Smax_out
    const int tcount = min(TILE, Smax_out - n0);
    const int32_t* w = win + 5 * (size_t)b;
    const int in_base = w[0], n_avail = min(max(w[1], 0), Smax), n_total = max(w[2], 0), out_start = max(w[3], 0);
    const int n_emit = min(max(w[4], 0), Smax_out);
    if (blockIdx.x == 0 && tid == 0) out_len[b] = n_emit;
    // the plan; anything the host did not validate (and 16 kHz itself: index outside [0, R), or p == q) is a copy
    const int ri = rate_idx[b];
    int p = 1, q = 1, ntaps = 1;
    const float* T = taps;
    if (ri >= 0 && ri < R) {
        const int pp = pq[2 * ri], qq = pq[2 * ri + 1], o0 = tap_off[ri], o1 = tap_off[ri + 1];
        if (pp != qq && pp >= 1 && qq >= 1 && qq <= Q_MAX && pp <= 8 * Q_MAX && o0 >= 0 && o1 > o0 && o1 <= taps_len && (o1 - o0) % qq == 0) {
            const int nt = (o1 - o0) / qq;
            if ((nt & 1) && nt >= 3 && nt <= NTAPS_MAX && (qq - 1 + (TILE - 1) * pp) / qq + nt + 8 <= XS) p = pp, q = qq, ntaps = nt, T = taps + o0;
        }
    }
    const bool copy = p == q;
    const int W = (ntaps - 1) >> 1;
    const long long row_in = (long long)b * Smax, row_out = (long long)b * Smax_out;
    const int tlive = min(tcount, n_emit - n0);         // outputs of this tile below n_emit (<= 0: the tile is padding only)
    const int opad = ptile::begin_tile(ys, row_out + n0, tlive, tcount, tid);      // ys[opad + t] = output n0 + t
    if (tlive > 0) {
        // exact index arithmetic: 64 bits once per workgroup ((out_start + n0) p passes 2^31 in a long stream), 32 bits per output
        const long long nf = (long long)out_start + n0, np0 = nf * p;
        const long long base0 = np0 / q;
        const int r0 = (int)(np0 % q), m0 = (int)(nf % q);
        // the part of the row that is real: sample k of the utterance sits at k - in_base, and 0 <= k < n_total
        const long long vlo64 = in_base < 0 ? -(long long)in_base : 0, vhi64 = min((long long)n_avail, (long long)n_total - in_base);
        const int vlo = (int)min(vlo64, (long long)n_avail), vhi = (int)max(min(vhi64, (long long)n_avail), 0LL);
        const long long lo64 = base0 - W - in_base;     // row-relative index of the first sample the tile reads
        const int lo = (int)min(max(lo64, -(1LL << 30)), 1LL << 30);      // far outside the row either way: zeros
        const int count = (r0 + (tlive - 1) * p) / q + ntaps;
        const int ipad = ptile::stage(xs, wav, row_in, lo, count, vlo, vhi, vec_in != 0, tid);
        __syncthreads();
        const int stride = q <= NT ? q * (NT / q) : NT;
        for (int tb = 0; tb < tlive; tb += NR * stride) {
            if (tid < stride) {
                int xo[NR], m[NR];
                bool live[NR];
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const int t = tb + tid + i * stride;
                    live[i] = t < tlive;
                    const int tt = live[i] ? t : 0;         // a dead slot recomputes output 0 of the tile (staged, in bounds) and drops it
                    xo[i] = ipad + (r0 + tt * p) / q;
                    m[i] = (m0 + tt) % q;
                }
                float acc[NR];
                if (copy) {
#pragma unroll
                    for (int i = 0; i < NR; ++i) acc[i] = xs[xo[i]];
                } else if (q == 1) {
                    fir<0>(xs, T, q, ntaps, xo, m, acc);
                } else if (q <= NT) {
                    fir<1>(xs, T, q, ntaps, xo, m, acc);
                } else {
                    fir<2>(xs, T, q, ntaps, xo, m, acc);
                }
#pragma unroll
                for (int i = 0; i < NR; ++i)
                    if (live[i]) ys[opad + tb + tid + i * stride] = acc[i];
            }
        }
    }
    ptile::store_tile(out + row_out + n0, ys, opad, tcount, vec_out != 0, tid);
}

}  // namespace

extern "C" int asr_resample_fwd(const float* wav, const int32_t* rate_idx, const int32_t* win, const int32_t* pq, const int32_t* tap_off, const float* taps,
                                float* out, int32_t* out_len, int B, int Smax, int Smax_out, int R, int taps_len, void* stream) {
    if (!wav || !rate_idx || !win || !pq || !tap_off || !taps || !out || !out_len) ASR_FAIL(ASR_EINVAL, "asr_resample_fwd: null pointer");
    if (B < 1 || Smax < 1 || Smax_out < 1 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_resample_fwd: bad shape B=%d Smax=%d Smax_out=%d", B, Smax, Smax_out);
    if (R < 1 || R > R_MAX || taps_len < 1) ASR_FAIL(ASR_EINVAL, "asr_resample_fwd: R=%d (1 .. %d) taps_len=%d", R, R_MAX, taps_len);
    dim3 grid(ceil_div(Smax_out, TILE), B);
    const int vec_in = ((uintptr_t)wav & 15) == 0, vec_out = ((uintptr_t)out & 15) == 0;
    resample_kernel<<<grid, NT, 0, (hipStream_t)stream>>>(wav, rate_idx, win, pq, tap_off, taps, out, out_len, Smax, Smax_out, R, taps_len, vec_in, vec_out);
    ASR_CHECK_LAUNCH("asr_resample_fwd");
    return ASR_OK;
}
