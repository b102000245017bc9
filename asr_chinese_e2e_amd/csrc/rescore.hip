// Rescoring of n-best lists (include/asr_hip.h: asr_lm_score_nbest, asr_nbest_sweep; the definition is tests/rescore_ref.py on top of
// lm.py::NgramLM's host methods, and the kernels agree with it in integers and float bits).
//
// 1. lm_score_nbest_kernel: one lane per hypothesis, workgroups of 64.  The lane walks its tokens from (lm.start, 0.0) with ngram_walk.h's
//    chain and the insertion bonus per token, as the beam search does, then adds the end-of-sentence chain without the bonus (NgramLM.final).  The device only adds fp64 table terms in the host's order, so score and bias equal
//    NgramLM.score / NgramLM.walk bit for bit.
// 2. nbest_sweep_kernel: one wave per (grid point, 64 utterances), lane = utterance.  The grid point's K weights are wave-uniform.  The
//    features are (K, N, U) planes and the error counts (3, N, U), so the lanes of a load read consecutive addresses.  The lane forms
//    every entry's total as the definition does - a rounded product, then a rounded sum, terms of weight 0.0 skipped - keeps the best
//    scorable entry (the lowest index on ties) and adds the pick's (sub, del, ins, wrong) to the wave's partial in the workspace.
// 3. nbest_sweep_sum_kernel: one wave per grid point sums the partials of its blocks.  Integers: any order gives the same bytes, and
//    there is no atomic.
#include "asr_common.h"
#include "ngram_walk.h"

namespace {

__global__ __launch_bounds__(64) void lm_score_nbest_kernel(const int32_t* __restrict__ tok, const int32_t* __restrict__ len, int P, int ld, NgramLm g,
                                                            int has_eos, int eos, double* __restrict__ out_score, double* __restrict__ out_bias,
                                                            int32_t* __restrict__ out_state, int32_t* __restrict__ out_ntok) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const int n = min(len[p], ld);
    if (n < 0) {      // an absent entry
        out_score[p] = 0.0;
        out_bias[p] = 0.0;
        out_state[p] = -1;
        out_ntok[p] = 0;
        return;
    }
    const int32_t* row = tok + (size_t)p * ld;
    int st = g.start;
    double bias = 0.0;
    for (int j = 0; j < n; ++j) {
        st = ngram_chain(g, row[j], st, bias);
        bias = bias + g.ins;
    }
    double score = bias;
    if (has_eos) (void)ngram_chain(g, eos, st, score);
    out_score[p] = score;
    out_bias[p] = bias;
    out_state[p] = st;
    out_ntok[p] = n;
}

// ---- the sweep --------------------------------------------------------------------------------------------------------------------------
constexpr int RS_MAX_K = ASR_RESCORE_MAX_K;

__device__ __forceinline__ bool rs_finite(double x) { return x - x == 0.0; }      // false for NaN and both infinities

__device__ __forceinline__ long long rs_wave_sum(long long v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// PRECONDITION of rs_wave_sum: the whole wave executes it - a lane past U stays and adds zeros.
__global__ __launch_bounds__(64) void nbest_sweep_kernel(const double* __restrict__ feat, const int32_t* __restrict__ len, const int32_t* __restrict__ err,
                                                         const double* __restrict__ grid, int U, int N, int K, int nb, int32_t* __restrict__ out_pick,
                                                         double* __restrict__ out_total, long long* __restrict__ ws) {
    const int g = blockIdx.x / nb, ub = blockIdx.x - g * nb, lane = threadIdx.x;
    const int u = ub * 64 + lane;
    const bool on = u < U;
    const int uu = on ? u : U - 1;      // a lane past U reads its neighbour's values and writes nothing
    double w[RS_MAX_K];
#pragma unroll
    for (int k = 0; k < RS_MAX_K; ++k) w[k] = k < K ? grid[(size_t)g * K + k] : 0.0;      // wave-uniform: scalar loads
    bool have = false;
    double best = 0.0;
    int pick = -1, first = -1;
    for (int e = 0; e < N; ++e) {
        const bool present = len[(size_t)e * U + uu] >= 0;
        bool scorable = true;
        double total = 0.0;
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int k = 0; k < RS_MAX_K; ++k) {
                if (k < K && w[k] != 0.0) {      // wave-uniform: a zero weight's plane is not read
                    const double f = feat[((size_t)k * N + e) * U + uu];
                    if (!rs_finite(f)) scorable = false;
                    const double t = w[k] * f;
                    total = total + t;
                }
            }
        }
        const bool ok = present && scorable;
        if (present && first < 0) first = e;
        if (ok && (!have || total > best)) {
            have = true;
            best = total;
            pick = e;
        }
        if (out_total && on) out_total[((size_t)g * U + u) * N + e] = ok ? total : -INFINITY;
    }
    if (pick < 0) pick = max(first, 0);      // nothing scorable: the first present entry (the launcher refused a list without one)
    long long s = 0, d = 0, i = 0, wr = 0;
    if (on) {
        out_pick[(size_t)g * U + u] = pick;
        s = err[((size_t)0 * N + pick) * U + u];
        d = err[((size_t)1 * N + pick) * U + u];
        i = err[((size_t)2 * N + pick) * U + u];
        wr = s + d + i > 0;
    }
    s = rs_wave_sum(s);
    d = rs_wave_sum(d);
    i = rs_wave_sum(i);
    wr = rs_wave_sum(wr);
    if (lane == 0) {
        long long* o = ws + ((size_t)g * nb + ub) * 4;
        o[0] = s;
        o[1] = d;
        o[2] = i;
        o[3] = wr;
    }
}

// one wave per grid point: lane l adds the partials of blocks l, l + 64, ... (a lane-per-total loop of nb dependent-latency loads took
// 33 us at nb = 113), then four wave sums.  The whole wave stays (rs_wave_sum's precondition): g is the workgroup's.
__global__ __launch_bounds__(64) void nbest_sweep_sum_kernel(const long long* __restrict__ ws, int nb, long long* __restrict__ out_tot) {
    const int g = blockIdx.x, lane = threadIdx.x;
    long long s[4] = {0, 0, 0, 0};
    for (int b = lane; b < nb; b += 64) {
        const long long* p = ws + ((size_t)g * nb + b) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += p[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] = rs_wave_sum(s[c]);
    if (lane < 4) out_tot[(size_t)g * 4 + lane] = lane == 0 ? s[0] : lane == 1 ? s[1] : lane == 2 ? s[2] : s[3];
}

size_t sweep_ws_bytes(int U, int G) { return (size_t)G * (size_t)((U + 63) / 64) * 4 * sizeof(long long); }

const char* sweep_shape_check(int U, int N, int K, int G) {
    if (U < 1 || U > ASR_RESCORE_MAX_U) return "U outside [1, ASR_RESCORE_MAX_U]";
    if (N < 1 || N > ASR_RESCORE_MAX_N) return "N outside [1, ASR_RESCORE_MAX_N]";
    if (K < 1 || K > ASR_RESCORE_MAX_K) return "K outside [1, ASR_RESCORE_MAX_K]";
    if (G < 1 || G > ASR_RESCORE_MAX_G) return "G outside [1, ASR_RESCORE_MAX_G]";
    return nullptr;
}

}  // namespace

extern "C" int asr_lm_score_nbest(const int32_t* tok, const int32_t* len, const int32_t* host_len, int P, int ld, const asr_ngram_lm* lm, int has_eos,
                                  int eos, double* out_score, double* out_bias, int32_t* out_state, int32_t* out_ntok, void* stream) {
    const char* name = "asr_lm_score_nbest";
    if (!tok || !len || !host_len || !out_score || !out_bias || !out_state || !out_ntok) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if ((((uintptr_t)tok | (uintptr_t)len | (uintptr_t)host_len | (uintptr_t)out_state | (uintptr_t)out_ntok) % 4) || (((uintptr_t)out_score | (uintptr_t)out_bias) % 8))
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (int32 arrays: 4 bytes, out_score / out_bias: 8)", name);
    if (P <= 0) ASR_FAIL(ASR_EINVAL, "%s: P=%d hypotheses", name, P);
    if (ld < 0) ASR_FAIL(ASR_EINVAL, "%s: ld=%d", name, ld);
    const NgramLm g = ngram_lm_of(lm);
    if (const char* why = lm ? ngram_lm_check(g) : "null LM") ASR_FAIL(ASR_EINVAL, "%s: %s", name, why);
    for (int p = 0; p < P; ++p) {
        if (host_len[p] < -1) ASR_FAIL(ASR_EINVAL, "%s: hypothesis %d has length %d (-1 = absent)", name, p, host_len[p]);
        if (host_len[p] > ld) ASR_FAIL(ASR_EINVAL, "%s: hypothesis %d has %d tokens, the rows are ld=%d apart", name, p, host_len[p], ld);
    }
    lm_score_nbest_kernel<<<dim3((P + 63) / 64), WAVE, 0, (hipStream_t)stream>>>(tok, len, P, ld, g, has_eos != 0, eos, out_score, out_bias, out_state, out_ntok);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}

extern "C" size_t asr_nbest_sweep_workspace_bytes(int U, int N, int K, int G) {
    if (const char* why = sweep_shape_check(U, N, K, G)) {
        asr_set_error("asr_nbest_sweep_workspace_bytes: %s (U=%d N=%d K=%d G=%d)", why, U, N, K, G);
        return 0;
    }
    return sweep_ws_bytes(U, G);
}

extern "C" int asr_nbest_sweep(const double* feat, const int32_t* len, const int32_t* err, const double* grid, const double* host_feat,
                               const int32_t* host_len, const double* host_grid, int U, int N, int K, int G, int32_t* out_pick, int64_t* out_tot,
                               double* out_total, void* ws, size_t ws_bytes, void* stream) {
    const char* name = "asr_nbest_sweep";
    if (!feat || !len || !err || !grid || !host_feat || !host_len || !host_grid || !out_pick || !out_tot || !ws) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if ((((uintptr_t)len | (uintptr_t)err | (uintptr_t)host_len | (uintptr_t)out_pick) % 4) ||
        (((uintptr_t)feat | (uintptr_t)grid | (uintptr_t)host_feat | (uintptr_t)host_grid | (uintptr_t)out_tot | (uintptr_t)out_total | (uintptr_t)ws) % 8))
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (int32 arrays: 4 bytes, fp64 / int64 arrays and ws: 8)", name);
    if (const char* why = sweep_shape_check(U, N, K, G)) ASR_FAIL(ASR_EINVAL, "%s: %s (U=%d N=%d K=%d G=%d)", name, why, U, N, K, G);
    for (size_t i = 0; i < (size_t)G * K; ++i)
        if (host_grid[i] - host_grid[i] != 0.0) ASR_FAIL(ASR_EINVAL, "%s: weight %d of grid point %d is not finite", name, (int)(i % K), (int)(i / K));
    for (size_t i = 0; i < (size_t)K * N * U; ++i) {
        const double f = host_feat[i];
        if (f != f || f == INFINITY)
            ASR_FAIL(ASR_EINVAL, "%s: feature %d of entry %d of utterance %d is NaN or +inf", name, (int)(i / ((size_t)N * U)), (int)(i / U % N), (int)(i % U));
    }
    for (int u = 0; u < U; ++u) {
        bool any = false;
        for (int e = 0; e < N && !any; ++e) any = host_len[(size_t)e * U + u] >= 0;
        if (!any) ASR_FAIL(ASR_EINVAL, "%s: utterance %d has no present entry", name, u);
    }
    const size_t need = sweep_ws_bytes(U, G);
    if (ws_bytes < need) ASR_FAIL(ASR_EWORKSPACE, "%s: workspace of %zu bytes, asr_nbest_sweep_workspace_bytes says %zu", name, ws_bytes, need);
    const int nb = (U + 63) / 64;
    nbest_sweep_kernel<<<dim3((unsigned)G * (unsigned)nb), WAVE, 0, (hipStream_t)stream>>>(feat, len, err, grid, U, N, K, nb, out_pick, out_total, (long long*)ws);
    ASR_CHECK_LAUNCH(name);
    nbest_sweep_sum_kernel<<<dim3(G), WAVE, 0, (hipStream_t)stream>>>((const long long*)ws, nb, (long long*)out_tot);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}
