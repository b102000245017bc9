// Token confidence and streamed token times from the CTC posteriors (asr_chinese_e2e_amd/confidence.py; definitions: tests/confidence_ref.py).
//   asr_ctc_frame_stats          per frame: best class, log p(best), log p(blank), log-sum-exp and the normalised entropy confidence
//   asr_ctc_token_conf           per aligned token (asr_ctc_align's spans): {post_max, post_min, post_mean, ent_mean, ent_min}
//   asr_session_ctc_step_tokens  asr_session_ctc_step, and per slot the runs of the greedy path that closed in this tick (id, first and
//                                last frame, the five measures) and the run that is still open
// A token's sums are fp32, started at 0.f, and take its frames one at a time in ascending order - in the offline kernel and in the
// streamed one, whose open run carries them across ticks - so a token's measures do not depend on how the audio was cut.
#include "asr_common.h"

namespace {

// One wave per frame: frame_best_blank_kernel's two passes (its argmax pass, its order of the sum of exponentials - path and blank_lp have
// that kernel's bits), the second pass also summing u = sum (x - m) e^(x - m): H = ln s - u / s.  A class whose exponential is 0 (a -inf
// logit, an underflow) adds nothing to u: (-inf) * 0 is never formed.
template <typename T>
__global__ __launch_bounds__(256) void frame_stats_kernel(const T* __restrict__ logits, const int32_t* __restrict__ in_len, int32_t* __restrict__ path,
                                                          float* __restrict__ best_lp, float* __restrict__ blank_lp, float* __restrict__ lse_out,
                                                          float* __restrict__ ent, int B, int T_, int V, int ld, int blank) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rows = B * T_;
    const float ln_v = logf((float)V);
    for (int row = blockIdx.x * 4 + w; row < rows; row += gridDim.x * 4) {
        const int b = row / T_, t = row - b * T_;
        if (in_len && t >= in_len[b]) {      // wave-uniform
            if (lane == 0) { path[row] = blank; best_lp[row] = 0.f; blank_lp[row] = 0.f; lse_out[row] = 0.f; ent[row] = 0.f; }
            continue;
        }
        const T* x = logits + (size_t)row * ld;
        float best = -INFINITY;
        int bi = 0x7fffffff;
        bool vec = false;
        if constexpr (sizeof(T) == 2) vec = V % 8 == 0 && ((uintptr_t)x % 16) == 0;
        if (vec) {
            const int nvec = V >> 3;
            for (int k = lane; k < nvec; k += 64) {   // ascending index inside a lane: strict > keeps the first maximum
                const u32x4 q = *(const u32x4*)(x + (size_t)k * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float lo = bf16_lo(q[j]), hi = bf16_hi(q[j]);
                    if (lo > best) { best = lo; bi = k * 8 + 2 * j; }
                    if (hi > best) { best = hi; bi = k * 8 + 2 * j + 1; }
                }
            }
        } else {
            for (int i = lane; i < V; i += 64) {
                const float v = to_f32<T>(x[i]);
                if (v > best) { best = v; bi = i; }
            }
        }
        wave_argmax_first(best, bi);
        const float m = best;
        float s = 0.f, u = 0.f;
        for (int i = lane; i < V; i += 64) {
            const float d = to_f32<T>(x[i]) - m;
            const float e = expf(d);
            s += e;
            if (e > 0.f) u += d * e;
        }
        s = wave_sum(s);
        u = wave_sum(u);
        const float lse = m + logf(s);
        if (lane == 0) {
            const float h = logf(s) - u / s;
            path[row] = bi;
            best_lp[row] = m - lse;
            blank_lp[row] = to_f32<T>(x[blank]) - lse;
            lse_out[row] = lse;
            ent[row] = fminf(1.f, fmaxf(0.f, 1.f - h / ln_v));
        }
    }
}

// the five measures of a token from its running sums over n >= 1 frames
struct Measures { float post_max, post_min, post_mean, ent_mean, ent_min; };
__device__ __forceinline__ Measures token_measures(int n, float lp_sum, float lp_max, float lp_min, float ent_sum, float ent_min) {
    const float fn = (float)n;
    return {expf(lp_max), expf(lp_min), expf(lp_sum / fn), ent_sum / fn, ent_min};
}

// One wave per utterance, a lane per token (tokens lane, lane + 64, ...), each walking its span's frames in ascending order.
template <typename T>
__global__ __launch_bounds__(64) void token_conf_kernel(const T* __restrict__ logits, const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_len,
                                                        const int32_t* __restrict__ spans, const float* __restrict__ lse, const float* __restrict__ ent,
                                                        float* __restrict__ out, int T_, int V, int ld, int Lmax) {
    const int b = blockIdx.x;
    const int L = max(0, min(lab_len[b], Lmax));
    for (int l = threadIdx.x; l < Lmax; l += 64) {
        float* o = out + ((size_t)b * Lmax + l) * 5;
        if (l >= L) {
#pragma unroll
            for (int k = 0; k < 5; ++k) o[k] = 0.f;
            continue;
        }
        const int y = labels[(size_t)b * Lmax + l];
        const int s0 = spans[((size_t)b * Lmax + l) * 2], s1 = spans[((size_t)b * Lmax + l) * 2 + 1];
        if (s0 < 0 || s1 < s0 || s1 >= T_ || y < 0 || y >= V) {      // not aligned (an infeasible utterance), or not a span of these frames
#pragma unroll
            for (int k = 0; k < 5; ++k) o[k] = NAN;
            continue;
        }
        float lp_sum = 0.f, lp_max = -INFINITY, lp_min = INFINITY, ent_sum = 0.f, ent_min = INFINITY;
        for (int t = s0; t <= s1; ++t) {
            const size_t row = (size_t)b * T_ + t;
            const float lp = to_f32<T>(logits[row * ld + y]) - lse[row];
            const float en = ent[row];
            lp_sum += lp;
            lp_max = fmaxf(lp_max, lp);
            lp_min = fminf(lp_min, lp);
            ent_sum += en;
            ent_min = fminf(ent_min, en);
        }
        const Measures q = token_measures(s1 - s0 + 1, lp_sum, lp_max, lp_min, ent_sum, ent_min);
        o[0] = q.post_max; o[1] = q.post_min; o[2] = q.post_mean; o[3] = q.ent_mean; o[4] = q.ent_min;
    }
}

constexpr int REC = 8;      // words of a run's record: id, first frame, last frame, the five measures

__device__ __forceinline__ void run_record(int32_t* __restrict__ r, int cls, int start, int count, float lp_sum, float lp_max, float lp_min, float ent_sum,
                                           float ent_min) {
    r[0] = cls; r[1] = start; r[2] = start + count - 1;
    const Measures q = token_measures(count, lp_sum, lp_max, lp_min, ent_sum, ent_min);
    r[3] = __float_as_int(q.post_max); r[4] = __float_as_int(q.post_min); r[5] = __float_as_int(q.post_mean);
    r[6] = __float_as_int(q.ent_mean); r[7] = __float_as_int(q.ent_min);
}

// One wave per slot.  The ids and counters are session_ctc_step_kernel's, statement by statement.  The runs are walked frame by frame, 64
// frames per trip held one per lane and handed round by v_readlane: every lane follows the same run (wave-uniform), lane 0 writes.
// run (slots, 8) = {class (blank: no open run), first frame, frames, sum / max / min of lp, sum / min of ent} (floats as their bits).
// out (slots, 13 + 9 C) = {session_ctc_step's 4 + C words, runs closed, C records, the open run's record (id -1: none)}.
__global__ __launch_bounds__(64) void session_ctc_step_tokens_kernel(const int32_t* __restrict__ path, const float* __restrict__ blank_lp,
                                                                     const float* __restrict__ best_lp, const float* __restrict__ ent,
                                                                     const int32_t* __restrict__ n_valid, const int32_t* __restrict__ reset,
                                                                     int32_t* __restrict__ state, int32_t* __restrict__ run, int32_t* __restrict__ out, int C,
                                                                     int blank, float silence_lp) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int32_t* st = state + (size_t)b * 4;
    int32_t* rn = run + (size_t)b * REC;
    int32_t* o = out + (size_t)b * (13 + 9 * (size_t)C);
    int32_t* recs = o + 5 + C;
    const bool fresh = reset[b] != 0;
    int last = fresh ? blank : st[0], trailing = fresh ? 0 : st[1], frames = fresh ? 0 : st[2], decoded = fresh ? 0 : st[3];
    int r_cls = fresh ? blank : rn[0], r_start = fresh ? 0 : rn[1], r_count = fresh ? 0 : rn[2];
    float r_lp_sum = fresh ? 0.f : __int_as_float(rn[3]), r_lp_max = fresh ? 0.f : __int_as_float(rn[4]), r_lp_min = fresh ? 0.f : __int_as_float(rn[5]);
    float r_ent_sum = fresh ? 0.f : __int_as_float(rn[6]), r_ent_min = fresh ? 0.f : __int_as_float(rn[7]);
    const int n = max(0, min(n_valid[b], C));
    int n_out = 0, n_closed = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane, here = min(64, n - t0);
        const bool live = t < n;
        const size_t row = (size_t)b * C + (live ? t : 0);
        const int cur = live ? path[row] : blank;
        int left = __shfl_up(cur, 1, 64);
        if (lane == 0) left = last;
        const bool keep = live && cur != blank && cur != left;
        const unsigned long long m = __ballot(keep);
        if (keep) o[4 + n_out + __popcll(m & ((1ull << lane) - 1ull))] = cur;
        n_out += __popcll(m);
        last = __shfl(cur, here - 1, 64);
        const bool speech = live && !(blank_lp[row] > silence_lp);
        const unsigned long long sp = __ballot(speech);
        if (sp == 0ull) trailing += here;
        else trailing = here - 1 - (63 - __builtin_clzll(sp));
        // the runs: frame j of this trip is session frame frames + t0 + j
        const float lp = best_lp[row], en = ent[row];
        for (int j = 0; j < here; ++j) {
            const int c = __shfl(cur, j, 64);
            const float lp_j = __shfl(lp, j, 64), en_j = __shfl(en, j, 64);
            if (c == r_cls) {
                if (c != blank) {
                    r_count += 1;
                    r_lp_sum += lp_j; r_lp_max = fmaxf(r_lp_max, lp_j); r_lp_min = fminf(r_lp_min, lp_j);
                    r_ent_sum += en_j; r_ent_min = fminf(r_ent_min, en_j);
                }
                continue;
            }
            if (r_cls != blank) {      // the open run ends in front of this frame; n_closed < C: every closing takes a frame of this tick
                if (lane == 0) run_record(recs + (size_t)n_closed * REC, r_cls, r_start, r_count, r_lp_sum, r_lp_max, r_lp_min, r_ent_sum, r_ent_min);
                n_closed += 1;
            }
            r_cls = c;
            if (c != blank) {
                r_start = frames + t0 + j; r_count = 1;
                r_lp_sum = 0.f + lp_j; r_lp_max = lp_j; r_lp_min = lp_j;
                r_ent_sum = 0.f + en_j; r_ent_min = en_j;
            }
        }
    }
    frames += n;
    if (n_out > 0) decoded = 1;
    for (int i = n_out + lane; i < C; i += 64) o[4 + i] = 0;
    for (int i = n_closed * REC + lane; i < C * REC; i += 64) recs[i] = 0;
    if (lane == 0) {
        st[0] = last; st[1] = trailing; st[2] = frames; st[3] = decoded;
        o[0] = n_out; o[1] = trailing; o[2] = frames; o[3] = decoded;
        o[4 + C] = n_closed;
        int32_t* open_rec = recs + (size_t)C * REC;
        if (r_cls != blank) {
            run_record(open_rec, r_cls, r_start, r_count, r_lp_sum, r_lp_max, r_lp_min, r_ent_sum, r_ent_min);
        } else {
            open_rec[0] = -1;
#pragma unroll
            for (int k = 1; k < REC; ++k) open_rec[k] = 0;
            r_start = 0; r_count = 0; r_lp_sum = r_lp_max = r_lp_min = r_ent_sum = r_ent_min = 0.f;
        }
        rn[0] = r_cls; rn[1] = r_start; rn[2] = r_count;
        rn[3] = __float_as_int(r_lp_sum); rn[4] = __float_as_int(r_lp_max); rn[5] = __float_as_int(r_lp_min);
        rn[6] = __float_as_int(r_ent_sum); rn[7] = __float_as_int(r_ent_min);
    }
}

int logits_args(const char* name, const void* logits, int B, int T, int V, int ld, int dtype) {
    if (B <= 0 || T <= 0 || V <= 1 || (size_t)B * T > (size_t)INT_MAX) ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d T=%d V=%d", name, B, T, V);
    if (ld < V) ASR_FAIL(ASR_EINVAL, "%s: row stride ld=%d < V=%d", name, ld, V);
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "%s: dtype %d", name, dtype);
    if ((uintptr_t)logits % (dtype == ASR_F32 ? 4 : 2)) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    return ASR_OK;
}

}  // namespace

extern "C" int asr_ctc_frame_stats(const void* logits, const int32_t* in_len, int32_t* path, float* best_lp, float* blank_lp, float* lse, float* ent, int B,
                                   int T, int V, int ld, int blank, int dtype, void* stream) {
    if (!logits || !path || !best_lp || !blank_lp || !lse || !ent) ASR_FAIL(ASR_EINVAL, "asr_ctc_frame_stats: null pointer");
    const int rc = logits_args("asr_ctc_frame_stats", logits, B, T, V, ld, dtype);
    if (rc != ASR_OK) return rc;
    if (blank < 0 || blank >= V) ASR_FAIL(ASR_EINVAL, "asr_ctc_frame_stats: blank=%d outside [0, V=%d)", blank, V);
    if (((uintptr_t)in_len | (uintptr_t)path | (uintptr_t)best_lp | (uintptr_t)blank_lp | (uintptr_t)lse | (uintptr_t)ent) % 4)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_frame_stats: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    int g = ceil_div(B * T, 4);
    if (g > 4096) g = 4096;
    if (dtype == ASR_F32) frame_stats_kernel<float><<<g, 256, 0, st>>>((const float*)logits, in_len, path, best_lp, blank_lp, lse, ent, B, T, V, ld, blank);
    else frame_stats_kernel<bf16_t><<<g, 256, 0, st>>>((const bf16_t*)logits, in_len, path, best_lp, blank_lp, lse, ent, B, T, V, ld, blank);
    ASR_CHECK_LAUNCH("asr_ctc_frame_stats");
    return ASR_OK;
}

extern "C" int asr_ctc_token_conf(const void* logits, const int32_t* labels, const int32_t* lab_len, const int32_t* spans, const float* lse, const float* ent,
                                  float* out, int B, int T, int V, int ld, int Lmax, int dtype, void* stream) {
    if (!logits || !labels || !lab_len || !spans || !lse || !ent || !out) ASR_FAIL(ASR_EINVAL, "asr_ctc_token_conf: null pointer");
    const int rc = logits_args("asr_ctc_token_conf", logits, B, T, V, ld, dtype);
    if (rc != ASR_OK) return rc;
    if (Lmax <= 0 || Lmax > 255) ASR_FAIL(ASR_EINVAL, "asr_ctc_token_conf: Lmax = %d: 1 to 255 labels per utterance", Lmax);
    if (((uintptr_t)labels | (uintptr_t)lab_len | (uintptr_t)spans | (uintptr_t)lse | (uintptr_t)ent | (uintptr_t)out) % 4)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_token_conf: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ASR_F32) token_conf_kernel<float><<<B, 64, 0, st>>>((const float*)logits, labels, lab_len, spans, lse, ent, out, T, V, ld, Lmax);
    else token_conf_kernel<bf16_t><<<B, 64, 0, st>>>((const bf16_t*)logits, labels, lab_len, spans, lse, ent, out, T, V, ld, Lmax);
    ASR_CHECK_LAUNCH("asr_ctc_token_conf");
    return ASR_OK;
}

extern "C" int asr_session_ctc_step_tokens(const int32_t* path, const float* blank_lp, const float* best_lp, const float* ent, const int32_t* n_valid,
                                           const int32_t* reset, int32_t* state, int32_t* run, int32_t* out, int slots, int C, int blank, float silence_lp,
                                           void* stream) {
    if (!path || !blank_lp || !best_lp || !ent || !n_valid || !reset || !state || !run || !out) ASR_FAIL(ASR_EINVAL, "asr_session_ctc_step_tokens: null pointer");
    if (slots <= 0 || C <= 0 || blank < 0 || (size_t)slots * (13 + 9 * (size_t)C) > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "asr_session_ctc_step_tokens: bad shape slots=%d C=%d blank=%d", slots, C, blank);
    if (silence_lp != silence_lp) ASR_FAIL(ASR_EINVAL, "asr_session_ctc_step_tokens: the silence threshold is not a number");
    if (((uintptr_t)path | (uintptr_t)blank_lp | (uintptr_t)best_lp | (uintptr_t)ent | (uintptr_t)n_valid | (uintptr_t)reset | (uintptr_t)state | (uintptr_t)run |
         (uintptr_t)out) % 4)
        ASR_FAIL(ASR_EINVAL, "asr_session_ctc_step_tokens: misaligned pointer");
    session_ctc_step_tokens_kernel<<<slots, 64, 0, (hipStream_t)stream>>>(path, blank_lp, best_lp, ent, n_valid, reset, state, run, out, C, blank, silence_lp);
    ASR_CHECK_LAUNCH("asr_session_ctc_step_tokens");
    return ASR_OK;
}
