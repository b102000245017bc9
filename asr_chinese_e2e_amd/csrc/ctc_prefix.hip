// CTC prefix scoring for one-pass joint CTC / attention beam search (Watanabe et al. 2017, "Hybrid CTC/Attention Architecture for
// End-to-End Speech Recognition", section 3.2 and algorithm 2).  NOT in the reference (it has no CTC); the host restatement the
// tests check against is tests/joint_ref.py, pinned by brute-force enumeration of every frame path.
//
//   asr_ctc_prefix_logprobs   log_softmax of the CTC head, once per batch, transposed to (B, V, T) f32: a candidate's column over
//                             the frames is one contiguous read
//   asr_ctc_prefix_score      per step: for every (hypothesis g, attention candidate c) the forward variables of h = g + c, the
//                             prefix probability log psi(h), the joint candidate score, and per hypothesis the `beam` best
//                             candidates
//   asr_ctc_prefix_gather     every survivor takes the forward variables of the candidate it came from (parent, token)
//   asr_joint_beam_step       asr_beam_step for joint scores: drops -inf candidates, carries the attention and CTC parts, and
//                             adds the CTC end-of-sentence correction to the hypotheses that get eos appended at the last step
//
// State of a hypothesis g over its utterance's frames t < in_len[b], log domain, fp64, stored (T, R) (frame-major):
//   rb_t(g) = log r^b_t(g) (paths that end in a blank), rt_t(g) = log (r^n_t(g) + r^b_t(g)).  g = [sos] is not stored: its
//   r^n is -inf and rb_t = sum_{tau <= t} log y_tau(blank), which the step-0 launch accumulates on the fly.
#include "asr_common.h"

namespace {

// log(exp(a) + exp(b)): the larger term in fp64, the correction log1p(exp(-|a - b|)) in [0, ln 2] in fp32 (absolute error ~1e-7
// per call, against a tolerance of 1e-4 on the result; a full fp64 log1p / exp costs ~60 fp64 operations)
__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + (double)log1pf(expf((float)(fmin(a, b) - m)));
}

// 64 frames of one utterance per 256-thread workgroup: the log-sum-exp of each frame, then 64 x 64 tiles transposed through LDS so
// that both the reads (along the classes) and the writes (along the frames) are contiguous
template <typename T>
__global__ __launch_bounds__(256) void ctc_prefix_logprobs_kernel(const T* __restrict__ logits, float* __restrict__ lpT, int T_, int V, int ld) {
    ASR_FULL_WAVES(256);
    __shared__ float tile[64][65];
    __shared__ float s_lse[64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nblk = (T_ + 63) / 64;
    const int b = blockIdx.x / nblk, t0 = (blockIdx.x - b * nblk) * 64;
    for (int k = w; k < 64; k += 4) {                  // wave-uniform: t depends on k only
        const int t = t0 + k;
        float lse = 0.f;
        if (t < T_) {
            const T* x = logits + ((size_t)b * T_ + t) * ld;
            float m = -INFINITY;
            for (int i = lane; i < V; i += 64) m = fmaxf(m, to_f32<T>(x[i]));
            m = wave_max(m);
            float s = 0.f;
            for (int i = lane; i < V; i += 64) s += expf(to_f32<T>(x[i]) - m);
            s = wave_sum(s);
            lse = m + logf(s);                         // as asr_logsoftmax_topk
        }
        if (lane == 0) s_lse[k] = lse;
    }
    __syncthreads();
    for (int c0 = 0; c0 < V; c0 += 64) {
        for (int k = w; k < 64; k += 4) {              // frame t0 + k, class c0 + lane
            const int t = t0 + k, c = c0 + lane;
            tile[lane][k] = (t < T_ && c < V) ? to_f32<T>(logits[((size_t)b * T_ + t) * ld + c]) - s_lse[k] : 0.f;
        }
        __syncthreads();
        for (int k = w; k < 64; k += 4) {              // class c0 + k, frame t0 + lane
            const int t = t0 + lane, c = c0 + k;
            if (t < T_ && c < V) lpT[((size_t)b * V + c) * T_ + t] = tile[k][lane];
        }
        __syncthreads();
    }
}

// One lane per (hypothesis r, candidate j): 16 lanes per hypothesis (C <= 16), four hypotheses per wave.  The lane runs the two
// first-order recurrences of h = g + c over the utterance's frames:
//   phi_t = rb_t(g) if c == last(g) else rt_t(g)
//   r^n_0(h) = log y_0(c) if g = [sos] else -inf,  r^b_0(h) = -inf
//   r^n_t(h) = (r^n_{t-1}(h) (+) phi_{t-1}) + log y_t(c),  r^b_t(h) = (r^b_{t-1}(h) (+) r^n_{t-1}(h)) + log y_t(blank)
//   log psi(h) = r^n_0(h) (+) sum(+)_{t >= 1} (phi_{t-1} + log y_t(c))
template <int G>
__global__ __launch_bounds__(256) void ctc_prefix_score_kernel(const float* __restrict__ lpT, const int32_t* __restrict__ in_len,
                                                               const double* __restrict__ st_rb, const double* __restrict__ st_rt,
                                                               const float* __restrict__ hyp_psi, const int32_t* __restrict__ last_tok,
                                                               const int32_t* __restrict__ alive, const float* __restrict__ att_vals,
                                                               const int32_t* __restrict__ att_ids, double* __restrict__ cand_rb,
                                                               double* __restrict__ cand_rt, float* __restrict__ out_vals, int32_t* __restrict__ out_ids,
                                                               float* __restrict__ out_att, float* __restrict__ out_psi, float* __restrict__ out_full,
                                                               int B, int T_, int V, int beam, int C, int step, float lam, int eos, int blank) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = gid / G, j = gid - r * G;
    const int R = B * beam;
    if (r >= R) return;                                // whole groups of G lanes leave together
    const int b = r / beam;
    const int Tb = min(max(in_len[b], 0), T_);
    const bool sos = step == 0;
    const bool live = alive[r] != 0;
    const bool cand = j < C;
    const int c = cand ? att_ids[(size_t)r * C + j] : -1;
    const float att = cand ? att_vals[(size_t)r * C + j] : -INFINITY;
    const size_t RC = (size_t)R * C, col = (size_t)r * C + j;
    double psi = -INFINITY, full = -INFINITY;
    if (live && cand && c >= 0 && c < V && c != blank) {
        if (c == eos && !sos) {
            psi = Tb > 0 ? st_rt[(size_t)(Tb - 1) * R + r] : -INFINITY;      // log p_ctc(g): every path of the frames spells g
        } else if (c == eos && Tb == 0) {
            psi = 0.0;                                                       // [sos] over no frames: the empty labelling, probability 1
        } else {
            const bool ext = c != eos;                                       // eos after [sos] only needs g's rt at the last frame
            const int last = sos ? -1 : last_tok[r];
            const float* xc = lpT + ((size_t)b * V + (ext ? c : blank)) * T_;
            const float* xb = lpT + ((size_t)b * V + blank) * T_;
            double rn = -INFINITY, rb = -INFINITY, ps = -INFINITY;
            double g_rb = 0.0, g_rt = 0.0;                                   // state of g at the previous frame
            // frames in chunks of PF: the chunk's inputs are loaded before its recurrence steps run, so that one step waits for
            // the log-adds of the previous one and not for a memory round trip
            constexpr int PF = 8;
            for (int t0 = 0; t0 < Tb; t0 += PF) {
                float xs[PF], ybs[PF];
                double grb[PF], grt[PF];
#pragma unroll
                for (int k = 0; k < PF; ++k) {
                    const int t = min(t0 + k, Tb - 1);                      // clamped: the loads stay inside the utterance
                    xs[k] = xc[t];
                    ybs[k] = xb[t];
                    grb[k] = sos ? 0.0 : st_rb[(size_t)t * R + r];
                    grt[k] = sos ? 0.0 : st_rt[(size_t)t * R + r];
                }
#pragma unroll
                for (int k = 0; k < PF; ++k) {
                    const int t = t0 + k;
                    if (t < Tb) {
                        const double x = (double)xs[k], yb = (double)ybs[k];
                        double n_rb, n_rt;                                   // state of g at frame t
                        if (sos) {
                            n_rb = (t == 0 ? 0.0 : g_rb) + yb;
                            n_rt = n_rb;
                        } else {
                            n_rb = grb[k];
                            n_rt = grt[k];
                        }
                        if (ext) {
                            if (t == 0) {
                                rn = sos ? x : -INFINITY;
                                ps = rn;
                            } else {
                                const double phi = c == last ? g_rb : g_rt;
                                const double nrn = lse2(rn, phi) + x;
                                const double nrb = lse2(rb, rn) + yb;
                                ps = lse2(ps, phi + x);
                                rn = nrn;
                                rb = nrb;
                            }
                            cand_rb[(size_t)t * RC + col] = rb;
                            cand_rt[(size_t)t * RC + col] = lse2(rn, rb);
                        }
                        g_rb = n_rb;
                        g_rt = n_rt;
                    }
                }
            }
            if (ext) {
                psi = ps;
                full = Tb > 0 ? lse2(rn, rb) : -INFINITY;
            } else {
                psi = g_rt;
            }
        }
    }
    float v = -INFINITY;
    if (live && cand && psi > -INFINITY) {
        const double psi_g = sos ? 0.0 : (double)hyp_psi[r];
        v = (float)((lam < 1.f ? (1.0 - (double)lam) * (double)att : 0.0) + (double)lam * (psi - psi_g));
    }
    // stable rank inside the hypothesis' group: larger joint score first, ties by the lower candidate index (lanes j >= C hold -inf
    // and the highest indices, so they rank after every candidate)
    int rank = 0;
    for (int o = 0; o < G; ++o) {
        const float vo = __shfl(v, o, G);
        if (vo > v || (vo == v && o < j)) ++rank;
    }
    if (cand && rank < beam) {
        const size_t k = (size_t)r * beam + rank;
        out_vals[k] = v;
        out_ids[k] = c;
        out_att[k] = att;
        out_psi[k] = (float)psi;
        out_full[k] = (float)full;
    }
}

// survivor r (alive after the step) <- the candidate of its parent p = b*beam + parent[r] whose token is last_tok[r]
__global__ __launch_bounds__(256) void ctc_prefix_gather_kernel(const double* __restrict__ cand_rb, const double* __restrict__ cand_rt,
                                                                double* __restrict__ st_rb, double* __restrict__ st_rt, const int32_t* __restrict__ parent,
                                                                const int32_t* __restrict__ last_tok, const int32_t* __restrict__ alive,
                                                                const int32_t* __restrict__ att_ids, const int32_t* __restrict__ in_len,
                                                                int B, int T_, int beam, int C) {
    const int r = blockIdx.y;
    if (!alive[r]) return;
    const int b = r / beam, p = b * beam + parent[r], tok = last_tok[r];
    int j = -1;
    for (int k = 0; k < C; ++k)
        if (att_ids[(size_t)p * C + k] == tok) { j = k; break; }    // the top-C ids of a row are distinct
    if (j < 0) return;
    const size_t R = (size_t)B * beam, RC = R * C, col = (size_t)p * C + j;
    const int Tb = min(max(in_len[b], 0), T_);
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < Tb; t += gridDim.x * blockDim.x) {
        st_rb[(size_t)t * R + r] = cand_rb[(size_t)t * RC + col];
        st_rt[(size_t)t * R + r] = cand_rt[(size_t)t * RC + col];
    }
}

// one 64-lane workgroup per utterance; beam * beam <= 64.  asr_beam_step's merge (stable rank of score(g) + joint increment) with
// -inf candidates dropped instead of kept, and per slot the accumulated attention score and the CTC prefix score
__global__ __launch_bounds__(64) void joint_beam_step_kernel(const float* __restrict__ top_vals, const int32_t* __restrict__ top_ids,
                                                             const float* __restrict__ top_att, const float* __restrict__ top_psi,
                                                             const float* __restrict__ top_full, float* __restrict__ score, float* __restrict__ att_sc,
                                                             float* __restrict__ ctc_sc, int32_t* __restrict__ alive, int32_t* __restrict__ last_tok,
                                                             int32_t* __restrict__ parent, int32_t* __restrict__ rec_tok, int32_t* __restrict__ rec_par,
                                                             int32_t* __restrict__ rec_end, float* __restrict__ rec_score, float* __restrict__ rec_att,
                                                             float* __restrict__ rec_ctc, const int32_t* __restrict__ maxlen,
                                                             int32_t* __restrict__ alive_total, int B, int beam, int step, int eos, float lam) {
    const int b = blockIdx.x, c = threadIdx.x;
    const int h = c / beam, j = c - h * beam;
    const size_t ci = (size_t)(b * beam + h) * beam + j;
    const float inc = c < beam * beam ? top_vals[ci] : -INFINITY;
    const bool valid = c < beam * beam && alive[b * beam + h] != 0 && step < maxlen[b] && inc > -INFINITY;
    const float cs = valid ? score[b * beam + h] + inc : -INFINITY;
    int rank = 0;
    for (int o = 0; o < 64; ++o) {
        const float so = __shfl(cs, o, 64);
        const int vo = __shfl((int)valid, o, 64);
        if (vo && (so > cs || (so == cs && o < c))) ++rank;
    }
    const bool keep = valid && rank < beam;
    const int tok = keep ? top_ids[ci] : 0;
    const float att = keep ? att_sc[b * beam + h] + top_att[ci] : 0.f;
    const float psi = keep ? top_psi[ci] : 0.f;
    const float full = keep ? top_full[ci] : 0.f;
    const bool last = step == maxlen[b] - 1;
    __syncthreads();   // every lane has read the old state
    if (c < beam) {
        const size_t rec = ((size_t)step * B + b) * beam + c;
        alive[b * beam + c] = 0;
        parent[b * beam + c] = c;
        rec_tok[rec] = 0;
        rec_par[rec] = 0;
        rec_end[rec] = 0;
        rec_score[rec] = -INFINITY;
        rec_att[rec] = -INFINITY;
        rec_ctc[rec] = -INFINITY;
    }
    __syncthreads();
    if (keep) {
        const int kslot = rank;
        const size_t rec = ((size_t)step * B + b) * beam + kslot;
        // eos ends a hypothesis (its psi is already log p_ctc(g)); at the last step every other survivor gets eos appended, and
        // its CTC part becomes the full-sequence probability log p_ctc(h) instead of the prefix probability
        const int end = tok == eos ? 1 : (last ? 2 : 0);
        const float ctc = end == 2 ? full : psi;
        const float s = end == 2 ? cs + lam * (full - psi) : cs;
        score[b * beam + kslot] = s;
        att_sc[b * beam + kslot] = att;
        ctc_sc[b * beam + kslot] = ctc;
        last_tok[b * beam + kslot] = tok;
        parent[b * beam + kslot] = h;
        alive[b * beam + kslot] = end ? 0 : 1;
        rec_tok[rec] = tok;
        rec_par[rec] = h;
        rec_end[rec] = end;
        rec_score[rec] = s;
        rec_att[rec] = att;
        rec_ctc[rec] = ctc;
        if (!end) atomicAdd(alive_total, 1);
    }
}

}  // namespace

extern "C" int asr_ctc_prefix_logprobs(const void* logits, float* lpT, int B, int T, int V, int ld, int dtype, void* stream) {
    if (!logits || !lpT) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_logprobs: null pointer");
    if (B <= 0 || T <= 0 || V <= 0 || ld < V) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_logprobs: bad shape B=%d T=%d V=%d ld=%d", B, T, V, ld);
    hipStream_t st = (hipStream_t)stream;
    const int grid = B * ceil_div(T, 64);
    if (dtype == ASR_F32) ctc_prefix_logprobs_kernel<float><<<grid, 256, 0, st>>>((const float*)logits, lpT, T, V, ld);
    else if (dtype == ASR_BF16) ctc_prefix_logprobs_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)logits, lpT, T, V, ld);
    else ASR_FAIL(ASR_EDTYPE, "asr_ctc_prefix_logprobs: dtype %d", dtype);
    ASR_CHECK_LAUNCH("asr_ctc_prefix_logprobs");
    return ASR_OK;
}

extern "C" int asr_ctc_prefix_score(const float* lpT, const int32_t* in_len, const double* st_rb, const double* st_rt, const float* hyp_psi,
                                    const int32_t* last_tok, const int32_t* alive, const float* att_vals, const int32_t* att_ids, double* cand_rb,
                                    double* cand_rt, float* out_vals, int32_t* out_ids, float* out_att, float* out_psi, float* out_full, int B, int T,
                                    int V, int beam, int C, int step, float ctc_weight, int eos, int blank, void* stream) {
    if (!lpT || !in_len || !alive || !att_vals || !att_ids || !cand_rb || !cand_rt || !out_vals || !out_ids || !out_att || !out_psi || !out_full)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_score: null pointer");
    if (step > 0 && (!st_rb || !st_rt || !hyp_psi || !last_tok)) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_score: null state pointer at step %d", step);
    if (B <= 0 || T <= 0 || V <= 0 || beam <= 0 || C < beam || C > 16 || C > V || step < 0 || blank < 0 || blank >= V)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_score: bad shape B=%d T=%d V=%d beam=%d C=%d (beam <= C <= 16) step=%d", B, T, V, beam, C, step);
    if (!(ctc_weight > 0.f && ctc_weight <= 1.f)) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_score: ctc_weight %g outside (0, 1]", (double)ctc_weight);
    const int threads = B * beam * 16;
    ctc_prefix_score_kernel<16><<<ceil_div(threads, 256), 256, 0, (hipStream_t)stream>>>(lpT, in_len, st_rb, st_rt, hyp_psi, last_tok, alive, att_vals,
                                                                                        att_ids, cand_rb, cand_rt, out_vals, out_ids, out_att, out_psi,
                                                                                        out_full, B, T, V, beam, C, step, ctc_weight, eos, blank);
    ASR_CHECK_LAUNCH("asr_ctc_prefix_score");
    return ASR_OK;
}

extern "C" int asr_ctc_prefix_gather(const double* cand_rb, const double* cand_rt, double* st_rb, double* st_rt, const int32_t* parent,
                                     const int32_t* last_tok, const int32_t* alive, const int32_t* att_ids, const int32_t* in_len, int B, int T,
                                     int beam, int C, void* stream) {
    if (!cand_rb || !cand_rt || !st_rb || !st_rt || !parent || !last_tok || !alive || !att_ids || !in_len)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_gather: null pointer");
    if (B <= 0 || T <= 0 || beam <= 0 || C < beam || C > 16) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_gather: bad shape B=%d T=%d beam=%d C=%d", B, T, beam, C);
    const dim3 grid(ceil_div(T, 256), B * beam);
    ctc_prefix_gather_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(cand_rb, cand_rt, st_rb, st_rt, parent, last_tok, alive, att_ids, in_len, B, T, beam, C);
    ASR_CHECK_LAUNCH("asr_ctc_prefix_gather");
    return ASR_OK;
}

extern "C" int asr_joint_beam_step(const float* top_vals, const int32_t* top_ids, const float* top_att, const float* top_psi, const float* top_full,
                                   float* score, float* att_score, float* ctc_score, int32_t* alive, int32_t* last_tok, int32_t* parent, int32_t* rec_tok,
                                   int32_t* rec_par, int32_t* rec_end, float* rec_score, float* rec_att, float* rec_ctc, const int32_t* maxlen,
                                   int32_t* alive_total, int B, int beam, int step, int eos, float ctc_weight, void* stream) {
    if (!top_vals || !top_ids || !top_att || !top_psi || !top_full || !score || !att_score || !ctc_score || !alive || !last_tok || !parent || !rec_tok ||
        !rec_par || !rec_end || !rec_score || !rec_att || !rec_ctc || !maxlen || !alive_total)
        ASR_FAIL(ASR_EINVAL, "asr_joint_beam_step: null pointer");
    if (B <= 0 || beam <= 0 || beam * beam > 64 || step < 0) ASR_FAIL(ASR_EINVAL, "asr_joint_beam_step: bad shape B=%d beam=%d (beam <= 8) step=%d", B, beam, step);
    joint_beam_step_kernel<<<B, 64, 0, (hipStream_t)stream>>>(top_vals, top_ids, top_att, top_psi, top_full, score, att_score, ctc_score, alive, last_tok,
                                                             parent, rec_tok, rec_par, rec_end, rec_score, rec_att, rec_ctc, maxlen, alive_total, B, beam,
                                                             step, eos, ctc_weight);
    ASR_CHECK_LAUNCH("asr_joint_beam_step");
    return ASR_OK;
}
