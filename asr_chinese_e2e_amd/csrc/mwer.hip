// MWER training for the CTC head: the expected number of errors over an n-best list and its gradient with respect to the logits
// (include/asr_hip.h: asr_mwer_errors, asr_ctc_mwer_lattice, asr_ctc_mwer_grad; the definition is tests/mwer_ref.py).
//
//   loss = scale * sum_b risk_b,  risk_b = sum_i P_i e_i,  P_i = softmax_i log p(h_i | x) over the entries that take part
//   d loss / d x[b,t,v] = scale * sum_i c_i gamma_i(t, v),  c_i = P_i (e_i - risk_b)
// gamma_i(t, v) is the posterior that an alignment of h_i emits v at frame t.  d log p(h_i | x) / d x_t = gamma_i(t, .) - softmax(x_t) and
// sum_i c_i = 0, so the dense softmax terms cancel: per frame the gradient touches the blank and the tokens of the list, nothing else.
//
// 1. mwer_errors_kernel   one wave per (utterance, entry): the Levenshtein distance to the reference, lengths read on the device.
//                         The distance-only forward pass of edit_wave.h.
// 2. mwer_lse_kernel      one wave per frame: the log-sum-exp of the row in fp64.  It is common to all entries and cancels in P.
// 3. mwer_lattice_kernel  one workgroup per (utterance, entry), state s of the blank-augmented sequence on thread s.  The alpha recursion
//                         forward in time, the beta recursion backward, both in the LOG domain in fp64: no value can leave the range, so a
//                         long entry under blank-dominated posteriors never reads as infeasible and no fallback is needed.  The previous
//                         column lives in LDS (two buffers, one barrier per frame).  alpha goes to the workspace; the backward pass turns
//                         it into the state posteriors g[t][s] = exp(alpha + beta - lp - ll), f32, which is all the gradient needs.
// 4. mwer_post_kernel     one workgroup per utterance: P, risk, c from ll and err (one thread, entries ascending), then the token chains:
//                         slot k = (entry i, position j); a slot OWNS its token when no earlier slot of the utterance holds the same id,
//                         next[k] is the following slot with that id.  The gradient of a cell is the sum along its chain.
// 5. mwer_grad_kernel     one workgroup per frame.  Never reads the logits.  A thread per owned token walks its chain (entries ascending,
//                         positions ascending), one thread sums the blank states in the same order; no atomics, two runs write the same
//                         bytes.  accumulate = 0: the row is zeroed first; accumulate = 1: only the touched cells are read and rewritten.
//
// Ids are compared, never used as indices, except as a column < V of the logits / dlogits: an entry with an id outside [0, V) or equal to
// the blank takes part in nothing.  Every length read from the device is clamped to the shape the host stated.
#include "asr_common.h"
#include "edit_wave.h"

namespace {

constexpr int MWER_MAX_N = ASR_MWER_MAX_N;        // entries per list
constexpr int MWER_MAX_LEN = ASR_MWER_MAX_LEN;    // tokens per entry and per reference
constexpr double MWER_NEG_INF = -INFINITY;

__device__ __forceinline__ int mwer_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Workspace layout, in bytes from `ws` (16-byte aligned).  SS = 2 Lh + 1 states per lattice row.
struct MwerLayout {
    size_t lse, alpha, g, next, own, part, bytes;
};
__host__ __device__ __forceinline__ MwerLayout mwer_layout(int B, int N, int T, int Lh) {
    const size_t b = (size_t)B, n = (size_t)N, t = (size_t)T, ss = 2 * (size_t)Lh + 1;
    auto up = [](size_t v) { return (v + 15) / 16 * 16; };
    MwerLayout o;
    o.lse = 0;
    o.alpha = up(o.lse + b * t * sizeof(double));
    o.g = up(o.alpha + b * n * t * ss * sizeof(double));
    o.next = up(o.g + b * n * t * ss * sizeof(float));
    o.own = up(o.next + b * n * (size_t)Lh * sizeof(int32_t));
    o.part = up(o.own + b * n * (size_t)Lh * sizeof(int32_t));
    o.bytes = up(o.part + b * n * sizeof(int32_t));
    return o;
}

// ---------------------------------------------------------------------------------- 1. errors
__global__ __launch_bounds__(64) void mwer_errors_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len,
                                                         const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len,
                                                         int32_t* __restrict__ err, int32_t* __restrict__ flags, int N, int Lh, int ldn, int ldb,
                                                         int Lr, int ldr) {
    __shared__ int carryD[MWER_MAX_LEN + 1];
    const int b = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    const int n = hyp_len[(size_t)b * N + i];
    const int flag = n < 0 ? ASR_MWER_ABSENT : (n > Lh ? ASR_MWER_LONG : 0);      // wave-uniform
    int dist = 0;
    if (!flag) {
        const int m = mwer_clamp(ref_len[b], 0, Lr);
        EditSinkNone none;
        dist = edit_wave_forward(ref + (size_t)b * ldr, m, hyp + (size_t)b * ldb + (size_t)i * ldn, n, carryD, lane, none);
    }
    if (lane == 0) {
        err[(size_t)b * N + i] = dist;
        flags[(size_t)b * N + i] = flag;
    }
}

// ---------------------------------------------------------------------------------- 2. log-sum-exp of every frame
template <typename T>
__global__ __launch_bounds__(256) void mwer_lse_kernel(const T* __restrict__ logits, const int32_t* __restrict__ in_len, double* __restrict__ lse,
                                                       int B, int T_, int V, int ld) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long rows = (long long)B * T_;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < rows; row += (long long)gridDim.x * 4) {
        const int b = (int)(row / T_), t = (int)(row - (long long)b * T_);
        if (t >= mwer_clamp(in_len[b], 0, T_)) continue;      // wave-uniform
        const T* x = logits + (size_t)row * ld;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, to_f32<T>(x[v]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        double s = 0.0;
        for (int v = lane; v < V; v += 64) s += exp((double)to_f32<T>(x[v]) - (double)m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) lse[row] = (double)m + log(s);
    }
}

// ---------------------------------------------------------------------------------- 3. the lattice of one entry
__device__ __forceinline__ double mwer_lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    if (m == MWER_NEG_INF) return MWER_NEG_INF;
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

template <typename T>
__global__ __launch_bounds__(512) void mwer_lattice_kernel(const T* __restrict__ logits, const int32_t* __restrict__ in_len,
                                                           const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len,
                                                           double* __restrict__ ll_out, unsigned char* __restrict__ ws, MwerLayout o, int B, int T_,
                                                           int V, int ld, int N, int Lh, int ldn, int ldb, int blank) {
    __shared__ double col[2][512 + 4];      // the previous column at [s + 2]; [0], [1] and the entries past the last state stay -inf
    const int b = blockIdx.y, i = blockIdx.x, s = threadIdx.x, nthr = blockDim.x;
    const int SS = 2 * Lh + 1;
    const size_t e = (size_t)b * N + i;
    int32_t* part = (int32_t*)(ws + o.part);
    const int Tb = mwer_clamp(in_len[b], 0, T_);
    const int n_raw = hyp_len[e];
    bool ok = n_raw >= 0 && n_raw <= Lh && Tb > 0;      // uniform over the workgroup
    const int n = ok ? n_raw : 0;
    const int32_t* h = hyp + (size_t)b * ldb + (size_t)i * ldn;
    // ids and feasibility: thread j looks at token j (the workgroup has more than Lh threads)
    int bad = 0, rep = 0;
    if (s < n) {
        const int tk = h[s];
        bad = tk < 0 || tk >= V || tk == blank;
        rep = s > 0 && tk == h[s - 1];
    }
    const int nbad = __syncthreads_count(bad), nrep = __syncthreads_count(rep);
    ok = ok && nbad == 0 && n + nrep <= Tb;
    if (!ok) {
        if (s == 0) {
            ll_out[e] = MWER_NEG_INF;
            part[e] = 0;
        }
        return;
    }
    const int S = 2 * n + 1;
    const bool act = s < S, odd = s & 1;
    const int j = (s - 1) >> 1;                              // the token of an odd state
    const int tok = act && odd ? h[j] : blank;               // validated above: a column < V
    const bool skip_f = act && odd && j >= 1 && tok != h[j - 1];          // s - 2 -> s
    const bool skip_b = act && odd && j + 1 < n && tok != h[j + 1];       // s -> s + 2
    const T* x = logits + (size_t)b * T_ * ld + tok;
    const double* lse = (const double*)(ws + o.lse) + (size_t)b * T_;
    double* alpha = (double*)(ws + o.alpha) + e * T_ * SS + s;      // row t at alpha + t * SS (dereferenced by active threads only)
    float* g = (float*)(ws + o.g) + e * T_ * SS + s;
    for (int k = s; k < 2 * (512 + 4); k += nthr) (&col[0][0])[k] = MWER_NEG_INF;
    __syncthreads();
    // ---- forward
    double lp = (double)to_f32<T>(x[0]) - lse[0];
    double a = act && s <= 1 ? lp : MWER_NEG_INF;
    int c = 0;
    col[0][s + 2] = a;
    if (act) alpha[0] = a;
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
        lp = (double)to_f32<T>(x[(size_t)t * ld]) - lse[t];
        const double p0 = col[c][s + 2], p1 = col[c][s + 1], p2 = skip_f ? col[c][s] : MWER_NEG_INF;
        const double m = mwer_lse3(p0, p1, p2);
        a = act ? lp + m : MWER_NEG_INF;
        c ^= 1;
        col[c][s + 2] = a;
        if (act) alpha[(size_t)t * SS] = a;
        __syncthreads();
    }
    const double ll = mwer_lse3(col[c][S - 1 + 2], col[c][S - 2 + 2], MWER_NEG_INF);      // S = 1: [1] is -inf
    __syncthreads();      // every thread has read the last column
    if (!(ll > MWER_NEG_INF)) {      // -inf or NaN logits: the entry takes part in nothing (uniform: ll comes from LDS)
        if (s == 0) {
            ll_out[e] = MWER_NEG_INF;
            part[e] = 0;
        }
        return;
    }
    // ---- backward: beta_t(s) includes y_t(s) as alpha does, so the state posterior is alpha beta / (y p)
    double bt = act && (s == S - 1 || s == S - 2) ? lp : MWER_NEG_INF;      // lp is still frame Tb - 1
    c = 0;
    col[0][s + 2] = bt;
    if (act) g[(size_t)(Tb - 1) * SS] = (a == MWER_NEG_INF || bt == MWER_NEG_INF) ? 0.f : (float)exp(a + bt - lp - ll);
    __syncthreads();
    for (int t = Tb - 2; t >= 0; --t) {
        lp = (double)to_f32<T>(x[(size_t)t * ld]) - lse[t];
        a = act ? alpha[(size_t)t * SS] : MWER_NEG_INF;
        const double p0 = col[c][s + 2], p1 = col[c][s + 3], p2 = skip_b ? col[c][s + 4] : MWER_NEG_INF;
        const double m = mwer_lse3(p0, p1, p2);
        bt = act ? lp + m : MWER_NEG_INF;
        c ^= 1;
        col[c][s + 2] = bt;
        if (act) g[(size_t)t * SS] = (a == MWER_NEG_INF || bt == MWER_NEG_INF) ? 0.f : (float)exp(a + bt - lp - ll);
        __syncthreads();
    }
    if (s == 0) {
        ll_out[e] = ll;
        part[e] = 1;
    }
}

// ---------------------------------------------------------------------------------- 4. posteriors, risk, coefficients, token chains
__global__ __launch_bounds__(256) void mwer_post_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len,
                                                        const int32_t* __restrict__ err, const double* __restrict__ ll, float* __restrict__ post,
                                                        float* __restrict__ coef, float* __restrict__ risk, int32_t* __restrict__ present,
                                                        unsigned char* __restrict__ ws, MwerLayout o, int N, int Lh, int ldn, int ldb) {
    __shared__ int stok[MWER_MAX_N * MWER_MAX_LEN];      // the token of every slot, -1 where there is none (valid ids are >= 0)
    const int b = blockIdx.x;
    const int32_t* part = (const int32_t*)(ws + o.part) + (size_t)b * N;
    if (threadIdx.x == 0) {      // one fixed order: entries ascending
        double mx = MWER_NEG_INF;
        for (int i = 0; i < N; ++i)
            if (part[i]) mx = fmax(mx, ll[(size_t)b * N + i]);
        double den = 0.0;
        for (int i = 0; i < N; ++i)
            if (part[i]) den += exp(ll[(size_t)b * N + i] - mx);
        double r = 0.0;
        for (int i = 0; i < N; ++i)
            if (part[i]) r += exp(ll[(size_t)b * N + i] - mx) / den * (double)err[(size_t)b * N + i];
        for (int i = 0; i < N; ++i) {
            const double p = part[i] ? exp(ll[(size_t)b * N + i] - mx) / den : 0.0;
            post[(size_t)b * N + i] = (float)p;
            coef[(size_t)b * N + i] = part[i] ? (float)(p * ((double)err[(size_t)b * N + i] - r)) : 0.f;
            present[(size_t)b * N + i] = part[i] ? 1 : 0;
        }
        risk[b] = (float)r;      // 0 when no entry takes part
    }
    const int slots = N * Lh;
    for (int k = threadIdx.x; k < slots; k += blockDim.x) {
        const int i = k / Lh, j = k - i * Lh;
        const bool on = part[i] && j < mwer_clamp(hyp_len[(size_t)b * N + i], 0, Lh);
        stok[k] = on ? hyp[(size_t)b * ldb + (size_t)i * ldn + j] : -1;
    }
    __syncthreads();
    int32_t* next = (int32_t*)(ws + o.next) + (size_t)b * slots;
    int32_t* own = (int32_t*)(ws + o.own) + (size_t)b * slots;
    for (int k = threadIdx.x; k < slots; k += blockDim.x) {
        const int tk = stok[k];
        int nx = -1, ow = tk >= 0;
        if (tk >= 0) {
            for (int q = 0; q < k; ++q)
                if (stok[q] == tk) {
                    ow = 0;
                    break;
                }
            for (int q = k + 1; q < slots; ++q)
                if (stok[q] == tk) {
                    nx = q;
                    break;
                }
        }
        next[k] = nx;
        own[k] = ow;
    }
}

// ---------------------------------------------------------------------------------- 5. the gradient of one frame
template <typename T>
__global__ __launch_bounds__(256) void mwer_grad_kernel(T* __restrict__ dlogits, const int32_t* __restrict__ in_len, const int32_t* __restrict__ hyp,
                                                        const int32_t* __restrict__ hyp_len, const float* __restrict__ coef,
                                                        const unsigned char* __restrict__ ws, MwerLayout o, int T_, int V, int ld, int N, int Lh,
                                                        int ldn, int ldb, int blank, float scale_in, const float* __restrict__ scale_div,
                                                        int accumulate) {
    const int b = blockIdx.y, t = blockIdx.x;
    const int Tb = mwer_clamp(in_len[b], 0, T_);
    T* dl = dlogits + ((size_t)b * T_ + t) * ld;
    if (!accumulate) {
        for (int v = threadIdx.x; v < V; v += 256) dl[v] = from_f32<T>(0.f);
        __syncthreads();      // the zeros of this workgroup are ordered before its own cells below
    }
    if (t >= Tb) return;
    const float scale = scale_div ? scale_in / *scale_div : scale_in;
    const int SS = 2 * Lh + 1, slots = N * Lh;
    const int32_t* part = (const int32_t*)(ws + o.part) + (size_t)b * N;
    const int32_t* next = (const int32_t*)(ws + o.next) + (size_t)b * slots;
    const int32_t* own = (const int32_t*)(ws + o.own) + (size_t)b * slots;
    const float* g = (const float*)(ws + o.g) + ((size_t)b * N * T_ + t) * SS;      // entry i, state s: g[i * T_ * SS + s]
    const float* cf = coef + (size_t)b * N;
    const size_t estride = (size_t)T_ * SS;
    auto put = [&](int colv, float sum) {
        const float v = __fmul_rn(scale, sum);      // rounded on its own in both modes: never fused into the addition below
        dl[colv] = from_f32<T>(accumulate ? __fadd_rn(to_f32<T>(dl[colv]), v) : v);
    };
    if (threadIdx.x == 255) {      // the blank: entries ascending, even states ascending
        float sum = 0.f;
        bool any = false;
        for (int i = 0; i < N; ++i) {
            if (!part[i]) continue;
            any = true;
            const int n = mwer_clamp(hyp_len[(size_t)b * N + i], 0, Lh);
            const float c = cf[i];
            const float* gi = g + (size_t)i * estride;
            for (int s = 0; s <= 2 * n; s += 2) sum += c * gi[s];
        }
        if (any && blank >= 0 && blank < V) put(blank, sum);
    }
    for (int k = threadIdx.x; k < slots; k += 256) {
        if (!own[k]) continue;
        const int i0 = k / Lh, j0 = k - i0 * Lh;
        const int tk = hyp[(size_t)b * ldb + (size_t)i0 * ldn + j0];
        if (tk < 0 || tk >= V || tk == blank) continue;      // the lattice validated it; checked again where it becomes a column
        float sum = 0.f;
        int q = k;
        for (int guard = 0; guard < slots && q >= k && q < slots; ++guard) {      // a chain only moves forward
            const int i = q / Lh, j = q - i * Lh;
            sum += cf[i] * g[(size_t)i * estride + 2 * j + 1];
            const int nx = next[q];
            if (nx <= q) break;
            q = nx;
        }
        put(tk, sum);
    }
}

int mwer_list_check(const char* name, int B, int N, int Lh, int ldn, int ldb) {
    if (B <= 0 || B > 65535) ASR_FAIL(ASR_EINVAL, "%s: B=%d utterances outside [1, 65535]", name, B);
    if (N < 1 || N > MWER_MAX_N) ASR_FAIL(ASR_EINVAL, "%s: N=%d entries outside [1, %d]", name, N, MWER_MAX_N);
    if (Lh < 1 || Lh > MWER_MAX_LEN) ASR_FAIL(ASR_EINVAL, "%s: Lh=%d outside [1, %d]", name, Lh, MWER_MAX_LEN);
    if (ldn < Lh || (long long)ldb < (long long)(N - 1) * ldn + Lh)
        ASR_FAIL(ASR_EINVAL, "%s: stride below the row length (ldn=%d ldb=%d Lh=%d N=%d)", name, ldn, ldb, Lh, N);
    return ASR_OK;
}

int mwer_frames_check(const char* name, const void* p, int T, int V, int ld, int blank, int dtype) {
    if (T <= 0 || V <= 1 || blank < 0 || blank >= V) ASR_FAIL(ASR_EINVAL, "%s: bad shape T=%d V=%d blank=%d", name, T, V, blank);
    if (ld < V) ASR_FAIL(ASR_EINVAL, "%s: row stride ld=%d below V=%d", name, ld, V);
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "%s: dtype %d", name, dtype);
    if ((uintptr_t)p % (dtype == ASR_F32 ? 4 : 2)) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    return ASR_OK;
}

}  // namespace

extern "C" size_t asr_ctc_mwer_workspace_bytes(int B, int N, int T, int Lh) {
    if (B <= 0 || N < 1 || N > MWER_MAX_N || T <= 0 || Lh < 1 || Lh > MWER_MAX_LEN) {
        asr_set_error("asr_ctc_mwer_workspace_bytes: bad shape B=%d N=%d T=%d Lh=%d", B, N, T, Lh);
        return 0;
    }
    return mwer_layout(B, N, T, Lh).bytes;
}

extern "C" int asr_mwer_errors(const int32_t* hyp, const int32_t* hyp_len, const int32_t* ref, const int32_t* ref_len, int32_t* err, int32_t* flags,
                               int B, int N, int Lh, int ldn, int ldb, int Lr, int ldr, void* stream) {
    const char* name = "asr_mwer_errors";
    if (!hyp || !hyp_len || !ref || !ref_len || !err || !flags) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if (((uintptr_t)hyp | (uintptr_t)hyp_len | (uintptr_t)ref | (uintptr_t)ref_len | (uintptr_t)err | (uintptr_t)flags) % 4)
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    const int rc = mwer_list_check(name, B, N, Lh, ldn, ldb);
    if (rc != ASR_OK) return rc;
    if (Lr < 1 || Lr > MWER_MAX_LEN) ASR_FAIL(ASR_EINVAL, "%s: Lr=%d outside [1, %d]", name, Lr, MWER_MAX_LEN);
    if (ldr < Lr) ASR_FAIL(ASR_EINVAL, "%s: stride below the row length (ldr=%d Lr=%d)", name, ldr, Lr);
    mwer_errors_kernel<<<dim3(N, B), WAVE, 0, (hipStream_t)stream>>>(hyp, hyp_len, ref, ref_len, err, flags, N, Lh, ldn, ldb, Lr, ldr);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}

extern "C" int asr_ctc_mwer_lattice(const void* logits, const int32_t* in_len, const int32_t* hyp, const int32_t* hyp_len, const int32_t* err,
                                    double* ll, float* post, float* coef, float* risk, int32_t* present, int B, int T, int V, int ld, int N, int Lh,
                                    int ldn, int ldb, int blank, void* ws, size_t ws_bytes, int dtype, void* stream) {
    const char* name = "asr_ctc_mwer_lattice";
    if (!logits || !in_len || !hyp || !hyp_len || !err || !ll || !post || !coef || !risk || !present || !ws) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if (((uintptr_t)in_len | (uintptr_t)hyp | (uintptr_t)hyp_len | (uintptr_t)err | (uintptr_t)post | (uintptr_t)coef | (uintptr_t)risk | (uintptr_t)present) % 4 ||
        (uintptr_t)ll % 8 || (uintptr_t)ws % 16)
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    int rc = mwer_list_check(name, B, N, Lh, ldn, ldb);
    if (rc != ASR_OK) return rc;
    rc = mwer_frames_check(name, logits, T, V, ld, blank, dtype);
    if (rc != ASR_OK) return rc;
    const MwerLayout o = mwer_layout(B, N, T, Lh);
    if (ws_bytes < o.bytes) ASR_FAIL(ASR_EWORKSPACE, "%s: workspace %zu < %zu", name, ws_bytes, o.bytes);
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * T;
    const int g1 = (int)(rows / 4 + 1 > 4096 ? 4096 : rows / 4 + 1);
    const int threads = (2 * Lh + 1 + 63) / 64 * 64;      // a thread per state: 64 .. 512
    unsigned char* w = (unsigned char*)ws;
    if (dtype == ASR_F32) {
        mwer_lse_kernel<float><<<g1, 256, 0, st>>>((const float*)logits, in_len, (double*)(w + o.lse), B, T, V, ld);
        mwer_lattice_kernel<float><<<dim3(N, B), threads, 0, st>>>((const float*)logits, in_len, hyp, hyp_len, ll, w, o, B, T, V, ld, N, Lh, ldn, ldb, blank);
    } else {
        mwer_lse_kernel<bf16_t><<<g1, 256, 0, st>>>((const bf16_t*)logits, in_len, (double*)(w + o.lse), B, T, V, ld);
        mwer_lattice_kernel<bf16_t><<<dim3(N, B), threads, 0, st>>>((const bf16_t*)logits, in_len, hyp, hyp_len, ll, w, o, B, T, V, ld, N, Lh, ldn, ldb, blank);
    }
    mwer_post_kernel<<<B, 256, 0, st>>>(hyp, hyp_len, err, ll, post, coef, risk, present, w, o, N, Lh, ldn, ldb);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}

extern "C" int asr_ctc_mwer_grad(void* dlogits, const int32_t* in_len, const int32_t* hyp, const int32_t* hyp_len, const float* coef, int B, int T,
                                 int V, int ld, int N, int Lh, int ldn, int ldb, int blank, float grad_scale, const float* grad_scale_div,
                                 int accumulate, const void* ws, size_t ws_bytes, int dtype, void* stream) {
    const char* name = "asr_ctc_mwer_grad";
    if (!dlogits || !in_len || !hyp || !hyp_len || !coef || !ws) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if (((uintptr_t)in_len | (uintptr_t)hyp | (uintptr_t)hyp_len | (uintptr_t)coef | (uintptr_t)grad_scale_div) % 4 || (uintptr_t)ws % 16)
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    int rc = mwer_list_check(name, B, N, Lh, ldn, ldb);
    if (rc != ASR_OK) return rc;
    rc = mwer_frames_check(name, dlogits, T, V, ld, blank, dtype);
    if (rc != ASR_OK) return rc;
    if (!(grad_scale == grad_scale) || grad_scale - grad_scale != 0.f) ASR_FAIL(ASR_EINVAL, "%s: grad_scale is not finite", name);
    if (accumulate != 0 && accumulate != 1) ASR_FAIL(ASR_EINVAL, "%s: accumulate=%d (0 or 1)", name, accumulate);
    const MwerLayout o = mwer_layout(B, N, T, Lh);
    if (ws_bytes < o.bytes) ASR_FAIL(ASR_EWORKSPACE, "%s: workspace %zu < %zu", name, ws_bytes, o.bytes);
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* w = (const unsigned char*)ws;
    if (dtype == ASR_F32)
        mwer_grad_kernel<float><<<dim3(T, B), 256, 0, st>>>((float*)dlogits, in_len, hyp, hyp_len, coef, w, o, T, V, ld, N, Lh, ldn, ldb, blank, grad_scale, grad_scale_div, accumulate);
    else
        mwer_grad_kernel<bf16_t><<<dim3(T, B), 256, 0, st>>>((bf16_t*)dlogits, in_len, hyp, hyp_len, coef, w, o, T, V, ld, N, Lh, ldn, ldb, blank, grad_scale, grad_scale_div, accumulate);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}
