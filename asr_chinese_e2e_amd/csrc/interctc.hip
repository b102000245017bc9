// Intermediate CTC with self-conditioning: the dense softmax passes of the conditioning (include/asr_hip.h: asr_softmax_rows,
// asr_softmax_bwd_add; the definition is tests/interctc_ref.py).  HBM-bound passes over (B, T, V) frames in rows of ld >= V elements.
//
//   softmax_rows_kernel    : p = softmax(z) of every frame t < in_len[b], zeros on the other frames.
//   softmax_bwd_add_kernel : grad (+)= p (dp - sum_u p[u] dp[u]) of every frame t < in_len[b].
//
// Both follow cr_ctc.hip's dense pass: one workgroup of 256 threads per frame, 16 B per thread and access (element by element when V, ld
// or a base address is no multiple of the vector), the row - for the backward both p and dp - in registers from the load to the store up
// to ASR_INTERCTC_RESIDENT_MAX_V elements (IC_E values per thread and row); a longer row is read again for each pass (it is L2-hot) with
// the same element-to-thread mapping and the same arithmetic, so that a thread adds the same terms in the same order on both paths.
// Exponentials and products are f32; the row sums are carried in fp64 (block_sum_f64, as in cr_ctc.hip: one f32 rounding of a sum of
// 4232 terms is 6e-8 of a probability near 1, the allowance of the tests' gate is of that size) and rounded once.  No atomics, one
// summation order: two runs write the same bytes.
#include "asr_common.h"

namespace {

constexpr int IC_THREADS = 256;
constexpr int IC_E = ASR_INTERCTC_RESIDENT_MAX_V / IC_THREADS;      // elements per thread and row in registers: 24 (V = 4232: 17 of them used)
static_assert(IC_E * IC_THREADS == ASR_INTERCTC_RESIDENT_MAX_V && IC_E % 8 == 0, "the resident cap is whole 16-byte vectors per thread");
ASR_FULL_WAVES(IC_THREADS);

// columns [0, V) of one row <- 0 (the whole workgroup; chunk c = elements [c N, c N + N), N divides V on the vector path)
template <typename T, int N>
__device__ __forceinline__ void zero_row(T* row, int nch) {
    float z[N];
#pragma unroll
    for (int j = 0; j < N; ++j) z[j] = 0.f;
    for (int c = threadIdx.x; c < nch; c += IC_THREADS) storev<T, N>(row + (size_t)c * N, z);
}

// f(k, c): called for every chunk c of this thread, k its register slot.  RES: slots 0 .. KC-1, unrolled; else slot 0 in a loop.
// Thread i owns the chunks i, i + 256, i + 512, ... on both paths.
template <int KC, bool RES, typename F>
__device__ __forceinline__ void each_chunk(int nch, F&& f) {
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int c = threadIdx.x + IC_THREADS * k;
            if (c < nch) f(k, c);
        }
    } else {
        for (int c = threadIdx.x; c < nch; c += IC_THREADS) f(0, c);
    }
}

// N: elements per access (Vec<T>::N, or 1).  RES: the row stays in registers.
template <typename T, int N, bool RES>
__global__ __launch_bounds__(IC_THREADS) void softmax_rows_kernel(const T* __restrict__ logits, T* __restrict__ out, const int32_t* __restrict__ in_len,
                                                                  int T_, int V, int ld) {
    __shared__ float red[16];
    __shared__ double red64[IC_THREADS / 64];
    constexpr int KC = RES ? IC_E / N : 1;      // chunks per thread held in registers
    const int t = blockIdx.x, b = blockIdx.y;
    const int n = min(max(in_len[b], 0), T_);
    const size_t o = ((size_t)b * T_ + t) * ld;
    const int nch = V / N;
    if (t >= n) {      // the whole workgroup: no barrier below is reached by a part of it
        zero_row<T, N>(out + o, nch);
        return;
    }
    const T* x_g = logits + o;
    float x[KC][N];
    auto fetch = [&](int k, int c) {      // the path that re-reads loads the chunk in front of every use
        if constexpr (!RES) loadv<T, N>(x_g + (size_t)c * N, x[k]);
    };
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {      // all loads of the row in flight at once
            const int c = threadIdx.x + IC_THREADS * k;
            if (c < nch) loadv<T, N>(x_g + (size_t)c * N, x[k]);
        }
    }
    float m = -INFINITY;
    each_chunk<KC, RES>(nch, [&](int k, int c) {
        fetch(k, c);
#pragma unroll
        for (int j = 0; j < N; ++j) m = fmaxf(m, x[k][j]);
    });
    m = block_max(m, red);
    if (!(fabsf(m) < INFINITY)) {      // every lane holds the same m: a row of -inf (or with a +inf) has no softmax, it gets zeros
        zero_row<T, N>(out + o, nch);
        return;
    }
    double s = 0.0;
    each_chunk<KC, RES>(nch, [&](int k, int c) {
        fetch(k, c);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float e = expf(x[k][j] - m);      // exp(-inf) = 0 exactly
            if constexpr (RES) x[k][j] = e;         // the resident row keeps the exponential; the other path computes the same float again
            s += (double)e;
        }
    });
    s = block_sum_f64<IC_THREADS>(s, red64);
    const float inv = (float)(1.0 / s);      // s >= 1: the maximum's own term.  One rounding of the fp64 sum's reciprocal, then f32 products
    each_chunk<KC, RES>(nch, [&](int k, int c) {
        fetch(k, c);
        float p[N];
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = (RES ? x[k][j] : expf(x[k][j] - m)) * inv;
        storev<T, N>(out + o + (size_t)c * N, p);
    });
}

template <typename T, int N, bool RES>
__global__ __launch_bounds__(IC_THREADS) void softmax_bwd_add_kernel(const T* __restrict__ p, const T* __restrict__ dp, T* __restrict__ grad,
                                                                     const int32_t* __restrict__ in_len, int T_, int V, int ld, int accumulate) {
    __shared__ double red64[IC_THREADS / 64];
    constexpr int KC = RES ? IC_E / N : 1;
    const int t = blockIdx.x, b = blockIdx.y;
    const int n = min(max(in_len[b], 0), T_);
    const size_t o = ((size_t)b * T_ + t) * ld;
    const int nch = V / N;
    if (t >= n) {
        if (!accumulate) zero_row<T, N>(grad + o, nch);
        return;
    }
    const T* p_g = p + o;
    const T* d_g = dp + o;
    float pr[KC][N], dr[KC][N];
    auto fetch = [&](int k, int c) {
        if constexpr (!RES) {
            loadv<T, N>(p_g + (size_t)c * N, pr[k]);
            loadv<T, N>(d_g + (size_t)c * N, dr[k]);
        }
    };
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {      // all loads of both rows in flight at once
            const int c = threadIdx.x + IC_THREADS * k;
            if (c < nch) {
                loadv<T, N>(p_g + (size_t)c * N, pr[k]);
                loadv<T, N>(d_g + (size_t)c * N, dr[k]);
            }
        }
    }
    double s = 0.0;
    each_chunk<KC, RES>(nch, [&](int k, int c) {
        fetch(k, c);
#pragma unroll
        for (int j = 0; j < N; ++j) s += (double)(pr[k][j] * dr[k][j]);
    });
    const float sf = (float)block_sum_f64<IC_THREADS>(s, red64);
    each_chunk<KC, RES>(nch, [&](int k, int c) {
        // no contraction: accumulate = 1 must add the rounded product that accumulate = 0 writes, and p = 0 gives a term of exactly 0
#pragma clang fp contract(off)
        fetch(k, c);
        float g[N];
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] = pr[k][j] * (dr[k][j] - sf);
        T* dst = grad + o + (size_t)c * N;
        if (accumulate) {      // read, add in fp32, round once
            float q[N];
            loadv<T, N>(dst, q);
#pragma unroll
            for (int j = 0; j < N; ++j) g[j] += q[j];
        }
        storev<T, N>(dst, g);
    });
}

template <typename T> bool ic_vec(int V, int ld, uintptr_t ptrs) { return V % Vec<T>::N == 0 && ld % Vec<T>::N == 0 && ptrs % 16 == 0; }

template <typename T>
void softmax_rows_launch(const void* logits, void* out, const int32_t* in_len, int B, int T_, int V, int ld, hipStream_t st) {
    constexpr int N = Vec<T>::N;
    const bool vec = ic_vec<T>(V, ld, (uintptr_t)logits | (uintptr_t)out), res = V <= ASR_INTERCTC_RESIDENT_MAX_V;
    const dim3 grid(T_, B);
#define IC_LAUNCH(N_, RES_) softmax_rows_kernel<T, N_, RES_><<<grid, IC_THREADS, 0, st>>>((const T*)logits, (T*)out, in_len, T_, V, ld)
    if (vec && res) IC_LAUNCH(N, true);
    else if (vec) IC_LAUNCH(N, false);
    else if (res) IC_LAUNCH(1, true);
    else IC_LAUNCH(1, false);
#undef IC_LAUNCH
}

template <typename T>
void softmax_bwd_add_launch(const void* p, const void* dp, void* grad, const int32_t* in_len, int B, int T_, int V, int ld, int accumulate, hipStream_t st) {
    constexpr int N = Vec<T>::N;
    const bool vec = ic_vec<T>(V, ld, (uintptr_t)p | (uintptr_t)dp | (uintptr_t)grad), res = V <= ASR_INTERCTC_RESIDENT_MAX_V;
    const dim3 grid(T_, B);
#define IC_LAUNCH(N_, RES_) \
    softmax_bwd_add_kernel<T, N_, RES_><<<grid, IC_THREADS, 0, st>>>((const T*)p, (const T*)dp, (T*)grad, in_len, T_, V, ld, accumulate)
    if (vec && res) IC_LAUNCH(N, true);
    else if (vec) IC_LAUNCH(N, false);
    else if (res) IC_LAUNCH(1, true);
    else IC_LAUNCH(1, false);
#undef IC_LAUNCH
}

// the shape checks both entry points share; es: the element size
int ic_check(const char* name, int B, int T, int V, int ld, int dtype, size_t* es) {
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "%s: dtype %d", name, dtype);
    *es = dtype == ASR_F32 ? 4 : 2;
    if (B <= 0 || B > 65535 || T <= 0 || V <= 0 || ld < V) ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d (1 .. 65535) T=%d V=%d ld=%d", name, B, T, V, ld);
    return ASR_OK;
}

bool ic_overlap(const void* a, const void* b, size_t span) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + span && y < x + span;
}

}  // namespace

extern "C" int asr_softmax_rows(const void* logits, const int32_t* in_len, void* out, int B, int T, int V, int ld, int dtype, void* stream) {
    const char* name = "asr_softmax_rows";
    if (!logits || !in_len || !out) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    size_t es;
    if (int rc = ic_check(name, B, T, V, ld, dtype, &es)) return rc;
    if ((uintptr_t)in_len % 4 || ((uintptr_t)logits | (uintptr_t)out) % es) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    const size_t span = (((size_t)B * T - 1) * ld + V) * es;      // both blocks span (B T - 1) ld + V elements
    if (ic_overlap(logits, out, span)) ASR_FAIL(ASR_EINVAL, "%s: the output overlaps the logits", name);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ASR_F32) softmax_rows_launch<float>(logits, out, in_len, B, T, V, ld, st);
    else softmax_rows_launch<bf16_t>(logits, out, in_len, B, T, V, ld, st);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}

extern "C" int asr_softmax_bwd_add(const void* p, const void* dp, const int32_t* in_len, void* grad, int B, int T, int V, int ld, int accumulate,
                                   int dtype, void* stream) {
    const char* name = "asr_softmax_bwd_add";
    if (!p || !dp || !in_len || !grad) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    size_t es;
    if (int rc = ic_check(name, B, T, V, ld, dtype, &es)) return rc;
    if ((uintptr_t)in_len % 4 || ((uintptr_t)p | (uintptr_t)dp | (uintptr_t)grad) % es) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    if (accumulate != 0 && accumulate != 1) ASR_FAIL(ASR_EINVAL, "%s: accumulate=%d (0 or 1)", name, accumulate);
    const size_t span = (((size_t)B * T - 1) * ld + V) * es;
    if (ic_overlap(p, grad, span) || ic_overlap(dp, grad, span))
        ASR_FAIL(ASR_EINVAL, "%s: the gradient block overlaps p or dp (a row is read again after the first store)", name);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ASR_F32) softmax_bwd_add_launch<float>(p, dp, grad, in_len, B, T, V, ld, accumulate, st);
    else softmax_bwd_add_launch<bf16_t>(p, dp, grad, in_len, B, T, V, ld, accumulate, st);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}
