// Intermediate CTC with self-conditioning: the dense softmax passes of the conditioning (include/asr_hip.h: asr_softmax_rows,
// asr_softmax_bwd_add; the definition is tests/interctc_ref.py).  HBM-bound passes over (B, T, V) frames in rows of ld >= V elements.
//
//   softmax_rows_kernel    : p = softmax(z) of every frame t < in_len[b], zeros on the other frames.
//   softmax_bwd_add_kernel : grad (+)= p (dp - sum_u p[u] dp[u]) of every frame t < in_len[b].
//
// Both are the dense row pass of dense_row.h, one workgroup of 256 threads per frame: the row - for the backward both p and dp - in
// registers from the load to the store up to ASR_INTERCTC_RESIDENT_MAX_V elements, a longer row read again for each pass with the same
// arithmetic.  Exponentials and products are f32; the row sums are carried in fp64 (block_sum_f64, as in cr_ctc.hip: one f32 rounding of
// a sum of 4232 terms is 6e-8 of a probability near 1, the allowance of the tests' gate is of that size) and rounded once.  No atomics,
// one summation order: two runs write the same bytes.
#include "dense_row.h"

namespace {

constexpr int IC_THREADS = 256;      // elements per thread and row in registers: 6144 / 256 = 24 (V = 4232: 17 of them used)
template <typename T, int N, bool RES, int NR> using IcRows = DenseRows<T, N, RES, IC_THREADS, ASR_INTERCTC_RESIDENT_MAX_V, NR>;

// N, RES: dense_row.h
template <typename T, int N, bool RES>
__global__ __launch_bounds__(IC_THREADS) void softmax_rows_kernel(const T* __restrict__ logits, T* __restrict__ out, const int32_t* __restrict__ in_len,
                                                                  int T_, int V, int ld) {
    __shared__ float red[16];
    __shared__ double red64[IC_THREADS / 64];
    const int t = blockIdx.x, b = blockIdx.y;
    const int n = min(max(in_len[b], 0), T_);
    const size_t o = ((size_t)b * T_ + t) * ld;
    const int nch = V / N;
    if (t >= n) {      // the whole workgroup: no barrier below is reached by a part of it
        zero_row<T, N, IC_THREADS>(nch, out + o);
        return;
    }
    IcRows<T, N, RES, 1> r;
    r.g[0] = logits + o;
    r.nch = nch;
    r.load();
    auto& x = r.x[0];
    float m = -INFINITY;
    r.each([&](int k, int c) {
#pragma unroll
        for (int j = 0; j < N; ++j) m = fmaxf(m, x[k][j]);
    });
    m = block_max(m, red);
    if (!(fabsf(m) < INFINITY)) {      // every lane holds the same m: a row of -inf (or with a +inf) has no softmax, it gets zeros
        zero_row<T, N, IC_THREADS>(nch, out + o);
        return;
    }
    double s = 0.0;
    r.each([&](int k, int c) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float e = expf(x[k][j] - m);      // exp(-inf) = 0 exactly
            if constexpr (RES) x[k][j] = e;         // the resident row keeps the exponential; the other path computes the same float again
            s += (double)e;
        }
    });
    s = block_sum_f64<IC_THREADS>(s, red64);
    const float inv = (float)(1.0 / s);      // s >= 1: the maximum's own term.  One rounding of the fp64 sum's reciprocal, then f32 products
    r.each([&](int k, int c) {
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
    const int t = blockIdx.x, b = blockIdx.y;
    const int n = min(max(in_len[b], 0), T_);
    const size_t o = ((size_t)b * T_ + t) * ld;
    const int nch = V / N;
    if (t >= n) {
        if (!accumulate) zero_row<T, N, IC_THREADS>(nch, grad + o);
        return;
    }
    IcRows<T, N, RES, 2> r;
    r.g[0] = p + o;
    r.g[1] = dp + o;
    r.nch = nch;
    r.load();
    auto& pr = r.x[0];
    auto& dr = r.x[1];
    double s = 0.0;
    r.each([&](int k, int c) {
#pragma unroll
        for (int j = 0; j < N; ++j) s += (double)(pr[k][j] * dr[k][j]);
    });
    const float sf = (float)block_sum_f64<IC_THREADS>(s, red64);
    r.each([&](int k, int c) {
        // no contraction: accumulate = 1 must add the rounded product that accumulate = 0 writes, and p = 0 gives a term of exactly 0
#pragma clang fp contract(off)
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

// the shape checks both entry points share; es: the element size
int ic_check(const char* name, int B, int T, int V, int ld, int dtype, size_t* es) {
    if (int rc = dense_check_dtype(name, dtype, es)) return rc;
    if (B <= 0 || B > 65535 || T <= 0 || V <= 0 || ld < V) ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d (1 .. 65535) T=%d V=%d ld=%d", name, B, T, V, ld);
    return ASR_OK;
}

}  // namespace

extern "C" int asr_softmax_rows(const void* logits, const int32_t* in_len, void* out, int B, int T, int V, int ld, int dtype, void* stream) {
    const char* name = "asr_softmax_rows";
    if (!logits || !in_len || !out) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    size_t es;
    if (int rc = ic_check(name, B, T, V, ld, dtype, &es)) return rc;
    if ((uintptr_t)in_len % 4 || ((uintptr_t)logits | (uintptr_t)out) % es) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    if (dense_overlap(logits, out, (size_t)B * T, V, ld, es)) ASR_FAIL(ASR_EINVAL, "%s: the output overlaps the logits", name);
    hipStream_t st = (hipStream_t)stream;
    dense_row_dispatch<ASR_INTERCTC_RESIDENT_MAX_V>(dtype, V, ld, (uintptr_t)logits | (uintptr_t)out, [&](auto e, auto n, auto res) {
        using E = decltype(e);
        softmax_rows_kernel<E, n, res><<<dim3(T, B), IC_THREADS, 0, st>>>((const E*)logits, (E*)out, in_len, T, V, ld);
    });
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
    if (int rc = dense_check_accumulate(name, accumulate)) return rc;
    if (dense_overlap(p, grad, (size_t)B * T, V, ld, es) || dense_overlap(dp, grad, (size_t)B * T, V, ld, es))
        ASR_FAIL(ASR_EINVAL, "%s: the gradient block overlaps p or dp (a row is read again after the first store)", name);
    hipStream_t st = (hipStream_t)stream;
    dense_row_dispatch<ASR_INTERCTC_RESIDENT_MAX_V>(dtype, V, ld, (uintptr_t)p | (uintptr_t)dp | (uintptr_t)grad, [&](auto e, auto n, auto res) {
        using E = decltype(e);
        softmax_bwd_add_kernel<E, n, res><<<dim3(T, B), IC_THREADS, 0, st>>>((const E*)p, (const E*)dp, (E*)grad, in_len, T, V, ld, accumulate);
    });
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}
