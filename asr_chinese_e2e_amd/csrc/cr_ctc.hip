// CR-CTC: the consistency term between the frame posteriors of two views of an utterance, and its gradient with respect to the logits
// (include/asr_hip.h: asr_cr_ctc_fwd_bwd; the definition is tests/cr_ctc_ref.py).  An HBM-bound pass over (2P, T, V) logits.
//
// Two kernels on one stream:
//   1. cr_ctc_kernel   : one workgroup of 256 threads per (pair, frame), the dense row pass of dense_row.h over the frame's row of BOTH
//      views (in registers up to ASR_CR_CTC_RESIDENT_MAX_V elements, else read again for each of the three passes): per row block_max
//      and the block's sum of exp(x - max), then per
//      element p = exp(x - max) / sum, lp = x - lse, J += (p_a - p_b) (lp_a - lp_b), g = scale/2 (p_a - p_b) -> row a, -g -> row b.
//      The exponentials are f32 (expf); their sum, p, lp and J are carried in fp64 (see the note below).  Both rows go through one
//      instruction sequence: identical views give exactly 0, swapped views swapped bytes.
//   2. cr_ctc_pair_sum_kernel : one workgroup per pair adds frame_loss[p, :] in frame order (fp64 accumulator, one thread, rows staged
//      through LDS).  No atomics anywhere: two runs write the same bytes.
#include "dense_row.h"

namespace {

constexpr int CR_THREADS = 256;      // elements per thread and row in registers: 6144 / 256 = 24 (V = 4232: 17 of them used)

// Why fp64 behind the f32 exponentials: with peaked posteriors (logits spread over +-100) J is a sum of terms (p_a - p_b)(lp_a - lp_b) with
// p ~ 1 and lp differences ~ 100, so a relative error of 6e-8 in a sum of exponentials (one f32 rounding) moves J by 6e-6 - more than the
// f32 spacing of the result allows a kernel to be away from the definition.  Sums, p, lp and J in fp64 cost ~15 fp64 instructions per
// pair of elements beside two expf and the memory traffic, and leave the f32 rounding of expf itself (p tiny wherever lp is large) and
// of the results.  block_sum_f64 adds in one fixed order.

// N, RES: dense_row.h.  xa, xb = r.x[0], r.x[1]: the frame's row of view a and of view b.
template <typename T, int N, bool RES>
__global__ __launch_bounds__(CR_THREADS) void cr_ctc_kernel(const T* __restrict__ logits, T* __restrict__ grad, const int32_t* __restrict__ in_len,
                                                            float* __restrict__ frame_loss, int P, int T_, int V, int ld, float grad_scale,
                                                            const float* __restrict__ grad_scale_div, int accumulate) {
    __shared__ float red[16];
    __shared__ double red64[CR_THREADS / 64];
    const int t = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(min(in_len[p], in_len[p + P]), 0), T_);
    const size_t oa = ((size_t)p * T_ + t) * ld, ob = ((size_t)(p + P) * T_ + t) * ld;
    const int nch = V / N;      // N divides V on the vector path
    if (t >= n) {      // the whole workgroup: no barrier below is reached by a part of it
        if (tid == 0) frame_loss[(size_t)p * T_ + t] = 0.f;
        if (grad && !accumulate) zero_row<T, N, CR_THREADS>(nch, grad + oa, grad + ob);
        return;
    }
    DenseRows<T, N, RES, CR_THREADS, ASR_CR_CTC_RESIDENT_MAX_V, 2> r;
    r.g[0] = logits + oa;
    r.g[1] = logits + ob;
    r.nch = nch;
    r.load();
    auto& xa = r.x[0];
    auto& xb = r.x[1];
    float ma = -INFINITY, mb = -INFINITY;
    r.each([&](int k, int c) {
#pragma unroll
        for (int j = 0; j < N; ++j) { ma = fmaxf(ma, xa[k][j]); mb = fmaxf(mb, xb[k][j]); }
    });
    ma = block_max(ma, red);
    mb = block_max(mb, red);
    double sa = 0.0, sb = 0.0;
    r.each([&](int k, int c) {
#pragma unroll
        for (int j = 0; j < N; ++j) { sa += (double)expf(xa[k][j] - ma); sb += (double)expf(xb[k][j] - mb); }
    });
    sa = block_sum_f64<CR_THREADS>(sa, red64);
    sb = block_sum_f64<CR_THREADS>(sb, red64);
    const double ia = 1.0 / sa, ib = 1.0 / sb;
    const double dlse = ((double)ma + log(sa)) - ((double)mb + log(sb));      // lse_a - lse_b
    float h = 0.f;
    if (grad) h = 0.5f * (grad_scale_div ? grad_scale / *grad_scale_div : grad_scale);
    double js = 0.0;
    r.each([&](int k, int c) {
        // No contraction in this block (hipcc fuses a * b + c into one fma by default, across statements, and __dmul_rn / __fmul_rn are
        // plain products to it): p_a - p_b must be the difference of two ROUNDED products - as one fused multiply-subtract equal rows
        // gave 1e-20 instead of exactly 0 - and accumulate = 1 must add the rounded h * d that accumulate = 0 writes.
#pragma clang fp contract(off)
        float ga[N], gb[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double d = (double)expf(xa[k][j] - ma) * ia - (double)expf(xb[k][j] - mb) * ib;      // p_a - p_b
            js += d * (((double)xa[k][j] - (double)xb[k][j]) - dlse);                                    // ... times lp_a - lp_b
            ga[j] = h * (float)d;
            gb[j] = -ga[j];
        }
        if (grad) {
            T* da = grad + oa + (size_t)c * N;
            T* db = grad + ob + (size_t)c * N;
            if (accumulate) {      // read, add in fp32, round once
                float qa[N], qb[N];
                loadv<T, N>(da, qa);
                loadv<T, N>(db, qb);
#pragma unroll
                for (int j = 0; j < N; ++j) { ga[j] += qa[j]; gb[j] += qb[j]; }
            }
            storev<T, N>(da, ga);
            storev<T, N>(db, gb);
        }
    });
    js = block_sum_f64<CR_THREADS>(js, red64);
    if (tid == 0) frame_loss[(size_t)p * T_ + t] = (float)(0.5 * js);
}

// pair_loss[p] = sum_t frame_loss[p, t] in frame order (frames t >= n hold zeros)
__global__ __launch_bounds__(CR_THREADS) void cr_ctc_pair_sum_kernel(const float* __restrict__ frame_loss, float* __restrict__ pair_loss, int T_) {
    __shared__ float row[4 * CR_THREADS];
    const int p = blockIdx.x;
    const float* f = frame_loss + (size_t)p * T_;
    double acc = 0.0;
    for (int t0 = 0; t0 < T_; t0 += 4 * CR_THREADS) {
        const int m = min(4 * CR_THREADS, T_ - t0);
        __syncthreads();      // the previous part has been added
        for (int i = threadIdx.x; i < m; i += CR_THREADS) row[i] = f[t0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) acc += (double)row[i];
    }
    if (threadIdx.x == 0) pair_loss[p] = (float)acc;
}

}  // namespace

extern "C" int asr_cr_ctc_fwd_bwd(const void* logits, const int32_t* in_len, void* grad, float* frame_loss, float* pair_loss, int P, int T, int V,
                                  int ld, float grad_scale, const float* grad_scale_div, int accumulate, int dtype, void* stream) {
    const char* name = "asr_cr_ctc_fwd_bwd";
    if (!logits || !in_len || !frame_loss || !pair_loss) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    size_t es;
    if (int rc = dense_check_dtype(name, dtype, &es)) return rc;
    if (((uintptr_t)in_len | (uintptr_t)frame_loss | (uintptr_t)pair_loss | (uintptr_t)grad_scale_div) % 4 || ((uintptr_t)logits | (uintptr_t)grad) % es)
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    if (P <= 0 || P > 65535 || T <= 0 || V < 2 || ld < V) ASR_FAIL(ASR_EINVAL, "%s: bad shape P=%d (1 .. 65535) T=%d V=%d ld=%d", name, P, T, V, ld);
    if (int rc = dense_check_accumulate(name, accumulate)) return rc;
    if (accumulate && !grad) ASR_FAIL(ASR_EINVAL, "%s: accumulate=1 needs the gradient block to add to", name);
    if (int rc = dense_check_grad_scale(name, grad_scale)) return rc;
    if (grad && dense_overlap(logits, grad, (size_t)2 * P * T, V, ld, es))
        ASR_FAIL(ASR_EINVAL, "%s: the gradient block overlaps the logits (the logits are read after the first store)", name);
    hipStream_t st = (hipStream_t)stream;
    dense_row_dispatch<ASR_CR_CTC_RESIDENT_MAX_V>(dtype, V, ld, (uintptr_t)logits | (uintptr_t)grad, [&](auto e, auto n, auto res) {
        using E = decltype(e);
        cr_ctc_kernel<E, n, res><<<dim3(T, P), CR_THREADS, 0, st>>>((const E*)logits, (E*)grad, in_len, frame_loss, P, T, V, ld, grad_scale, grad_scale_div, accumulate);
    });
    cr_ctc_pair_sum_kernel<<<P, CR_THREADS, 0, st>>>(frame_loss, pair_loss, T);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}
