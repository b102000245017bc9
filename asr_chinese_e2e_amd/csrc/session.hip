// Independent streaming sessions (sessions.py): the per-slot device work of one tick.  Every kernel here takes its per-slot parameters
// (start rows, counts, n_valid, reset flags) as int32 device arrays - rows of the one parameter block a push uploads - and treats a slot
// on its own: nothing a slot reads or writes depends on another slot's parameters.
//   asr_slot_rows_put         append each slot's valid rows of a (slots * C, ld) matrix to its window of a (slots, cap, cols) buffer
//   asr_slot_rows_slide       copy each slot's kept keys to the front of the other cache buffer (never in place)
//   asr_ctc_frame_best_blank  per frame: the best class (asr_ctc_frame_argmax's) and log p(blank) (asr_ctc_frame_topk's, bit for bit)
//   asr_session_ctc_step      per slot: CTC collapse with the carried last class, trailing-silence and frame counters
#include "asr_common.h"

namespace {

constexpr int SR_WAVES = 4;      // rows (waves) per workgroup of the row movers

// one wave per row, 16-byte vectors; a row is `vecs` vectors.  Rows outside [0, cap) of the destination are never written.
__global__ __launch_bounds__(SR_WAVES* WAVE) void slot_rows_put_kernel(const char* __restrict__ src, char* __restrict__ dst, const int32_t* __restrict__ start,
                                                                      const int32_t* __restrict__ n, int C, int cap, size_t src_row_bytes, int vecs) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, t = blockIdx.x * SR_WAVES + w;
    const int nb = min(n[b], C), s0 = start[b];
    if (t >= nb || s0 < 0 || s0 + t >= cap) return;      // wave-uniform
    const u32x4* s = (const u32x4*)(src + ((size_t)b * C + t) * src_row_bytes);
    u32x4* d = (u32x4*)(dst + ((size_t)b * cap + s0 + t) * ((size_t)vecs * 16));
    for (int v = lane; v < vecs; v += 64) d[v] = s[v];
}

// dst[b, t] = src[b, from[b] + t] for t < count[b]; src and dst are different buffers of the same (slots, cap, vecs * 16 bytes) layout
__global__ __launch_bounds__(SR_WAVES* WAVE) void slot_rows_slide_kernel(const char* __restrict__ src, char* __restrict__ dst, const int32_t* __restrict__ from,
                                                                        const int32_t* __restrict__ count, int cap, int vecs) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y, t = blockIdx.x * SR_WAVES + w;
    const int f0 = from[b], cnt = min(count[b], cap);
    if (t >= cnt || f0 < 0 || f0 + t >= cap) return;      // wave-uniform
    const size_t row_bytes = (size_t)vecs * 16;
    const u32x4* s = (const u32x4*)(src + ((size_t)b * cap + f0 + t) * row_bytes);
    u32x4* d = (u32x4*)(dst + ((size_t)b * cap + t) * row_bytes);
    for (int v = lane; v < vecs; v += 64) d[v] = s[v];
}

// One wave per frame.  The argmax pass is frame_argmax_kernel's (16-byte loads for bf16 rows that allow them); its maximum is the m of the
// log-sum-exp, so the row is read from memory once and from cache a second time for the sum.  The sum keeps logsoftmax_topk_kernel's order
// (lane l adds classes l, l + 64, ... and the lanes meet in wave_sum): blank_lp has that kernel's bits.
template <typename T>
__global__ __launch_bounds__(256) void frame_best_blank_kernel(const T* __restrict__ logits, const int32_t* __restrict__ in_len, int32_t* __restrict__ path,
                                                               float* __restrict__ blank_lp, int B, int T_, int V, int ld, int blank) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rows = B * T_;
    for (int row = blockIdx.x * 4 + w; row < rows; row += gridDim.x * 4) {
        const int b = row / T_, t = row - b * T_;
        if (in_len && t >= in_len[b]) {      // wave-uniform
            if (lane == 0) { path[row] = blank; blank_lp[row] = 0.f; }
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
        float s = 0.f;
        for (int i = lane; i < V; i += 64) s += expf(to_f32<T>(x[i]) - m);
        s = wave_sum(s);
        const float lse = m + logf(s);
        if (lane == 0) {
            path[row] = bi;
            blank_lp[row] = to_f32<T>(x[blank]) - lse;
        }
    }
}

// One wave per slot.  state (slots, 4) = {last class, trailing silent frames, frames consumed, decoded}; out (slots, 4 + C) =
// {new ids, trailing, frames, decoded, ids[C]}.  64 frames per trip: ballots give the collapse ranks and the last non-silent frame.
__global__ __launch_bounds__(64) void session_ctc_step_kernel(const int32_t* __restrict__ path, const float* __restrict__ blank_lp,
                                                              const int32_t* __restrict__ n_valid, const int32_t* __restrict__ reset,
                                                              int32_t* __restrict__ state, int32_t* __restrict__ out, int C, int blank, float silence_lp) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int32_t* st = state + (size_t)b * 4;
    int32_t* o = out + (size_t)b * (4 + C);
    const bool fresh = reset[b] != 0;
    int last = fresh ? blank : st[0], trailing = fresh ? 0 : st[1], frames = fresh ? 0 : st[2], decoded = fresh ? 0 : st[3];
    const int n = max(0, min(n_valid[b], C));
    int n_out = 0;
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane, here = min(64, n - t0);
        const bool live = t < n;
        const size_t row = (size_t)b * C + (live ? t : 0);
        if (path) {
            const int cur = live ? path[row] : blank;
            int left = __shfl_up(cur, 1, 64);
            if (lane == 0) left = last;
            const bool keep = live && cur != blank && cur != left;
            const unsigned long long m = __ballot(keep);
            if (keep) o[4 + n_out + __popcll(m & ((1ull << lane) - 1ull))] = cur;
            n_out += __popcll(m);
            last = __shfl(cur, here - 1, 64);
        }
        const bool speech = live && !(blank_lp[row] > silence_lp);
        const unsigned long long sp = __ballot(speech);
        if (sp == 0ull) trailing += here;
        else trailing = here - 1 - (63 - __builtin_clzll(sp));
    }
    frames += n;
    if (n_out > 0) decoded = 1;
    for (int i = n_out + lane; i < C; i += 64) o[4 + i] = 0;
    if (lane == 0) {
        st[0] = last; st[1] = trailing; st[2] = frames; st[3] = decoded;
        o[0] = n_out; o[1] = trailing; o[2] = frames; o[3] = decoded;
    }
}

int rows_args(const char* name, const void* src, void* dst, const void* a, const void* b, int slots, int cap, int cols, int esize) {
    if (!src || !dst || !a || !b) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if (slots <= 0 || slots > 65535 || cap <= 0 || cols <= 0 || (esize != 2 && esize != 4))
        ASR_FAIL(ASR_EINVAL, "%s: bad shape slots=%d (1..65535) cap=%d cols=%d element size %d", name, slots, cap, cols, esize);
    if (((size_t)cols * esize) % 16) ASR_FAIL(ASR_EINVAL, "%s: a row of %d elements of %d bytes is no multiple of 16 bytes", name, cols, esize);
    if (((uintptr_t)src | (uintptr_t)dst) % 16 || ((uintptr_t)a | (uintptr_t)b) % 4) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (rows: 16 bytes, parameters: 4)", name);
    return ASR_OK;
}

}  // namespace

extern "C" int asr_slot_rows_put(const void* src, void* dst, const int32_t* start, const int32_t* n, int slots, int C, int cap, int cols, int ld_src,
                                 int dtype, void* stream) {
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "asr_slot_rows_put: dtype %d", dtype);
    const int esize = dtype == ASR_F32 ? 4 : 2;
    const int rc = rows_args("asr_slot_rows_put", src, dst, start, n, slots, cap, cols, esize);
    if (rc != ASR_OK) return rc;
    if (C <= 0 || C > cap) ASR_FAIL(ASR_EINVAL, "asr_slot_rows_put: C=%d must be in [1, cap=%d]", C, cap);
    if (ld_src < cols || ((size_t)ld_src * esize) % 16) ASR_FAIL(ASR_EINVAL, "asr_slot_rows_put: source row stride %d (>= cols=%d, a multiple of 16 bytes)", ld_src, cols);
    slot_rows_put_kernel<<<dim3(ceil_div(C, SR_WAVES), slots), SR_WAVES * WAVE, 0, (hipStream_t)stream>>>(
        (const char*)src, (char*)dst, start, n, C, cap, (size_t)ld_src * esize, cols * esize / 16);
    ASR_CHECK_LAUNCH("asr_slot_rows_put");
    return ASR_OK;
}

extern "C" int asr_slot_rows_slide(const void* src, void* dst, const int32_t* from, const int32_t* count, int slots, int max_count, int cap, int cols,
                                   int dtype, void* stream) {
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "asr_slot_rows_slide: dtype %d", dtype);
    const int esize = dtype == ASR_F32 ? 4 : 2;
    const int rc = rows_args("asr_slot_rows_slide", src, dst, from, count, slots, cap, cols, esize);
    if (rc != ASR_OK) return rc;
    if (max_count <= 0 || max_count > cap) ASR_FAIL(ASR_EINVAL, "asr_slot_rows_slide: max_count=%d must be in [1, cap=%d]", max_count, cap);
    const size_t bytes = (size_t)slots * cap * cols * esize;
    if ((const char*)src < (char*)dst + bytes && (char*)dst < (const char*)src + bytes) ASR_FAIL(ASR_EINVAL, "asr_slot_rows_slide: source and destination overlap (the copy is never in place)");
    slot_rows_slide_kernel<<<dim3(ceil_div(max_count, SR_WAVES), slots), SR_WAVES * WAVE, 0, (hipStream_t)stream>>>(
        (const char*)src, (char*)dst, from, count, cap, cols * esize / 16);
    ASR_CHECK_LAUNCH("asr_slot_rows_slide");
    return ASR_OK;
}

extern "C" int asr_ctc_frame_best_blank(const void* logits, const int32_t* in_len, int32_t* path, float* blank_lp, int B, int T, int V, int ld, int blank,
                                        int dtype, void* stream) {
    if (!logits || !path || !blank_lp) ASR_FAIL(ASR_EINVAL, "asr_ctc_frame_best_blank: null pointer");
    if (B <= 0 || T <= 0 || V <= 1 || blank < 0 || blank >= V || (size_t)B * T > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_frame_best_blank: bad shape B=%d T=%d V=%d blank=%d", B, T, V, blank);
    if (ld < V) ASR_FAIL(ASR_EINVAL, "asr_ctc_frame_best_blank: row stride ld=%d < V=%d", ld, V);
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "asr_ctc_frame_best_blank: dtype %d", dtype);
    if ((uintptr_t)logits % (dtype == ASR_F32 ? 4 : 2) || ((uintptr_t)in_len | (uintptr_t)path | (uintptr_t)blank_lp) % 4)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_frame_best_blank: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    int g = ceil_div(B * T, 4);
    if (g > 4096) g = 4096;
    if (dtype == ASR_F32) frame_best_blank_kernel<float><<<g, 256, 0, st>>>((const float*)logits, in_len, path, blank_lp, B, T, V, ld, blank);
    else frame_best_blank_kernel<bf16_t><<<g, 256, 0, st>>>((const bf16_t*)logits, in_len, path, blank_lp, B, T, V, ld, blank);
    ASR_CHECK_LAUNCH("asr_ctc_frame_best_blank");
    return ASR_OK;
}

extern "C" int asr_session_ctc_step(const int32_t* path, const float* blank_lp, const int32_t* n_valid, const int32_t* reset, int32_t* state, int32_t* out,
                                    int slots, int C, int blank, float silence_lp, void* stream) {
    if (!blank_lp || !n_valid || !reset || !state || !out) ASR_FAIL(ASR_EINVAL, "asr_session_ctc_step: null pointer");
    if (slots <= 0 || C <= 0 || blank < 0 || (size_t)slots * (4 + (size_t)C) > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "asr_session_ctc_step: bad shape slots=%d C=%d blank=%d", slots, C, blank);
    if (silence_lp != silence_lp) ASR_FAIL(ASR_EINVAL, "asr_session_ctc_step: the silence threshold is not a number");
    if (((uintptr_t)path | (uintptr_t)blank_lp | (uintptr_t)n_valid | (uintptr_t)reset | (uintptr_t)state | (uintptr_t)out) % 4)
        ASR_FAIL(ASR_EINVAL, "asr_session_ctc_step: misaligned pointer");
    session_ctc_step_kernel<<<slots, 64, 0, (hipStream_t)stream>>>(path, blank_lp, n_valid, reset, state, out, C, blank, silence_lp);
    ASR_CHECK_LAUNCH("asr_session_ctc_step");
    return ASR_OK;
}
