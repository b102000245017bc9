// The dense row pass of the CTC-side training losses (cr_ctc.hip: cr_ctc_kernel; interctc.hip: softmax_rows_kernel, softmax_bwd_add_kernel):
// one workgroup of THREADS threads works on NR rows of V elements at once (the two views of a frame; p and dp of a frame), 16 B per thread
// and access, element by element when V, ld or a base address is no multiple of the vector.  Rows of up to CAP elements stay in registers
// from the load to the store (CAP / THREADS values per thread and row); longer ones are read again in front of every pass (they are
// L2-hot) with the same element-to-thread mapping, so that a thread adds the same terms in the same order on both paths.  A kernel
// writes what it does with one chunk and nothing about where the chunk comes from.
#pragma once
#include <type_traits>

#include "asr_common.h"

// N: elements per access (Vec<T>::N, or 1).  RES: the rows stay in registers.  Chunk c of a row = its elements [c N, c N + N), N divides V
// on the vector path; thread i owns the chunks i, i + THREADS, i + 2 THREADS, ... on both paths.
template <typename T, int N, bool RES, int THREADS, int CAP, int NR>
struct DenseRows {
    static_assert(CAP % THREADS == 0 && CAP / THREADS % 8 == 0, "the resident cap is whole 16-byte vectors per thread");
    ASR_FULL_WAVES(THREADS);
    static constexpr int KC = RES ? CAP / THREADS / N : 1;      // chunks per thread and row held in registers
    const T* g[NR];
    int nch;
    float x[NR][KC][N];      // x[r][k]: row r's chunk in register slot k

    __device__ __forceinline__ void load() {      // RES: all loads of all rows in flight at once; else nothing (each() fetches)
        if constexpr (RES) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const int c = threadIdx.x + THREADS * k;
                if (c < nch) fetch(k, c);
            }
        }
    }
    // f(k, c): called for every chunk c of this thread, k its register slot.  RES: slots 0 .. KC-1, unrolled; else slot 0 in a loop, the
    // chunk loaded again in front of every call
    template <typename F>
    __device__ __forceinline__ void each(F&& f) {
        if constexpr (RES) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const int c = threadIdx.x + THREADS * k;
                if (c < nch) f(k, c);
            }
        } else {
            for (int c = threadIdx.x; c < nch; c += THREADS) {
                fetch(0, c);
                f(0, c);
            }
        }
    }

private:
    __device__ __forceinline__ void fetch(int k, int c) {
#pragma unroll
        for (int r = 0; r < NR; ++r) loadv<T, N>(g[r] + (size_t)c * N, x[r][k]);
    }
};

// columns [0, N nch) of every given row <- 0 (the whole workgroup)
template <typename T, int N, int THREADS, typename... Rows>
__device__ __forceinline__ void zero_row(int nch, Rows*... rows) {
    float z[N];
#pragma unroll
    for (int j = 0; j < N; ++j) z[j] = 0.f;
    for (int c = threadIdx.x; c < nch; c += THREADS) (storev<T, N>(rows + (size_t)c * N, z), ...);
}

// ---- host side ------------------------------------------------------------------------------
// f(T(), N, RES): the element type as a value, N and RES as std::integral_constant.  ptrs: the base addresses of every block, or-ed.
template <int CAP, typename F>
inline void dense_row_dispatch(int dtype, int V, int ld, uintptr_t ptrs, F&& f) {
    auto with_type = [&](auto t) {
        constexpr int N = Vec<decltype(t)>::N;
        const bool vec = V % N == 0 && ld % N == 0 && ptrs % 16 == 0, res = V <= CAP;
        if (vec && res) f(t, std::integral_constant<int, N>(), std::true_type());
        else if (vec) f(t, std::integral_constant<int, N>(), std::false_type());
        else if (res) f(t, std::integral_constant<int, 1>(), std::true_type());
        else f(t, std::integral_constant<int, 1>(), std::false_type());
    };
    if (dtype == ASR_F32) with_type(0.f);
    else with_type(bf16_t());
}

// the checks the entry points share; each sets the error and returns its code, ASR_OK otherwise
inline int dense_check_dtype(const char* name, int dtype, size_t* es) {
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "%s: dtype %d", name, dtype);
    *es = dtype == ASR_F32 ? 4 : 2;
    return ASR_OK;
}
inline int dense_check_accumulate(const char* name, int accumulate) {
    if (accumulate != 0 && accumulate != 1) ASR_FAIL(ASR_EINVAL, "%s: accumulate=%d (0 or 1)", name, accumulate);
    return ASR_OK;
}
inline int dense_check_grad_scale(const char* name, float grad_scale) {
    if (!(grad_scale == grad_scale) || grad_scale - grad_scale != 0.f) ASR_FAIL(ASR_EINVAL, "%s: grad_scale is not finite", name);
    return ASR_OK;
}
// two blocks of `rows` rows of V elements, ld apart, of `es` bytes each: do their spans of (rows - 1) ld + V elements overlap?
inline bool dense_overlap(const void* a, const void* b, size_t rows, int V, int ld, size_t es) {
    const size_t span = ((rows - 1) * ld + V) * es;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + span && y < x + span;
}
