// CTC forced alignment of whole recordings (asr_ctc_align_long): the best single path of up to 8192 labels through any number of frames,
// in the log domain and in fp64, bit for bit the definition of tests/align_long_ref.py.
//
// One workgroup per recording.  Pair i = (Bk[i], Lb[i]) = the states (2i, 2i+1), i < L, lives in registers of thread i / P (a contiguous
// block of P pairs per thread, P = 1, 2, 4, 8 by L); the last state 2L ("tail") is one more register of every thread, meaningful in the
// thread that owns pair L-1.  A frame step needs one value from outside the thread, Lb[i0 - 1]: inside a wave it comes over the DPP
// crossbar, across waves through a double-buffered LDS slot, so ONE workgroup barrier per frame orders both buffers (a wave can be at
// most one frame ahead of the slowest, and then it writes the other buffer).  Emissions are gathered by the thread that owns the label,
// AL_DEPTH frames ahead of the step.  Every step stores one back-pointer byte per pair (coalesced, P bytes per thread):
//   bit 0      blank state 2i:   0 = stay, 1 = from Lb[i-1]
//   bits 1..2  label state 2i+1: 0 = stay, 1 = from Bk[i], 2 = from Lb[i-1] (skip)            (the coding of ctc_viterbi_recursion)
//   bit 3      the tail 2L, in the byte of pair L-1: 0 = stay, 1 = from Lb[L-1]
// Ties prefer the state itself, then s-1, then s-2 (strict >); the end prefers the blank.
// The backtrace is a chain of one dependent read per frame.  The byte that holds a state's code ("column": s >> 1, L-1 for the tail)
// moves down by at most one per frame, so AL_F frames need the AL_F + 1 columns below the current one: that window of the back-pointer
// rows is staged into LDS by the whole workgroup, one thread walks it, and the workgroup writes the block's frames of path[].
// Spans come from a pass with a thread per frame, the token sums from a pass with a thread per token over its run, ascending t.
//
// FILL (asr_ctc_align_long_filler; the definition is tests/align_filler_ref.py): the blank states whose flag is set (gap[i] for state 2i,
// gap_tail for 2L) are wide: on frame t they emit star[t] where star[t] > lp(t, blank), the blank's value otherwise.  The blank column,
// lse[t] and star[t] are the same for the whole workgroup, so the wide emission is ONE more value per frame and every pair selects
// between two uniform values by its flag, which - like skip[] - does not change over the frames.  Nothing more is stored per frame: the
// per-block pass of the backtrace, which has a thread per frame, recomputes the choice and writes -2 for a filler frame.
#include "asr_common.h"

namespace {

constexpr int AL_MAXL = ASR_ALIGN_LONG_MAX_LABELS;
constexpr int AL_F = 128;         // frames per staged backtrace window
constexpr int AL_WB = AL_F + 8;   // bytes per window row: AL_F + 1 columns, the start aligned down to 4, rounded up to 8

template <typename T> __device__ __forceinline__ float al_ld(const T* p) { return to_f32<T>(*p); }

template <int P> struct al_code;
template <> struct al_code<1> { typedef uint8_t type; };
template <> struct al_code<2> { typedef uint16_t type; };
template <> struct al_code<4> { typedef uint32_t type; };
template <> struct al_code<8> { typedef uint64_t type; };

__device__ __forceinline__ int al_row_bytes(int L) { return (max(L, 1) + 63) & ~63; }

// the class (pairs per thread) of a label count: 64, 128, 256 and 1024 threads
__host__ __device__ constexpr int al_threads(int P) { return P == 1 ? 64 : P == 2 ? 128 : P == 4 ? 256 : 1024; }
__device__ __forceinline__ int al_class(int L) { return L <= 64 ? 1 : L <= 256 ? 2 : L <= 1024 ? 4 : 8; }

template <bool FILL> struct al_star { float v; };      // a ring slot's star[t]: no member without FILL
template <> struct al_star<false> {};

// what a wide blank state emits on a frame whose blank emits eb (strict >: the blank wins ties)
__device__ __forceinline__ float al_wide(float star, float eb) { return star > eb ? star : eb; }

template <typename T, int P, bool FILL>
__global__ __launch_bounds__(al_threads(P)) void ctc_align_long_kernel(const T* __restrict__ rows, const float* __restrict__ lse,
                                                                       const int32_t* __restrict__ row_off, const int32_t* __restrict__ labels,
                                                                       const int32_t* __restrict__ lab_off, const float* __restrict__ star,
                                                                       const uint8_t* __restrict__ gap,
                                                                       const uint8_t* __restrict__ gap_tail, int32_t* __restrict__ path,
                                                                       int32_t* __restrict__ spans, float* __restrict__ tok,
                                                                       double* __restrict__ score, uint8_t* __restrict__ ws, size_t ws_bytes,
                                                                       int V, int ld, int blank) {
    constexpr int NT = al_threads(P);
    constexpr int NW = NT / 64;
    constexpr int AL_DEPTH = P == 8 ? 3 : 4;      // frames of emissions in flight ahead of the step: a ring of slots, each refilled as soon as it
                                                  // is used (P = 8: 16 waves leave 128 registers a lane, and a fourth slot spills)
    typedef typename al_code<P>::type code_t;
    __shared__ double s_x[2][NW + 1];
    __shared__ double s_fin[2];
    __shared__ int s_state;
    __shared__ int s_path[AL_F];
    __shared__ __attribute__((aligned(16))) uint8_t s_win[AL_F * AL_WB];

    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = row_off[r], l0 = lab_off[r];
    const int Tn = max(row_off[r + 1] - r0, 0);
    const int Lraw = max(lab_off[r + 1] - l0, 0);
    if (al_class(min(Lraw, AL_MAXL)) != P) return;      // another instantiation's recording (uniform: the whole workgroup leaves)
    const bool too_long = Lraw > AL_MAXL;                // refused by the wrapper; here: reported as infeasible, nothing past the tables
    const int L = too_long ? 0 : Lraw;
    // this recording's back-pointer rows: behind those of the recordings before it
    size_t off = 0;
    for (int q = 0; q < r; ++q) {
        const int Tq = max(row_off[q + 1] - row_off[q], 0), Lq = max(lab_off[q + 1] - lab_off[q], 0);
        if (Lq >= 1 && Lq <= AL_MAXL) off += (size_t)Tq * al_row_bytes(Lq);
    }
    const int Wr = al_row_bytes(L);
    const bool ws_ok = L == 0 || off + (size_t)Tn * Wr <= ws_bytes;
    uint8_t* bp = ws + off;
    const T* rw = rows + (size_t)max(r0, 0) * ld;
    const float* ls = lse + max(r0, 0);
    const int32_t* lab = labels + max(l0, 0);
    int32_t* pth = path + max(r0, 0);
    int32_t* spn = spans + (size_t)max(l0, 0) * 2;
    float* tk = tok + (size_t)max(l0, 0) * 3;
    const float* sr = FILL ? star + max(r0, 0) : nullptr;
    const uint8_t* gp = FILL ? gap + max(l0, 0) : nullptr;
    const bool wtail = FILL && gap_tail[r] != 0;

    for (int i = tid; i < L; i += NT) {      // overwritten below for a feasible alignment
        spn[2 * i] = -1;
        spn[2 * i + 1] = -1;
        tk[3 * i] = -INFINITY;
        tk[3 * i + 1] = -INFINITY;
        tk[3 * i + 2] = -INFINITY;
    }
    for (int t = tid; t < Tn; t += NT) pth[t] = -1;

    if (L == 0 || Tn == 0 || !ws_ok) {
        if (tid == 0) {
            double v = (L == 0 && Lraw == 0 && ws_ok) ? 0.0 : -INFINITY;      // T = 0 is feasible iff L = 0
            if (L == 0 && !too_long)
                for (int t = 0; t < Tn; ++t) {
                    float eb = al_ld(rw + (size_t)t * ld + blank) - ls[t];
                    if (FILL && wtail) eb = al_wide(sr[t], eb);
                    const double e = (double)eb;
                    v = t == 0 ? e : v + e;
                }
            score[r] = v;
        }
        if (FILL && wtail && L == 0 && !too_long)      // the one state is the tail; pth[t] = -1 above came from the same thread
            for (int t = tid; t < Tn; t += NT)
                if (sr[t] > al_ld(rw + (size_t)t * ld + blank) - ls[t]) pth[t] = -2;
        return;
    }

    // ------------------------------------------------------------------ recursion
    const int i0 = tid * P;
    const bool active = wave * 64 * P < L;      // wave-uniform: a wave without pairs only keeps the barriers
    unsigned cls[P];      // byte offsets of the thread's labels in a row
    bool skip[P], wide[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int i = i0 + j;
        const int c = i < L ? lab[i] : blank;
        cls[j] = (unsigned)min(max(c, 0), V - 1) * (unsigned)sizeof(T);
        skip[j] = i >= 1 && i < L && lab[i] != lab[i - 1];
        wide[j] = false;
        if constexpr (FILL) wide[j] = i < L && gp[i] != 0;
    }
    const int jl = L - 1 - i0;      // the pair L-1 within this thread, if 0 <= jl < P
    double bk[P], lb[P], tl = -INFINITY;
    {
        const float l = ls[0];
        float e0 = al_ld(rw + blank) - l;
        const float e1 = al_ld((const T*)((const char*)rw + cls[0])) - l;
        if constexpr (FILL)
            if (gp[0] != 0) e0 = al_wide(sr[0], e0);      // state 0 of the recording (used by thread 0 alone)
#pragma unroll
        for (int j = 0; j < P; ++j) {
            bk[j] = (tid == 0 && j == 0) ? (double)e0 : -INFINITY;
            lb[j] = (tid == 0 && j == 0) ? (double)e1 : -INFINITY;
        }
    }
    struct Ring { float lse; T eb, el[P]; al_star<FILL> st; };      // as loaded: a conversion at load time would wait for the load
    Ring q[AL_DEPTH];
    auto fetch = [&](Ring& d, int t) {
        t = min(t, Tn - 1);
        const T* p = rw + (size_t)t * ld;
        d.lse = ls[t];
        d.eb = p[blank];
        if constexpr (FILL) d.st.v = sr[t];
#pragma unroll
        for (int j = 0; j < P; ++j) d.el[j] = *(const T*)((const char*)p + cls[j]);
    };
    if (active) {
#pragma unroll
        for (int k = 0; k < AL_DEPTH; ++k) fetch(q[k], 1 + k);
    }
    for (int t0 = 1; t0 < Tn; t0 += AL_DEPTH) {
#pragma unroll
        for (int k = 0; k < AL_DEPTH; ++k) {
            const int t = t0 + k;
            if (t >= Tn) break;      // uniform
            double up = -INFINITY;
            if (active) up = wave_shr1(lb[P - 1]);
            if (NW > 1) {
                if (active && lane == 63) s_x[t & 1][wave + 1] = lb[P - 1];
                __syncthreads();
                if (active && lane == 0 && wave > 0) up = s_x[t & 1][wave];
            }
            if (active) {
                if (tid == 0) up = -INFINITY;
                const float ebf = to_f32<T>(q[k].eb) - q[k].lse;
                const double eb = (double)ebf;
                double ew = eb;      // what a wide blank emits on this frame: uniform, like eb
                if constexpr (FILL) ew = (double)al_wide(q[k].st.v, ebf);
                double lsel = -INFINITY;      // Lb[L-1] of the previous frame, in the thread that owns it
                code_t code = 0;
                double carry = up;
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const double el = (double)(to_f32<T>(q[k].el[j]) - q[k].lse);
                    const double b = bk[j], l = lb[j];
                    if (j == jl) lsel = l;
                    const bool fb = carry > b;
                    double ml = l;
                    unsigned cl = 0u;
                    if (b > ml) { ml = b; cl = 1u; }
                    if (skip[j] && carry > ml) { ml = carry; cl = 2u; }
                    bk[j] = (fb ? carry : b) + (FILL && wide[j] ? ew : eb);
                    lb[j] = ml + el;
                    unsigned cj = (fb ? 1u : 0u) | (cl << 1);
                    if (j == jl && lsel > tl) cj |= 8u;
                    code |= (code_t)cj << (8 * j);
                    carry = l;
                }
                tl = (lsel > tl ? lsel : tl) + (wtail ? ew : eb);
                if (i0 < Wr) *(code_t*)(bp + (size_t)t * Wr + i0) = code;
                fetch(q[k], t + AL_DEPTH);      // the slot's next frame
            }
        }
    }
    if (jl >= 0 && jl < P) {
        double lsel = lb[0];
#pragma unroll
        for (int j = 1; j < P; ++j)
            if (j == jl) lsel = lb[j];
        s_fin[0] = tl;
        s_fin[1] = lsel;
    }
    __syncthreads();      // s_fin, and every back-pointer store of the workgroup, before the backtrace reads them

    // ------------------------------------------------------------------ backtrace
    const double fb = s_fin[0], fl = s_fin[1];
    const double best = fb >= fl ? fb : fl;      // ties: end in the blank
    const bool feasible = best > -INFINITY;
    if (tid == 0) score[r] = feasible ? best : -INFINITY;
    if (!feasible) return;      // uniform
    int s = fb >= fl ? 2 * L : 2 * L - 1;
    for (int thi = Tn - 1; thi >= 0; thi -= AL_F) {
        const int tlo = max(thi - AL_F + 1, 0), nrow = thi - tlo + 1;
        const int col = min(s >> 1, L - 1);
        const int c0 = max(col - AL_F, 0) & ~3;
        // rows tlo .. thi, columns c0 .. c0 + AL_WB - 1 (inside the row) -> LDS, 4 bytes a piece
        for (int k = tid; k < nrow * (AL_WB / 4); k += NT) {
            const int row = k / (AL_WB / 4), w = k - row * (AL_WB / 4);
            const int c = c0 + 4 * w, t = tlo + row;
            uint32_t v = 0u;
            if (c < Wr && t > 0) v = *(const uint32_t*)(bp + (size_t)t * Wr + c);      // row 0 is never written
            *(uint32_t*)(s_win + row * AL_WB + 4 * w) = v;
        }
        __syncthreads();
        if (tid == 0) {
            for (int t = thi; t >= tlo; --t) {
                s_path[t - tlo] = s;
                if (t > 0) {
                    const int cc = min(max(min(s >> 1, L - 1) - c0, 0), AL_WB - 1);
                    const unsigned cb = s_win[(t - tlo) * AL_WB + cc];
                    const int d = s == 2 * L ? (int)((cb >> 3) & 1u) : (s & 1) ? (int)((cb >> 1) & 3u) : (int)(cb & 1u);
                    s = max(s - min(d, 2), 0);
                }
            }
            s_state = s;
        }
        __syncthreads();
        s = s_state;
        for (int k = tid; k < nrow; k += NT) {
            const int st = s_path[k];
            int out = (st & 1) ? min(st >> 1, L - 1) : -1;
            if constexpr (FILL) {
                if (!(st & 1) && (st >= 2 * L ? wtail : gp[max(st >> 1, 0)] != 0)) {
                    const int t = tlo + k;
                    if (sr[t] > al_ld(rw + (size_t)t * ld + blank) - ls[t]) out = -2;
                }
            }
            pth[tlo + k] = out;
        }
    }
    __syncthreads();      // path[] of the whole recording

    // ------------------------------------------------------------------ spans, then the token sums over each run
    for (int t = tid; t < Tn; t += NT) {
        const int i = pth[t];
        if (i < 0) continue;
        if (t == 0 || pth[t - 1] != i) spn[2 * i] = t;
        if (t == Tn - 1 || pth[t + 1] != i) spn[2 * i + 1] = t;
    }
    __syncthreads();
    for (int i = tid; i < L; i += NT) {
        const int a = min(max(spn[2 * i], 0), Tn - 1), e = min(spn[2 * i + 1], Tn - 1);
        const int c = min(max(lab[i], 0), V - 1);
        float sm = 0.f, mx = -INFINITY, mn = INFINITY;
        for (int t = a; t <= e; ++t) {
            const float v = al_ld(rw + (size_t)t * ld + c) - ls[t];
            sm += v;
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
        }
        tk[3 * i] = sm;
        tk[3 * i + 1] = mx;
        tk[3 * i + 2] = mn;
    }
}

}      // namespace

extern "C" size_t asr_ctc_align_long_workspace_bytes(int R, int T_total, int Lmax) {
    if (R <= 0 || T_total < 0 || Lmax < 0) return 0;
    const size_t row = ((size_t)(Lmax > 1 ? Lmax : 1) + 63) / 64 * 64;
    return (size_t)T_total * row + 64;
}

// validation shared by the two entry points (what = the entry point's name, for the message)
static int al_validate(const char* what, const void* rows, const float* lse, const int32_t* row_off, const int32_t* labels, const int32_t* lab_off,
                       const int32_t* path, const int32_t* spans, const float* tok, const double* score, const void* ws, size_t ws_bytes, int R,
                       int V, int ld, int dtype, int blank) {
    if (!rows || !lse || !row_off || !labels || !lab_off || !path || !spans || !tok || !score || !ws) ASR_FAIL(ASR_EINVAL, "%s: null pointer", what);
    if (R <= 0 || V <= 1 || blank < 0 || blank >= V) ASR_FAIL(ASR_EINVAL, "%s: bad shape R=%d V=%d blank=%d", what, R, V, blank);
    if (ld < V) ASR_FAIL(ASR_EINVAL, "%s: row stride ld=%d below V=%d", what, ld, V);
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "%s: dtype %d", what, dtype);
    if (ws_bytes < 64) ASR_FAIL(ASR_EINVAL, "%s: workspace %zu < 64", what, ws_bytes);
    if (((uintptr_t)ws & 15) || ((uintptr_t)score & 7) || ((uintptr_t)rows & (dtype == ASR_F32 ? 3 : 1))) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", what);
    return 0;
}

// one launch per instantiation: a workgroup whose recording belongs to another one leaves at once
#define AL_LAUNCH(TY, PP, FF)                                                                                                                  \
    ctc_align_long_kernel<TY, PP, FF><<<R, al_threads(PP), 0, st>>>((const TY*)rows, lse, row_off, labels, lab_off, star, gap, gap_tail, path, \
                                                                      spans, tok, score, (uint8_t*)ws, ws_bytes, V, ld, blank)
#define AL_LAUNCH_ALL(FF)                                                                                                    \
    if (dtype == ASR_F32) {                                                                                                  \
        AL_LAUNCH(float, 1, FF); AL_LAUNCH(float, 2, FF); AL_LAUNCH(float, 4, FF); AL_LAUNCH(float, 8, FF);                  \
    } else {                                                                                                                 \
        AL_LAUNCH(bf16_t, 1, FF); AL_LAUNCH(bf16_t, 2, FF); AL_LAUNCH(bf16_t, 4, FF); AL_LAUNCH(bf16_t, 8, FF);              \
    }

extern "C" int asr_ctc_align_long(const void* rows, const float* lse, const int32_t* row_off, const int32_t* labels, const int32_t* lab_off,
                                  int32_t* path, int32_t* spans, float* tok, double* score, void* ws, size_t ws_bytes, int R, int V, int ld,
                                  int dtype, int blank, void* stream) {
    if (int rc = al_validate("asr_ctc_align_long", rows, lse, row_off, labels, lab_off, path, spans, tok, score, ws, ws_bytes, R, V, ld, dtype, blank)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float* star = nullptr;
    const uint8_t *gap = nullptr, *gap_tail = nullptr;      // never read without FILL
    AL_LAUNCH_ALL(false)
    ASR_CHECK_LAUNCH("asr_ctc_align_long");
    return 0;
}

extern "C" int asr_ctc_align_long_filler(const void* rows, const float* lse, const float* star, const int32_t* row_off, const int32_t* labels,
                                         const int32_t* lab_off, const uint8_t* gap, const uint8_t* gap_tail, int32_t* path, int32_t* spans,
                                         float* tok, double* score, void* ws, size_t ws_bytes, int R, int V, int ld, int dtype, int blank,
                                         void* stream) {
    if (!star || !gap || !gap_tail) ASR_FAIL(ASR_EINVAL, "asr_ctc_align_long_filler: null pointer");
    if (int rc = al_validate("asr_ctc_align_long_filler", rows, lse, row_off, labels, lab_off, path, spans, tok, score, ws, ws_bytes, R, V, ld, dtype, blank))
        return rc;
    if ((uintptr_t)star & 3) ASR_FAIL(ASR_EINVAL, "asr_ctc_align_long_filler: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    AL_LAUNCH_ALL(true)
    ASR_CHECK_LAUNCH("asr_ctc_align_long_filler");
    return 0;
}
#undef AL_LAUNCH_ALL
#undef AL_LAUNCH
