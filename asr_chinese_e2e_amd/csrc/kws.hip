// Keyword spotting on the CTC posteriors (asr_chinese_e2e_amd/keywords.py; the definition: tests/kws_ref.py, restated in include/asr_hip.h).
//   asr_kws_search       every keyword against every frame of every utterance, free start and free end: the hits per (utterance, keyword)
//   asr_kws_chunk        the same a chunk at a time, the lattice column and the open run carried in a state: the hits a chunk closes
//   asr_kws_compact      the hits of an utterance in one list, keyword ascending then end ascending (ballot / popcount offsets, no atomics)
//   asr_kws_state_init / asr_kws_state_reset, asr_kws_state_bytes / asr_kws_records_bytes
// One wave per (utterance, 64 keywords), a lane per keyword: the 2L-1 scores and start frames of a keyword's lattice column live in
// registers, the frame loop is serial, and the states of a frame do not depend on each other (one compare-select-add deep per frame).
// The bodies are templates on a length bucket LB (L <= 4, 8, 16): a block's bucket is that of its longest keyword, and the kernel
// branches once (wave-uniform) into that bucket's body - one launch for every bucket, so that short and long keywords run side by side
// (a launch per bucket runs them one after the other).  A keyword list sorted by bucket (keywords.KeywordList) wastes no lane on short
// keywords; any order gives the same bits.  The loads of a group of G frames (LB + 1 gathered logits and the frame's lse each) are
// issued before the selects of the group in front of it, so a wave waits for memory once per group.
#include <vector>

#include "asr_common.h"

namespace {

constexpr int MAXL = ASR_KWS_MAX_LEN;
constexpr int ST_WORDS = 2 * (2 * MAXL - 1) + 5;      // D, start (31 each), the open run {open, start, end, H}, frames consumed
constexpr int W_D = 0, W_ST = 2 * MAXL - 1, W_RUN = 2 * (2 * MAXL - 1), W_FRAMES = W_RUN + 4;

__host__ __device__ constexpr int bucket_of(int L) { return L <= 4 ? 4 : L <= 8 ? 8 : 16; }
template <int LB> struct Group { static constexpr int G = LB == 4 ? 8 : LB == 8 ? 4 : 2; };      // frames whose loads are in flight together

struct Run { int open, start, end; float H; };

// One frame of one keyword: (D, st) of frame t - 1 -> frame t, in place (descending s: a state reads lower states of the frame before).
// e[i] = lp_t(w_i), eb = lp_t(blank); bit i of neq: w_i != w_{i-1}.  Compare-and-select exactly as the definition says, no fmaxf.
template <int LB>
__device__ __forceinline__ void kws_frame_step(float (&D)[2 * LB - 1], int (&st)[2 * LB - 1], const float (&e)[LB], float eb, unsigned neq, int t) {
#pragma unroll
    for (int s = 2 * LB - 2; s >= 1; --s) {
        float best = D[s];
        int bs = st[s];
        if (D[s - 1] > best) { best = D[s - 1]; bs = st[s - 1]; }
        if ((s & 1) == 0 && ((neq >> (s / 2)) & 1u) && D[s - 2] > best) { best = D[s - 2]; bs = st[s - 2]; }
        D[s] = best + ((s & 1) ? eb : e[s / 2]);
        st[s] = best > -INFINITY ? bs : -1;
    }
    D[0] = 0.f + e[0];
    st[0] = t;
}

// a closed run becomes a record while there is room; the count keeps counting
__device__ __forceinline__ void kws_emit(const Run& r, int& cnt, int32_t* __restrict__ rec, int cap) {
    if (cnt < cap) {
        rec[cnt * 3] = r.start; rec[cnt * 3 + 1] = r.end; rec[cnt * 3 + 2] = __float_as_int(r.H);
    }
    cnt += 1;
}

// the candidate rule and the run of one keyword on frame t (H, hs: its end state)
__device__ __forceinline__ void kws_frame_hit(Run& r, float H, int hs, int t, float thr, int span, int& cnt, int32_t* __restrict__ rec, int cap) {
    const bool cand = H >= thr && hs >= 0 && t - hs + 1 <= span;
    if (cand) {
        if (!r.open || H > r.H) { r.start = hs; r.end = t; r.H = H; }      // strict: the first frame of equal H keeps the run
        r.open = 1;
    } else if (r.open) {
        kws_emit(r, cnt, rec, cap);
        r.open = 0;
    }
}

// What a lane knows of its keyword.
template <int LB> struct Lane {
    int tok[LB];      // w_i, clamped to [0, V); entries past L repeat w_0 (loaded, computed with, never read)
    unsigned neq;
    int L, span;
    float thr;
};

// n frames of one utterance / slot through one keyword per lane; both kernels run this.  rows: the utterance's frame 0, lse its lse,
// t0 the session frame of frame 0.  n >= 1; frames past n - 1 in the last group load frame n - 1 again and are not computed with.
template <typename T, int LB>
__device__ __forceinline__ void kws_frames(const T* __restrict__ rows, const float* __restrict__ lse, size_t ld, int n, int t0, int blank, const Lane<LB>& kw,
                                           float (&D)[2 * LB - 1], int (&st)[2 * LB - 1], Run& run, int& cnt, int32_t* __restrict__ rec, int cap) {
    constexpr int G = Group<LB>::G;
    float x[G][LB + 1], l[G];
    auto load = [&](int base, float (&xx)[G][LB + 1], float (&ll)[G]) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int t = min(base + g, n - 1);
            const T* r = rows + (size_t)t * ld;
#pragma unroll
            for (int i = 0; i < LB; ++i) xx[g][i] = to_f32<T>(r[kw.tok[i]]);
            xx[g][LB] = to_f32<T>(r[blank]);
            ll[g] = lse[t];
        }
    };
    load(0, x, l);
    for (int base = 0; base < n; base += G) {
        float xn[G][LB + 1], ln[G];
        load(base + G, xn, ln);      // the next group's loads, ahead of this group's selects (clamped: always in bounds)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (base + g < n) {      // wave-uniform
                float e[LB];
#pragma unroll
                for (int i = 0; i < LB; ++i) e[i] = x[g][i] - l[g];
                const int t = t0 + base + g;
                kws_frame_step<LB>(D, st, e, x[g][LB] - l[g], kw.neq, t);
                float H = D[0];
                int hs = st[0];
#pragma unroll
                for (int i = 1; i < LB; ++i)
                    if (i == kw.L - 1) { H = D[2 * i]; hs = st[2 * i]; }
                kws_frame_hit(run, H, hs, t, kw.thr, kw.span, cnt, rec, cap);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int i = 0; i <= LB; ++i) x[g][i] = xn[g][i];
            l[g] = ln[g];
        }
    }
}

struct Tab { const int32_t* tok; const int32_t* len; const float* thr; const int32_t* span; const int32_t* index; int K; };

// the bucket of the block's longest keyword (wave-uniform)
__device__ __forceinline__ int kws_bucket(const Tab& tab, int j) {
    int Lm = max(1, min(tab.len[min(j, tab.K - 1)], MAXL));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) Lm = max(Lm, __shfl_xor(Lm, o, 64));
    return __builtin_amdgcn_readfirstlane(bucket_of(Lm));
}

// the lane's keyword (row j of the tables, the last row for lanes past K, which write nothing)
template <int LB>
__device__ __forceinline__ void kws_lane(const Tab& tab, int j, int V, Lane<LB>& kw, int& k_out) {
    const int jj = min(j, tab.K - 1);
    const int L = max(1, min(tab.len[jj], LB));
    kw.L = L;
    kw.neq = 0u;
    const int32_t* w = tab.tok + (size_t)jj * MAXL;
#pragma unroll
    for (int i = 0; i < LB; ++i) kw.tok[i] = max(0, min(w[i < L ? i : 0], V - 1));      // i < LB <= MAXL: inside the row
#pragma unroll
    for (int i = 1; i < LB; ++i)
        if (i < L && kw.tok[i] != kw.tok[i - 1]) kw.neq |= 1u << i;
    kw.thr = tab.thr[jj];
    kw.span = tab.span[jj];
    k_out = max(0, min(tab.index[jj], tab.K - 1));
}

__device__ __forceinline__ void kws_finish(int cnt, int32_t* __restrict__ cnt_out, int32_t* __restrict__ rec, int cap) {
    for (int i = min(cnt, cap); i < cap; ++i) { rec[i * 3] = 0; rec[i * 3 + 1] = 0; rec[i * 3 + 2] = 0; }
    *cnt_out = cnt;
}

template <typename T, int LB>
__device__ __forceinline__ void kws_search_body(const T* __restrict__ logits, const float* __restrict__ lse, const int32_t* __restrict__ in_len, const Tab& tab,
                                                int32_t* __restrict__ cnt_out, int32_t* __restrict__ rec_out, int T_, int V, int ld, int blank, int cap) {
    const int b = blockIdx.y, j = blockIdx.x * WAVE + threadIdx.x;
    Lane<LB> kw;
    int k;
    kws_lane<LB>(tab, j, V, kw, k);
    const bool live = j < tab.K;
    const int n = in_len ? max(0, min(in_len[b], T_)) : T_;
    float D[2 * LB - 1];
    int st[2 * LB - 1];
#pragma unroll
    for (int s = 0; s < 2 * LB - 1; ++s) { D[s] = -INFINITY; st[s] = -1; }
    Run run = {0, 0, 0, 0.f};
    int cnt = 0;
    int32_t* rec = rec_out + ((size_t)b * tab.K + k) * cap * 3;
    const int room = live ? cap : 0;      // a lane past K computes its neighbour's keyword again and writes nothing
    if (n > 0) kws_frames<T, LB>(logits + (size_t)b * T_ * ld, lse + (size_t)b * T_, (size_t)ld, n, 0, blank, kw, D, st, run, cnt, rec, room);
    if (run.open) kws_emit(run, cnt, rec, room);      // a run still open behind the last frame closes there
    if (live) kws_finish(cnt, cnt_out + (size_t)b * tab.K + k, rec, cap);
}

// grid (ceil(K / 64), B), one wave.  cnt (B, K), rec (B, K, cap, 3), both indexed by the keyword's own index (tab.index).
template <typename T>
__global__ __launch_bounds__(WAVE) void kws_search_kernel(const T* __restrict__ logits, const float* __restrict__ lse, const int32_t* __restrict__ in_len, Tab tab,
                                                         int32_t* __restrict__ cnt_out, int32_t* __restrict__ rec_out, int T_, int V, int ld, int blank, int cap) {
    switch (kws_bucket(tab, blockIdx.x * WAVE + threadIdx.x)) {
        case 4: kws_search_body<T, 4>(logits, lse, in_len, tab, cnt_out, rec_out, T_, V, ld, blank, cap); break;
        case 8: kws_search_body<T, 8>(logits, lse, in_len, tab, cnt_out, rec_out, T_, V, ld, blank, cap); break;
        default: kws_search_body<T, 16>(logits, lse, in_len, tab, cnt_out, rec_out, T_, V, ld, blank, cap); break;
    }
}

// grid (ceil(K / 64), slots), one wave.  state: per (slot, block of 64 keywords) ST_WORDS rows of 64 lanes (a wave reads and writes whole
// rows) = {D[31], start[31] in session frames, the open run {open, start, end, H}, frames consumed}; a block touches its own rows only.
template <typename T, int LB>
__device__ __forceinline__ void kws_chunk_body(const T* __restrict__ logits, const float* __restrict__ lse, const int32_t* __restrict__ n_valid,
                                               const int32_t* __restrict__ reset, const int32_t* __restrict__ fin, const Tab& tab, int32_t* __restrict__ state,
                                               int32_t* __restrict__ cnt_out, int32_t* __restrict__ rec_out, int C, int V, int ld, int blank, int cap) {
    const int b = blockIdx.y, lane = threadIdx.x, j = blockIdx.x * WAVE + lane;
    Lane<LB> kw;
    int k;
    kws_lane<LB>(tab, j, V, kw, k);
    const bool live = j < tab.K;
    const int n = max(0, min(n_valid[b], C));
    const bool fresh = reset[b] != 0;
    int32_t* sw = state + ((size_t)b * gridDim.x + blockIdx.x) * ST_WORDS * WAVE + lane;
    float D[2 * LB - 1];
    int st[2 * LB - 1];
#pragma unroll
    for (int s = 0; s < 2 * LB - 1; ++s) {
        D[s] = fresh ? -INFINITY : __int_as_float(sw[(W_D + s) * WAVE]);
        st[s] = fresh ? -1 : sw[(W_ST + s) * WAVE];
    }
    Run run = {0, 0, 0, 0.f};
    int frames = 0;
    if (!fresh) {
        run.open = sw[W_RUN * WAVE]; run.start = sw[(W_RUN + 1) * WAVE]; run.end = sw[(W_RUN + 2) * WAVE]; run.H = __int_as_float(sw[(W_RUN + 3) * WAVE]);
        frames = sw[W_FRAMES * WAVE];
    }
    int cnt = 0;
    int32_t* rec = rec_out + ((size_t)b * tab.K + k) * cap * 3;
    const int room = live ? cap : 0;
    if (n > 0) kws_frames<T, LB>(logits + (size_t)b * C * ld, lse + (size_t)b * C, (size_t)ld, n, frames, blank, kw, D, st, run, cnt, rec, room);
    if (fin[b] != 0 && run.open) {
        kws_emit(run, cnt, rec, room);
        run.open = 0;
    }
    if (live) kws_finish(cnt, cnt_out + (size_t)b * tab.K + k, rec, cap);
    if (n > 0 || fresh || fin[b] != 0) {      // otherwise every word keeps its value: the slot sits this tick out
#pragma unroll
        for (int s = 0; s < 2 * LB - 1; ++s) {
            sw[(W_D + s) * WAVE] = __float_as_int(D[s]);
            sw[(W_ST + s) * WAVE] = st[s];
        }
        sw[W_RUN * WAVE] = run.open; sw[(W_RUN + 1) * WAVE] = run.start; sw[(W_RUN + 2) * WAVE] = run.end; sw[(W_RUN + 3) * WAVE] = __float_as_int(run.H);
        sw[W_FRAMES * WAVE] = frames + n;
    }
}

template <typename T>
__global__ __launch_bounds__(WAVE) void kws_chunk_kernel(const T* __restrict__ logits, const float* __restrict__ lse, const int32_t* __restrict__ n_valid,
                                                        const int32_t* __restrict__ reset, const int32_t* __restrict__ fin, Tab tab, int32_t* __restrict__ state,
                                                        int32_t* __restrict__ cnt_out, int32_t* __restrict__ rec_out, int C, int V, int ld, int blank, int cap) {
    switch (kws_bucket(tab, blockIdx.x * WAVE + threadIdx.x)) {
        case 4: kws_chunk_body<T, 4>(logits, lse, n_valid, reset, fin, tab, state, cnt_out, rec_out, C, V, ld, blank, cap); break;
        case 8: kws_chunk_body<T, 8>(logits, lse, n_valid, reset, fin, tab, state, cnt_out, rec_out, C, V, ld, blank, cap); break;
        default: kws_chunk_body<T, 16>(logits, lse, n_valid, reset, fin, tab, state, cnt_out, rec_out, C, V, ld, blank, cap); break;
    }
}

// flags == NULL: every slot.  One thread per state word.
__global__ __launch_bounds__(256) void kws_state_reset_kernel(int32_t* __restrict__ state, const int32_t* __restrict__ flags, int per_slot) {
    const int b = blockIdx.y;
    if (flags && flags[b] == 0) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per_slot; i += gridDim.x * blockDim.x) {
        const int w = (i / WAVE) % ST_WORDS;
        state[(size_t)b * per_slot + i] = w < W_ST ? __float_as_int(-INFINITY) : w < W_RUN ? -1 : 0;
    }
}

// One wave per utterance.  The place of keyword k's r-th record is the number of kept records of the keywords in front of it plus r: the
// keywords of a block of 64 count them with one ballot per record index (kept > r) and the popcount of the lanes below.
__global__ __launch_bounds__(WAVE) void kws_compact_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ rec, int32_t* __restrict__ count,
                                                          int32_t* __restrict__ dropped, int32_t* __restrict__ hits, int K, int cap, int max_hits) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    int32_t* out = hits + (size_t)b * max_hits * 4;
    int base = 0;
    long long found = 0;
    for (int k0 = 0; k0 < K; k0 += WAVE) {
        const int k = k0 + lane;
        const int c = k < K ? max(0, cnt[(size_t)b * K + k]) : 0;
        const int kept = min(c, cap);
        int pre = 0, tot = 0;
        for (int r = 0; r < cap; ++r) {
            const unsigned long long m = __ballot(kept > r);
            if (m == 0ull) break;      // wave-uniform
            pre += __popcll(m & below);
            tot += __popcll(m);
        }
        const int32_t* src = rec + ((size_t)b * K + min(k, K - 1)) * cap * 3;
        for (int r = 0; r < kept; ++r) {
            const int pos = base + pre + r;
            if (pos < max_hits) {
                out[pos * 4] = k; out[pos * 4 + 1] = src[r * 3]; out[pos * 4 + 2] = src[r * 3 + 1]; out[pos * 4 + 3] = src[r * 3 + 2];
            }
        }
        base += tot;
        long long f = c;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) f += __shfl_xor(f, o, 64);
        found += f;
    }
    const int n = min(base, max_hits);
    for (int i = n * 4 + lane; i < max_hits * 4; i += WAVE) out[i] = 0;
    if (lane == 0) {
        count[b] = n;
        dropped[b] = (int32_t)min(found - n, (long long)INT_MAX);
    }
}

// The list as the launchers check it, on the host and before any launch: the kernels clamp what they read from the device tables, this
// is what makes the clamps idle.
int kws_list_args(const char* name, const asr_kws_list* kw, int V, int blank) {
    if (!kw) ASR_FAIL(ASR_EINVAL, "%s: null keyword list", name);
    if (kw->K < 1 || kw->K > ASR_KWS_MAX_KEYWORDS) ASR_FAIL(ASR_EINVAL, "%s: K=%d keywords (1..%d)", name, kw->K, ASR_KWS_MAX_KEYWORDS);
    if (!kw->tok || !kw->len || !kw->thr || !kw->span || !kw->index || !kw->host_tok || !kw->host_len || !kw->host_index)
        ASR_FAIL(ASR_EINVAL, "%s: null pointer in the keyword list", name);
    if (((uintptr_t)kw->tok | (uintptr_t)kw->len | (uintptr_t)kw->thr | (uintptr_t)kw->span | (uintptr_t)kw->index | (uintptr_t)kw->host_tok |
         (uintptr_t)kw->host_len | (uintptr_t)kw->host_index) % 4)
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer in the keyword list", name);
    if (V < 2 || blank < 0 || blank >= V) ASR_FAIL(ASR_EINVAL, "%s: bad shape V=%d blank=%d", name, V, blank);
    std::vector<bool> seen((size_t)kw->K, false);
    for (int j = 0; j < kw->K; ++j) {
        const int L = kw->host_len[j];
        if (L < 1 || L > MAXL) ASR_FAIL(ASR_EINVAL, "%s: keyword row %d has length %d (1..%d)", name, j, L, MAXL);
        for (int i = 0; i < L; ++i) {
            const int w = kw->host_tok[(size_t)j * MAXL + i];
            if (w < 0 || w >= V || w == blank) ASR_FAIL(ASR_EINVAL, "%s: keyword row %d, token %d: id %d is the blank or outside [0, %d)", name, j, i, w, V);
        }
        const int k = kw->host_index[j];
        if (k < 0 || k >= kw->K || seen[(size_t)k]) ASR_FAIL(ASR_EINVAL, "%s: keyword row %d: index %d is outside [0, %d) or taken", name, j, k, kw->K);
        seen[(size_t)k] = true;
    }
    return ASR_OK;
}

int kws_frame_args(const char* name, const void* logits, int B, int T, int V, int ld, int dtype, int K, int cap) {
    if (B <= 0 || B > 65535 || T <= 0 || V <= 1 || (size_t)B * T > (size_t)INT_MAX) ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d (1..65535) T=%d V=%d", name, B, T, V);
    if (ld < V) ASR_FAIL(ASR_EINVAL, "%s: row stride ld=%d < V=%d", name, ld, V);
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "%s: dtype %d", name, dtype);
    if ((uintptr_t)logits % (dtype == ASR_F32 ? 4 : 2)) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    if (cap < 1 || cap > ASR_KWS_MAX_CAP || (size_t)B * K * cap * 3 > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "%s: bad shape cap=%d (1..%d) for B=%d K=%d", name, cap, ASR_KWS_MAX_CAP, B, K);
    return ASR_OK;
}

Tab tab_of(const asr_kws_list* kw) { return {kw->tok, kw->len, kw->thr, kw->span, kw->index, kw->K}; }

}  // namespace

extern "C" size_t asr_kws_state_bytes(int slots, int K) {
    if (slots <= 0 || K <= 0) return 0;
    return (size_t)slots * ceil_div(K, WAVE) * ST_WORDS * WAVE * sizeof(int32_t);
}

extern "C" size_t asr_kws_records_bytes(int B, int K, int cap) {
    if (B <= 0 || K <= 0 || cap <= 0) return 0;
    return (size_t)B * K * cap * 3 * sizeof(int32_t);
}

extern "C" int asr_kws_search(const void* logits, const float* lse, const int32_t* in_len, const asr_kws_list* kw, int32_t* cnt, int32_t* rec, int B, int T, int V,
                              int ld, int blank, int cap, int dtype, void* stream) {
    if (!logits || !lse || !cnt || !rec) ASR_FAIL(ASR_EINVAL, "asr_kws_search: null pointer");
    int rc = kws_list_args("asr_kws_search", kw, V, blank);
    if (rc != ASR_OK) return rc;
    rc = kws_frame_args("asr_kws_search", logits, B, T, V, ld, dtype, kw->K, cap);
    if (rc != ASR_OK) return rc;
    if (((uintptr_t)lse | (uintptr_t)in_len | (uintptr_t)cnt | (uintptr_t)rec) % 4) ASR_FAIL(ASR_EINVAL, "asr_kws_search: misaligned pointer");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(kw->K, WAVE), B);
    const Tab tab = tab_of(kw);
    if (dtype == ASR_F32) kws_search_kernel<float><<<grid, WAVE, 0, st>>>((const float*)logits, lse, in_len, tab, cnt, rec, T, V, ld, blank, cap);
    else kws_search_kernel<bf16_t><<<grid, WAVE, 0, st>>>((const bf16_t*)logits, lse, in_len, tab, cnt, rec, T, V, ld, blank, cap);
    ASR_CHECK_LAUNCH("asr_kws_search");
    return ASR_OK;
}

extern "C" int asr_kws_chunk(const void* logits, const float* lse, const int32_t* n_valid, const int32_t* reset, const int32_t* final, const asr_kws_list* kw,
                             int32_t* state, int32_t* cnt, int32_t* rec, int slots, int C, int V, int ld, int blank, int cap, int dtype, void* stream) {
    if (!logits || !lse || !n_valid || !reset || !final || !state || !cnt || !rec) ASR_FAIL(ASR_EINVAL, "asr_kws_chunk: null pointer");
    int rc = kws_list_args("asr_kws_chunk", kw, V, blank);
    if (rc != ASR_OK) return rc;
    rc = kws_frame_args("asr_kws_chunk", logits, slots, C, V, ld, dtype, kw->K, cap);
    if (rc != ASR_OK) return rc;
    if (((uintptr_t)lse | (uintptr_t)n_valid | (uintptr_t)reset | (uintptr_t)final | (uintptr_t)state | (uintptr_t)cnt | (uintptr_t)rec) % 4)
        ASR_FAIL(ASR_EINVAL, "asr_kws_chunk: misaligned pointer");
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(kw->K, WAVE), slots);
    const Tab tab = tab_of(kw);
    if (dtype == ASR_F32)
        kws_chunk_kernel<float><<<grid, WAVE, 0, st>>>((const float*)logits, lse, n_valid, reset, final, tab, state, cnt, rec, C, V, ld, blank, cap);
    else
        kws_chunk_kernel<bf16_t><<<grid, WAVE, 0, st>>>((const bf16_t*)logits, lse, n_valid, reset, final, tab, state, cnt, rec, C, V, ld, blank, cap);
    ASR_CHECK_LAUNCH("asr_kws_chunk");
    return ASR_OK;
}

extern "C" int asr_kws_compact(const int32_t* cnt, const int32_t* rec, int32_t* count, int32_t* dropped, int32_t* hits, int B, int K, int cap, int max_hits,
                               void* stream) {
    if (!cnt || !rec || !count || !dropped || !hits) ASR_FAIL(ASR_EINVAL, "asr_kws_compact: null pointer");
    if (B <= 0 || B > 65535 || K < 1 || K > ASR_KWS_MAX_KEYWORDS || cap < 1 || cap > ASR_KWS_MAX_CAP || max_hits < 1 || (size_t)B * K * cap * 3 > (size_t)INT_MAX ||
        (size_t)B * max_hits * 4 > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "asr_kws_compact: bad shape B=%d (1..65535) K=%d (1..%d) cap=%d (1..%d) max_hits=%d", B, K, ASR_KWS_MAX_KEYWORDS, cap, ASR_KWS_MAX_CAP,
                 max_hits);
    if (((uintptr_t)cnt | (uintptr_t)rec | (uintptr_t)count | (uintptr_t)dropped | (uintptr_t)hits) % 4) ASR_FAIL(ASR_EINVAL, "asr_kws_compact: misaligned pointer");
    kws_compact_kernel<<<B, WAVE, 0, (hipStream_t)stream>>>(cnt, rec, count, dropped, hits, K, cap, max_hits);
    ASR_CHECK_LAUNCH("asr_kws_compact");
    return ASR_OK;
}

static int kws_state_launch(const char* name, int32_t* state, const int32_t* flags, int slots, int K, void* stream) {
    if (slots <= 0 || slots > 65535 || K < 1 || K > ASR_KWS_MAX_KEYWORDS || asr_kws_state_bytes(slots, K) / 4 > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "%s: bad shape slots=%d (1..65535) K=%d (1..%d)", name, slots, K, ASR_KWS_MAX_KEYWORDS);
    if (((uintptr_t)state | (uintptr_t)flags) % 4) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    const int per_slot = ceil_div(K, WAVE) * ST_WORDS * WAVE;
    kws_state_reset_kernel<<<dim3(min(ceil_div(per_slot, 256), 64), slots), 256, 0, (hipStream_t)stream>>>(state, flags, per_slot);
    ASR_CHECK_LAUNCH(name);
    return ASR_OK;
}

extern "C" int asr_kws_state_init(int32_t* state, int slots, int K, void* stream) {
    if (!state) ASR_FAIL(ASR_EINVAL, "asr_kws_state_init: null pointer");
    return kws_state_launch("asr_kws_state_init", state, nullptr, slots, K, stream);
}

extern "C" int asr_kws_state_reset(int32_t* state, const int32_t* flags, int slots, int K, void* stream) {
    if (!state || !flags) ASR_FAIL(ASR_EINVAL, "asr_kws_state_reset: null pointer");
    return kws_state_launch("asr_kws_state_reset", state, flags, slots, K, stream);
}
