// Consensus decoding of n-best lists (include/asr_hip.h: asr_nbest_consensus; the definition is tests/consensus_ref.py, and the kernels
// agree with it integer for integer).  Three launches on one stream, no atomics, a fixed order everywhere: two runs write the same bytes.
//
// 1. nbest_pair_dist_kernel: one wave per (utterance, pair i < k).  The distance-only forward pass of edit_wave.h, h_i on the row side
//    and h_k on the column side.  Writes d[u][i][k] and d[u][k][i]; one more workgroup per utterance writes the diagonal.
// 2. nbest_pivot_votes_kernel: one wave per (utterance, entry k).  Every wave recomputes the utterance's risks from d (lane i sums over k
//    in index order, int64) and takes the pivot by a wave argmin on (risk, i), so no launch stands between the risks and their use.  It
//    aligns h_k to the pivot (the pivot is the row side; edit_wave.h with its masks sink) with the two direction bits of a cell as ballot
//    masks in LDS, 16 bytes per (row, column block): at most 256 * 4 * 16 = 16 KB.  Lane 0 walks back from (m, n) and writes h_k's votes into an LDS image of the 2 m + 1
//    slots; the walk meets an insertion run last token first, so the LAST write into a gap's slot is the run's first token and every
//    earlier one is an extra insertion.  The wave then copies the image out.
// 3. nbest_slot_vote_kernel: one wave per (utterance, slot).  Lane k holds entry k's vote and weight.  A 64-step v_readlane sweep gives
//    every lane its group's weight and leader (the lowest lane with the same vote); a second sweep ranks the leaders by (weight
//    descending, lane ascending); the top A write (token, weight).
//
// PRECONDITION of the forward pass and of the v_readlane sweeps: the whole wave executes them - every loop around them has wave-uniform
// bounds, and a wave that leaves early leaves as a whole.
#include <limits.h>

#include "asr_common.h"
#include "edit_wave.h"

namespace {

constexpr int NBEST_EPS = ASR_NBEST_EPS;
constexpr int NBEST_NB = ASR_NBEST_MAX_LEN / 64;      // column blocks of the longest hypothesis

__host__ __device__ __forceinline__ int nbest_len(int v, int L) { return v < 0 ? -1 : (v > L ? L : v); }      // -1: absent

// Output layout, in int32 words from `out` (8-byte aligned; the risks come first because they are int64).  S = 2 L + 1.
struct NbestLayout {
    size_t risk, d, pivot, wsum, extra, n_alts, pivot_w, votes, alts, words;
};
__host__ __device__ __forceinline__ NbestLayout nbest_layout(int U, int N, int L, int A) {
    const size_t u = (size_t)U, n = (size_t)N, s = 2 * (size_t)L + 1;
    NbestLayout o;
    o.risk = 0;
    o.d = o.risk + 2 * u * n;
    o.pivot = o.d + u * n * n;
    o.wsum = o.pivot + u;
    o.extra = o.wsum + u;
    o.n_alts = o.extra + u * n;
    o.pivot_w = o.n_alts + u * s;
    o.votes = o.pivot_w + u * s;
    o.alts = o.votes + u * n * s;
    o.words = o.alts + u * s * (size_t)A * 2;
    return o;
}

struct NbestArgs {
    const int32_t* tok;
    const int32_t* len;
    const int32_t* weights;
    int L, ldn, ldu, U, N, A;
    int32_t* out;
};

__global__ __launch_bounds__(64) void nbest_pair_dist_kernel(NbestArgs a, size_t off_d) {
    __shared__ int carryD[ASR_NBEST_MAX_LEN + 1];
    const int u = blockIdx.y, lane = threadIdx.x, N = a.N;
    const int npairs = N * (N - 1) / 2;
    int32_t* d = a.out + off_d + (size_t)u * N * N;
    int p = blockIdx.x;
    if (p >= npairs) {      // the last workgroup of an utterance: the diagonal
        if (lane < N) d[lane * N + lane] = 0;
        return;
    }
    int i = 0;      // pair p of the upper triangle, row by row
    while (p >= N - 1 - i) {
        p -= N - 1 - i;
        ++i;
    }
    const int k = i + 1 + p;
    const int m = nbest_len(a.len[(size_t)u * N + i], a.L), n = nbest_len(a.len[(size_t)u * N + k], a.L);
    int dist = 0;      // a pair with an absent side
    if (m >= 0 && n >= 0) {
        const int32_t* row = a.tok + (size_t)u * a.ldu;
        EditSinkNone none;
        dist = edit_wave_forward(row + (size_t)i * a.ldn, m, row + (size_t)k * a.ldn, n, carryD, lane, none);
    }
    if (lane == 0) {
        d[i * N + k] = dist;
        d[k * N + i] = dist;
    }
}

__global__ __launch_bounds__(64) void nbest_pivot_votes_kernel(NbestArgs a, NbestLayout o) {
    __shared__ __align__(16) ulonglong2 dir[ASR_NBEST_MAX_LEN * NBEST_NB];
    __shared__ int carryD[ASR_NBEST_MAX_LEN + 1];
    __shared__ int image[2 * ASR_NBEST_MAX_LEN + 1];
    __shared__ int hk[ASR_NBEST_MAX_LEN];
    const int u = blockIdx.y, k = blockIdx.x, lane = threadIdx.x, N = a.N, S = 2 * a.L + 1;
    const int32_t* len = a.len + (size_t)u * N;
    const int32_t* wts = a.weights + (size_t)u * N;
    const int32_t* d = a.out + o.d + (size_t)u * N * N;
    // the risks: lane i sums w_k * d[i][k] over the present k in index order
    const bool mine = lane < N && nbest_len(len[min(lane, N - 1)], a.L) >= 0;
    long long risk = 0;
    int W = 0;
    for (int q = 0; q < N; ++q) {
        if (nbest_len(len[q], a.L) < 0) continue;      // wave-uniform
        const int w = max(wts[q], 0);
        W += w;
        if (mine) risk += (long long)w * d[lane * N + q];
    }
    // argmin on (risk, lane) over the present lanes
    long long br = mine ? risk : LLONG_MAX;
    int bi = mine ? lane : INT_MAX;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const long long orisk = __shfl_xor(br, s, 64);
        const int oi = __shfl_xor(bi, s, 64);
        if (orisk < br || (orisk == br && oi < bi)) {
            br = orisk;
            bi = oi;
        }
    }
    const int pivot = min(max(bi, 0), N - 1);      // the launcher refused an utterance without a present entry; clamped all the same
    if (k == 0) {
        if (lane < N) ((long long*)(a.out + o.risk))[(size_t)u * N + lane] = mine ? risk : 0ll;
        if (lane == 0) {
            a.out[o.pivot + u] = pivot;
            a.out[o.wsum + u] = W;
        }
    }
    int32_t* votes = a.out + o.votes + ((size_t)u * N + k) * S;
    const int n = nbest_len(len[k], a.L), m = max(nbest_len(len[pivot], a.L), 0);
    if (n < 0) {      // an absent entry votes nowhere (wave-uniform: k is the workgroup's)
        for (int s = lane; s < S; s += 64) votes[s] = NBEST_EPS;
        if (lane == 0) a.out[o.extra + (size_t)u * N + k] = 0;
        return;
    }
    const int32_t* row = a.tok + (size_t)u * a.ldu;
    const int32_t* h = row + (size_t)k * a.ldn;
    for (int j = lane; j < n; j += 64) hk[j] = h[j];
    for (int s = lane; s < S; s += 64) image[s] = NBEST_EPS;
    EditSinkMasks masks{dir};
    (void)edit_wave_forward(row + (size_t)pivot * a.ldn, m, h, n, carryD, lane, masks);
    __syncthreads();
    if (lane == 0) {
        const int nb = (n + 63) >> 6;
        int i = m, j = n, extra = 0, gap = -1;      // gap: the gap of the insertion run the walk is in
        while (i > 0 || j > 0) {
            int code;
            if (i == 0) code = ASR_EDIT_INS;
            else if (j == 0) code = ASR_EDIT_DEL;
            else code = edit_wave_code_at(dir[(i - 1) * nb + ((j - 1) >> 6)], j);
            if (code == ASR_EDIT_INS) {
                extra += gap == i;
                gap = i;
                image[2 * i] = hk[j - 1];
                --j;
            } else {
                gap = -1;
                if (code != ASR_EDIT_DEL) {
                    image[2 * i - 1] = hk[j - 1];
                    --j;
                }
                --i;
            }
        }
        a.out[o.extra + (size_t)u * N + k] = extra;
    }
    __syncthreads();
    for (int s = lane; s < S; s += 64) votes[s] = image[s];
}

__global__ __launch_bounds__(64) void nbest_slot_vote_kernel(NbestArgs a, NbestLayout o) {
    const int u = blockIdx.y, s = blockIdx.x, lane = threadIdx.x, N = a.N, A = a.A, S = 2 * a.L + 1;
    const int32_t* len = a.len + (size_t)u * N;
    const int pivot = min(max(a.out[o.pivot + u], 0), N - 1);
    const int m = max(nbest_len(len[pivot], a.L), 0);
    int32_t* alts = a.out + o.alts + ((size_t)u * S + s) * A * 2;
    if (s > 2 * m) {      // past the pivot's slots (wave-uniform)
        if (lane < A) {
            alts[2 * lane] = NBEST_EPS;
            alts[2 * lane + 1] = 0;
        }
        if (lane == 0) {
            a.out[o.n_alts + (size_t)u * S + s] = 0;
            a.out[o.pivot_w + (size_t)u * S + s] = 0;
        }
        return;
    }
    const bool on = lane < N && nbest_len(len[min(lane, N - 1)], a.L) >= 0;
    const int v = on ? a.out[o.votes + ((size_t)u * N + lane) * S + s] : NBEST_EPS;
    const int w = on ? max(a.weights[(size_t)u * N + lane], 0) : 0;
    const unsigned long long present = __ballot(on);
    int gw = 0, leader = 64;
    for (int l = 0; l < N; ++l) {      // wave-uniform bounds: v_readlane takes a scalar lane
        const int vl = __builtin_amdgcn_readlane(v, l), wl = __builtin_amdgcn_readlane(w, l);
        if (((present >> l) & 1ull) && vl == v) {
            gw += wl;
            leader = min(leader, l);
        }
    }
    const bool lead = on && leader == lane;
    const unsigned long long leaders = __ballot(lead);
    int rank = 0;
    for (int l = 0; l < N; ++l) {
        const int gl = __builtin_amdgcn_readlane(gw, l);
        if (((leaders >> l) & 1ull) && (gl > gw || (gl == gw && l < lane))) ++rank;
    }
    const int n_alts = __popcll(leaders);
    if (lead && rank < A) {
        alts[2 * rank] = v;
        alts[2 * rank + 1] = gw;
    }
    if (lane >= n_alts && lane < A) {
        alts[2 * lane] = NBEST_EPS;
        alts[2 * lane + 1] = 0;
    }
    const int pw = __builtin_amdgcn_readlane(gw, pivot);
    if (lane == 0) {
        a.out[o.n_alts + (size_t)u * S + s] = n_alts;
        a.out[o.pivot_w + (size_t)u * S + s] = pw;
    }
}

// every refusal, on the host and before any launch
int nbest_check(const char* name, const int32_t* tok, const int32_t* len, const int32_t* weights, int L, int ldn, int ldu, const int32_t* host_len,
                const int32_t* host_weights, int U, int N, int A, int32_t* out, size_t out_bytes, NbestArgs* a) {
    if (!tok || !len || !weights || !host_len || !host_weights || !out) ASR_FAIL(ASR_EINVAL, "%s: null pointer", name);
    if (((uintptr_t)tok | (uintptr_t)len | (uintptr_t)weights | (uintptr_t)host_len | (uintptr_t)host_weights) % 4 || (uintptr_t)out % 8)
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer", name);
    if (U <= 0 || U > 65535) ASR_FAIL(ASR_EINVAL, "%s: U=%d utterances outside [1, 65535]", name, U);
    if (N < 1 || N > ASR_NBEST_MAX_N) ASR_FAIL(ASR_EINVAL, "%s: N=%d entries outside [1, %d]", name, N, ASR_NBEST_MAX_N);
    if (L < 0 || L > ASR_NBEST_MAX_LEN) ASR_FAIL(ASR_EINVAL, "%s: L=%d outside [0, %d]", name, L, ASR_NBEST_MAX_LEN);
    if (A < 1 || A > ASR_NBEST_MAX_ALTS) ASR_FAIL(ASR_EINVAL, "%s: A=%d alternatives outside [1, %d]", name, A, ASR_NBEST_MAX_ALTS);
    if (ldn < L || (long long)ldu < (long long)(N - 1) * ldn + L)
        ASR_FAIL(ASR_EINVAL, "%s: stride below the row length (ldn=%d ldu=%d L=%d N=%d)", name, ldn, ldu, L, N);
    for (int u = 0; u < U; ++u) {
        long long sum = 0;
        int present = 0;
        for (int k = 0; k < N; ++k) {
            const int n = host_len[(size_t)u * N + k], w = host_weights[(size_t)u * N + k];
            if (n > ASR_NBEST_MAX_LEN) ASR_FAIL(ASR_EINVAL, "%s: hypothesis %d of utterance %d has %d tokens, the limit is %d", name, k, u, n, ASR_NBEST_MAX_LEN);
            if (w < 0) ASR_FAIL(ASR_EINVAL, "%s: weight %d of utterance %d is negative (%d)", name, k, u, w);
            if (n >= 0) {
                ++present;
                sum += w;
            }
        }
        if (!present) ASR_FAIL(ASR_EINVAL, "%s: utterance %d has no present entry", name, u);
        if (sum > (1ll << 30)) ASR_FAIL(ASR_EINVAL, "%s: the weights of utterance %d sum to %lld, the limit is 2^30", name, u, sum);
    }
    const size_t need = nbest_layout(U, N, L, A).words * 4;
    if (out_bytes < need) ASR_FAIL(ASR_EWORKSPACE, "%s: output of %zu bytes, asr_nbest_out_bytes says %zu", name, out_bytes, need);
    *a = NbestArgs{tok, len, weights, L, ldn, ldu, U, N, A, out};
    return ASR_OK;
}

void nbest_launch(int stage, const NbestArgs& a, hipStream_t st) {
    const NbestLayout o = nbest_layout(a.U, a.N, a.L, a.A);
    if (stage == 0) nbest_pair_dist_kernel<<<dim3(a.N * (a.N - 1) / 2 + 1, a.U), WAVE, 0, st>>>(a, o.d);
    else if (stage == 1) nbest_pivot_votes_kernel<<<dim3(a.N, a.U), WAVE, 0, st>>>(a, o);
    else nbest_slot_vote_kernel<<<dim3(2 * a.L + 1, a.U), WAVE, 0, st>>>(a, o);
}

int nbest_entry(const char* name, int first, int last, const int32_t* tok, const int32_t* len, const int32_t* weights, int L, int ldn, int ldu,
                const int32_t* host_len, const int32_t* host_weights, int U, int N, int A, int32_t* out, size_t out_bytes, void* stream) {
    NbestArgs a;
    const int rc = nbest_check(name, tok, len, weights, L, ldn, ldu, host_len, host_weights, U, N, A, out, out_bytes, &a);
    if (rc != ASR_OK) return rc;
    for (int s = first; s <= last; ++s) {
        nbest_launch(s, a, (hipStream_t)stream);
        ASR_CHECK_LAUNCH(name);
    }
    return ASR_OK;
}

}  // namespace

extern "C" size_t asr_nbest_out_bytes(int U, int N, int L, int A) {
    if (U <= 0 || N < 1 || N > ASR_NBEST_MAX_N || L < 0 || L > ASR_NBEST_MAX_LEN || A < 1 || A > ASR_NBEST_MAX_ALTS) {
        asr_set_error("asr_nbest_out_bytes: bad shape U=%d N=%d L=%d A=%d", U, N, L, A);
        return 0;
    }
    return nbest_layout(U, N, L, A).words * 4;
}

#define NBEST_ENTRY(fn, first, last)                                                                                                                     \
    extern "C" int fn(const int32_t* tok, const int32_t* len, const int32_t* weights, int L, int ldn, int ldu, const int32_t* host_len,                  \
                      const int32_t* host_weights, int U, int N, int A, int32_t* out, size_t out_bytes, void* stream) {                                   \
        return nbest_entry(#fn, first, last, tok, len, weights, L, ldn, ldu, host_len, host_weights, U, N, A, out, out_bytes, stream);                  \
    }
NBEST_ENTRY(asr_nbest_pair_dist, 0, 0)
NBEST_ENTRY(asr_nbest_pivot_votes, 1, 1)
NBEST_ENTRY(asr_nbest_slot_vote, 2, 2)
NBEST_ENTRY(asr_nbest_consensus, 0, 2)
