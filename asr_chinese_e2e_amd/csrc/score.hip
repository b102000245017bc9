// Token-level scoring of hypotheses against references (include/asr_hip.h: asr_edit_align; the definition is tests/score_ref.py, and the
// kernel agrees with it integer for integer).  One wave per (hypothesis, reference) pair.
//
// Forward pass: edit_wave.h (lanes own hypothesis columns, the reference rows run serially), with one of two sinks of this file.
//
// Directions (ops mode).  The cell's code {COR, SUB, DEL, INS} is two bits, and the 64 cells leave the wave as two ballot masks, 16 bytes
// per (row, block), stored by lane 0 into LDS (pairs of up to ASR_EDIT_LDS_DIR_BYTES) or into the caller's workspace.
//
// Counts-only mode (ops == NULL) keeps no masks.  The walk from a cell to (0, 0) is fixed by the directions, so its substitution and
// deletion counts are a function of the cell: C[i][j] = C[predecessor] + the step.  They travel with D, packed in one int (sub | del << 16,
// both <= ASR_EDIT_MAX_REF); a LEFT cell takes the counts of the nearest non-LEFT cell on its left in the row (a ballot, a count of
// leading zeros and one lane read), or the boundary column's when there is none in the block.  cor and ins follow from cor + sub + del =
// i and cor + sub + ins = j.
//
// Backtrace.  Lane 0 walks from (m, n): a chain of dependent 16-byte reads.  It writes the codes in walk order into the tail of the
// pair's code plane; the wave then moves them to the front in forward order and adds the positions, which are running counts of the
// codes (ballot + popcount).
#include <limits.h>

#include "asr_common.h"
#include "edit_wave.h"

namespace {

constexpr int EDIT_LDS_MAX = 150 * 1024;      // what cer_kernel asks for

__host__ __device__ __forceinline__ int edit_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__host__ __device__ __forceinline__ unsigned edit_carry_bytes(int m) { return ((unsigned)(m + 1) * 4u + 15u) & ~15u; }
__host__ __device__ __forceinline__ unsigned long long edit_dir_bytes(int m, int n) { return (unsigned long long)m * (unsigned)((n + 63) >> 6) * 16ull; }
// workspace bytes of a pair in ops mode: 0 when its masks live in LDS (lds_bytes = the launch's dynamic LDS)
__host__ __device__ __forceinline__ unsigned long long edit_ws_need(int m, int n, int lds_bytes) {
    const unsigned long long db = edit_dir_bytes(m, n);
    return db <= (unsigned long long)ASR_EDIT_LDS_DIR_BYTES && edit_carry_bytes(m) + db <= (unsigned long long)lds_bytes ? 0ull : db;
}

// The masks of a cell go to LDS, to the workspace, or nowhere (!have_dir: the distance alone).
struct EditSinkDirs {
    ulonglong2* ldir;      // the direction masks, (m, nb) pairs: in LDS ...
    ulonglong2* gdir;      // ... or in the workspace
    bool have_dir;
    __device__ __forceinline__ ulonglong2 get(int i, int nb, int jb) const {
        const size_t at = (size_t)(i - 1) * nb + jb;
        return ldir ? ldir[at] : gdir[at];
    }
    __device__ __forceinline__ void block(int) {}
    __device__ __forceinline__ void cell(int i, int jb, int nb, int lane, bool valid, bool, int sub, int Dp, int Dd, int Dc) {
        if (!have_dir) return;
        const ulonglong2 mk = edit_wave_masks(valid, edit_wave_code(sub, Dp, Dd, Dc));
        if (lane == 0) {
            const size_t at = (size_t)(i - 1) * nb + jb;
            if (ldir) ldir[at] = mk;
            else gdir[at] = mk;
        }
    }
    __device__ __forceinline__ void finish(int) {}
};

// The packed counts C (sub | del << 16) travel with D; carryC (m + 1 ints of LDS) is their boundary column, read ahead like carryD.
struct EditSinkCounts {
    int* carryC;
    int m, Cp, dC, nextC, Cfin;
    __device__ __forceinline__ EditSinkCounts(int* c, int m_, int lane) : carryC(c), m(m_), Cp(0), dC(0), nextC(0), Cfin(m_ << 16) {      // Cfin: n == 0
        for (int i = lane; i <= m; i += 64) carryC[i] = i << 16;      // column 0 is all UP: i deletions (the pass's first barrier follows)
    }
    __device__ __forceinline__ void block(int) {
        Cp = 0;      // row 0: all LEFT
        dC = 0;      // the boundary column one row up
        nextC = carryC[min(1, m)];
    }
    __device__ __forceinline__ void cell(int i, int, int, int lane, bool valid, bool more, int sub, int Dp, int Dd, int Dc) {
        const bool isDiag = Dd + sub == Dc, isUp = !isDiag && Dp + 1 == Dc;
        const int Cd = wave_shift_in(Cp, dC);
        const int cinC = nextC;
        nextC = carryC[min(i + 1, m)];
        const int Cb = isDiag ? Cd + sub : Cp + 0x10000;
        const bool isLeft = valid && !isDiag && !isUp;
        const unsigned long long below = __ballot(!isLeft) & ((1ull << lane) - 1ull);
        const int src = below ? 63 - __clzll((long long)below) : 0;
        const int Cs = __shfl(Cb, src, 64);
        const int Cc = isLeft ? (below ? Cs : cinC) : Cb;
        if (more && lane == 63) carryC[i] = Cc;
        dC = cinC;
        Cp = Cc;
    }
    __device__ __forceinline__ void finish(int n) { Cfin = __shfl(Cp, (n - 1) & 63, 64); }
};

struct EditShape { int n, m, rr; };
__device__ __forceinline__ EditShape edit_shape(int p, const int32_t* __restrict__ hyp_len, const int32_t* __restrict__ ref_len, const int32_t* __restrict__ ref_of,
                                                int Lh, int Lr, int R, int m_cap) {
    EditShape s;
    s.rr = edit_clamp(ref_of[p], R - 1);
    s.n = edit_clamp(hyp_len[p], Lh);
    s.m = edit_clamp(ref_len[s.rr], min(Lr, m_cap));
    return s;
}

template <bool OPS>
__global__ __launch_bounds__(64) void edit_align_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, int Lh, int ldh,
                                                        const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len, int Lr, int ldr,
                                                        const int32_t* __restrict__ ref_of, int R, int32_t* __restrict__ counts, int32_t* __restrict__ ops,
                                                        int32_t* __restrict__ n_ops, int ldo, unsigned char* __restrict__ ws, unsigned long long ws_bytes,
                                                        int lds_bytes) {
    extern __shared__ __align__(16) unsigned char edit_smem[];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int m_cap = lds_bytes / (OPS ? 4 : 8) - 1;      // the rows the boundary columns have room for
    const EditShape sh = edit_shape(p, hyp_len, ref_len, ref_of, Lh, Lr, R, m_cap);
    const int n = sh.n, m = sh.m, nb = (n + 63) >> 6;
    int* carryD = (int*)edit_smem;      // D[i][64 b], i = 0 .. m
    const int32_t* h = hyp + (size_t)p * ldh;
    const int32_t* r = ref + (size_t)sh.rr * ldr;
    int32_t* cnt = counts + (size_t)p * 5;
    if (!OPS) {
        EditSinkCounts cs(carryD + (m + 1), m, lane);
        const int Dfin = edit_wave_forward(r, m, h, n, carryD, lane, cs);
        if (lane == 0) {
            const int s = cs.Cfin & 0xffff, d = cs.Cfin >> 16, c = m - s - d;
            cnt[0] = Dfin; cnt[1] = c; cnt[2] = s; cnt[3] = d; cnt[4] = n - c - s;
        }
        return;
    }
    EditSinkDirs ds{nullptr, nullptr, false};
    const unsigned long long need = edit_ws_need(m, n, lds_bytes);
    if (need == 0) {
        ds.ldir = (ulonglong2*)(edit_smem + edit_carry_bytes(m));
        ds.have_dir = true;
    } else if (ws) {      // the pair's slice begins behind those of the workspace pairs in front of it
        unsigned long long off = 0;
        for (int q = lane; q < p; q += 64) {
            const EditShape o = edit_shape(q, hyp_len, ref_len, ref_of, Lh, Lr, R, m_cap);
            off += edit_ws_need(o.m, o.n, lds_bytes);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
        if (off + need <= ws_bytes) {
            ds.gdir = (ulonglong2*)(ws + off);
            ds.have_dir = true;
        }
    }
    const int Dfin = edit_wave_forward(r, m, h, n, carryD, lane, ds);
    if (!ds.have_dir) {      // only when the device lengths are not the ones the caller sized the workspace by: the distance alone
        if (lane == 0) {
            cnt[0] = Dfin; cnt[1] = cnt[2] = cnt[3] = cnt[4] = -1;
            n_ops[p] = -1;
        }
        return;
    }
    int32_t* code_out = ops + (size_t)p * 3 * ldo;      // planes: code, ref_pos, hyp_pos
    int K = 0;
    if (lane == 0) {
        int i = m, j = n, tally[4] = {0, 0, 0, 0};
        while (i > 0 || j > 0) {
            int code;
            if (i == 0) code = ASR_EDIT_INS;
            else if (j == 0) code = ASR_EDIT_DEL;
            else code = edit_wave_code_at(ds.get(i, nb, (j - 1) >> 6), j);
            code_out[ldo - 1 - K] = code;
            ++K;
            ++tally[code];
            i -= code != ASR_EDIT_INS;
            j -= code != ASR_EDIT_DEL;
        }
        cnt[0] = Dfin; cnt[1] = tally[0]; cnt[2] = tally[1]; cnt[3] = tally[2]; cnt[4] = tally[3];
        n_ops[p] = K;
    }
    K = __shfl(K, 0, 64);
    __syncthreads();      // lane 0's codes are visible to the wave: one CU, one vector L1 (a device-scope fence here cost 15 x on short pairs)
    // forward order: op k is the walk's op K-1-k, which sits at ldo-K+k; k < ldo-K+k, so an ascending pass reads every word before it is overwritten
    const int src0 = ldo - K;
    int rbase = 0, hbase = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const bool on = k < K;
        const int code = on ? code_out[src0 + k] : -1;
        const bool ar = on && code != ASR_EDIT_INS, ah = on && code != ASR_EDIT_DEL;
        const unsigned long long mr = __ballot(ar), mh = __ballot(ah), lt = (1ull << lane) - 1ull;
        const int rpos = rbase + __popcll(mr & lt), hpos = hbase + __popcll(mh & lt);
        if (on) {
            code_out[k] = code;
            code_out[ldo + k] = ar ? rpos : -1;
            code_out[2 * (size_t)ldo + k] = ah ? hpos : -1;
        }
        rbase += __popcll(mr);
        hbase += __popcll(mh);
    }
}

// the launch's dynamic LDS by the host mirrors: the largest pair's boundary columns, and its masks where they stay in LDS
struct EditPlan { long long lds; unsigned long long ws; int max_m; };
EditPlan edit_plan(const int32_t* hyp_len, const int32_t* ref_len, const int32_t* ref_of, int P, int R, int Lh, int Lr, bool want_ops) {
    EditPlan pl = {16, 0, 0};
    for (int p = 0; p < P; ++p) {
        const int m = edit_clamp(ref_len[ref_of[p]], Lr), n = edit_clamp(hyp_len[p], Lh);
        long long need = want_ops ? (long long)edit_carry_bytes(m) : 8ll * (m + 1);
        if (want_ops) {
            const unsigned long long db = edit_dir_bytes(m, n);
            if (db <= (unsigned long long)ASR_EDIT_LDS_DIR_BYTES) need += (long long)db;
            else pl.ws += db;
        }
        pl.lds = need > pl.lds ? need : pl.lds;
        pl.max_m = m > pl.max_m ? m : pl.max_m;
    }
    return pl;
}

int edit_host_args(const char* name, const int32_t* hyp_len, const int32_t* ref_len, const int32_t* ref_of, int P, int R, int Lh, int Lr) {
    if (!hyp_len || !ref_len || !ref_of) ASR_FAIL(ASR_EINVAL, "%s: null host length / ref_of mirror", name);
    if (((uintptr_t)hyp_len | (uintptr_t)ref_len | (uintptr_t)ref_of) % 4) ASR_FAIL(ASR_EINVAL, "%s: misaligned host mirror", name);
    if (P <= 0 || R <= 0 || Lh < 0 || Lr < 0) ASR_FAIL(ASR_EINVAL, "%s: bad shape P=%d R=%d Lh=%d Lr=%d", name, P, R, Lh, Lr);
    for (int p = 0; p < P; ++p)
        if (ref_of[p] < 0 || ref_of[p] >= R) ASR_FAIL(ASR_EINVAL, "%s: ref_of[%d] = %d outside [0, %d)", name, p, ref_of[p], R);
    return ASR_OK;
}

}  // namespace

extern "C" size_t asr_edit_align_workspace_bytes(const int32_t* host_hyp_len, const int32_t* host_ref_len, const int32_t* host_ref_of, int P, int R, int Lh,
                                                 int Lr) {
    if (edit_host_args("asr_edit_align_workspace_bytes", host_hyp_len, host_ref_len, host_ref_of, P, R, Lh, Lr) != ASR_OK) return 0;
    return (size_t)edit_plan(host_hyp_len, host_ref_len, host_ref_of, P, R, Lh, Lr, true).ws;
}

extern "C" int asr_edit_align(const int32_t* hyp, const int32_t* hyp_len, int Lh, int ldh, const int32_t* ref, const int32_t* ref_len, int Lr, int ldr,
                              const int32_t* ref_of, const int32_t* host_hyp_len, const int32_t* host_ref_len, const int32_t* host_ref_of, int P, int R,
                              int32_t* counts, int32_t* ops, int32_t* n_ops, int ldo, void* ws, size_t ws_bytes, void* stream) {
    if (!hyp || !hyp_len || !ref || !ref_len || !ref_of || !counts) ASR_FAIL(ASR_EINVAL, "asr_edit_align: null pointer");
    if (ops && !n_ops) ASR_FAIL(ASR_EINVAL, "asr_edit_align: ops without n_ops");
    int rc = edit_host_args("asr_edit_align", host_hyp_len, host_ref_len, host_ref_of, P, R, Lh, Lr);
    if (rc != ASR_OK) return rc;
    if (ldh < Lh || ldr < Lr) ASR_FAIL(ASR_EINVAL, "asr_edit_align: row stride below the row length (ldh=%d Lh=%d ldr=%d Lr=%d)", ldh, Lh, ldr, Lr);
    if (((uintptr_t)hyp | (uintptr_t)hyp_len | (uintptr_t)ref | (uintptr_t)ref_len | (uintptr_t)ref_of | (uintptr_t)counts | (uintptr_t)ops | (uintptr_t)n_ops) % 4 ||
        (uintptr_t)ws % 16)
        ASR_FAIL(ASR_EINVAL, "asr_edit_align: misaligned pointer");
    if (ops && ((long long)ldo < (long long)Lh + Lr || ldo < 1)) ASR_FAIL(ASR_EINVAL, "asr_edit_align: ldo=%d below max(Lh + Lr, 1) = %lld", ldo, (long long)Lh + Lr);
    const EditPlan pl = edit_plan(host_hyp_len, host_ref_len, host_ref_of, P, R, Lh, Lr, ops != nullptr);
    if (pl.max_m > ASR_EDIT_MAX_REF) ASR_FAIL(ASR_EINVAL, "asr_edit_align: a reference of %d tokens, the limit is %d", pl.max_m, ASR_EDIT_MAX_REF);
    if (pl.lds > EDIT_LDS_MAX) ASR_FAIL(ASR_EINVAL, "asr_edit_align: %lld bytes of LDS", pl.lds);
    if (pl.ws > 0 && (!ws || ws_bytes < pl.ws))
        ASR_FAIL(ASR_EWORKSPACE, "asr_edit_align: workspace of %zu bytes, asr_edit_align_workspace_bytes says %llu", ws ? ws_bytes : (size_t)0, pl.ws);
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)edit_align_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, EDIT_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)edit_align_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, EDIT_LDS_MAX);
        attr = true;
    }
    const hipStream_t st = (hipStream_t)stream;
    const int lds = (int)align_up((size_t)pl.lds, 16);
    if (ops)
        edit_align_kernel<true><<<P, WAVE, (size_t)lds, st>>>(hyp, hyp_len, Lh, ldh, ref, ref_len, Lr, ldr, ref_of, R, counts, ops, n_ops, ldo, (unsigned char*)ws,
                                                              ws ? (unsigned long long)ws_bytes : 0ull, lds);
    else
        edit_align_kernel<false><<<P, WAVE, (size_t)lds, st>>>(hyp, hyp_len, Lh, ldh, ref, ref_len, Lr, ldr, ref_of, R, counts, nullptr, nullptr, 0, nullptr, 0ull, lds);
    ASR_CHECK_LAUNCH("asr_edit_align");
    return ASR_OK;
}
