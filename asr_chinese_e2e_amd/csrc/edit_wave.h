// The wave-parallel Levenshtein forward pass, once, for every kernel that needs a token distance (score.hip, consensus.hip, mwer.hip;
// decode.hip's cer_kernel uses the scan alone).  The definition is tests/score_ref.py.
//
// One wave aligns rows r[0..m) to columns h[0..n).  Lanes own columns, 64 at a time (a column block); inside a block the rows run
// serially, so a lane keeps its column's id and its D[i-1][j] in registers from row to row.  With
// t[j] = min(D[i-1][j] + 1, D[i-1][j-1] + (r_i != h_j)) the recurrence D[i][j] = min(t[j], D[i][j-1] + 1) is D[i][j] - j = prefix-min of
// (t[k] - k): a wave min-scan, with the block's left boundary column D[i][64 b] as the carry between blocks.  That column is the only
// per-row state that has to leave the registers: m + 1 ints of LDS (carryD), rewritten in place by lane 63 for the next block and read
// one row ahead of its use, so the LDS latency hides behind the scan.  The row ids never touch LDS: 64 of them are loaded at once, one per
// lane, and read back row by row with v_readlane.
//
// What a caller does with a finished cell is its sink (three hooks, all inlined):
//   block(jb)                                             before the rows of column block jb
//   cell(i, jb, nb, lane, valid, more, sub, Dp, Dd, Dc)    cell (i, j = 64 jb + lane + 1): Dp = D[i-1][j], Dd = D[i-1][j-1], Dc = D[i][j]
//   finish(n)                                             after the last column block (not called when n == 0)
#pragma once
#include "asr_common.h"

constexpr int EDIT_WAVE_BIG = 0x3fffffff;

// Lane crossings on the vector ALU's DPP path, not through the LDS crossbar (six __shfl_up steps per scan were six ds_bpermute round trips
// of ~100 cycles each: 350 ns per row step measured).  PRECONDITION of the three helpers, of edit_wave_forward and of every sink hook: the
// whole wave executes them - every loop around them has wave-uniform bounds, and a wave that leaves early leaves as a whole.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int wave_dpp_keep(int v) {      // a lane without a source, or in a masked row, keeps v
    return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ int wave_prefix_min(int v) {      // inclusive prefix minimum over the 64 lanes
    v = min(v, wave_dpp_keep<0x111>(v));            // row_shr:1
    v = min(v, wave_dpp_keep<0x112>(v));            // row_shr:2
    v = min(v, wave_dpp_keep<0x114>(v));            // row_shr:4
    v = min(v, wave_dpp_keep<0x118>(v));            // row_shr:8: every row of 16 lanes holds its own prefix minimum
    v = min(v, wave_dpp_keep<0x142, 0xA>(v));       // row_bcast15 into rows 1 and 3
    v = min(v, wave_dpp_keep<0x143, 0xC>(v));       // row_bcast31 into rows 2 and 3
    return v;
}
// lane l takes v of lane l - 1, lane 0 takes `first` (wave_shr:1)
__device__ __forceinline__ int wave_shift_in(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

// Returns D[m][n] in every lane.  carryD: m + 1 ints of LDS; the one-wave workgroup may have written other LDS before the call.
template <class Sink>
__device__ __forceinline__ int edit_wave_forward(const int32_t* __restrict__ r, int m, const int32_t* __restrict__ h, int n, int* carryD, int lane,
                                                 Sink& sink) {
    const int nb = (n + 63) >> 6;
    for (int i = lane; i <= m; i += 64) carryD[i] = i;
    __syncthreads();
    int Dfin = m;      // n == 0
    for (int jb = 0; jb < nb; ++jb) {
        const int c0 = jb << 6, j = c0 + lane + 1;
        const bool valid = j <= n, more = jb + 1 < nb;
        const int hj = valid ? h[j - 1] : 0;
        int Dp = j;       // row 0: D = j
        int dD = c0;      // the boundary column one row up
        int rblk = 0;
        int nextD = carryD[min(1, m)];      // the boundary column is read one row ahead of its use
        sink.block(jb);
        for (int i = 1; i <= m; ++i) {
            const int ii = (i - 1) & 63;
            if (ii == 0) rblk = i - 1 + lane < m ? r[i - 1 + lane] : 0;
            const int ri = __builtin_amdgcn_readlane(rblk, ii);
            const int cinD = nextD;
            nextD = carryD[min(i + 1, m)];      // row i + 1 is rewritten one iteration from now
            const int Dd = wave_shift_in(Dp, dD);
            const int sub = ri != hj;
            int v = valid ? min(Dp + 1, Dd + sub) - j : EDIT_WAVE_BIG;
            v = min(wave_prefix_min(v), cinD - c0);
            const int Dc = v + j;
            sink.cell(i, jb, nb, lane, valid, more, sub, Dp, Dd, Dc);
            if (more && lane == 63) carryD[i] = Dc;
            dD = cinD;
            Dp = Dc;
        }
        __syncthreads();
        if (!more) {
            Dfin = __shfl(Dp, (n - 1) & 63, 64);
            sink.finish(n);
        }
    }
    return Dfin;
}

// The direction of a cell: DIAG iff D[i-1][j-1] + sub == D[i][j], else UP iff D[i-1][j] + 1 == D[i][j], else LEFT (the third comparison
// is implied: one of the three candidates is the minimum).  The code {COR, SUB, DEL, INS} is two bits.
__device__ __forceinline__ int edit_wave_code(int sub, int Dp, int Dd, int Dc) {
    const bool isDiag = Dd + sub == Dc, isUp = !isDiag && Dp + 1 == Dc;
    return isDiag ? sub : (isUp ? ASR_EDIT_DEL : ASR_EDIT_INS);
}
// The 64 codes of a (row, column block) as two ballot masks, 16 bytes.
__device__ __forceinline__ ulonglong2 edit_wave_masks(bool valid, int code) {
    ulonglong2 mk;
    mk.x = __ballot(valid && (code & 1));
    mk.y = __ballot(valid && (code & 2));
    return mk;
}
// ... and the code of cell (i, j), i, j >= 1, read back from them
__device__ __forceinline__ int edit_wave_code_at(ulonglong2 mk, int j) {
    const int bit = (j - 1) & 63;
    return (int)((mk.x >> bit) & 1ull) | ((int)((mk.y >> bit) & 1ull) << 1);
}

// The distance alone.
struct EditSinkNone {
    __device__ __forceinline__ void block(int) {}
    __device__ __forceinline__ void cell(int, int, int, int, bool, bool, int, int, int, int) {}
    __device__ __forceinline__ void finish(int) {}
};
// The masks of cell (i, j) go to dir[(i - 1) * nb + (j - 1) / 64].
struct EditSinkMasks {
    ulonglong2* dir;
    __device__ __forceinline__ void block(int) {}
    __device__ __forceinline__ void cell(int i, int jb, int nb, int lane, bool valid, bool, int sub, int Dp, int Dd, int Dc) {
        const ulonglong2 mk = edit_wave_masks(valid, edit_wave_code(sub, Dp, Dd, Dc));
        if (lane == 0) dir[(i - 1) * nb + jb] = mk;
    }
    __device__ __forceinline__ void finish(int) {}
};
