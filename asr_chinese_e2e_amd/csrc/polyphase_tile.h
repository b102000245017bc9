// The data movement the two polyphase resamplers (speed.hip, resample.hip) share: one workgroup of NT threads stages the input span of
// its tile of one row in LDS, computes into an LDS row ys, and stores that row.  Both directions place every 16-byte-aligned quad of
// global memory on a 16-byte-aligned quad of LDS, so the quads that lie inside the row move as one 16-byte access and only the row ends go
// element by element.  The filters, the tap placement and the tile sizes stay with the kernels.
#pragma once
#include "asr_common.h"      // f32x4

namespace ptile {

constexpr int NT = 256;                   // threads of the workgroup

// Row-relative samples [lo, lo + count) of the row that starts at element row0 -> xs[pad + i]; only [vlo, vhi) of the row is real,
// everything else (halo before the utterance, beyond its end, beyond what a stream's row holds) is 0.  Returns pad = (row0 + lo) mod 4.
// vec: the base pointer is 16-byte aligned.
__device__ __forceinline__ int stage(float* xs, const float* __restrict__ wav, long long row0, int lo, int count, int vlo, int vhi, bool vec, int tid) {
    const int pad = (int)(((row0 + lo) % 4 + 4) % 4);
    const int lo_al = lo - pad;                         // row-relative index of xs[0]
    const int nquads = (pad + count + 3) >> 2;
    for (int qd = tid; qd < nquads; qd += NT) {
        const int k = lo_al + 4 * qd;
        f32x4 v;
        if (vec && k >= vlo && k + 4 <= vhi) {
            v = *(const f32x4*)(wav + row0 + k);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (k + e >= vlo && k + e < vhi) ? wav[row0 + k + e] : 0.f;
        }
        *(f32x4*)(xs + 4 * qd) = v;
    }
    return pad;
}

// Start of a tile of tcount outputs whose first one is element o0 of the output tensor: returns opad, with ys[opad + t] = output t of
// the tile, and zeroes ys beyond the tlive outputs the utterance really has (<= 0: the tile is padding only).  ys holds tcount + 4 words.
__device__ __forceinline__ int begin_tile(float* ys, long long o0, int tlive, int tcount, int tid) {
    const int opad = (int)(o0 & 3);
    for (int t = tlive > 0 ? tlive + tid : tid; t < tcount; t += NT) ys[opad + t] = 0.f;
    return opad;
}

// End of the tile: waits for every lane's ys, then stores quad i of ys = outputs 4 i - opad ... + 3 of the tile, whose first output goes to tile[0].
__device__ __forceinline__ void store_tile(float* tile, const float* ys, int opad, int tcount, bool vec, int tid) {
    __syncthreads();
    float* orow = tile - opad;
    for (int i = tid; 4 * i < opad + tcount; i += NT) {
        const int t = 4 * i - opad;
        if (vec && t >= 0 && t + 4 <= tcount) {
            *(f32x4*)(orow + 4 * i) = *(const f32x4*)(ys + 4 * i);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e >= 0 && t + e < tcount) orow[4 * i + e] = ys[4 * i + e];
        }
    }
}

}  // namespace ptile
