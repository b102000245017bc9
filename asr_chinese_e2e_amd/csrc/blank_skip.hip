// Blank-frame skipping in front of the CTC prefix beam search (decode.py, sessions.py; the definition: tests/blank_skip_ref.py).
//   asr_ctc_blank_skip_compact   drop every frame whose blank posterior is high and whose predecessor's is too: the kept rows of the
//                                per-frame candidates (asr_ctc_frame_topk) move to the front of their utterance, in order
//   asr_frame_index_remap        frame indices over the kept rows -> the frames they were (the timed searches' start / end)
// No atomics: a kept row's place is the number of kept rows in front of it, which every wave counts for itself from blank_lp in one fixed
// order - two runs write the same bytes.
#include "asr_common.h"

namespace {

// One wave per workgroup; workgroup (x, b) copies the 64-frame blocks x, x + gridDim.x, ... of utterance b and only counts the others in
// front of them (a ballot per block).  Lane = frame.  high = blank_lp > thr (float32, strict: a NaN is not high); a frame is dropped iff
// it and its predecessor are high, the predecessor of a block's lane 0 being bit 63 of the block before, of frame 0 the carry bit of the
// skip state (0 without one).  The copy runs over (kept row, column) pairs, so that a wave's stores are contiguous.
// state (B, 4) int32 {carry, frames seen, frames kept, 0}: read by every workgroup of its utterance, written by one - the wrapper
// launches a single workgroup per utterance when there is a state, so nobody reads what another has written.
__global__ __launch_bounds__(WAVE) void blank_skip_compact_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ ids,
                                                                  const float* __restrict__ blank_lp, const int32_t* __restrict__ count, float thr,
                                                                  int32_t* __restrict__ state, const int32_t* __restrict__ reset,
                                                                  uint32_t* __restrict__ out_vals, uint32_t* __restrict__ out_ids,
                                                                  float* __restrict__ out_blank_lp, int32_t* __restrict__ out_len,
                                                                  int32_t* __restrict__ out_frame, int T, int k, int map_cap) {
    __shared__ int src_lane[WAVE];
    const int lane = threadIdx.x, b = blockIdx.y;
    const int n = count ? max(0, min(count[b], T)) : T;
    const bool fresh = !state || (reset && reset[b] != 0);
    unsigned long long carry = fresh ? 0ull : (unsigned long long)(state[(size_t)b * 4] & 1);
    const int seen = fresh ? 0 : max(0, state[(size_t)b * 4 + 1]), kept0 = fresh ? 0 : max(0, state[(size_t)b * 4 + 2]);
    const int blocks = (n + WAVE - 1) / WAVE;
    const size_t row0 = (size_t)b * T;
    int base = 0;
    // the last block this workgroup copies; a workgroup without one still runs when it has the utterance's count or state to write
    const int own_last = (int)blockIdx.x < blocks ? (int)blockIdx.x + ((blocks - 1 - (int)blockIdx.x) / (int)gridDim.x) * (int)gridDim.x : -1;
    const bool writes_len = own_last == blocks - 1 && (blocks > 0 || blockIdx.x == 0);
    for (int j = 0; j <= own_last; ++j) {
        const int t = j * WAVE + lane;
        const bool live = t < n;
        const float lp = live ? blank_lp[row0 + t] : 0.f;
        const unsigned long long hb = __ballot(live && lp > thr);
        const unsigned long long lv = __ballot(live);
        const unsigned long long kb = lv & ~(hb & ((hb << 1) | carry));
        const int here = min(WAVE, n - j * WAVE);
        carry = (hb >> (here - 1)) & 1ull;      // the high bit of the block's last frame: the next block's, and after the last the state's
        const int cnt = __popcll(kb);
        if (j % (int)gridDim.x == (int)blockIdx.x) {      // wave-uniform
            const bool keep = (kb >> lane) & 1ull;
            const int rank = __popcll(kb & ((1ull << lane) - 1ull));
            if (keep) {
                src_lane[rank] = lane;
                out_blank_lp[row0 + base + rank] = lp;
                if (out_frame && kept0 + base + rank < map_cap) out_frame[(size_t)b * map_cap + kept0 + base + rank] = seen + t;
            }
            __syncthreads();
            const size_t in0 = (row0 + (size_t)j * WAVE) * k, o0 = (row0 + base) * k;
            for (int i = lane; i < cnt * k; i += WAVE) {
                const int r = i / k, c = i - r * k;
                const size_t s = in0 + (size_t)src_lane[r] * k + c;
                out_vals[o0 + i] = vals[s];
                out_ids[o0 + i] = ids[s];
            }
            __syncthreads();
        }
        base += cnt;
    }
    if (writes_len && lane == 0) {
        out_len[b] = base;
        if (state) {      // a single workgroup per utterance (see above); n == 0 keeps the carry bit
            int32_t* sw = state + (size_t)b * 4;
            sw[0] = (int)carry; sw[1] = seen + n; sw[2] = kept0 + base; sw[3] = 0;
        }
    }
}

// idx, out (B, per) int32 (out may be idx): idx < 0 stays, otherwise map[b, idx] (an index outside the map stays as well: nothing is read
// out of bounds).  Every element is read and written by one thread, so in place is fine.
__global__ __launch_bounds__(256) void frame_index_remap_kernel(const int32_t* idx, const int32_t* __restrict__ map, int32_t* out, int per, int map_cap) {
    const int b = blockIdx.y;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per; i += gridDim.x * blockDim.x) {
        const int v = idx[(size_t)b * per + i];
        out[(size_t)b * per + i] = v >= 0 && v < map_cap ? map[(size_t)b * map_cap + v] : v;
    }
}

}  // namespace

extern "C" int asr_ctc_blank_skip_compact(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* count, float thr, int32_t* state,
                                          const int32_t* reset, float* out_vals, int32_t* out_ids, float* out_blank_lp, int32_t* out_len,
                                          int32_t* out_frame, int B, int T, int k, int map_cap, void* stream) {
    if (!vals || !ids || !blank_lp || !out_vals || !out_ids || !out_blank_lp || !out_len) ASR_FAIL(ASR_EINVAL, "asr_ctc_blank_skip_compact: null pointer");
    if (B <= 0 || B > 65535 || T <= 0 || k <= 0 || k > 63 || (size_t)B * T * k > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_blank_skip_compact: bad shape B=%d (1..65535) T=%d k=%d (1..63)", B, T, k);
    if (!(thr <= 0.f)) ASR_FAIL(ASR_EINVAL, "asr_ctc_blank_skip_compact: the threshold must be the logarithm of a probability in (0, 1] (got %g)", (double)thr);
    if (reset && !state) ASR_FAIL(ASR_EINVAL, "asr_ctc_blank_skip_compact: reset flags without a skip state");
    if (out_frame ? (map_cap <= 0 || (!state && map_cap < T) || (size_t)B * map_cap > (size_t)INT_MAX) : map_cap != 0)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_blank_skip_compact: map_cap=%d (0 without out_frame, >= T=%d without a state)", map_cap, T);
    if (((uintptr_t)vals | (uintptr_t)ids | (uintptr_t)blank_lp | (uintptr_t)count | (uintptr_t)state | (uintptr_t)reset | (uintptr_t)out_vals |
         (uintptr_t)out_ids | (uintptr_t)out_blank_lp | (uintptr_t)out_len | (uintptr_t)out_frame) % 4)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_blank_skip_compact: misaligned pointer");
    if ((const void*)vals == (const void*)out_vals || (const void*)ids == (const void*)out_ids || blank_lp == out_blank_lp)
        ASR_FAIL(ASR_EINVAL, "asr_ctc_blank_skip_compact: the compaction is never in place");
    const int gx = state ? 1 : ceil_div(T, WAVE);
    blank_skip_compact_kernel<<<dim3(gx, B), WAVE, 0, (hipStream_t)stream>>>((const uint32_t*)vals, (const uint32_t*)ids, blank_lp, count, thr, state, reset,
                                                                            (uint32_t*)out_vals, (uint32_t*)out_ids, out_blank_lp, out_len, out_frame, T, k,
                                                                            map_cap);
    ASR_CHECK_LAUNCH("asr_ctc_blank_skip_compact");
    return ASR_OK;
}

extern "C" int asr_frame_index_remap(const int32_t* idx, const int32_t* map, int32_t* out, int B, int per, int map_cap, void* stream) {
    if (!idx || !map || !out) ASR_FAIL(ASR_EINVAL, "asr_frame_index_remap: null pointer");
    if (B <= 0 || B > 65535 || per <= 0 || map_cap <= 0 || (size_t)B * per > (size_t)INT_MAX || (size_t)B * map_cap > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "asr_frame_index_remap: bad shape B=%d (1..65535) per=%d map_cap=%d", B, per, map_cap);
    if (((uintptr_t)idx | (uintptr_t)map | (uintptr_t)out) % 4) ASR_FAIL(ASR_EINVAL, "asr_frame_index_remap: misaligned pointer");
    if ((const void*)map == (const void*)out) ASR_FAIL(ASR_EINVAL, "asr_frame_index_remap: the map is not an output");
    frame_index_remap_kernel<<<dim3(min(ceil_div(per, 256), 64), B), 256, 0, (hipStream_t)stream>>>(idx, map, out, per, map_cap);
    ASR_CHECK_LAUNCH("asr_frame_index_remap");
    return ASR_OK;
}
