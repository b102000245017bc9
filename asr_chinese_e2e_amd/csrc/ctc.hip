// CTC forward-backward fused with the log-softmax over the vocabulary, and softmax
// cross-entropy.  Both are HBM-bound passes over (rows, V) logits.
//
// CTC, four kernels on one stream:
//   1. ctc_lse_gather : one wave per frame (b,t < in_len[b]).  Streams the V logits once
//      (16 B per lane per load), online max/sum-exp per lane, wave-shuffle reduction -> lse[b,t];
//      then gathers the S = 2L+1 lattice inputs lp[b,t,s] = x[l'_s] - lse (row is L1/L2-hot).
//   2. ctc_alpha_beta : one workgroup of two waves per utterance.  Wave 0 runs the alpha
//      recursion forward in time, wave 1 the beta recursion backward, state s on lane s%64
//      (register j = s/64), predecessors via DPP wave shifts (no LDS in the recursion), lattice
//      inputs prefetched in chunks of 8 timesteps in registers so the serial chain never waits on
//      memory (lattice_row_walk, which the forced alignment's Viterbi recursion runs too).  Linear domain, rescaled by the column maximum every 2 steps (logs of the scales
//      summed for the loss): 5 VALU per step instead of 3 exp + 1 log.
//   3. ctc_grad       : one workgroup per frame.  Wave 0 forms the frame's state posteriors
//      softmax_s(alpha+beta-lp) (exact: the sum over s is p(l|x) at every t) and scatters them into an LDS
//      table indexed by label (ds_add_f32), then one streaming pass: read logits, write
//      dlogits = scale * (softmax - posterior).  Padded frames are written as zeros.
//   4. ctc_rescue     : one workgroup per utterance, idle unless kernels 2 / 3 found that the utterance left the range of the scaled
//      lattice (see LATTICE_TINY); such an utterance is redone in the log domain.
// Algorithmic HBM bytes: logits read twice + dlogits written once = 3 * B*T*V*e;
// the lattice (B*T*S*4 B * 3 arrays) stays in L2 / Infinity Cache.
// Host side: asr_ctc_fwd_bwd and asr_ctc_align share ctc_check (validation) and ctc_lattice_inputs (the launch of kernel 1).
#include <type_traits>

#include "asr_common.h"

namespace {

constexpr float NEG_INF = -INFINITY;
typedef __attribute__((ext_vector_type(2))) double f64x2;

// online (max, sum exp(x - max)) merge
__device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    if (mn == NEG_INF) { m = mn; s = 0.f; return; }
    s = s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
}

// lse of one row held by a whole wave
template <typename T>
__device__ __forceinline__ float wave_row_lse(const T* __restrict__ x, int V, int lane, float* sum_x) {
    constexpr int N = Vec<T>::N;
    float m = NEG_INF, s = 0.f, sx = 0.f;
    if (V % N == 0) {
        const int nv = V / N;
        for (int i = lane; i < nv; i += 64) {
            float v[N];
            loadv<T>(x + (size_t)i * N, v);
            float lm = v[0];
#pragma unroll
            for (int j = 1; j < N; ++j) lm = fmaxf(lm, v[j]);
            const float mn = fmaxf(m, lm);
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < N; ++j) { acc += expf(v[j] - mn); sx += v[j]; }
            s = s * expf(m - mn) + acc;
            m = mn;
        }
    } else {
        for (int i = lane; i < V; i += 64) {
            const float v = to_f32<T>(x[i]);
            const float mn = fmaxf(m, v);
            s = s * expf(m - mn) + expf(v - mn);
            m = mn;
            sx += v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        ms_merge(m, s, m2, s2);
        sx += __shfl_xor(sx, o, 64);
    }
    if (sum_x) *sum_x = sx;
    return m + logf(s);
}

// ---- bf16 fast path: a wave holds one whole row in registers (NV 16-byte vectors per lane)
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

template <int NV>
__device__ __forceinline__ void wave_row_load(const bf16_t* __restrict__ x, int nvec, int lane, u32x4 (&xv)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = lane + 64 * k;
        // out-of-range vectors repeat the row's last vector: harmless for the max, masked in the sum
        xv[k] = *(const u32x4*)(x + (size_t)min(i, nvec - 1) * 8);
    }
}
// log-sum-exp of the row in xv: all loads in flight at once, ONE maximum, then one fma + v_exp_f32
// per element (the online form costs an extra rescale exp per vector and a precise expf per element)
template <int NV>
__device__ __forceinline__ float wave_row_lse_regs(const u32x4 (&xv)[NV], int nvec, int lane, float* row_max = nullptr) {
    float m = NEG_INF;
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, fmaxf(bf16_lo(xv[k][j]), bf16_hi(xv[k][j])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (row_max) *row_max = m;
    const float mb = m * LOG2E;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            a += __builtin_amdgcn_exp2f(fmaf(bf16_lo(xv[k][j]), LOG2E, -mb)) + __builtin_amdgcn_exp2f(fmaf(bf16_hi(xv[k][j]), LOG2E, -mb));
        s += (lane + 64 * k < nvec) ? a : 0.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return m + __logf(s);
}

// Index of the FIRST element of the row that equals its maximum m (torch.argmax's tie rule): every lane scans its vectors from the
// last to the first (a lane's indices ascend with k and inside a vector, so the last overwrite is its smallest), then a wave minimum.
// Out-of-range vectors repeat the row's last vector (wave_row_load): excluded.
template <int NV>
__device__ __forceinline__ int wave_row_argmax_regs(const u32x4 (&xv)[NV], int nvec, int lane, float m) {
    int bi = 0x7fffffff;
#pragma unroll
    for (int k = NV - 1; k >= 0; --k) {
        const int i = lane + 64 * k;
        const int base = i < nvec ? i * 8 : 0x7ffffff0;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            bi = bf16_hi(xv[k][j]) == m ? base + 2 * j + 1 : bi;
            bi = bf16_lo(xv[k][j]) == m ? base + 2 * j : bi;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bi = min(bi, __shfl_xor(bi, o, 64));
    return bi;
}

// ---------------------------------------------------------------------------------- lattice layout
// The 2L+1 states of the blank-augmented label sequence are kept as two arrays per frame:
//   blanks  Bk[i] = state 2i     (i = 0..L)        labels  Lb[i] = state 2i+1  (i = 0..L-1)
// stored as one row of 2W doubles, INTERLEAVED: entry i = (Bk[i], Lb[i]) at doubles 2i, 2i+1 (round 5: one 16-byte load / store per
// lane and frame instead of two 8-byte ones - half the memory instructions the recursion has in flight, so that its prefetch can run
// three chunks ahead inside the 6-bit vmcnt counter), W = 32/64/128/256 >= L+1, zero beyond the valid entries.  In this form the recursions need ONE lane shift per step instead of two:
//   alpha: Bk'[i] = yB (Bk[i] + Lb[i-1])          Lb'[i] = yL[i] (Lb[i] + Bk[i]   + c[i]  Lb[i-1])
//   beta : Bk'[i] = yB (Bk[i] + Lb[i])            Lb'[i] = yL[i] (Lb[i] + Bk[i+1] + c'[i] Lb[i+1])
// with c[i] = lab[i] != lab[i-1], c'[i] = lab[i] != lab[i+1] (the skip transitions).

// ---------------------------------------------------------------------------------- kernel 1
// LOGD: the lattice inputs stay log-probabilities (-inf beyond the valid entries): the forced alignment's max / add recursion
template <typename T, bool LOGD>
__global__ __launch_bounds__(256) void ctc_lse_gather_kernel(const T* __restrict__ logits, const int32_t* __restrict__ in_len,
                                                             const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_len,
                                                             double* __restrict__ lp, float* __restrict__ lse_out, int B, int T_, int V, int ld, int Lmax,
                                                             int W, int blank) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rows = B * T_;
    for (int row = blockIdx.x * 4 + w; row < rows; row += gridDim.x * 4) {
        const int b = row / T_, t = row - b * T_;
        if (t >= in_len[b]) continue;
        const T* x = logits + (size_t)row * ld;
        const float lse = wave_row_lse<T>(x, V, lane, nullptr);
        if (lane == 0) lse_out[row] = lse;
        const int L = lab_len[b];
        double* out = lp + (size_t)row * 2 * W;
        const double lb = (double)(to_f32<T>(x[blank]) - lse);
        const double yb = LOGD ? lb : exp(lb);   // y_t(blank): linear domain, fp64
        const double none = LOGD ? -INFINITY : 0.0;
        for (int i = lane; i < W; i += 64) {   // zero beyond the valid entries: the recursion runs unpredicated
            const int c = labels[(size_t)b * Lmax + min(i, Lmax - 1)];
            const double ll = (double)(to_f32<T>(x[c]) - lse);
            const f64x2 e = {i <= L ? yb : none, i < L ? (LOGD ? ll : exp(ll)) : none};
            *(f64x2*)(out + 2 * i) = e;
        }
    }
}

// WRITE: the wave that holds the row also writes scale * softmax(row) to dlogits (zeros for padded frames) - the
// bulk of the CTC gradient, which does not depend on the lattice; ctc_label_fix_kernel later corrects the
// (at most L + 1) classes that occur in the label sequence.  One pass over the logits less than with a
// separate gradient kernel (270 instead of 406 MB at config 2).  dlogits may alias logits (no __restrict__:
// the gathers below must stay in front of the stores).
// PATH: the wave also writes the frame's best class (first index of the row maximum; `blank` for padded frames) to best_path - the
// greedy CTC path of the training step's CER, taken from the row while it is in registers (the gradient overwrites the logits in place).
// LOGD: as ctc_lse_gather_kernel
template <int NV, bool WRITE, bool PATH, bool LOGD = false>
__global__ __launch_bounds__(256) void ctc_lse_gather_rows_kernel(const bf16_t* logits, const int32_t* __restrict__ in_len,
                                                                  const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_len,
                                                                  double* __restrict__ lp, float* __restrict__ lse_out, int B, int T_, int V, int ld, int Lmax,
                                                                  int W, int blank, bf16_t* dlogits, float scale_in, const float* __restrict__ scale_div,
                                                                  int32_t* __restrict__ best_path) {
    const float scale = scale_div ? scale_in / *scale_div : scale_in;     // scale_div: a device scalar (global batch under data parallelism)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rows = B * T_, nvec = V >> 3;
    for (int row = blockIdx.x * 4 + w; row < rows; row += gridDim.x * 4) {
        const int b = row / T_, t = row - b * T_;
        if (t >= in_len[b]) {
            if (WRITE) {
                const u32x4 z = {0u, 0u, 0u, 0u};
                for (int i = lane; i < nvec; i += 64) *(u32x4*)(dlogits + (size_t)row * ld + (size_t)i * 8) = z;
            }
            if (PATH && lane == 0) best_path[row] = blank;
            continue;
        }
        const bf16_t* x = logits + (size_t)row * ld;
        u32x4 xv[NV];
        wave_row_load<NV>(x, nvec, lane, xv);
        const int L = lab_len[b];
        // the gathers are issued before the reduction so that their latency overlaps it
        float xl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = lane + 64 * j;
            xl[j] = (i < W) ? (float)x[labels[(size_t)b * Lmax + min(i, Lmax - 1)]] : 0.f;
        }
        const float xb = (float)x[blank];
        float row_max;
        const float lse = wave_row_lse_regs<NV>(xv, nvec, lane, &row_max);
        if (lane == 0) lse_out[row] = lse;
        if (PATH) {
            const int bi = wave_row_argmax_regs<NV>(xv, nvec, lane, row_max);
            if (lane == 0) best_path[row] = bi;
        }
        if (WRITE) {
            bf16_t* dl = dlogits + (size_t)row * ld;
            const float lb = lse * LOG2E;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int i = lane + 64 * k;
                float v[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[2 * j] = scale * __builtin_amdgcn_exp2f(fmaf(bf16_lo(xv[k][j]), LOG2E, -lb));
                    v[2 * j + 1] = scale * __builtin_amdgcn_exp2f(fmaf(bf16_hi(xv[k][j]), LOG2E, -lb));
                }
                if (i < nvec) store8<bf16_t>(dl + (size_t)i * 8, v);
            }
        }
        double* out = lp + (size_t)row * 2 * W;
        const double yb = LOGD ? (double)(xb - lse) : exp((double)(xb - lse));   // y_t(blank): linear domain, fp64
        const double none = LOGD ? -INFINITY : 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = lane + 64 * j;
            if (i < W) {   // zero beyond the valid entries: the recursion runs unpredicated
                const f64x2 e = {i <= L ? yb : none, i < L ? (LOGD ? (double)(xl[j] - lse) : exp((double)(xl[j] - lse))) : none};
                *(f64x2*)(out + 2 * i) = e;
            }
        }
    }
}

// ---------------------------------------------------------------------------------- kernel 2
// The recursion runs in the LINEAR domain with rescaling (the classic scaled forward-backward) in
// fp64 (alpha and beta of one frame can sit > 1e38 apart at the state where their PRODUCT peaks,
// which fp32 cannot hold once a column is scaled to its maximum): one step is a lane shift, an
// add, an fma and a multiply instead of 3 exp + 1 log, and the rescaling is an exact power of two
// folded into a LATER frame's y so that the wave-wide max reduction is off the dependent chain.
// The kernel is a pure dependent chain on B workgroups: instructions per step are what it costs.
// log p(l|x) = ln2 * (sum of exponents taken out) + log of the final column; per-frame scale
// factors cancel in the posterior (it is normalised over the states).
// Whole-wave shifts by one lane through DPP (no LDS round trip as ds_bpermute would need): the
// lane that has no source gets 0.  wave_shr1 is asr_common.h's.
__device__ __forceinline__ double wave_shl1(double v) {   // lane i <- lane i+1
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_bcast(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
// max over the 64 lanes of unsigned values, DPP only (prefix max inside each 16-lane row, then
// row broadcasts); the result is uniform.  Used on the HIGH words of non-negative doubles, whose
// bit patterns order like the values.
// LAST = highest active lane (63, or 31 when only half the wave runs).
template <int LAST>
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#define DPP_MAX(ctrl, rmask)                                                                                   \
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rmask, 0xf, false))
    DPP_MAX(0x111, 0xf);   // row_shr:1
    DPP_MAX(0x112, 0xf);   // row_shr:2
    DPP_MAX(0x114, 0xf);   // row_shr:4
    DPP_MAX(0x118, 0xf);   // row_shr:8   -> lane 15 of every row holds the row maximum
    DPP_MAX(0x142, 0xa);   // row_bcast:15 into rows 1 and 3
    if (LAST == 63) DPP_MAX(0x143, 0xc);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave maximum
#undef DPP_MAX
    return (unsigned)__builtin_amdgcn_readlane((int)v, LAST);
}

// What the scaled lattice holds.  A column is scaled by its MAXIMUM, so a state further than the fp64 range below it becomes 0 although
// it may be the one that matters: the final states of a long label sequence under blank-dominated posteriors (blank ~ 0.99, every label
// ~ 1e-5: the all-blank prefix is the maximum and the final states sit (p_label / p_blank)^L below it), or every alpha * beta of a frame.
// A loss tail or a frame's posterior sum below LATTICE_TINY (scaled units; ordinary utterances are within 1e-40 of 1) has left that
// range or is about to: what was lost on the way to a sum >= 2^-600 is below 2^-1022 * S / y, a relative 1e-120.  Such an utterance is
// marked (nll_raw = NaN) and ctc_rescue_kernel redoes it in the log domain; +inf is left to the utterances whose LENGTHS are infeasible.
constexpr double LATTICE_TINY = 0x1p-600;

// The lattice row walk of both recursions (ctc_recursion, ctc_viterbi_recursion): steps 1 .. nsteps over the rows of the lattice inputs,
// DT doubles apart (+-2W: forward or backward in time), prefetched in chunks of CH steps into NB register buffers.  NS = registers per
// lane per array (entry i = lane + 64 j); yp = this lane's pair of the row of step 0.
//   one_step(yv, off, k): one recursion step on the row yv; k = its place in its chunk (the scaled recursion's phases), off = its place
//                         among the steps since the last advance() - the step stores at off rows from its own running pointer;
//   advance(n)          : n steps are done, the step's pointer moves n rows.
// Every load and store of the steady-state loop is unconditional, at an
// immediate offset from one running pointer per array, and the loop body is one basic block, so the
// compiler counts outstanding memory operations (s_waitcnt vmcnt(N), N > 0) and the prefetched
// chunk really overlaps the dependent chain.  (With predicated loads it fell back to vmcnt(0)
// per chunk: ~1.5 us of exposed latency 60 times per utterance.)
template <int NS, ptrdiff_t DT, typename Step, typename Advance>
__device__ __forceinline__ void lattice_row_walk(const double* __restrict__ yp, int nsteps, Step&& one_step, Advance&& advance) {
    constexpr int CH = 8;  // steps per prefetch chunk; chunk c covers steps 1 + c*CH .. c*CH + CH
    // Prefetch depth.  The recursion is a dependent chain of ~25 ns per frame; a lattice row comes from memory (written by the kernel before
    // this one) in ~0.7 us.  With two chunk buffers (round 1 - 4) the chunk after the current one was requested one chunk = 8 frames earlier
    // and every chunk ended in a wait for memory: 88 ns per frame.  NB buffers = NB - 1 chunks in flight; memory instructions per chunk =
    // CH loads + CH stores (16-byte accesses; byte stores in the Viterbi walk), so three chunks in flight stay inside the 6-bit vmcnt
    // counter (stores count too on gfx950).
    constexpr int NB = NS == 1 ? 4 : 2;
    struct Chunk { f64x2 v[CH][NS]; };
    Chunk q[NB];
    auto fetch = [&](Chunk& d, const double* p) {   // p = row of the chunk's first step
#pragma unroll
        for (int k = 0; k < CH; ++k)
#pragma unroll
            for (int j = 0; j < NS; ++j) d.v[k][j] = *(const f64x2*)(p + k * DT + 128 * j);
    };
    auto fetch_clamped = [&](Chunk& d, int chunk) {   // rows past the last frame are clamped to it (never used)
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int step = min(1 + chunk * CH + k, nsteps);
#pragma unroll
            for (int j = 0; j < NS; ++j) d.v[k][j] = *(const f64x2*)(yp + (ptrdiff_t)step * DT + 128 * j);
        }
    };
    const int nfull = nsteps / CH;
    int c = 0;
#pragma unroll
    for (int i = 0; i < NB - 1; ++i) fetch_clamped(q[i], i);      // q[i] = chunk c + i for i < NB - 1
    const double* yq = yp + DT;   // row of step 1 + c*CH
    // steady state: the chunks requested in an iteration (c + NB - 1 .. c + 2 NB - 2) are full, every access unconditional
    for (; c + 2 * NB - 1 <= nfull; c += NB) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            fetch(q[(i + NB - 1) % NB], yq + (i + NB - 1) * CH * DT);
#pragma unroll
            for (int k = 0; k < CH; ++k) one_step(q[i].v[k], i * CH + k, k);
        }
        yq += NB * CH * DT;
        advance(NB * CH);
    }
    // the last chunks (fewer than 2 NB, the last one possibly partial); q[0 .. NB-2] hold chunks c .. c + NB - 2
    for (; c * CH < nsteps; ++c) {
        fetch_clamped(q[NB - 1], c + NB - 1);
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            if (1 + c * CH + k > nsteps) break;
            one_step(q[0].v[k], k, k);
        }
        advance(CH);
#pragma unroll
        for (int i = 0; i + 1 < NB; ++i) q[i] = q[i + 1];
    }
}

// W = row half-width (compile time: 32, 64, 128, 256), NS as in lattice_row_walk.
// Returns ln of the scale taken out (true value = stored value * exp(ret)), or -inf once every
// state has become 0 (infeasible alignment).
template <int W, bool BWD>
__device__ __forceinline__ double ctc_recursion(const double* __restrict__ y, double* __restrict__ out, const int32_t* __restrict__ lab,
                                                int Tb, int L, int lane) {
    constexpr int NS = W <= 64 ? 1 : W / 64;
    constexpr ptrdiff_t RW = 2 * W;             // row stride
    constexpr ptrdiff_t DT = BWD ? -RW : RW;    // the frame of recursion step k is t = k (alpha) or Tb-1-k (beta)
    int esum = 0;          // sum of the binary exponents scaled away so far
    bool dead = false;     // every state reached 0
    double skip[NS];       // 1.0 where the label-to-label skip transition into (alpha) / out of (beta) Lb[i] exists
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int i = lane + 64 * j;
        bool c;
        if (!BWD) c = i >= 1 && i < L && lab[i] != lab[i - 1];
        else c = i + 1 < L && lab[i] != lab[i + 1];
        skip[j] = c ? 1.0 : 0.0;
    }
    // entry i = lane + 64 j of a row sits at doubles 2 i (blank), 2 i + 1 (label): one 16-byte access per lane and register
    const double* yp = y + (BWD ? (size_t)(Tb - 1) * RW : 0) + 2 * lane;   // step 0
    double* op = out + (BWD ? (size_t)(Tb - 1) * RW : 0) + 2 * lane;
    double bk[NS], lb[NS];
    // step 0: the two entry states (alpha: Bk[0], Lb[0]; beta: Bk[L], Lb[L-1])
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int i = lane + 64 * j;
        const f64x2 y0 = *(const f64x2*)(yp + 128 * j);
        bk[j] = (BWD ? i == L : i == 0) ? y0[0] : 0.0;
        lb[j] = (BWD ? i == L - 1 : i == 0) ? y0[1] : 0.0;
        const f64x2 o0 = {bk[j], lb[j]};
        *(f64x2*)(op + 128 * j) = o0;
    }
    double sc = 1.0;   // power-of-two scale waiting to be applied
    int e_pending = 0;
    double* oq = op + DT;   // output row of the first step since the last advance
    auto one_step = [&](const f64x2 (&yv)[NS], int off, int k) {
        double yb[NS], yl[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) { yb[j] = yv[j][0]; yl[j] = yv[j][1]; }
        if ((k & 3) == 1) {   // apply the scale found two steps ago: off the chain, it multiplies y
#pragma unroll
            for (int j = 0; j < NS; ++j) { yb[j] *= sc; yl[j] *= sc; }
            esum += e_pending;
        }
        double nb[NS], nl[NS];
        if (!BWD) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                double sh = wave_shr1(lb[j]);          // Lb[i-1]
                if (j > 0) sh = lane == 0 ? lane_bcast(lb[j > 0 ? j - 1 : 0], 63) : sh;
                nb[j] = yb[j] * (bk[j] + sh);
                nl[j] = yl[j] * fma(skip[j], sh, lb[j] + bk[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                double sb = wave_shl1(bk[j]);          // Bk[i+1]
                double sl = wave_shl1(lb[j]);          // Lb[i+1]
                if (j + 1 < NS) {
                    sb = lane == 63 ? lane_bcast(bk[j + 1 < NS ? j + 1 : j], 0) : sb;
                    sl = lane == 63 ? lane_bcast(lb[j + 1 < NS ? j + 1 : j], 0) : sl;
                }
                nb[j] = yb[j] * (bk[j] + lb[j]);
                nl[j] = yl[j] * fma(skip[j], sl, lb[j] + sb);
            }
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) { bk[j] = nb[j]; lb[j] = nl[j]; }
        if ((k & 3) == 3) {
            // Every 4th step: binary exponent e of the column maximum (integer DPP max over the
            // doubles' high words); 2^-e is applied two steps later.  No division, no log: the
            // loss only needs the SUM of the exponents.  Six steps shrink the maximum by y^6, far
            // inside the fp64 range for any y a softmax can produce.  Branch-free.
            unsigned hi = 0u;
#pragma unroll
            for (int j = 0; j < NS; ++j) hi = max(hi, max((unsigned)__double2hiint(bk[j]), (unsigned)__double2hiint(lb[j])));
            hi = wave_max_u32<(W < 64 ? W : 64) - 1>(hi);
            const bool zero = (hi >> 20) == 0u;            // all states 0 (or denormal: treated as dead)
            e_pending = zero ? 0 : (int)(hi >> 20) - 1023;
            sc = __hiloint2double((1023 - e_pending) << 20, 0);
            dead |= zero;
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const f64x2 ov = {bk[j], lb[j]};
            *(f64x2*)(oq + off * DT + 128 * j) = ov;
        }
    };
    lattice_row_walk<NS, DT>(yp, Tb - 1, one_step, [&](int n) { oq += n * DT; });      // recursion steps 1 .. Tb-1
    return dead ? -INFINITY : (double)esum * 0.6931471805599453;
}

template <int W>
__global__ __launch_bounds__(128) void ctc_alpha_beta_kernel(const double* __restrict__ lp, double* __restrict__ alpha, double* __restrict__ beta,
                                                             const int32_t* __restrict__ in_len, const int32_t* __restrict__ labels,
                                                             const int32_t* __restrict__ lab_len, float* __restrict__ nll_out, float* __restrict__ nll_raw,
                                                             int T_, int Lmax, int blank, int zero_infinity) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: each wave runs only its own direction
    const int Tb = in_len[b], L = lab_len[b];
    constexpr size_t RW = 2 * (size_t)W;
    const double* lpb = lp + (size_t)b * T_ * RW;
    double* ab = alpha + (size_t)b * T_ * RW;
    double* bb = beta + (size_t)b * T_ * RW;
    const int32_t* lab = labels + (size_t)b * Lmax;
    __shared__ double s_logc;
    if (Tb > 0 && (W >= 64 || lane < W)) {   // W = 32: half a wave
        if (w == 0) {
            const double logc = ctc_recursion<W, false>(lpb, ab, lab, Tb, L, lane);
            if (lane == 0) s_logc = logc;
        } else {
            ctc_recursion<W, true>(lpb, bb, lab, Tb, L, lane);
        }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        float nll;
        if (Tb <= 0) {
            nll = (L == 0) ? 0.f : INFINITY;
        } else {
            const double* last = ab + (size_t)(Tb - 1) * RW;
            const double tail = last[2 * L] + (L > 0 ? last[2 * (L - 1) + 1] : 0.0);      // interleaved rows: (blank, label) pairs
            nll = (tail >= LATTICE_TINY && s_logc != -INFINITY) ? (float)(-(s_logc + log(tail))) : INFINITY;
        }
        if (nll == INFINITY) {
            // The lattice ended at 0 (or below what it holds at full precision).  Whether the labels fit the frames is a matter of the
            // lengths alone: in_len >= L + adjacent repeats.  If they fit, the lattice left the fp64 range below its column maxima
            // (blank-dominated posteriors, long labels): NaN hands the utterance to ctc_rescue_kernel.
            int need = L;
            for (int i = 1; i < L; ++i) need += lab[i] == lab[i - 1];
            if (Tb >= need && Tb > 0) nll = NAN;
        }
        nll_raw[b] = nll;
        nll_out[b] = (nll == INFINITY && zero_infinity) ? 0.f : nll;
    }
}

// ---------------------------------------------------------------------------------- kernel 3
template <typename T>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const T* __restrict__ logits, T* __restrict__ dlogits, const double* __restrict__ lp,
                                                       const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       const float* __restrict__ lse_in, const int32_t* __restrict__ in_len,
                                                       const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_len,
                                                       float* nll_raw, int B, int T_, int V, int ld, int Lmax, int W, int blank,
                                                       float scale_in, int det, const float* __restrict__ scale_div) {
    const float scale = scale_div ? scale_in / *scale_div : scale_in;
    extern __shared__ __attribute__((aligned(16))) float occ[];  // V floats: posterior mass per label
    constexpr int N = Vec<T>::N;
    const int rows = B * T_;
    for (int i = threadIdx.x; i < V; i += 256) occ[i] = 0.f;
    __syncthreads();
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int b = row / T_, t = row - b * T_;
        T* dl = dlogits + (size_t)row * ld;
        // padded frame, or infeasible utterance (nll = +inf): zero gradient
        if (t >= in_len[b] || nll_raw[b] == INFINITY) {
            if (V % N == 0) {
                float z[N];
#pragma unroll
                for (int j = 0; j < N; ++j) z[j] = 0.f;
                for (int i = threadIdx.x; i < V / N; i += 256) storev<T>(dl + (size_t)i * N, z);
            } else {
                for (int i = threadIdx.x; i < V; i += 256) dl[i] = from_f32<T>(0.f);
            }
            continue;
        }
        const T* x = logits + (size_t)row * ld;
        const int L = lab_len[b];
        const float lse = lse_in[row];
        // nll_raw = NaN: the utterance waits for ctc_rescue_kernel, which overwrites the label classes; the row is the plain softmax until then
        if (threadIdx.x < 64 && nll_raw[b] == nll_raw[b]) {
            // posterior of a state at this frame, up to a per-frame constant: alpha * beta / y
            // (both recursions include y_t).  sum_s alpha_t(s) beta_t(s) / y_t(l'_s) = p(l|x) for
            // EVERY t, so normalising over s is exact and needs neither nll nor the scale factors.
            const size_t o = (size_t)row * 2 * W;
            double sum_b = 0.0, sum_l = 0.0;
            for (int i = threadIdx.x; i <= L; i += 64) {
                const double yb = lp[o + 2 * i], yl = lp[o + 2 * i + 1];
                sum_b += yb > 0.0 ? alpha[o + 2 * i] * beta[o + 2 * i] / yb : 0.0;
                sum_l += (i < L && yl > 0.0) ? alpha[o + 2 * i + 1] * beta[o + 2 * i + 1] / yl : 0.0;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                sum_b += __shfl_xor(sum_b, off, 64);
                sum_l += __shfl_xor(sum_l, off, 64);
            }
            const double sum = sum_b + sum_l;
            if (!(sum >= LATTICE_TINY)) {      // every alpha * beta of this frame left the fp64 range: the whole utterance is redone
                if (threadIdx.x == 0) nll_raw[b] = NAN;
            } else {
                if (threadIdx.x == 0) occ[blank] = (float)(sum_b / sum);      // all blank states share one class
                if (det) {   // repeated labels share a class: add their states in label order (fixed order)
                    if (threadIdx.x == 0)
                        for (int i = 0; i < L; ++i) {
                            const double yl = lp[o + 2 * i + 1];
                            if (yl > 0.0) occ[labels[(size_t)b * Lmax + i]] += (float)(alpha[o + 2 * i + 1] * beta[o + 2 * i + 1] / yl / sum);
                        }
                } else
                for (int i = threadIdx.x; i < L; i += 64) {
                    const double yl = lp[o + 2 * i + 1];
                    if (yl > 0.0) atomicAdd(&occ[labels[(size_t)b * Lmax + i]], (float)(alpha[o + 2 * i + 1] * beta[o + 2 * i + 1] / yl / sum));
                }
            }
        }
        __syncthreads();
        if (V % N == 0) {
            for (int i = threadIdx.x; i < V / N; i += 256) {
                float v[N];
                loadv<T>(x + (size_t)i * N, v);
#pragma unroll
                for (int j = 0; j < N; ++j) v[j] = scale * (expf(v[j] - lse) - occ[i * N + j]);
                storev<T>(dl + (size_t)i * N, v);
            }
        } else {
            for (int i = threadIdx.x; i < V; i += 256) dl[i] = from_f32<T>(scale * (expf(to_f32<T>(x[i]) - lse) - occ[i]));
        }
        __syncthreads();
        if (threadIdx.x == 0) occ[blank] = 0.f;
        for (int i = threadIdx.x; i < L; i += 256) occ[labels[(size_t)b * Lmax + i]] = 0.f;
        __syncthreads();
    }
}

// Second half of the split gradient: the row already holds scale * softmax (ctc_lse_gather_rows_kernel<.., true>);
// one wave per frame subtracts the posterior mass of the classes that occur in the label sequence by
// overwriting those few elements, and zeroes the rows of infeasible utterances (nll = +inf).
__global__ __launch_bounds__(256) void ctc_label_fix_kernel(bf16_t* __restrict__ dlogits, const double* __restrict__ lp, const double* __restrict__ alpha,
                                                            const double* __restrict__ beta, const int32_t* __restrict__ in_len,
                                                            const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_len,
                                                            float* nll_raw, int B, int T_, int V, int ld, int Lmax, int W, int blank, float scale_in, const float* __restrict__ scale_div) {
    const float scale = scale_div ? scale_in / *scale_div : scale_in;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rows = B * T_, nvec = V >> 3;
    for (int row = blockIdx.x * 4 + w; row < rows; row += gridDim.x * 4) {
        const int b = row / T_, t = row - b * T_;
        if (t >= in_len[b]) continue;           // already zero
        bf16_t* dl = dlogits + (size_t)row * ld;
        if (nll_raw[b] == INFINITY) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            for (int i = lane; i < nvec; i += 64) *(u32x4*)(dl + (size_t)i * 8) = z;
            continue;
        }
        if (nll_raw[b] != nll_raw[b]) continue;      // NaN: waits for ctc_rescue_kernel; the row holds the plain softmax, which is what that kernel expects
        const int L = lab_len[b];
        // posterior of a state at this frame, up to a per-frame constant: alpha * beta / y; normalising over the
        // states is exact (see ctc_grad_kernel: the sum over s of alpha beta / y is p(l | x) at EVERY t, so it needs neither nll nor the scale factors)
        const size_t o = (size_t)row * 2 * W;
        double pb = 0.0, pl[4], yl[4];
        int lab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = lane + 64 * j;
            pl[j] = 0.0;
            yl[j] = 0.0;
            lab[j] = -1;
            if (i <= L && i < W) {
                // entry i = (blank, label) pair: one 16-byte load per array
                const f64x2 yv = *(const f64x2*)(lp + o + 2 * i), av = *(const f64x2*)(alpha + o + 2 * i), bv = *(const f64x2*)(beta + o + 2 * i);
                pb += yv[0] > 0.0 ? av[0] * bv[0] / yv[0] : 0.0;
                if (i < L) {
                    yl[j] = yv[1];
                    pl[j] = yl[j] > 0.0 ? av[1] * bv[1] / yl[j] : 0.0;
                    lab[j] = labels[(size_t)b * Lmax + i];
                }
            }
        }
        double sum = pb + pl[0] + pl[1] + pl[2] + pl[3];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sum += __shfl_xor(sum, off, 64);
            pb += __shfl_xor(pb, off, 64);
        }
        if (!(sum >= LATTICE_TINY)) {      // every alpha * beta of this frame left the fp64 range: the whole utterance is redone (ctc_rescue_kernel)
            if (lane == 0) nll_raw[b] = NAN;
            continue;
        }
        const double inv = 1.0 / sum;
        float occ[4] = {0.f, 0.f, 0.f, 0.f};   // occupancy of each label's class = sum over the positions that carry the same label
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (64 * jj >= L) break;
            const int cnt = min(64, L - 64 * jj);
            const float pj_all = (float)(pl[jj] * inv);
            for (int q = 0; q < cnt; ++q) {
                const int lq = __shfl(lab[jj], q, 64);
                const float pq = __shfl(pj_all, q, 64);
#pragma unroll
                for (int j = 0; j < 4; ++j) occ[j] += (lab[j] == lq) ? pq : 0.f;
            }
        }
        if (lane == 0) dl[blank] = (bf16_t)(scale * ((float)lp[o] - (float)(pb * inv)));   // every blank state has the same y
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lab[j] >= 0) dl[lab[j]] = (bf16_t)(scale * ((float)yl[j] - occ[j]));       // positions with equal labels write equal values
    }
}

// Loss without a gradient: no kernel 3 looks at the frames, and a loss tail in range does not show that no path mass was lost on the
// way (alpha may have dropped states that only a far-away beta maximum would have shown to matter).  One wave per frame forms the sum
// kernel 3 forms and marks the utterance by the same rule.
__global__ __launch_bounds__(256) void ctc_frame_check_kernel(const double* __restrict__ lp, const double* __restrict__ alpha, const double* __restrict__ beta,
                                                              const int32_t* __restrict__ in_len, const int32_t* __restrict__ lab_len, float* nll_raw,
                                                              int B, int T_, int W) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rows = B * T_;
    for (int row = blockIdx.x * 4 + w; row < rows; row += gridDim.x * 4) {
        const int b = row / T_, t = row - b * T_;
        const float raw = nll_raw[b];
        if (t >= in_len[b] || raw == INFINITY || raw != raw) continue;
        const int L = lab_len[b];
        const size_t o = (size_t)row * 2 * W;
        double sum = 0.0;
        for (int i = lane; i <= L; i += 64) {
            const f64x2 yv = *(const f64x2*)(lp + o + 2 * i), av = *(const f64x2*)(alpha + o + 2 * i), bv = *(const f64x2*)(beta + o + 2 * i);
            sum += yv[0] > 0.0 ? av[0] * bv[0] / yv[0] : 0.0;
            sum += (i < L && yv[1] > 0.0) ? av[1] * bv[1] / yv[1] : 0.0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (!(sum >= LATTICE_TINY) && lane == 0) nll_raw[b] = NAN;
    }
}

// ---------------------------------------------------------------------------------- kernel 4: out-of-range utterances
// Runs after the gradient kernels, one workgroup per utterance; returns at once unless the utterance is marked (nll_raw = NaN: the
// scaled lattice lost the loss tail or a frame's posteriors, see LATTICE_TINY).  A marked utterance is redone in the LOG domain in fp64,
// exact at any range and ~50 x slower per frame than the scaled recursion (an LDS exchange, three exp and a log per state and frame):
//   forward : log alpha, thread i = entry i = states 2i (blank) and 2i+1 (label), written over the utterance's rows of `alpha`;
//   loss    : nll = -logaddexp of the two final states;
//   backward: log beta in registers, frame by frame; the frame's state posteriors exp(la + lb - log y - log p) summed per class in
//             label order (fixed order) and the classes of the label sequence overwritten with scale * (y - posterior).
// Every other class of the row already holds scale * softmax: the gradient kernels subtract no label mass from a marked utterance.
// An utterance that is feasible by its lengths but has p = 0 (a y of exactly 0 on its only paths) ends as the infeasible ones do.
__device__ __forceinline__ double log_add(double a, double b) {
    const double m = fmax(a, b);
    return m == -INFINITY ? -INFINITY : m + log(exp(a - m) + exp(b - m));
}
__device__ __forceinline__ double log_of(double y) { return y > 0.0 ? log(y) : -INFINITY; }

template <typename T>
__global__ __launch_bounds__(256) void ctc_rescue_kernel(const double* __restrict__ lp, double* __restrict__ alpha, const int32_t* __restrict__ in_len,
                                                         const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_len,
                                                         float* __restrict__ nll_out, float* nll_raw, T* dlogits, int T_, int V, int ld, int Lmax,
                                                         int W, int blank, float scale_in, const float* __restrict__ scale_div, int zero_infinity) {
    const int b = blockIdx.x, i = threadIdx.x;
    if (nll_raw[b] == nll_raw[b]) return;      // uniform over the workgroup
    __shared__ double s_a[2][257], s_b[2][257], s_pb[2][256], s_pl[2][256];
    __shared__ int s_lab[256];
    __shared__ double s_fin[2];
    const int Tb = in_len[b], L = lab_len[b];
    const size_t RW = 2 * (size_t)W;
    const double* lpb = lp + (size_t)b * T_ * RW;
    double* ab = alpha + (size_t)b * T_ * RW;
    const int32_t* lab = labels + (size_t)b * Lmax;
    const bool in_row = i < W;                  // a row has W entries; L + 1 <= W of them are states
    const int mylab = i < L ? lab[i] : -1;
    const bool skip_in = i >= 1 && i < L && lab[i] != lab[i - 1];      // label-to-label transition into state 2i+1
    const bool skip_out = i + 1 < L && lab[i] != lab[i + 1];           // ... out of state 2i+1
    s_lab[i] = mylab;
    if (i < 2) { s_a[i][0] = -INFINITY; s_a[i][256] = -INFINITY; s_b[i][256] = -INFINITY; }
    // ---- forward.  s_a[p][i + 1] = log alpha of label state 2i+1 at the previous frame
    double a_b = -INFINITY, a_l = -INFINITY;
    for (int t = 0; t < Tb; ++t) {
        const int p = t & 1;
        f64x2 y = {0.0, 0.0};
        if (in_row) y = *(const f64x2*)(lpb + (size_t)t * RW + 2 * i);
        const double ly_b = log_of(y[0]), ly_l = log_of(y[1]);
        if (t == 0) {
            a_b = i == 0 ? ly_b : -INFINITY;
            a_l = i == 0 ? ly_l : -INFINITY;
        } else {
            s_a[p][i + 1] = a_l;
            __syncthreads();
            const double prev = s_a[p][i];      // state 2i-1
            const double n_b = ly_b + log_add(a_b, prev);
            const double n_l = ly_l + log_add(log_add(a_l, a_b), skip_in ? prev : -INFINITY);
            a_b = n_b;
            a_l = n_l;
        }
        if (in_row) {
            const f64x2 o = {a_b, a_l};
            *(f64x2*)(ab + (size_t)t * RW + 2 * i) = o;
        }
    }
    if (i == L) s_fin[0] = a_b;
    if (i == L - 1) s_fin[1] = a_l;
    if (L == 0 && i == 0) s_fin[1] = -INFINITY;
    __syncthreads();
    const double log_p = log_add(s_fin[0], s_fin[1]);
    const bool finite = log_p != -INFINITY;
    __syncthreads();      // everyone has read nll_raw[b] (top) before it changes
    if (i == 0) {
        const float nll = finite ? (float)(-log_p) : INFINITY;
        nll_raw[b] = nll;
        nll_out[b] = (!finite && zero_infinity) ? 0.f : nll;
    }
    if (!dlogits) return;
    T* dlb = dlogits + (size_t)b * T_ * ld;
    if (!finite) {
        for (int t = 0; t < Tb; ++t)
            for (int v = i; v < V; v += 256) dlb[(size_t)t * ld + v] = from_f32<T>(0.f);
        return;
    }
    const float scale = scale_div ? scale_in / *scale_div : scale_in;
    // ---- backward, and the frame's gradient.  s_a / s_b[p][i] = log beta of states 2i / 2i+1 at the frame after this one
    double b_b = -INFINITY, b_l = -INFINITY;
    for (int t = Tb - 1; t >= 0; --t) {
        const int p = t & 1;
        f64x2 y = {0.0, 0.0}, la = {-INFINITY, -INFINITY};
        if (in_row) {
            y = *(const f64x2*)(lpb + (size_t)t * RW + 2 * i);
            la = *(const f64x2*)(ab + (size_t)t * RW + 2 * i);
        }
        const double ly_b = log_of(y[0]), ly_l = log_of(y[1]);
        if (t == Tb - 1) {
            b_b = i == L ? ly_b : -INFINITY;
            b_l = i == L - 1 ? ly_l : -INFINITY;
        } else {
            const double nb_b = s_a[p ^ 1][i + 1], nb_l = s_b[p ^ 1][i + 1];      // states 2i+2, 2i+3
            const double n_b = ly_b + log_add(b_b, b_l);
            const double n_l = ly_l + log_add(log_add(b_l, nb_b), skip_out ? nb_l : -INFINITY);
            b_b = n_b;
            b_l = n_l;
        }
        s_a[p][i] = b_b;
        s_b[p][i] = b_l;
        // posterior of a state = alpha beta / (y p); a state that cannot be reached or cannot finish has none
        s_pb[p][i] = (la[0] == -INFINITY || b_b == -INFINITY) ? 0.0 : exp(la[0] + b_b - ly_b - log_p);
        s_pl[p][i] = (la[1] == -INFINITY || b_l == -INFINITY) ? 0.0 : exp(la[1] + b_l - ly_l - log_p);
        __syncthreads();
        T* dl = dlb + (size_t)t * ld;
        if (i == 0) {
            double occ = 0.0;
            for (int j = 0; j <= L; ++j) occ += s_pb[p][j];
            dl[blank] = from_f32<T>(scale * ((float)y[0] - (float)occ));      // every blank state has the same y
        }
        if (mylab >= 0) {
            double occ = 0.0;      // positions that carry the same label share a class and write equal values
            for (int j = 0; j < L; ++j) occ += s_lab[j] == mylab ? s_pl[p][j] : 0.0;
            dl[mylab] = from_f32<T>(scale * ((float)y[1] - (float)occ));
        }
    }
}

// ---------------------------------------------------------------------------------- forced alignment (Viterbi)
// The best single path through the lattice of kernel 1 (asr_ctc_align): the alpha recursion with max in place of +, one wave per
// utterance, same layout (entry i = lane + 64 j, interleaved (blank, label) rows) and the same prefetch, in the LOG domain (kernel 1 with
// LOGD): max and add cost what max and multiply do, nothing has to be rescaled, and no state can leave the fp64 range below the column
// maximum - which a best path under blank-dominated posteriors does in the scaled linear form (the all-blank prefix is the maximum, the
// path that spells L labels sits (p_label / p_blank)^L below it).  -inf = no path.  Every step also writes one back-pointer byte per entry:
//   bit 0      blank state 2i:   0 = stay, 1 = from Lb[i-1]
//   bits 1..2  label state 2i+1: 0 = stay, 1 = from Bk[i], 2 = from Lb[i-1] (skip)
// Ties prefer the state itself, then s-1, then s-2 (strict > below).  The rows (T x W bytes) live in LDS when they fit VIT_LDS_BP,
// else in the workspace, and the backtrace stages them into LDS VIT_LDS_BP bytes at a time: it is a chain of dependent reads, one per frame,
// and pays LDS latency per step instead of a global round trip.
constexpr int VIT_LDS_BP = 64 * 1024;

// fin_b / fin_l = the final column's Bk[L] and Lb[L-1] (log-probabilities of the best paths that end there; -inf = none).
template <int W>
__device__ __forceinline__ void ctc_viterbi_recursion(const double* __restrict__ y, uint8_t* bp, const int32_t* __restrict__ lab,
                                                        int Tb, int L, int lane, double& fin_b, double& fin_l) {
    constexpr int NS = W <= 64 ? 1 : W / 64;
    constexpr ptrdiff_t RW = 2 * W;
    bool skip[NS];         // the label-to-label transition into Lb[i] exists
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int i = lane + 64 * j;
        skip[j] = i >= 1 && i < L && lab[i] != lab[i - 1];
    }
    const double* yp = y + 2 * lane;
    uint8_t* op = bp + lane;            // back-pointer row t at op + t * W (row 0 is never written nor read)
    double bk[NS], lb[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int i = lane + 64 * j;
        const f64x2 y0 = *(const f64x2*)(yp + 128 * j);
        bk[j] = i == 0 ? y0[0] : -INFINITY;
        lb[j] = i == 0 ? y0[1] : -INFINITY;
    }
    uint8_t* oq = op + W;               // back-pointer row of the first step since the last advance
    auto one_step = [&](const f64x2 (&yv)[NS], int off, int) {
        double nb[NS], nl[NS];
        unsigned code[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            double sh = wave_shr1(lb[j]);          // Lb[i-1]; the shift leaves 0 in lane 0
            sh = lane == 0 ? (j > 0 ? lane_bcast(lb[j > 0 ? j - 1 : 0], 63) : -INFINITY) : sh;
            const bool fb = sh > bk[j];
            double ml = lb[j];
            unsigned cl = 0u;
            if (bk[j] > ml) { ml = bk[j]; cl = 1u; }
            if (skip[j] && sh > ml) { ml = sh; cl = 2u; }
            nb[j] = yv[j][0] + (fb ? sh : bk[j]);      // -inf stays -inf: no term is ever +inf
            nl[j] = yv[j][1] + ml;
            code[j] = (fb ? 1u : 0u) | (cl << 1);
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) { bk[j] = nb[j]; lb[j] = nl[j]; }
#pragma unroll
        for (int j = 0; j < NS; ++j) oq[off * W + 64 * j] = (uint8_t)code[j];
    };
    lattice_row_walk<NS, RW>(yp, Tb - 1, one_step, [&](int n) { oq += n * W; });      // the prefetch of ctc_recursion
    fin_b = -INFINITY;
    fin_l = -INFINITY;
#pragma unroll
    for (int j = 0; j < NS; ++j) {      // L is uniform: readlane of the one register that holds each end state
        if ((L >> 6) == j) fin_b = lane_bcast(bk[j], L & 63);
        if (L > 0 && ((L - 1) >> 6) == j) fin_l = lane_bcast(lb[j], (L - 1) & 63);
    }
}

// One wave per utterance: recursion, backtrace (state indices into path[]), then one pass over the frames, 64 at a time, that turns
// states into token ids and fills spans / token_logp (sums of log y over a token's frames by a segmented scan: fixed order).
template <int W, bool LDS_BP>
__global__ __launch_bounds__(64) void ctc_viterbi_kernel(const double* __restrict__ lp, uint8_t* __restrict__ bp_ws, const int32_t* __restrict__ in_len,
                                                         const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_len, int32_t* __restrict__ path,
                                                         int32_t* __restrict__ spans, float* __restrict__ token_logp, float* __restrict__ score,
                                                         int T_, int Lmax, int blank) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_bp[];
    __shared__ double s_fin[2];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = min(max(in_len[b], 0), T_);
    const int L = min(max(lab_len[b], 0), Lmax);
    constexpr size_t RW = 2 * (size_t)W;
    const double* lpb = lp + (size_t)b * T_ * RW;
    const int32_t* lab = labels + (size_t)b * Lmax;
    int32_t* pb = path + (size_t)b * T_;
    int32_t* spb = spans + (size_t)b * Lmax * 2;
    float* tlb = token_logp + (size_t)b * Lmax;
    uint8_t* bpg = bp_ws + (size_t)b * T_ * W;
    for (int i = lane; i < Lmax; i += 64) {     // overwritten below for the tokens of a feasible alignment
        spb[2 * i] = -1;
        spb[2 * i + 1] = -1;
        tlb[i] = i < L ? -INFINITY : 0.f;
    }
    if (Tb > 0 && (W >= 64 || lane < W)) {      // W = 32: half a wave
        double fb, fl;
        ctc_viterbi_recursion<W>(lpb, LDS_BP ? s_bp : bpg, lab, Tb, L, lane, fb, fl);
        if (lane == 0) { s_fin[0] = fb; s_fin[1] = fl; }
    }
    __syncthreads();
    bool feasible = L == 0;      // Tb = 0
    int s = 2 * L;
    if (Tb > 0) {
        const double fb = s_fin[0], fl = s_fin[1];
        s = fb >= fl ? 2 * L : 2 * L - 1;       // ties: end in the blank
        const double best = fb >= fl ? fb : fl;
        feasible = best > -INFINITY;            // a path exists: in_len >= L + adjacent repeats
        if (lane == 0) score[b] = (float)best;
    } else if (lane == 0) {
        score[b] = feasible ? 0.f : -INFINITY;
    }
    if (feasible && Tb > 0) {
        constexpr int F = VIT_LDS_BP / W;       // frames per staged block of back-pointer rows
        int t = Tb - 1;
        for (;;) {
            const int t0 = LDS_BP ? 0 : max(t - F + 1, 0);
            if (!LDS_BP) {      // rows t0 .. t of the workspace -> LDS (16-byte pieces; W is a multiple of 16)
                const int n16 = (t - t0 + 1) * (W / 16);
                const u32x4* src = (const u32x4*)(bpg + (size_t)t0 * W);
                for (int k = lane; k < n16; k += 64) ((u32x4*)s_bp)[k] = src[k];
                __syncthreads();
            }
            for (; t >= t0; --t) {
                if (lane == 0) pb[t] = s;
                if (t > 0) {
                    const unsigned cb = s_bp[(size_t)(t - t0) * W + (s >> 1)];
                    s = max((s & 1) ? s - (int)((cb >> 1) & 3u) : s - (int)(cb & 1u), 0);
                }
            }
            if (t < 0) break;
            __syncthreads();        // every lane is done with this block before the next one overwrites it
        }
    }
    __syncthreads();
    double carry = 0.0;     // running log y sum of the token that ends the previous block of frames
    int s_last = -1;        // state of the last frame of the previous block
    for (int t0 = 0; t0 < T_; t0 += 64) {
        const int t = t0 + lane;
        const int st = t < Tb ? (feasible ? pb[t] : 0) : -1;
        int nx = __shfl_down(st, 1, 64);
        if (lane == 63) nx = (feasible && t + 1 < Tb) ? pb[t + 1] : -1;
        int pv = __shfl_up(st, 1, 64);
        if (lane == 0) pv = s_last;
        const bool tok = st > 0 && (st & 1);
        double v = tok ? lpb[(size_t)t * RW + st] : 0.0;     // log y: the state index is the double's index in the interleaved row
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {      // inclusive scan over runs of one state (a token's frames are contiguous)
            const double u = __shfl_up(v, o, 64);
            const int su = __shfl_up(st, o, 64);
            if (lane >= o && su == st) v += u;
        }
        if (tok && st == s_last) v += carry;
        carry = __shfl(v, 63, 64);
        s_last = __shfl(st, 63, 64);
        if (tok) {
            const int i = st >> 1;
            if (pv != st) spb[2 * i] = t;
            if (nx != st) { spb[2 * i + 1] = t; tlb[i] = (float)v; }
        }
        if (t < T_) pb[t] = t < Tb ? (tok ? lab[st >> 1] : blank) : -1;
    }
}

// ---------------------------------------------------------------------------------- xent
// (value, index) of the row maximum over the workgroup, first index on ties (torch.argmax): every thread brings the first maximum of its own
// elements (ascending indices, strict >); `redi` = 8 ints of LDS
__device__ __forceinline__ int block_argmax(float v, int i, float* red, int* redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o, 64);
        const int i2 = __shfl_xor(i, o, 64);
        if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) { red[w] = v; redi[w] = i; }
    __syncthreads();
    float bv = red[0];
    int bi = redi[0];
    for (int k = 1; k < nw; ++k)
        if (red[k] > bv || (red[k] == bv && redi[k] < bi)) { bv = red[k]; bi = redi[k]; }
    return bi;
}

// ARGMAX: also write the row's greedy class (first index of the maximum) to argmax_out[row] - for EVERY row, ignored ones included: the
// reference's per-step CER takes pred.topk(1) of all rows (transformer_official.py:87-91), and the gradient overwrites the logits in place.
template <typename T, bool ARGMAX>
__global__ __launch_bounds__(256) void xent_kernel(const T* __restrict__ logits, const int32_t* __restrict__ gold, const float* __restrict__ n_valid,
                                                   float* __restrict__ row_nll, T* __restrict__ dlogits, int M, int V, int ignore_index,
                                                   float smoothing, float grad_scale, int32_t* __restrict__ argmax_out) {
    __shared__ float red[16];
    __shared__ int redi[8];
    constexpr int N = Vec<T>::N;
    const int row = blockIdx.x;
    const T* x = logits + (size_t)row * V;
    const int g = gold[row];
    const bool ignored = (g == ignore_index) || g < 0 || g >= V;
    T* dl = dlogits ? dlogits + (size_t)row * V : nullptr;
    float best = NEG_INF;
    int bi = 0x7fffffff;
    if (ignored) {
        if (ARGMAX) {
            for (int i = threadIdx.x; i < V; i += 256) {
                const float v = to_f32<T>(x[i]);
                if (v > best) { best = v; bi = i; }
            }
            const int a = block_argmax(best, bi, red, redi);      // contains barriers: every thread of the row's workgroup is here
            if (threadIdx.x == 0) argmax_out[row] = a;
        }
        if (threadIdx.x == 0) row_nll[row] = 0.f;
        if (dl) for (int i = threadIdx.x; i < V; i += 256) dl[i] = from_f32<T>(0.f);
        return;
    }
    float m = NEG_INF, s = 0.f, sx = 0.f;
    const bool vec = (V % N == 0);
    if (vec) {
        for (int i = threadIdx.x; i < V / N; i += 256) {
            float v[N];
            loadv<T>(x + (size_t)i * N, v);
            if (ARGMAX) {
#pragma unroll
                for (int j = 0; j < N; ++j)
                    if (v[j] > best) { best = v[j]; bi = i * N + j; }
            }
            float lm = v[0];
#pragma unroll
            for (int j = 1; j < N; ++j) lm = fmaxf(lm, v[j]);
            const float mn = fmaxf(m, lm);
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < N; ++j) { acc += expf(v[j] - mn); sx += v[j]; }
            s = s * expf(m - mn) + acc;
            m = mn;
        }
    } else {
        for (int i = threadIdx.x; i < V; i += 256) {
            const float v = to_f32<T>(x[i]);
            if (ARGMAX && v > best) { best = v; bi = i; }
            const float mn = fmaxf(m, v);
            s = s * expf(m - mn) + expf(v - mn);
            m = mn;
            sx += v;
        }
    }
    if (ARGMAX) {
        const int a = block_argmax(best, bi, red, redi);
        if (threadIdx.x == 0) argmax_out[row] = a;
    }
    const float gm = block_max(m, red);
    const float gs = block_sum(gm == NEG_INF ? 0.f : s * expf(m - gm), red);
    const float lse = gm + logf(gs);
    const float xg = to_f32<T>(x[g]);
    float q_gold = 1.f, q_other = 0.f;
    float loss = lse - xg;
    if (smoothing > 0.f) {  // Utils/loss.py:30-45
        const float tot_x = block_sum(sx, red);
        q_gold = 1.f - smoothing;
        q_other = smoothing / (float)V;
        const float sum_logp = tot_x - (float)V * lse;
        loss = -(q_gold * (xg - lse) + q_other * (sum_logp - (xg - lse)));
    }
    if (threadIdx.x == 0) row_nll[row] = loss;
    if (!dl) return;
    const float qsum = q_gold + q_other * (float)(V - 1);
    const float sc = grad_scale / *n_valid;
    if (vec) {
        for (int i = threadIdx.x; i < V / N; i += 256) {
            float v[N];
            loadv<T>(x + (size_t)i * N, v);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float q = (i * N + j == g) ? q_gold : q_other;
                v[j] = sc * (qsum * expf(v[j] - lse) - q);
            }
            storev<T>(dl + (size_t)i * N, v);
        }
    } else {
        for (int i = threadIdx.x; i < V; i += 256) {
            const float q = (i == g) ? q_gold : q_other;
            dl[i] = from_f32<T>(sc * (qsum * expf(to_f32<T>(x[i]) - lse) - q));
        }
    }
}

// lattice row stride: whole waves (see ctc_recursion)
// half-width W of a lattice row ([blanks | labels], 2W doubles): L+1 blanks must fit
static inline int width_of(int Lmax) { return Lmax < 32 ? 32 : Lmax < 64 ? 64 : Lmax < 128 ? 128 : 256; }
static inline int smax_of(int Lmax) { return 2 * width_of(Lmax); }

// the checks asr_ctc_fwd_bwd and asr_ctc_align share (after their own null-pointer check); a workspace below ws_need fails with ws_code
int ctc_check(const char* name, int B, int T, int V, int ld, int Lmax, int blank, size_t ws_bytes, size_t ws_need, int ws_code, int dtype) {
    if (B <= 0 || T <= 0 || V <= 1 || Lmax <= 0 || blank < 0 || blank >= V) ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d T=%d V=%d Lmax=%d blank=%d", name, B, T, V, Lmax, blank);
    if (ld < V || (ld != V && ld % 8)) ASR_FAIL(ASR_EINVAL, "%s: row stride ld=%d (V=%d): V, or a multiple of 8 above it", name, ld, V);
    if (Lmax > 255) ASR_FAIL(ASR_EINVAL, "%s: Lmax = %d: label sequences longer than 255 are not supported", name, Lmax);
    if (ws_bytes < ws_need) ASR_FAIL(ws_code, "%s: workspace %zu < %zu", name, ws_bytes, ws_need);
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "%s: dtype %d", name, dtype);
    return ASR_OK;
}

template <int I> using int_c = std::integral_constant<int, I>;

// Kernel 1 of both entry points: the lattice inputs lp and lse of every frame, LOGD for the forced alignment.  With dlogits the rows path
// also writes scale * softmax, with best_path the greedy path (off the rows path: asr_ctc_frame_argmax, in front of the gradient kernel
// that may overwrite the logits in place).  *g1 = the grid of the one-wave-per-frame kernels, *rows_path = the row-in-registers kernels ran.
template <bool LOGD>
int ctc_lattice_inputs(const void* logits, void* dlogits, int32_t* best_path, const int32_t* in_len, const int32_t* labels, const int32_t* lab_len,
                       double* lp, float* lse, int B, int T, int V, int ld, int Lmax, int W, int blank, float grad_scale, const float* grad_scale_div,
                       int dtype, hipStream_t st, int* g1_out, bool* rows_path_out) {
    const int rows = B * T;
    int g1 = ceil_div(rows, 4);
    if (g1 > 4096) g1 = 4096;
    // tuning option "cu_limit" (> 0 while the CTC branch of the joint model runs beside the decoder's chain of small kernels): the row kernels are
    // grid-stride loops - size them for that many CUs (8 four-wave workgroups each) instead of flooding every CU with 4096 short workgroups
    const int cu_lim = asr_option(ASR_OPT_CU_LIMIT);
    if (cu_lim > 0 && g1 > 8 * cu_lim) g1 = 8 * cu_lim;
    // bf16 rows of whole 16-byte vectors that fit a wave's registers take the row-in-registers kernels
    const int need = ceil_div(V / 8, 64);
    const bool rows_path = dtype == ASR_BF16 && V % 8 == 0 && ld % 8 == 0 && need <= 16 && ((uintptr_t)logits % 16) == 0 && (!dlogits || ((uintptr_t)dlogits % 16) == 0);
    *g1_out = g1;
    *rows_path_out = rows_path;
    if (best_path && !rows_path) {      // fp32 / odd shapes: the decoding kernel
        const int rc = asr_ctc_frame_argmax(logits, in_len, best_path, B, T, V, ld, blank, dtype, (void*)st);
        if (rc != ASR_OK) return rc;
    }
    if (rows_path) {
        // with a gradient: the softmax part of it is written by the same wave that reduces the row (one pass over the logits less than
        // with a separate row-in-registers gradient kernel: 110 vs 127 us; that kernel, ctc_grad_rows_kernel, is in the git history)
        auto launch = [&](auto write, auto path) {
            constexpr bool WRITE = decltype(write)::value, PATH = decltype(path)::value;
            auto k1 = [&](auto nv) {
                ctc_lse_gather_rows_kernel<decltype(nv)::value, WRITE, PATH, LOGD><<<g1, 256, 0, st>>>(
                    (const bf16_t*)logits, in_len, labels, lab_len, lp, lse, B, T, V, ld, Lmax, W, blank, WRITE ? (bf16_t*)dlogits : nullptr,
                    WRITE ? grad_scale : 0.f, WRITE ? grad_scale_div : nullptr, PATH ? best_path : nullptr);
            };
            if (need <= 2) k1(int_c<2>());
            else if (need <= 4) k1(int_c<4>());
            else if (need <= 6) k1(int_c<6>());
            else if (need <= 9) k1(int_c<9>());
            else if (need <= 12) k1(int_c<12>());
            else k1(int_c<16>());
        };
        if constexpr (LOGD) launch(std::false_type(), std::false_type());      // the alignment has neither
        else if (dlogits && best_path) launch(std::true_type(), std::true_type());
        else if (dlogits) launch(std::true_type(), std::false_type());
        else if (best_path) launch(std::false_type(), std::true_type());
        else launch(std::false_type(), std::false_type());
    } else if (dtype == ASR_F32) ctc_lse_gather_kernel<float, LOGD><<<g1, 256, 0, st>>>((const float*)logits, in_len, labels, lab_len, lp, lse, B, T, V, ld, Lmax, W, blank);
    else ctc_lse_gather_kernel<bf16_t, LOGD><<<g1, 256, 0, st>>>((const bf16_t*)logits, in_len, labels, lab_len, lp, lse, B, T, V, ld, Lmax, W, blank);
    return ASR_OK;
}

// one launch; arm: it may carry the stream's armed completion event (asr_launch_armed)
template <typename... KArgs, typename... Args>
void launch_maybe_armed(bool arm, void (*kernel)(KArgs...), dim3 grid, dim3 block, hipStream_t st, Args... args) {
    if (arm) asr_launch_armed(kernel, grid, block, 0, st, args...);
    else kernel<<<grid, block, 0, st>>>(static_cast<KArgs>(args)...);
}

}  // namespace

extern "C" size_t asr_ctc_workspace_bytes(int B, int T, int Lmax) {
    return (size_t)3 * B * T * smax_of(Lmax) * sizeof(double) + ((size_t)B * T + (size_t)B) * sizeof(float);
}

extern "C" int asr_ctc_fwd_bwd(const void* logits, void* dlogits, const int32_t* in_len, const int32_t* labels, const int32_t* lab_len,
                               float* nll, int B, int T, int V, int ld, int Lmax, int blank, float grad_scale, const float* grad_scale_div,
                               int zero_infinity, int32_t* best_path, void* ws, size_t ws_bytes, int dtype, void* stream) {
    if (!logits || !in_len || !labels || !lab_len || !nll || !ws) ASR_FAIL(ASR_EINVAL, "asr_ctc_fwd_bwd: null pointer");
    if (int rc = ctc_check("asr_ctc_fwd_bwd", B, T, V, ld, Lmax, blank, ws_bytes, asr_ctc_workspace_bytes(B, T, Lmax), ASR_EWORKSPACE, dtype)) return rc;
    const size_t lds = (size_t)((V + 3) & ~3) * sizeof(float);
    if (dlogits && lds > 160 * 1024 && !(dtype == ASR_BF16 && V % 8 == 0 && V <= 8192)) ASR_FAIL(ASR_EINVAL, "asr_ctc_fwd_bwd: V=%d does not fit the LDS posterior table", V);
    hipStream_t st = (hipStream_t)stream;
    const int W = width_of(Lmax), Smax = 2 * W;
    double* lp = (double*)ws;
    double* alpha = lp + (size_t)B * T * Smax;
    double* beta = alpha + (size_t)B * T * Smax;
    float* lse = (float*)(beta + (size_t)B * T * Smax);
    float* nll_raw = lse + (size_t)B * T;
    const int rows = B * T;
    int g1;
    bool rows_path;
    if (int rc = ctc_lattice_inputs<false>(logits, dlogits, best_path, in_len, labels, lab_len, lp, lse, B, T, V, ld, Lmax, W, blank, grad_scale, grad_scale_div, dtype, st, &g1, &rows_path))
        return rc;
#define AB(N) ctc_alpha_beta_kernel<N><<<B, 128, 0, st>>>(lp, alpha, beta, in_len, labels, lab_len, nll, nll_raw, T, Lmax, blank, zero_infinity)
    if (W == 32) AB(32);
    else if (W == 64) AB(64);
    else if (W == 128) AB(128);
    else AB(256);
#undef AB
    if (dlogits) {
        int g3 = rows < 2048 ? rows : 2048;
        if (rows_path) {
            ctc_label_fix_kernel<<<g1, 256, 0, st>>>((bf16_t*)dlogits, lp, alpha, beta, in_len, labels, lab_len, nll_raw, B, T, V, ld, Lmax, W, blank, grad_scale, grad_scale_div);
        } else if (dtype == ASR_F32) ctc_grad_kernel<float><<<g3, 256, lds, st>>>((const float*)logits, (float*)dlogits, lp, alpha, beta, lse, in_len, labels, lab_len, nll_raw, B, T, V, ld, Lmax, W, blank, grad_scale, asr_deterministic(), grad_scale_div);
        else ctc_grad_kernel<bf16_t><<<g3, 256, lds, st>>>((const bf16_t*)logits, (bf16_t*)dlogits, lp, alpha, beta, lse, in_len, labels, lab_len, nll_raw, B, T, V, ld, Lmax, W, blank, grad_scale, asr_deterministic(), grad_scale_div);
    }
    if (!dlogits) ctc_frame_check_kernel<<<g1, 256, 0, st>>>(lp, alpha, beta, in_len, lab_len, nll_raw, B, T, W);
    // utterances whose lattice left the fp64 range (marked by the kernels above): redone in the log domain; a workgroup of any other returns at once.
    // The last kernel: on the bf16 rows path with a gradient it may carry an armed completion event
    auto rescue = [&](auto e) {
        using E = decltype(e);
        launch_maybe_armed(rows_path && dlogits, ctc_rescue_kernel<E>, dim3(B), dim3(256), st, lp, alpha, in_len, labels, lab_len, nll, nll_raw, (E*)dlogits, T, V, ld, Lmax, W, blank,
                           grad_scale, grad_scale_div, zero_infinity);
    };
    if (dtype == ASR_F32) rescue(0.f);
    else rescue(bf16_t());
    ASR_CHECK_LAUNCH("asr_ctc_fwd_bwd");
    return ASR_OK;
}

extern "C" int asr_xent_fwd_bwd(const void* logits, const int32_t* gold, const float* n_valid, float* row_nll, void* dlogits, int M,
                                int V, int ignore_index, float smoothing, float grad_scale, int32_t* argmax_out, int dtype, void* stream) {
    if (!logits || !gold || !row_nll || (dlogits && !n_valid)) ASR_FAIL(ASR_EINVAL, "asr_xent_fwd_bwd: null pointer");
    if (M <= 0 || V <= 1) ASR_FAIL(ASR_EINVAL, "asr_xent_fwd_bwd: bad shape M=%d V=%d", M, V);
    hipStream_t st = (hipStream_t)stream;
    if (dtype != ASR_F32 && dtype != ASR_BF16) ASR_FAIL(ASR_EDTYPE, "asr_xent_fwd_bwd: dtype %d", dtype);
#define XENT(T_, A_) xent_kernel<T_, A_><<<M, 256, 0, st>>>((const T_*)logits, gold, n_valid, row_nll, (T_*)dlogits, M, V, ignore_index, smoothing, grad_scale, argmax_out)
    if (dtype == ASR_F32) { if (argmax_out) XENT(float, true); else XENT(float, false); }
    else { if (argmax_out) XENT(bf16_t, true); else XENT(bf16_t, false); }
#undef XENT
    ASR_CHECK_LAUNCH("asr_xent_fwd_bwd");
    return ASR_OK;
}

// ---------------------------------------------------------------------------------- forced alignment
// workspace: the lattice of kernel 1 in the log domain (B T 2W doubles), back-pointer rows (B T W bytes; used when T W > VIT_LDS_BP), lse (B T floats)
extern "C" size_t asr_ctc_align_workspace_bytes(int B, int T, int Lmax) {
    if (B <= 0 || T <= 0) return 0;
    const size_t n = (size_t)B * T, W = (size_t)width_of(Lmax);
    return n * 2 * W * sizeof(double) + n * W + n * sizeof(float);
}

extern "C" int asr_ctc_align(const void* logits, const int32_t* in_len, const int32_t* labels, const int32_t* lab_len, int32_t* path,
                             int32_t* spans, float* token_logp, float* score, int B, int T, int V, int ld, int Lmax, int blank, void* ws,
                             size_t ws_bytes, int dtype, void* stream) {
    if (!logits || !in_len || !labels || !lab_len || !path || !spans || !token_logp || !score || !ws) ASR_FAIL(ASR_EINVAL, "asr_ctc_align: null pointer");
    if (int rc = ctc_check("asr_ctc_align", B, T, V, ld, Lmax, blank, ws_bytes, asr_ctc_align_workspace_bytes(B, T, Lmax), ASR_EINVAL, dtype)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int W = width_of(Lmax);
    double* lp = (double*)ws;
    uint8_t* bp = (uint8_t*)(lp + (size_t)B * T * 2 * W);
    float* lse = (float*)(bp + (size_t)B * T * W);
    // kernel 1 of asr_ctc_fwd_bwd without gradient or path: the logits are read once into the lattice, kept as log-probabilities
    int g1;
    bool rows_path;
    (void)ctc_lattice_inputs<true>(logits, nullptr, nullptr, in_len, labels, lab_len, lp, lse, B, T, V, ld, Lmax, W, blank, 0.f, nullptr, dtype, st, &g1, &rows_path);
    const bool lds_bp = (size_t)T * W <= (size_t)VIT_LDS_BP;
    const size_t lds = lds_bp ? (size_t)T * W : (size_t)VIT_LDS_BP;
#define VIT(N, M)                                                                                                                        \
    do {                                                                                                                                 \
        static bool attr = false;                                                                                                        \
        if (!attr) { (void)hipFuncSetAttribute((const void*)ctc_viterbi_kernel<N, M>, hipFuncAttributeMaxDynamicSharedMemorySize, VIT_LDS_BP); attr = true; } \
        ctc_viterbi_kernel<N, M><<<B, 64, lds, st>>>(lp, bp, in_len, labels, lab_len, path, spans, token_logp, score, T, Lmax, blank);  \
    } while (0)
#define VIT_W(N) do { if (lds_bp) VIT(N, true); else VIT(N, false); } while (0)
    if (W == 32) VIT_W(32);
    else if (W == 64) VIT_W(64);
    else if (W == 128) VIT_W(128);
    else VIT_W(256);
#undef VIT_W
#undef VIT
    ASR_CHECK_LAUNCH("asr_ctc_align");
    return ASR_OK;
}
