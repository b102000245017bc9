// Reverberation by uniformly partitioned overlap-save convolution: the second path beside the direct FIR of augment.hip, for responses
// of up to ASR_REVERB_FFT_MAX_TAPS taps.  Same definition (include/asr_hip.h, tests/noise_ref.py), another evaluation:
//   window j of utterance b   = x[(j - 1) Bk, (j + 1) Bk), 0 outside [0, len)         -> spectrum X[b, j]
//   partition q of a response = h[q Bk, (q + 1) Bk) zero-padded to N                  -> spectrum H[b, q]     (Bk = N / 2 = 2048)
//   full[i Bk, (i + 1) Bk)    = last Bk samples of IFFT(sum_{q < P_b, q <= i} H[b, q] X[b, i - q]),   out[b, m - p] = full[m]
// Two launches.  reverb_fft_spectra_kernel: one workgroup per window and per partition of the responses the batch drew (per utterance:
// at most B responses, P_b = ceil(L_b / Bk) partitions each - spectra of the bank are never kept).  reverb_fft_apply_kernel: one
// workgroup per (utterance, output block): the products are accumulated over q in ascending order in registers, eight spectrum words per
// lane, then transformed back in LDS and stored shifted by the peak.  No atomics: the same input gives the same bits.  Windows that lie
// beyond the utterance and partitions beyond the response are neither computed nor read (the workspace may hold anything there).
// The transform itself is reverb_fft_core.h.
#include "asr_common.h"
#include "reverb_fft_core.h"

namespace {

using rfft::cf;
constexpr int FN = rfft::N, FM = rfft::M, BK = rfft::BK, FNT = rfft::NT;
static_assert(ASR_REVERB_FFT_MAX_TAPS % BK == 0 && FM == 8 * FNT, "eight spectrum words per lane");

struct Utt {
    int len, r, L, p, P, nwin;      // r < 0: no response; P partitions; windows 0 .. nwin - 1 are the ones that hold samples
};

__device__ __forceinline__ Utt utterance(const int32_t* __restrict__ wav_len, const int32_t* __restrict__ rir_idx, const int32_t* __restrict__ rir_len,
                                         const int32_t* __restrict__ rir_peak, int b, int Smax, int R, int Lcap) {
    Utt u;
    u.len = min(max(wav_len[b], 0), Smax);
    u.r = rir_idx[b];
    u.L = u.p = u.P = u.nwin = 0;
    if (u.r < 0 || u.r >= R) {
        u.r = -1;
        return u;
    }
    u.L = min(max(rir_len[u.r], 1), Lcap);
    u.p = min(max(rir_peak[u.r], 0), u.L - 1);
    u.P = (u.L + BK - 1) / BK;
    u.nwin = u.len > 0 ? (u.len + BK - 1) / BK + 1 : 0;
    return u;
}

// grid (NW + Pcap, B): workgroups x < NW transform window x of the utterance, the others partition x - NW of its response
__global__ __launch_bounds__(FNT) void reverb_fft_spectra_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ rir_idx,
                                                                 const float* __restrict__ rir, const int32_t* __restrict__ rir_len,
                                                                 const int32_t* __restrict__ rir_peak, const cf* __restrict__ tw, cf* __restrict__ Xs,
                                                                 cf* __restrict__ Hs, int Smax, int R, int Lcap, int NW, int Pcap) {
    __shared__ cf A[rfft::LDS_WORDS], Bf[rfft::LDS_WORDS];
    const int b = blockIdx.y, t = threadIdx.x;
    const Utt u = utterance(wav_len, rir_idx, rir_len, rir_peak, b, Smax, R, Lcap);
    if (u.r < 0) return;
    cf* dst;
    if ((int)blockIdx.x < NW) {
        const int j = blockIdx.x;
        if (j >= u.nwin) return;
        const float* __restrict__ x = wav + (size_t)b * Smax;
        const int g0 = (j - 1) * BK, len = u.len;
        rfft::fwd_first(t, tw, [&](int g) { return g0 + g >= 0 && g0 + g < len ? x[g0 + g] : 0.f; }, A);
        dst = Xs + ((size_t)b * NW + j) * FM;
    } else {
        const int q = blockIdx.x - NW;
        if (q >= u.P) return;
        const float* __restrict__ h = rir + (size_t)u.r * Lcap;
        const int k0 = q * BK, L = u.L;
        rfft::fwd_first(t, tw, [&](int g) { return g < BK && k0 + g < L ? h[k0 + g] : 0.f; }, A);      // nothing at or beyond rir_len is read
        dst = Hs + ((size_t)b * Pcap + q) * FM;
    }
    __syncthreads();
    rfft::lds_pass<8, 8, false>(t, tw, A, Bf);
    __syncthreads();
    rfft::lds_pass<8, 64, false>(t, tw, Bf, A);
    __syncthreads();
    rfft::lds_pass<4, 512, false>(t, tw, A, Bf);
    __syncthreads();
    rfft::fwd_store(t, tw, Bf, dst);
}

__device__ __forceinline__ void cmac(cf& acc, float hx, float hy, float xx, float xy) {
    acc.x = fmaf(hx, xx, acc.x);
    acc.x = fmaf(-hy, xy, acc.x);
    acc.y = fmaf(hx, xy, acc.y);
    acc.y = fmaf(hy, xx, acc.y);
}

// grid (NB, B): output block i = p / Bk + blockIdx.x of utterance b, i.e. out[b, n] for n in [i Bk - p, (i + 1) Bk - p) and [0, Smax):
// the NB = ceil(Smax / Bk) + 1 blocks of an utterance tile [0, Smax) exactly once whatever p is
__global__ __launch_bounds__(FNT) void reverb_fft_apply_kernel(const float* __restrict__ wav, const int32_t* __restrict__ wav_len, const int32_t* __restrict__ rir_idx,
                                                               const int32_t* __restrict__ rir_len, const int32_t* __restrict__ rir_peak, const cf* __restrict__ tw,
                                                               const cf* __restrict__ Xs, const cf* __restrict__ Hs, float* __restrict__ out, int Smax, int R,
                                                               int Lcap, int NW, int Pcap) {
    __shared__ __attribute__((aligned(16))) cf A[rfft::LDS_WORDS], Bf[rfft::LDS_WORDS];
    const int b = blockIdx.y, t = threadIdx.x;
    const Utt u = utterance(wav_len, rir_idx, rir_len, rir_peak, b, Smax, R, Lcap);
    const size_t row = (size_t)b * Smax;
    const int i = u.p / BK + blockIdx.x;
    const int nbase = i * BK - u.p;                        // out index of the block's first sample: > -Bk
    const int n_lo = max(nbase, 0), n_hi = min(nbase + BK, Smax);
    if (u.r < 0 || n_lo >= u.len) {                        // no response drawn: a copy (p = 0); nothing below len in this block: zeros
        for (int n = n_lo + t; n < n_hi; n += FNT) out[row + n] = n < u.len ? wav[row + n] : 0.f;
        return;
    }
    // words 2 t, 2 t + 1 (+ 512 e) of the product's sum; word 0 is the pair of real bins (0, N / 2): multiplied component by component
    cf acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = cf{0.f, 0.f};
    cf dc = cf{0.f, 0.f};
    const int q_lo = max(0, i - u.nwin + 1), q_hi = min(u.P - 1, i);      // windows at and beyond nwin are zero
    const f32x4* __restrict__ Hb = (const f32x4*)(Hs + (size_t)b * Pcap * FM) + t;
    const f32x4* __restrict__ Xb = (const f32x4*)(Xs + (size_t)b * NW * FM) + t;
    for (int q = q_lo; q <= q_hi; ++q) {
        const f32x4* __restrict__ hp = Hb + (size_t)q * (FM / 2);
        const f32x4* __restrict__ xp = Xb + (size_t)(i - q) * (FM / 2);
        f32x4 hv[4], xv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            hv[e] = hp[e * FNT];
            xv[e] = xp[e * FNT];
        }
        dc.x = fmaf(hv[0][0], xv[0][0], dc.x);
        dc.y = fmaf(hv[0][1], xv[0][1], dc.y);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            cmac(acc[2 * e], hv[e][0], hv[e][1], xv[e][0], xv[e][1]);
            cmac(acc[2 * e + 1], hv[e][2], hv[e][3], xv[e][2], xv[e][3]);
        }
    }
    if (t == 0) acc[0] = dc;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        A[rfft::pad(2 * t + 512 * e)] = acc[2 * e];      // 2 t and 2 t + 1 never straddle a padding word
        A[rfft::pad(2 * t + 512 * e) + 1] = acc[2 * e + 1];
    }
    __syncthreads();
    rfft::inv_first(t, tw, A, Bf);
    __syncthreads();
    rfft::lds_pass<8, 8, true>(t, tw, Bf, A);
    __syncthreads();
    rfft::lds_pass<8, 64, true>(t, tw, A, Bf);
    __syncthreads();
    const int len = u.len;
    float* __restrict__ o = out + row;
    rfft::inv_last(t, tw, Bf, [&](int s, float v) {
        const int n = nbase + s;
        if (n >= 0 && n < Smax) o[n] = n < len ? v : 0.f;
    });
}

}  // namespace

extern "C" size_t asr_reverb_fft_workspace_bytes(int B, int Smax, int Lcap) {
    if (B < 1 || Smax < 1 || Lcap < 1) return 0;
    return (size_t)B * (ceil_div(Smax, BK) + 1 + ceil_div(Lcap, BK)) * FM * sizeof(cf);
}

extern "C" int asr_reverb_fft_fwd(const float* wav, const int32_t* wav_len, const int32_t* rir_idx, const float* rir, const int32_t* rir_len,
                                  const int32_t* rir_peak, const float* twiddle, float* out, void* ws, size_t ws_bytes, int B, int Smax, int R, int Lcap,
                                  void* stream) {
    if (!wav || !wav_len || !rir_idx || !rir || !rir_len || !rir_peak || !twiddle || !out || !ws) ASR_FAIL(ASR_EINVAL, "asr_reverb_fft_fwd: null pointer");
    if (B < 1 || Smax < 1 || B > 65535) ASR_FAIL(ASR_EINVAL, "asr_reverb_fft_fwd: bad shape B=%d Smax=%d", B, Smax);
    if (R < 1 || Lcap < 1 || Lcap > ASR_REVERB_FFT_MAX_TAPS)
        ASR_FAIL(ASR_EINVAL, "asr_reverb_fft_fwd: R=%d Lcap=%d (1 .. %d)", R, Lcap, ASR_REVERB_FFT_MAX_TAPS);
    if (out == wav) ASR_FAIL(ASR_EINVAL, "asr_reverb_fft_fwd: out must not alias wav");
    const size_t need = asr_reverb_fft_workspace_bytes(B, Smax, Lcap);
    if (ws_bytes < need) ASR_FAIL(ASR_EWORKSPACE, "asr_reverb_fft_fwd: workspace %zu < %zu bytes", ws_bytes, need);
    if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)twiddle & 7) != 0) ASR_FAIL(ASR_EINVAL, "asr_reverb_fft_fwd: workspace not 16-byte aligned (twiddle table: 8)");
    const int NW = ceil_div(Smax, BK) + 1, Pcap = ceil_div(Lcap, BK);
    cf* Xs = (cf*)ws;
    cf* Hs = Xs + (size_t)B * NW * FM;
    const cf* tw = (const cf*)twiddle;
    reverb_fft_spectra_kernel<<<dim3(NW + Pcap, B), FNT, 0, (hipStream_t)stream>>>(wav, wav_len, rir_idx, rir, rir_len, rir_peak, tw, Xs, Hs, Smax, R, Lcap, NW,
                                                                                    Pcap);
    ASR_CHECK_LAUNCH("asr_reverb_fft_fwd (spectra)");
    reverb_fft_apply_kernel<<<dim3(NW, B), FNT, 0, (hipStream_t)stream>>>(wav, wav_len, rir_idx, rir_len, rir_peak, tw, Xs, Hs, out, Smax, R, Lcap, NW, Pcap);
    ASR_CHECK_LAUNCH("asr_reverb_fft_fwd");
    return ASR_OK;
}
