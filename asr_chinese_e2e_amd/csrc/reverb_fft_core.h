// The transform of the FFT reverberation path (reverb_fft.hip), as functions of a thread index so that the same text runs as a kernel
// phase (between workgroup barriers) and as a plain host loop over the 256 threads.
//
// A real sequence of N = 4096 samples is transformed as M = N / 2 complex points z[n] = x[2n] + i x[2n + 1] followed by a Hermitian
// split: X[k] = E[k] + W_N^k O[k], E = (Z[k] + conj Z[M - k]) / 2, O = (Z[k] - conj Z[M - k]) / 2i, k = 0 .. M.  The spectrum is kept as
// M complex words: word 0 holds the two real bins (X[0], X[M]), word k the bin X[k].  The inverse undoes the split and runs the
// conjugate transform.  The M-point transform is a Stockham autosort (natural order in, natural order out, no bit reversal) of
// radices 8, 8, 8, 4: butterfly j of a pass with sub-transform length NS reads in[j + r M / R], multiplies by W_M^(r (j mod NS) M / (NS R)),
// takes a DFT of R points in registers and writes out[(j - j mod NS) R + j mod NS + r NS].  Twiddles come from a table of the N-th
// roots of unity computed in float64 and rounded once (tw[t] = exp(-2 pi i t / N)); the inverse conjugates them.
#pragma once
#ifndef RF_HD
#define RF_HD __host__ __device__ __forceinline__
#endif

namespace rfft {

typedef float cf __attribute__((ext_vector_type(2)));      // (re, im)

constexpr int N = ASR_REVERB_FFT_N, M = N / 2, BK = N / 2, NT = 256;
// LDS image of M complex words, one word of padding behind every 16: a store of 8 bytes per lane is served 16 lanes at a time over
// 32 banks of 4 bytes, so 16 lanes writing words 8 apart (the first pass: out[8 j + r]) would share two pairs of banks - padded, lane l
// writes word 8 l + (l >> 1), banks {l, l + 1} (even l) and {16 + l - 1, 16 + l} (odd l): no two lanes meet.  Reads are of consecutive words.
constexpr int LDS_WORDS = M + M / 16;
RF_HD int pad(int i) { return i + (i >> 4); }

RF_HD cf cmul(cf a, cf b) { return cf{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
template <bool INV> RF_HD cf twid(const cf* __restrict__ tw, int t) {
    cf w = tw[t];
    if (INV) w.y = -w.y;
    return w;
}
// a times -i (forward) or +i (inverse)
template <bool INV> RF_HD cf rot90(cf a) { return INV ? cf{-a.y, a.x} : cf{a.y, -a.x}; }
RF_HD void bf2(cf& a, cf& b) {
    const cf t = a;
    a = t + b;
    b = t - b;
}
template <bool INV> RF_HD void dft4(cf& v0, cf& v1, cf& v2, cf& v3) {
    bf2(v0, v2);
    bf2(v1, v3);
    v3 = rot90<INV>(v3);
    bf2(v0, v1);      // X0, X2
    bf2(v2, v3);      // X1, X3
    const cf t = v1;
    v1 = v2;
    v2 = t;
}
template <int R, bool INV> RF_HD void dft(cf (&v)[R]) {
    static_assert(R == 4 || R == 8, "radix");
    if constexpr (R == 4) {
        dft4<INV>(v[0], v[1], v[2], v[3]);
    } else {
        constexpr float h = 0.70710678118654752f;
        bf2(v[0], v[4]);
        bf2(v[1], v[5]);
        bf2(v[2], v[6]);
        bf2(v[3], v[7]);
        // the odd half times W_8^n, n = 1, 2, 3
        v[5] = INV ? cf{(v[5].x - v[5].y) * h, (v[5].x + v[5].y) * h} : cf{(v[5].x + v[5].y) * h, (v[5].y - v[5].x) * h};
        v[6] = rot90<INV>(v[6]);
        v[7] = INV ? cf{(-v[7].x - v[7].y) * h, (v[7].x - v[7].y) * h} : cf{(v[7].y - v[7].x) * h, (-v[7].x - v[7].y) * h};
        dft4<INV>(v[0], v[1], v[2], v[3]);      // X0, X2, X4, X6
        dft4<INV>(v[4], v[5], v[6], v[7]);      // X1, X3, X5, X7
        const cf e1 = v[1], e2 = v[2], e3 = v[3], o0 = v[4], o1 = v[5], o2 = v[6];
        v[1] = o0;
        v[2] = e1;
        v[3] = o1;
        v[4] = e2;
        v[5] = o2;
        v[6] = e3;
    }
}

// one butterfly of one pass; in(index) -> cf, out(index, cf)
template <int R, int NS, bool INV, class In, class Out> RF_HD void pass(int j, const cf* __restrict__ tw, In in, Out out) {
    cf v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = in(j + r * (M / R));
    const int k = j & (NS - 1);
    if (NS > 1) {
        const int ts = k * (N / (NS * R));
#pragma unroll
        for (int r = 1; r < R; ++r) v[r] = cmul(v[r], twid<INV>(tw, r * ts));
    }
    dft<R, INV>(v);
    const int j0 = (j - k) * R + k;
#pragma unroll
    for (int r = 0; r < R; ++r) out(j0 + r * NS, v[r]);
}

// passes between two padded LDS images (thread t of NT)
template <int R, int NS, bool INV> RF_HD void lds_pass(int t, const cf* __restrict__ tw, const cf* in, cf* out) {
#pragma unroll
    for (int j = t; j < M / R; j += NT)
        pass<R, NS, INV>(j, tw, [&](int i) { return in[pad(i)]; }, [&](int i, cf v) { out[pad(i)] = v; });
}

// word k of the spectrum from the M-point transform Z (padded LDS image)
RF_HD cf split_fwd(int k, const cf* Z, const cf* __restrict__ tw) {
    const cf a = Z[pad(k)];
    if (k == 0) return cf{a.x + a.y, a.x - a.y};
    const cf b = Z[pad(M - k)];
    const cf e = cf{0.5f * (a.x + b.x), 0.5f * (a.y - b.y)}, d = cf{0.5f * (a.x - b.x), 0.5f * (a.y + b.y)};
    return e + cmul(twid<false>(tw, k), cf{d.y, -d.x});
}
// input k of the inverse M-point transform from the spectrum Y (padded LDS image), scaled by 1 / M
RF_HD cf split_inv(int k, const cf* Y, const cf* __restrict__ tw) {
    constexpr float s = 1.0f / M;
    const cf a = Y[pad(k)];
    if (k == 0) return cf{0.5f * s * (a.x + a.y), 0.5f * s * (a.x - a.y)};
    const cf b = Y[pad(M - k)];
    const cf e = cf{0.5f * s * (a.x + b.x), 0.5f * s * (a.y - b.y)}, d = cf{0.5f * s * (a.x - b.x), 0.5f * s * (a.y + b.y)};
    const cf o = cmul(twid<true>(tw, k), d);
    return cf{e.x - o.y, e.y + o.x};
}

// ---- the phases; a workgroup barrier stands between two of them -----------------------------------------------------------------
// forward: sample(g) -> real sample g of the N the transform takes, g < N
template <class Sample> RF_HD void fwd_first(int t, const cf* __restrict__ tw, Sample sample, cf* A) {
    pass<8, 1, false>(t, tw, [&](int n) { return cf{sample(2 * n), sample(2 * n + 1)}; }, [&](int i, cf v) { A[pad(i)] = v; });
}
// the spectrum's words t, t + NT, ... to dst
RF_HD void fwd_store(int t, const cf* __restrict__ tw, const cf* Z, cf* __restrict__ dst) {
#pragma unroll
    for (int e = 0; e < M / NT; ++e) dst[t + e * NT] = split_fwd(t + e * NT, Z, tw);
}
// inverse: the split and the first pass, Y -> B
RF_HD void inv_first(int t, const cf* __restrict__ tw, const cf* Y, cf* B) {
    pass<8, 1, true>(t, tw, [&](int k) { return split_inv(k, Y, tw); }, [&](int i, cf v) { B[pad(i)] = v; });
}
// inverse: the last pass; put(s, value) receives real sample s of the transform's second half, s < BK
template <class Put> RF_HD void inv_last(int t, const cf* __restrict__ tw, const cf* in, Put put) {
#pragma unroll
    for (int j = t; j < M / 4; j += NT)
        pass<4, 512, true>(j, tw, [&](int i) { return in[pad(i)]; }, [&](int n, cf v) {
            if (n >= M / 2) {
                put(2 * (n - M / 2), v.x);
                put(2 * (n - M / 2) + 1, v.y);
            }
        });
}

}  // namespace rfft
