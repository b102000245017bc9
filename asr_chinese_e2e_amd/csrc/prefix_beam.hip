// The CTC prefix beam search: offline and resumable, plain, hotword-biased (ctx), with an n-gram LM (lm) and with token times (timed).
// One frame step, one offline kernel and one resumable kernel, each a template on <MODE, TIMES>; one validated host launcher per family.
#include "asr_common.h"
#include "ngram_walk.h"

// ---------------------------------------------------------------------------------------------
// CTC prefix beam search on the device (Hannun et al. 2014, algorithm 1 without a language model; the restatement the tests
// check against is oracle/decode_ref.py::ctc_prefix_beam_search).  One wave per utterance walks the frames; the prefixes of the
// beam are nodes of a trie kept in global scratch (parent, token), so "the same string" is "the same (parent node, token)".
// Per frame and beam entry l = (node, last token e, log pb, log pnb), tot = pb (+) pnb:
//     slot 0       stay:       pb' = tot + lp(blank);  pnb' = pnb + lp(e) if e is among the frame's k candidates
//     slot m >= 1  extend c:   pnb' = (c == e ? pb : tot) + lp(c)         (c = m-th candidate, blank skipped)
// An extension (node_l, c) that spells a prefix already in the beam (entry i with parent node_l and token c) is merged into that
// entry's stay slot; the beam * (k + 1) <= 64 slots are ranked (ties: lower slot first, as the stable host sort) and the best
// `beam` form the next beam in rank order; extensions that survive get a new trie node.  Log-probabilities in fp64: rankings
// must not flip against the fp64 host restatement on near ties.  Results: the n best prefixes, spelled by walking parents.
namespace {

__device__ __forceinline__ double pb_logadd(double a, double b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    const double m = a > b ? a : b;
    return m + log(exp(a - m) + exp(b - m));
}

constexpr int PB_MAX_BEAM = 16, PB_MAX_K = 32;

// The search's LDS: the beam (rank order) and one frame's slots.  s_dep = the prefix length of a beam entry (its trie node's depth).
struct PbLds {
    double pb[PB_MAX_BEAM], pnb[PB_MAX_BEAM], merge[PB_MAX_BEAM], sc[64], npb[64], npnb[64];
    int node[PB_MAX_BEAM], tok[PB_MAX_BEAM], par[PB_MAX_BEAM], dep[PB_MAX_BEAM], id[PB_MAX_K], nnode[64], ntok_[64], npar_[64], ndep_[64];
    float lp[PB_MAX_K];
};

// ---- hotword biasing (CTX instantiations only; the tables come from asr_chinese_e2e_amd/context.py::ContextGraph) --------------------
// A beam entry carries (context state, bias): a function of its prefix alone, so the entry an extension is merged into holds the same
// pair and the merge rule needs no change.  Candidates are ranked by log p + bias; pb / pnb stay pure probabilities.
struct PbCtx {
    const int32_t* __restrict__ st_off;
    const int32_t* __restrict__ arc_tok;
    const int32_t* __restrict__ arc_next;
    const double* __restrict__ st_held;
    int S, A;
    double w;
};

// the beam's (state, bias) in rank order and one frame's slots, beside PbLds
struct PbCtxLds {
    double bias[PB_MAX_BEAM], nbias[64];
    int st[PB_MAX_BEAM], nst[64];
};

// the state the arc (st, c) leads to, or -1: binary search of st's arc range (ascending tokens).  Every index is clamped to its table.
__device__ __forceinline__ int pb_ctx_find(const PbCtx& g, int st, int c) {
    int lo = min(max(g.st_off[st], 0), g.A);
    const int end = min(max(g.st_off[st + 1], lo), g.A);
    int hi = end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.arc_tok[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    if (lo < end && g.arc_tok[lo] == c) {
        const int nx = g.arc_next[lo];
        return (unsigned)nx < (unsigned)g.S ? nx : -1;
    }
    return -1;
}

// (st, bias) of a prefix -> of the prefix + c (context.py::ContextGraph.advance, the same fp64 additions in the same order).
// root < 0: the utterance is not biased, (st, bias) stays (-1, 0.0).
__device__ __forceinline__ void pb_ctx_advance(const PbCtx& g, int root, int c, int& st, double& bias) {
    if (root < 0) return;
    if ((unsigned)st >= (unsigned)g.S) st = root;    // never from a state outside the table
    int m = pb_ctx_find(g, st, c);
    if (m >= 0) { bias = bias + g.w; st = m; return; }
    bias = bias - g.st_held[st];
    st = root;
    m = pb_ctx_find(g, root, c);
    if (m >= 0) { bias = bias + g.w; st = m; }
}

// ---- n-gram LM shallow fusion (PB_LM instantiations only; the tables come from asr_chinese_e2e_amd/lm.py::NgramLM) -------------------------
// A beam entry carries (LM state, bias): the state is the longest suffix of the prefix's last order - 1 tokens that the model knows as a
// context, the bias the sum of the weighted LM log-probabilities of its tokens - both functions of the prefix alone, so merging and the
// stable prefix hold as they do for hotwords.  The tables and the walk are ngram_walk.h's.
// the beam's (LM state, bias) in rank order and one frame's slots, beside PbLds; apart from PbCtxLds, so that a later change can run both
struct PbLmLds {
    double bias[PB_MAX_BEAM], nbias[64];
    int st[PB_MAX_BEAM], nst[64];
    int nnew[PB_MAX_BEAM], nold[PB_MAX_BEAM];      // per survivor: it got a new trie node; its parent's first child before this frame
};

// (st, bias) of a prefix -> of the prefix + c (lm.py::NgramLM.advance, the same fp64 additions in the same order): the chain's terms,
// then the insertion bonus.
__device__ __forceinline__ void pb_lm_advance(const NgramLm& g, int c, int& st, double& bias) {
    st = ngram_chain(g, c, st, bias);
    bias = bias + g.ins;
}

// (state, bias) of the n best, beside pb_spell's outputs
__device__ __forceinline__ void pb_lm_report(const PbLmLds& ls, int nb, double* __restrict__ out_bias, int32_t* __restrict__ out_state, int b, int nbest) {
    const int lane = threadIdx.x;
    if (lane < nbest) {
        out_bias[b * nbest + lane] = lane < nb ? ls.bias[lane] : 0.0;
        out_state[b * nbest + lane] = lane < nb ? ls.st[lane] : -1;
    }
}

// ---- token times (TIMES instantiations only) ----------------------------------------------------------------------------------------------
// Beside pb / pnb a beam entry carries the best single alignment of its prefix that ends in blank / in non-blank: its fp64 log-probability
// (vb / vnb) and the frames of its tokens (hb / hnb), a persistent list in a second trie: node = one record {parent, depth, start, end,
// mx, mn, sm} (32 bytes with a pad word: one hop of a walk is one cache line) = the list without its last record, the list's length, the first and last frame of the last token's run and the largest,
// the smallest and the float32 sum of the token's log-posteriors over the run.  Node 0 is the empty list; a copy is the same index, `append`
// makes a node under the source list's head, `ext` (the run grows by a frame) a node beside it.  The definition the tests check against is
// tests/beam_times_ref.py.
struct alignas(8) PbTimeNode {
    int32_t par, dep, start, end;
    float mx, mn, sm;
    int32_t pad;
};
using PbTimeTrie = PbTimeNode*;

constexpr int PB_TIME_WORDS = sizeof(PbTimeNode) / 4;      // words per node of the time trie

// utterance b's time trie: the B time tries lie behind the B prefix tries (2 words per node, so 8-aligned when the workspace is)
__device__ __forceinline__ PbTimeTrie pb_time_trie(int32_t* nodes, int B, int b, size_t cap_nodes) {
    return (PbTimeNode*)(nodes + (size_t)B * 2 * cap_nodes) + (size_t)b * cap_nodes;
}

// the beam's Viterbi values and list heads in rank order, what a merged extension hands to the stay slot (next to s.merge), one frame's slots
struct PbTimesLds {
    double vb[PB_MAX_BEAM], vnb[PB_MAX_BEAM], mv[PB_MAX_BEAM], nvb[64], nvnb[64];
    int hb[PB_MAX_BEAM], hnb[PB_MAX_BEAM], mh[PB_MAX_BEAM], nhb[64], nhnb[64];
    float mlp[PB_MAX_BEAM];
};

// what a TIMES frame step takes beside the others: the LDS part, the trie, the absolute frame and the nodes in use (wave-uniform, carried across frames)
struct PbTimes {
    PbTimesLds* ts;
    PbTimeTrie tt;
    int t;
    int next;
};

// The three flavours of the one frame step: the plain search, hotword biasing, n-gram LM fusion.
constexpr int PB_PLAIN = 0, PB_CTX = 1, PB_LM = 2;

// what the PB_CTX / PB_LM kernels take beside the plain ones' arguments (nothing for PB_PLAIN)
template <int MODE> struct PbArgs {};
template <> struct PbArgs<PB_CTX> {
    PbCtx g;
    const int32_t* root;      // offline: (B) the utterance's root state, -1 = not biased; resumable: unused, the root lives in the state
    double* out_bias;         // (B, nbest) the entries' raw bias (held(state) not yet taken off)
    int32_t* out_state;       // (B, nbest) their context state (-1: no entry, or not biased)
};
template <> struct PbArgs<PB_LM> {
    NgramLm lm;
    double* out_bias;         // (B, nbest) the entries' bias (the end-of-sentence term not yet added)
    int32_t* out_state;       // (B, nbest) their LM state (-1: no entry)
};

// a root outside the table means "not biased"
__device__ __forceinline__ int pb_ctx_root(const PbCtx& g, int root) { return (root >= 0 && root < g.S) ? root : -1; }

// (state, bias) of the n best, beside pb_spell's outputs
__device__ __forceinline__ void pb_ctx_report(const PbCtxLds& cs, int nb, double* __restrict__ out_bias, int32_t* __restrict__ out_state, int b, int nbest) {
    const int lane = threadIdx.x;
    if (lane < nbest) {
        out_bias[b * nbest + lane] = lane < nb ? cs.bias[lane] : 0.0;
        out_state[b * nbest + lane] = lane < nb ? cs.st[lane] : -1;
    }
}

// The empty-prefix beam every search starts from (lane 0 writes; the caller synchronises).
__device__ __forceinline__ void pb_empty_beam(PbLds& s) {
    s.node[0] = 0; s.tok[0] = -1; s.par[0] = -1; s.dep[0] = 0; s.pb[0] = 0.0; s.pnb[0] = -INFINITY;
}

// ... and its Viterbi part: the empty alignment, probability one, ends "in blank"; both lists empty.  Node 0 of the time trie is the empty list.
__device__ __forceinline__ void pb_time_empty(PbTimesLds& ts, PbTimeTrie tt) {
    ts.vb[0] = 0.0; ts.vnb[0] = -INFINITY; ts.hb[0] = 0; ts.hnb[0] = 0;
    tt[0] = PbTimeNode{-1, 0, -1, -1, 0.0f, 0.0f, 0.0f, 0};
}

// One frame of the search: the only copy, run by the offline kernel and by the resumable one.  row_* = the frame's candidates;
// nb / next_node = beam entries / trie nodes in use (wave-uniform, carried across frames).
// PB_LM also keeps child lists in the trie (nfirst: a node's newest child, nsib: the next older child of the same parent): with an insertion
// bonus a prefix can leave the beam while a longer one stays, and come back later.  The plain search gives it a new node then, and the
// longer one - whose parent is the old node - is no longer recognised as its extension, so the same string would enter the beam twice with
// its probability split.  Here a surviving extension takes the node its (parent, token) already has, so node = string as in the definition.
// All 64 lanes call it; it ends with a barrier.  PB_PLAIN is the search without biasing (cs / g / root / ls / lm unused); PB_CTX adds the
// entries' context state and bias (cs), PB_LM their LM state and bias (ls), and both rank by log p + bias.
// TIMES (orthogonal to MODE): the entries' best single alignments ride along (tm); a kept entry whose non-blank alignment is finite gets a
// node of the time trie, so at most `beam` per frame.  Every Viterbi sum is v + (double)lp in that order.
template <int MODE, bool TIMES = false>
__device__ __forceinline__ void pb_frame_step(PbLds& s, const float* __restrict__ row_vals, const int32_t* __restrict__ row_ids, double lb, int k, int beam,
                                              int blank, int& nb, int& next_node, int32_t* npar, int32_t* ntok, PbCtxLds* cs = nullptr,
                                              const PbCtx* g = nullptr, int root = -1, PbLmLds* ls = nullptr, const NgramLm* lm = nullptr, int32_t* nfirst = nullptr,
                                              int32_t* nsib = nullptr, PbTimes* tm = nullptr) {
    constexpr bool CTX = MODE == PB_CTX, LM = MODE == PB_LM;
    const int lane = threadIdx.x, per = k + 1;
    if (lane < k) { s.id[lane] = row_ids[lane]; s.lp[lane] = row_vals[lane]; }
    if (lane < PB_MAX_BEAM) s.merge[lane] = -INFINITY;
    if constexpr (TIMES) {
        if (lane < PB_MAX_BEAM) tm->ts->mv[lane] = -INFINITY;
    }
    __syncthreads();
    const int j = lane / per, m = lane - j * per;
    bool valid = j < nb;
    double pb2 = -INFINITY, pnb2 = -INFINITY;
    int c = -1, ident_par = -1, dep = 0;
    int cst = -1;
    double cbias = 0.0;
    if constexpr (CTX) {
        if (valid) { cst = cs->st[j]; cbias = cs->bias[j]; }     // a stay slot inherits them
    }
    if constexpr (LM) {
        if (valid) { cst = ls->st[j]; cbias = ls->bias[j]; }
    }
    // TIMES: the slot's Viterbi values; its non-blank list is `tkind` of list tsrc with the frame's tlp (0: none, 1: ext, 2: append)
    [[maybe_unused]] double vb2 = -INFINITY, vnb2 = -INFINITY;
    [[maybe_unused]] int hb2 = 0, tsrc = 0, tkind = 0;
    [[maybe_unused]] float tlp = 0.0f;
    if (valid) {
        const double pb = s.pb[j], pnb = s.pnb[j], tot = pb_logadd(pb, pnb);
        const int e = s.tok[j];
        if (m == 0) {                                // stay
            pb2 = tot + lb;
            for (int q = 0; q < k; ++q)
                if (s.id[q] == e && e != blank) pnb2 = pb_logadd(pnb2, pnb + (double)s.lp[q]);
            c = e;
            ident_par = s.par[j];
            dep = s.dep[j];
            if constexpr (TIMES) {
                const double vb = tm->ts->vb[j], vnb = tm->ts->vnb[j];
                const bool nbw = vnb > vb;               // best(): the non-blank alignment only if it is strictly better
                vb2 = (nbw ? vnb : vb) + lb;
                hb2 = vb2 > -INFINITY ? (nbw ? tm->ts->hnb[j] : tm->ts->hb[j]) : 0;
                for (int q = 0; q < k; ++q)
                    if (s.id[q] == e && e != blank) {
                        const double x = vnb + (double)s.lp[q];
                        if (x > vnb2) { vnb2 = x; tsrc = tm->ts->hnb[j]; tkind = 1; tlp = s.lp[q]; }
                    }
            }
        } else {                                     // extend with the (m-1)-th candidate
            c = s.id[m - 1];
            if (c == blank) valid = false;
            else {
                pnb2 = (c == e ? pb : tot) + (double)s.lp[m - 1];
                ident_par = s.node[j];
                dep = s.dep[j] + 1;
                if constexpr (CTX) pb_ctx_advance(*g, root, c, cst, cbias);
                if constexpr (LM) pb_lm_advance(*lm, c, cst, cbias);
                if constexpr (TIMES) {
                    const double vb = tm->ts->vb[j], vnb = tm->ts->vnb[j];
                    const bool nbw = vnb > vb, rep = c == e;
                    const double x = (rep ? vb : nbw ? vnb : vb) + (double)s.lp[m - 1];
                    if (x > -INFINITY) { vnb2 = x; tsrc = (rep || !nbw) ? tm->ts->hb[j] : tm->ts->hnb[j]; tkind = 2; tlp = s.lp[m - 1]; }
                }
            }
        }
    }
    // an extension that spells a prefix of the current beam goes into that entry's stay slot
    if (valid && m > 0) {
        for (int i = 0; i < nb; ++i)
            if (s.par[i] == ident_par && s.tok[i] == c) {
                s.merge[i] = pnb2;                   // at most one extension matches an entry (parent and token are unique)
                if constexpr (TIMES) { tm->ts->mv[i] = vnb2; tm->ts->mh[i] = tsrc; tm->ts->mlp[i] = tlp; }
                valid = false;
                break;
            }
    }
    __syncthreads();
    if (valid && m == 0) pnb2 = pb_logadd(pnb2, s.merge[j]);
    if constexpr (TIMES) {
        if (valid && m == 0) {                       // the prefix's own repeat against its parent's extension: the repeat wins a tie
            const double mv = tm->ts->mv[j];
            if (mv > vnb2) { vnb2 = mv; tsrc = tm->ts->mh[j]; tkind = 2; tlp = tm->ts->mlp[j]; }
        }
    }
    double sc = valid ? pb_logadd(pb2, pnb2) : -INFINITY;
    if constexpr (CTX || LM) {
        if (sc > -INFINITY) sc = sc + cbias;         // -inf stays -inf
    }
    // a slot whose whole probability is zero cannot enter the beam (the host dictionary would hold it with -inf, ranked last)
    valid = valid && sc > -INFINITY;
    s.sc[lane] = sc;
    __syncthreads();
    int rank = 0;
    if (valid) {
        for (int o = 0; o < 64; ++o) {
            const double so = s.sc[o];
            if (so > sc || (so == sc && o < lane && so > -INFINITY)) ++rank;
        }
    }
    const bool keep = valid && rank < beam;
    const unsigned long long keep_mask = __ballot(keep);
    [[maybe_unused]] int found = -1, old_first = 0;
    if constexpr (LM) {
        if (keep && m > 0) {                         // the node this string already has, if it was in the beam before (bounded walk, inside the trie)
            old_first = nfirst[ident_par];
            int ch = old_first;
            for (int it = 0; ch > 0 && ch < next_node && it < next_node; ++it) {
                if (ntok[ch] == c) { found = ch; break; }
                ch = nsib[ch];
            }
        }
    }
    const unsigned long long ext_mask = __ballot(keep && m > 0 && found < 0);      // the survivors that need a new node
    [[maybe_unused]] unsigned long long time_mask = 0;
    if constexpr (TIMES) {
        time_mask = __ballot(keep && tkind != 0);    // ... and those that need a node of the time trie
        if (keep) {
            int hnb2 = 0;
            if (tkind != 0) {
                const PbTimeTrie tt = tm->tt;
                hnb2 = tm->next + __popcll(time_mask & ((1ull << lane) - 1ull));
                if (tkind == 2) {                    // append: a new token's run opens under the source list
                    tt[hnb2] = PbTimeNode{tsrc, dep, tm->t, tm->t, tlp, tlp, tlp, 0};
                } else {                             // ext: the last token's run grows by this frame
                    const PbTimeNode o = tt[tsrc];
                    tt[hnb2] = PbTimeNode{o.par, dep, o.start, tm->t, tlp > o.mx ? tlp : o.mx, tlp < o.mn ? tlp : o.mn, o.sm + tlp, 0};
                }
            }
            tm->ts->nvb[rank] = vb2; tm->ts->nvnb[rank] = vnb2; tm->ts->nhb[rank] = hb2; tm->ts->nhnb[rank] = hnb2;
        }
    }
    if (keep) {
        int node = m == 0 ? s.node[j] : found >= 0 ? found : next_node + __popcll(ext_mask & ((1ull << lane) - 1ull));
        if (m > 0 && found < 0) { npar[node] = ident_par; ntok[node] = c; }
        if constexpr (LM) { ls->nnew[rank] = m > 0 && found < 0; ls->nold[rank] = old_first; }
        s.nnode[rank] = node;
        s.ntok_[rank] = c;
        s.npar_[rank] = ident_par;
        s.ndep_[rank] = dep;
        s.npb[rank] = pb2;
        s.npnb[rank] = pnb2;
        if constexpr (CTX) { cs->nst[rank] = cst; cs->nbias[rank] = cbias; }
        if constexpr (LM) { ls->nst[rank] = cst; ls->nbias[rank] = cbias; }
    }
    __syncthreads();
    nb = __popcll(keep_mask);
    next_node += __popcll(ext_mask);
    if constexpr (TIMES) {
        tm->next += __popcll(time_mask);
        if (lane < nb) {
            PbTimesLds& ts = *tm->ts;
            ts.vb[lane] = ts.nvb[lane]; ts.vnb[lane] = ts.nvnb[lane]; ts.hb[lane] = ts.nhb[lane]; ts.hnb[lane] = ts.nhnb[lane];
        }
    }
    if (lane < nb) {
        s.node[lane] = s.nnode[lane]; s.tok[lane] = s.ntok_[lane]; s.par[lane] = s.npar_[lane]; s.dep[lane] = s.ndep_[lane];
        s.pb[lane] = s.npb[lane]; s.pnb[lane] = s.npnb[lane];
        if constexpr (CTX) { cs->st[lane] = cs->nst[lane]; cs->bias[lane] = cs->nbias[lane]; }
        if constexpr (LM) {
            ls->st[lane] = ls->nst[lane]; ls->bias[lane] = ls->nbias[lane];
            if (ls->nnew[lane]) {                    // link the new node in front of its parent's children; each address has one writer
                const int par = s.npar_[lane], node = s.nnode[lane];
                int prev = -1;
                bool last = true;
                for (int r = 0; r < nb; ++r)
                    if (r != lane && ls->nnew[r] && s.npar_[r] == par) {
                        if (r < lane) prev = s.nnode[r];
                        else last = false;
                    }
                nsib[node] = prev >= 0 ? prev : ls->nold[lane];
                nfirst[node] = 0;
                if (last) nfirst[par] = node;
            }
        }
    }
    __syncthreads();
}

// The beam is in rank order of its total probability: spell the n best of utterance b by walking parents.
__device__ __forceinline__ void pb_spell(const PbLds& s, int nb, const int32_t* npar, const int32_t* ntok, int32_t* __restrict__ out_tok,
                                         int32_t* __restrict__ out_len, float* __restrict__ out_score, int b, int nbest, int Lcap) {
    const int lane = threadIdx.x;
    if (lane < nbest) {
        int32_t* dst = out_tok + ((size_t)b * nbest + lane) * Lcap;
        if (lane < nb) {
            int n = 0;
            for (int nd = s.node[lane]; nd > 0; nd = npar[nd]) ++n;
            out_len[b * nbest + lane] = n;
            out_score[b * nbest + lane] = (float)pb_logadd(s.pb[lane], s.pnb[lane]);
            int pos = min(n, Lcap);
            int skip = n - pos;                          // a prefix longer than the output row keeps its first Lcap tokens
            for (int nd = s.node[lane]; nd > 0; nd = npar[nd]) {
                if (skip > 0) { --skip; continue; }
                dst[--pos] = ntok[nd];
            }
        } else {
            out_len[b * nbest + lane] = -1;              // fewer prefixes than asked for
            out_score[b * nbest + lane] = -INFINITY;
        }
    }
}

// what the TIMES kernels take beside the others' arguments (nothing without TIMES)
template <bool TIMES> struct PbTimeArgs {};
template <> struct PbTimeArgs<true> {
    double* out_vit;          // (B, nbest) the log-probability of the entry's best single alignment (-inf: no entry)
    int32_t* out_start;       // (B, nbest, Lcap) per token of the entry the first ...
    int32_t* out_end;         // ... and the last frame of its run in that alignment
    float* out_mx;            // (B, nbest, Lcap) the largest, ...
    float* out_mn;            // ... the smallest ...
    float* out_sm;            // ... and the sum of the token's log-posteriors over the run
    int32_t* out_final;       // resumable: (B) the count of final records; offline: unused
};

// The records of the n best of utterance b: the list of best(), spelled by walking parents as pb_spell walks the prefixes.  A list longer
// than the output row keeps its first Lcap records.  Every index is kept inside the trie (n_nodes in use).
__device__ __forceinline__ void pb_spell_times(const PbTimesLds& ts, const PbTimeTrie tt, int nb, int n_nodes, const PbTimeArgs<true>& o, int b, int nbest, int Lcap) {
    const int lane = threadIdx.x;
    if (lane < nbest) {
        if (lane < nb) {
            const bool nbw = ts.vnb[lane] > ts.vb[lane];
            o.out_vit[b * nbest + lane] = nbw ? ts.vnb[lane] : ts.vb[lane];
            const size_t row = ((size_t)b * nbest + lane) * Lcap;
            int nd = nbw ? ts.hnb[lane] : ts.hb[lane];
            for (int it = 0; nd > 0 && nd < n_nodes && it < n_nodes; ++it) {
                const PbTimeNode x = tt[nd];
                const int pos = x.dep - 1;
                if (pos >= 0 && pos < Lcap) {
                    o.out_start[row + pos] = x.start; o.out_end[row + pos] = x.end;
                    o.out_mx[row + pos] = x.mx; o.out_mn[row + pos] = x.mn; o.out_sm[row + pos] = x.sm;
                }
                nd = x.par;
            }
        } else {
            o.out_vit[b * nbest + lane] = -INFINITY;
        }
    }
}

template <int MODE, bool TIMES = false>
__global__ __launch_bounds__(64) void ctc_prefix_beam_kernel(const float* __restrict__ vals, const int32_t* __restrict__ ids, const float* __restrict__ blank_lp,
                                                             const int32_t* __restrict__ in_len, int32_t* nodes, int32_t* __restrict__ out_tok,
                                                             int32_t* __restrict__ out_len, float* __restrict__ out_score, int T, int k, int beam, int nbest,
                                                             int Lcap, int blank, PbArgs<MODE> cx, PbTimeArgs<TIMES> tx) {
    constexpr bool CTX = MODE == PB_CTX, LM = MODE == PB_LM;
    static_assert(!TIMES || MODE == PB_PLAIN, "the time trie lies behind the plain trie");
    __shared__ PbLds s;
    [[maybe_unused]] PbCtxLds* cs = nullptr;
    [[maybe_unused]] PbCtx g{};
    [[maybe_unused]] int root = -1;
    if constexpr (CTX) {
        __shared__ PbCtxLds cs_mem;
        cs = &cs_mem;
        g = cx.g;
    }
    [[maybe_unused]] PbLmLds* ls = nullptr;
    if constexpr (LM) {
        __shared__ PbLmLds ls_mem;
        ls = &ls_mem;
    }
    const int b = blockIdx.x, lane = threadIdx.x;
    const int cap_nodes = T * beam + 1;                  // node 0 = the empty prefix; at most `beam` new nodes per frame
    int32_t* npar = nodes + (size_t)b * (LM ? 4 : 2) * cap_nodes;   // [parent | token] per node; PB_LM: [parent | token | first child | sibling]
    int32_t* ntok = npar + cap_nodes;
    [[maybe_unused]] int32_t* nfirst = ntok + cap_nodes;
    [[maybe_unused]] int32_t* nsib = ntok + 2 * (size_t)cap_nodes;
    const int len = min(in_len ? in_len[b] : T, T);
    if (lane == 0) {
        npar[0] = -1;
        ntok[0] = -1;
        if constexpr (LM) nfirst[0] = 0;
        pb_empty_beam(s);
    }
    [[maybe_unused]] PbTimes tm{};
    if constexpr (TIMES) {                               // the time tries lie behind the B prefix tries
        __shared__ PbTimesLds ts_mem;
        tm.ts = &ts_mem;
        tm.tt = pb_time_trie(nodes, gridDim.x, b, cap_nodes);
        tm.next = 1;
        if (lane == 0) pb_time_empty(ts_mem, tm.tt);
    }
    if constexpr (CTX) {
        root = pb_ctx_root(g, cx.root[b]);
        if (lane == 0) { cs->st[0] = root; cs->bias[0] = 0.0; }
    }
    if constexpr (LM) {
        if (lane == 0) { ls->st[0] = (unsigned)cx.lm.start < (unsigned)cx.lm.S ? cx.lm.start : 0; ls->bias[0] = 0.0; }
    }
    int nb = 1, next_node = 1;                           // wave-uniform copies
    __syncthreads();
    for (int t = 0; t < len; ++t) {
        const size_t row = (size_t)b * T + t;
        if constexpr (CTX) pb_frame_step<PB_CTX>(s, vals + row * k, ids + row * k, (double)blank_lp[row], k, beam, blank, nb, next_node, npar, ntok, cs, &g, root);
        else if constexpr (LM) pb_frame_step<PB_LM>(s, vals + row * k, ids + row * k, (double)blank_lp[row], k, beam, blank, nb, next_node, npar, ntok, nullptr, nullptr, -1, ls, &cx.lm, nfirst, nsib);
        else if constexpr (TIMES) {
            tm.t = t;
            pb_frame_step<PB_PLAIN, true>(s, vals + row * k, ids + row * k, (double)blank_lp[row], k, beam, blank, nb, next_node, npar, ntok, nullptr, nullptr, -1, nullptr, nullptr, nullptr, nullptr, &tm);
        } else pb_frame_step<PB_PLAIN>(s, vals + row * k, ids + row * k, (double)blank_lp[row], k, beam, blank, nb, next_node, npar, ntok);
    }
    pb_spell(s, nb, npar, ntok, out_tok, out_len, out_score, b, nbest, Lcap);
    if constexpr (CTX) pb_ctx_report(*cs, nb, cx.out_bias, cx.out_state, b, nbest);
    if constexpr (LM) pb_lm_report(*ls, nb, cx.out_bias, cx.out_state, b, nbest);
    if constexpr (TIMES) pb_spell_times(*tm.ts, tm.tt, nb, min(tm.next, cap_nodes), tx, b, nbest, Lcap);
}

// ---- the resumable search: the beam leaves LDS between launches ------------------------------------------------------------------
// State of one utterance (asr_ctc_prefix_beam_state_bytes / B bytes, 8-aligned): int32 {nb, next_node, frames consumed, 0}, then per beam
// entry int32 node[beam], token[beam], parent[beam], depth[beam], then fp64 pb[beam], pnb[beam] - everything pb_frame_step carries from
// one frame to the next.  Trie of one utterance: int32 [parent | token] x (T_cap * beam + 1) nodes, numbered and laid out as offline; an entry's depth
// (its prefix length, for the stable prefix) travels with the entry, so the trie needs none.
constexpr int PB_STATE_HDR = 4;

__host__ __device__ inline size_t pb_state_bytes1(int beam) { return (size_t)PB_STATE_HDR * 4 + (size_t)beam * (4 * 4 + 2 * 8); }
// The context state of one utterance: the plain state, then fp64 bias[beam], int32 ctx[beam], int32 root, padded to 8 bytes.
__host__ __device__ inline size_t pb_ctx_state_bytes1(int beam) { return pb_state_bytes1(beam) + (size_t)beam * 8 + (((size_t)beam * 4 + 4 + 7) & ~(size_t)7); }

// The LM state of one utterance: the plain state, then fp64 bias[beam], int32 st[beam], padded to 8 bytes.
__host__ __device__ inline size_t pb_lm_state_bytes1(int beam) { return pb_state_bytes1(beam) + (size_t)beam * 8 + (((size_t)beam * 4 + 7) & ~(size_t)7); }

// The timed state of one utterance: the plain state, then fp64 vb[beam], vnb[beam], int32 hb[beam], hnb[beam], the time trie's nodes in use, padded to 8 bytes.
__host__ __device__ inline size_t pb_time_state_bytes1(int beam) { return pb_state_bytes1(beam) + (size_t)beam * 16 + (((size_t)beam * 8 + 4 + 7) & ~(size_t)7); }

// The empty-prefix state of utterance b and its trie's root: what the init kernel leaves for every utterance and the reset kernel for the flagged ones.
// bytes1: the bytes of one utterance's state (pb_state_bytes1, or pb_ctx_state_bytes1 / pb_lm_state_bytes1 when a context / LM part follows).
__device__ __forceinline__ void pb_state_init_one(char* state, int32_t* nodes, int b, int beam, int T_cap, size_t bytes1, int narr = 2) {
    const size_t cap_nodes = (size_t)T_cap * beam + 1;
    int32_t* hdr = (int32_t*)(state + (size_t)b * bytes1);
    int32_t* ent = hdr + PB_STATE_HDR;
    double* sc = (double*)(ent + 4 * beam);
    hdr[0] = 1; hdr[1] = 1; hdr[2] = 0; hdr[3] = 0;
    for (int i = 0; i < beam; ++i) {
        ent[i] = 0; ent[beam + i] = -1; ent[2 * beam + i] = -1; ent[3 * beam + i] = 0;
        sc[i] = i == 0 ? 0.0 : -INFINITY; sc[beam + i] = -INFINITY;
    }
    int32_t* npar = nodes + (size_t)b * narr * cap_nodes;      // narr = 4: the LM trie, whose root has no child yet
    npar[0] = -1; npar[cap_nodes] = -1;
    if (narr == 4) npar[2 * cap_nodes] = 0;
}

__global__ __launch_bounds__(64) void ctc_prefix_beam_state_init_kernel(char* state, int32_t* nodes, int B, int beam, int T_cap) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    pb_state_init_one(state, nodes, b, beam, T_cap, pb_state_bytes1(beam));
}

// only the utterances with flags[b] != 0 (independent sessions: a slot that is reopened); the others keep every byte
__global__ __launch_bounds__(64) void ctc_prefix_beam_state_reset_kernel(char* state, int32_t* nodes, const int32_t* __restrict__ flags, int B, int beam, int T_cap) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B || flags[b] == 0) return;
    pb_state_init_one(state, nodes, b, beam, T_cap, pb_state_bytes1(beam));
}

// the context part of utterance b's state: every entry on the root with no bias, the root, a zero pad word
__device__ __forceinline__ void pb_ctx_state_init_one(char* state, int b, int beam, int root) {
    char* base = state + (size_t)b * pb_ctx_state_bytes1(beam) + pb_state_bytes1(beam);
    double* bias = (double*)base;
    int32_t* ctx = (int32_t*)(base + (size_t)beam * 8);
    for (int i = 0; i < beam; ++i) { bias[i] = 0.0; ctx[i] = root; }
    ctx[beam] = root;
    if ((beam & 1) == 0) ctx[beam + 1] = 0;
}

// flags == nullptr: every utterance (init); otherwise the flagged ones (reset), each with its new root
__global__ __launch_bounds__(64) void ctc_prefix_beam_ctx_state_init_kernel(char* state, int32_t* nodes, const int32_t* __restrict__ flags,
                                                                            const int32_t* __restrict__ root, int B, int beam, int T_cap) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B || (flags && flags[b] == 0)) return;
    pb_state_init_one(state, nodes, b, beam, T_cap, pb_ctx_state_bytes1(beam));
    pb_ctx_state_init_one(state, b, beam, max(root[b], -1));
}

// the LM part of utterance b's state: every entry on the start state with no bias, a zero pad word
// flags == nullptr: every utterance (init); otherwise the flagged ones (reset)
__global__ __launch_bounds__(64) void ctc_prefix_beam_lm_state_init_kernel(char* state, int32_t* nodes, const int32_t* __restrict__ flags, int start, int B,
                                                                           int beam, int T_cap) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B || (flags && flags[b] == 0)) return;
    pb_state_init_one(state, nodes, b, beam, T_cap, pb_lm_state_bytes1(beam), 4);
    char* base = state + (size_t)b * pb_lm_state_bytes1(beam) + pb_state_bytes1(beam);
    double* bias = (double*)base;
    int32_t* st = (int32_t*)(base + (size_t)beam * 8);
    for (int i = 0; i < beam; ++i) { bias[i] = 0.0; st[i] = start; }
    if (beam & 1) st[beam] = 0;
}

// the Viterbi part of utterance b's timed state and the root of its time trie (behind the B prefix tries)
// flags == nullptr: every utterance (init); otherwise the flagged ones (reset)
__global__ __launch_bounds__(64) void ctc_prefix_beam_timed_state_init_kernel(char* state, int32_t* nodes, const int32_t* __restrict__ flags, int B, int beam, int T_cap) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B || (flags && flags[b] == 0)) return;
    pb_state_init_one(state, nodes, b, beam, T_cap, pb_time_state_bytes1(beam));
    const size_t cap_nodes = (size_t)T_cap * beam + 1;
    double* v = (double*)(state + (size_t)b * pb_time_state_bytes1(beam) + pb_state_bytes1(beam));
    int32_t* h = (int32_t*)(v + 2 * beam);
    for (int i = 0; i < beam; ++i) { v[i] = i == 0 ? 0.0 : -INFINITY; v[beam + i] = -INFINITY; h[i] = 0; h[beam + i] = 0; }
    h[2 * beam] = 1;
    h[2 * beam + 1] = 0;
    pb_time_trie(nodes, B, b, cap_nodes)[0] = PbTimeNode{-1, 0, -1, -1, 0.0f, 0.0f, 0.0f, 0};
}

template <int MODE, bool TIMES = false>
__global__ __launch_bounds__(64) void ctc_prefix_beam_chunk_kernel(const float* __restrict__ vals, const int32_t* __restrict__ ids, const float* __restrict__ blank_lp,
                                                                   const int32_t* __restrict__ n_valid, char* state, int32_t* nodes, int32_t* __restrict__ out_tok,
                                                                   int32_t* __restrict__ out_len, float* __restrict__ out_score, int32_t* __restrict__ out_stable,
                                                                   int C, int k, int beam, int nbest, int Lcap, int T_cap, int blank, PbArgs<MODE> cx, PbTimeArgs<TIMES> tx) {
    constexpr bool CTX = MODE == PB_CTX, LM = MODE == PB_LM;
    static_assert(!TIMES || MODE == PB_PLAIN, "the time trie lies behind the plain trie");
    __shared__ PbLds s;
    __shared__ int s_walk[TIMES ? 2 * PB_MAX_BEAM : PB_MAX_BEAM];
    [[maybe_unused]] PbCtxLds* cs = nullptr;
    [[maybe_unused]] PbCtx g{};
    if constexpr (CTX) {
        __shared__ PbCtxLds cs_mem;
        cs = &cs_mem;
        g = cx.g;
    }
    [[maybe_unused]] PbLmLds* ls = nullptr;
    if constexpr (LM) {
        __shared__ PbLmLds ls_mem;
        ls = &ls_mem;
    }
    const int b = blockIdx.x, lane = threadIdx.x;
    const int cap_nodes = T_cap * beam + 1;
    int32_t* npar = nodes + (size_t)b * (LM ? 4 : 2) * cap_nodes;   // [parent | token] per node; PB_LM: [parent | token | first child | sibling]
    int32_t* ntok = npar + cap_nodes;
    [[maybe_unused]] int32_t* nfirst = ntok + cap_nodes;
    [[maybe_unused]] int32_t* nsib = ntok + 2 * (size_t)cap_nodes;
    int32_t* hdr = (int32_t*)(state + (size_t)b * (CTX ? pb_ctx_state_bytes1(beam) : LM ? pb_lm_state_bytes1(beam) : TIMES ? pb_time_state_bytes1(beam) : pb_state_bytes1(beam)));
    int32_t* ent = hdr + PB_STATE_HDR;
    double* sc = (double*)(ent + 4 * beam);
    int nb = min(max(hdr[0], 0), beam), next_node = hdr[1];      // wave-uniform copies
    const int frames = hdr[2];
    if (lane < nb) {
        s.node[lane] = ent[lane]; s.tok[lane] = ent[beam + lane]; s.par[lane] = ent[2 * beam + lane]; s.dep[lane] = ent[3 * beam + lane];
        s.pb[lane] = sc[lane]; s.pnb[lane] = sc[beam + lane];
    }
    [[maybe_unused]] double* st_bias = sc + 2 * beam;            // the context / LM part of the state (PB_CTX: bias, ctx, root; PB_LM: bias, st)
    [[maybe_unused]] int32_t* st_ctx = (int32_t*)(st_bias + beam);
    [[maybe_unused]] int root = -1;
    if constexpr (CTX) {
        root = pb_ctx_root(g, st_ctx[beam]);
        if (lane < nb) { cs->st[lane] = root < 0 ? -1 : st_ctx[lane]; cs->bias[lane] = st_bias[lane]; }
    }
    if constexpr (LM) {
        if (lane < nb) { ls->st[lane] = st_ctx[lane]; ls->bias[lane] = st_bias[lane]; }
    }
    [[maybe_unused]] PbTimes tm{};
    [[maybe_unused]] double* st_v = sc + 2 * beam;               // the Viterbi part of a timed state: vb, vnb, then hb, hnb, the time trie's nodes in use
    [[maybe_unused]] int32_t* st_h = (int32_t*)(st_v + 2 * beam);
    if constexpr (TIMES) {
        __shared__ PbTimesLds ts_mem;
        tm.ts = &ts_mem;
        tm.tt = pb_time_trie(nodes, gridDim.x, b, cap_nodes);
        tm.next = st_h[2 * beam];
        if (lane < nb) {                                         // a list head outside the trie reads as the empty list
            ts_mem.vb[lane] = st_v[lane]; ts_mem.vnb[lane] = st_v[beam + lane];
            const int hb = st_h[lane], hnb = st_h[beam + lane];
            ts_mem.hb[lane] = (hb > 0 && hb < min(tm.next, cap_nodes)) ? hb : 0;
            ts_mem.hnb[lane] = (hnb > 0 && hnb < min(tm.next, cap_nodes)) ? hnb : 0;
        }
    }
    __syncthreads();
    // never past the trie: at most T_cap frames in all (the wrapper refuses such a push; this keeps every write inside the workspace)
    const int n = max(0, min(min(n_valid[b], C), T_cap - frames));
    int done = 0;
    for (int t = 0; t < n; ++t) {
        if (next_node < 1 || next_node + beam > cap_nodes) break;
        if constexpr (TIMES) {
            if (tm.next < 1 || tm.next + beam > cap_nodes) break;
        }
        const size_t row = (size_t)b * C + t;
        if constexpr (CTX) pb_frame_step<PB_CTX>(s, vals + row * k, ids + row * k, (double)blank_lp[row], k, beam, blank, nb, next_node, npar, ntok, cs, &g, root);
        else if constexpr (LM) pb_frame_step<PB_LM>(s, vals + row * k, ids + row * k, (double)blank_lp[row], k, beam, blank, nb, next_node, npar, ntok, nullptr, nullptr, -1, ls, &cx.lm, nfirst, nsib);
        else if constexpr (TIMES) {
            tm.t = frames + t;
            pb_frame_step<PB_PLAIN, true>(s, vals + row * k, ids + row * k, (double)blank_lp[row], k, beam, blank, nb, next_node, npar, ntok, nullptr, nullptr, -1, nullptr, nullptr, nullptr, nullptr, &tm);
        } else pb_frame_step<PB_PLAIN>(s, vals + row * k, ids + row * k, (double)blank_lp[row], k, beam, blank, nb, next_node, npar, ntok);
        ++done;
    }
    if (done > 0) {                                      // a chunk without frames leaves every byte of the state as it is
        if (lane == 0) { hdr[0] = nb; hdr[1] = next_node; hdr[2] = frames + done; }
        if (lane < nb) {
            ent[lane] = s.node[lane]; ent[beam + lane] = s.tok[lane]; ent[2 * beam + lane] = s.par[lane]; ent[3 * beam + lane] = s.dep[lane];
            sc[lane] = s.pb[lane]; sc[beam + lane] = s.pnb[lane];
            if constexpr (CTX) { st_ctx[lane] = cs->st[lane]; st_bias[lane] = cs->bias[lane]; }
            if constexpr (LM) { st_ctx[lane] = ls->st[lane]; st_bias[lane] = ls->bias[lane]; }
            if constexpr (TIMES) { st_v[lane] = tm.ts->vb[lane]; st_v[beam + lane] = tm.ts->vnb[lane]; st_h[lane] = tm.ts->hb[lane]; st_h[beam + lane] = tm.ts->hnb[lane]; }
        }
        if constexpr (TIMES) {
            if (lane == 0) st_h[2 * beam] = tm.next;
        }
    }
    pb_spell(s, nb, npar, ntok, out_tok, out_len, out_score, b, nbest, Lcap);
    if constexpr (CTX) pb_ctx_report(*cs, nb, cx.out_bias, cx.out_state, b, nbest);
    if constexpr (LM) pb_lm_report(*ls, nb, cx.out_bias, cx.out_state, b, nbest);
    if constexpr (TIMES) pb_spell_times(*tm.ts, tm.tt, nb, min(tm.next, cap_nodes), tx, b, nbest, Lcap);
    // the stable prefix: the depth of the lowest common ancestor of the beam's nodes.  Every entry first climbs to the smallest depth
    // among them, then all climb together until they stand on one node.
    int mind = INT_MAX;
    for (int i = 0; i < nb; ++i) mind = min(mind, s.dep[i]);
    int nd = lane < nb ? s.node[lane] : 0, d = lane < nb ? s.dep[lane] : 0;
    while (d > mind && nd > 0) { nd = npar[nd]; --d; }
    for (;;) {
        if (lane < nb) s_walk[lane] = nd;
        __syncthreads();
        bool same = true;
        for (int i = 1; i < nb; ++i) same = same && s_walk[i] == s_walk[0];
        __syncthreads();
        if (same || mind <= 0) break;                    // wave-uniform
        if (lane < nb && nd > 0) nd = npar[nd];
        --mind;
    }
    if (lane == 0) out_stable[b] = nb > 0 ? mind : 0;
    if constexpr (TIMES) {
        // the final records: the depth of the lowest common ancestor of S = the lists without their last record, over every non-empty list
        // of a finite alignment (two walkers per entry, lane = 2 * entry + (0: hb, 1: hnb)).  An empty list among them: nothing is final.
        // A list of entry i has dep[i] records, so its parent stands at depth dep[i] - 1; the walk is the stable prefix's.
        __syncthreads();                                 // s_walk is free again
        const PbTimesLds& ts = *tm.ts;
        const int n_nodes = min(tm.next, cap_nodes), e = lane >> 1;
        const bool live = lane < 2 * nb && ((lane & 1) ? ts.vnb[e] : ts.vb[e]) > -INFINITY;
        const int head = live ? ((lane & 1) ? ts.hnb[e] : ts.hb[e]) : 0;
        const unsigned long long live_mask = __ballot(live), empty_mask = __ballot(live && head <= 0);
        int fin = 0;
        if (live_mask != 0 && empty_mask == 0) {         // wave-uniform
            int w = tm.tt[head < n_nodes ? head : 0].par, wd = live ? s.dep[e] - 1 : INT_MAX;
            if (!live || w < 0) w = 0;
            fin = wd;
            for (int o = 32; o > 0; o >>= 1) fin = min(fin, __shfl_xor(fin, o));
            fin = max(fin, 0);
            while (live && wd > fin && w > 0 && w < n_nodes) { w = tm.tt[w].par; --wd; }
            for (;;) {
                if (lane < 2 * PB_MAX_BEAM) s_walk[lane] = live ? w : -1;
                __syncthreads();
                int first = -1;
                bool same = true;
                for (int i = 0; i < 2 * nb; ++i) {
                    const int x = s_walk[i];
                    if (x < 0) continue;
                    if (first < 0) first = x;
                    same = same && x == first;
                }
                __syncthreads();
                if (same || fin <= 0) break;             // wave-uniform
                if (live && w > 0 && w < n_nodes) w = tm.tt[w].par;
                --fin;
            }
        }
        if (lane == 0) tx.out_final[b] = fin;
    }
}

}  // namespace

// ---- the host side: one validated launcher per family (offline search, resumable chunk, state init / reset) ------------------------------
// The extern "C" entry points below only build their mode's PbArgs / PbTimeArgs and call their family's launcher; what differs between the
// modes on the host is in PbHost, pb_args_check and the `if constexpr` of pb_state_launch.
namespace {

template <int MODE, bool TIMES>
struct PbHost {
    // int32 words per trie node: [parent | token], PB_LM: [parent | token | first child | sibling], TIMES: the time trie's record behind the prefix trie's
    static constexpr int node_words = TIMES ? 2 + PB_TIME_WORDS : MODE == PB_LM ? 4 : 2;
    static constexpr int ws_align = TIMES ? 8 : 4;      // PbTimeNode is read and written whole
    static size_t state_bytes1(int beam) {
        return TIMES ? pb_time_state_bytes1(beam) : MODE == PB_CTX ? pb_ctx_state_bytes1(beam) : MODE == PB_LM ? pb_lm_state_bytes1(beam) : pb_state_bytes1(beam);
    }
    // the B tries of `frames` frames each (offline: T, resumable: T_cap)
    static size_t workspace_bytes(int B, int frames, int beam) {
        if (B <= 0 || frames <= 0 || beam <= 0) return 0;
        return (size_t)B * node_words * ((size_t)frames * beam + 1) * sizeof(int32_t);
    }
    static size_t state_bytes(int B, int beam) {
        if (B <= 0 || beam <= 0) return 0;
        return (size_t)B * state_bytes1(beam);
    }
};

PbCtx pb_ctx_of(const asr_context_graph* ctx) { return ctx ? PbCtx{ctx->st_off, ctx->arc_tok, ctx->arc_next, ctx->st_held, ctx->S, ctx->A, ctx->w} : PbCtx{}; }

// a null graph / LM struct arrives as all-null tables
const char* pb_ctx_check(const PbCtx& g) {
    if (!g.st_off || !g.arc_tok || !g.arc_next || !g.st_held) return "null context table";
    if (g.S < 1 || g.A < 0) return "a context graph has S >= 1 states and A >= 0 arcs";
    if ((((uintptr_t)g.st_off | (uintptr_t)g.arc_tok | (uintptr_t)g.arc_next) % 4) || ((uintptr_t)g.st_held % 8))
        return "misaligned context table (int32 tables: 4 bytes, st_held: 8)";
    if (!(g.w == g.w) || g.w - g.w != 0.0) return "the context score w must be finite";
    return nullptr;
}
const char* pb_bias_out_check(const double* out_bias, const int32_t* out_state) {
    if (!out_bias || !out_state) return "null pointer";
    if (((uintptr_t)out_bias % 8) || ((uintptr_t)out_state % 4)) return "misaligned pointer (out_bias: 8 bytes, out_state: 4)";
    return nullptr;
}

// the mode's tables and extra outputs (the offline ctx search's root: pb_search_launch)
const char* pb_args_check(const PbArgs<PB_PLAIN>&) { return nullptr; }
const char* pb_args_check(const PbArgs<PB_CTX>& cx) {
    const char* why = pb_ctx_check(cx.g);
    return why ? why : pb_bias_out_check(cx.out_bias, cx.out_state);
}
const char* pb_args_check(const PbArgs<PB_LM>& cx) {
    const char* why = ngram_lm_check(cx.lm);
    return why ? why : pb_bias_out_check(cx.out_bias, cx.out_state);
}
// ... and the time outputs (the resumable search's out_final: pb_chunk_launch)
const char* pb_time_out_check(const PbTimeArgs<false>&) { return nullptr; }
const char* pb_time_out_check(const PbTimeArgs<true>& tx) {
    if (!tx.out_vit || !tx.out_start || !tx.out_end || !tx.out_mx || !tx.out_mn || !tx.out_sm) return "null pointer";
    if (((uintptr_t)tx.out_vit % 8) || (((uintptr_t)tx.out_start | (uintptr_t)tx.out_end | (uintptr_t)tx.out_mx | (uintptr_t)tx.out_mn | (uintptr_t)tx.out_sm) % 4))
        return "misaligned pointer (out_vit: 8 bytes, the other time outputs: 4)";
    return nullptr;
}

// What both searches check alike, after their own shapes and pointers; `frames` = the trie's capacity (offline: T, resumable: T_cap).
// The workspace comes last: everything before it is ASR_EINVAL.
template <int MODE, bool TIMES>
int pb_check(const char* what, const float* vals, const int32_t* ids, const float* blank_lp, const void* ws, size_t ws_bytes, const int32_t* out_tok,
             const int32_t* out_len, const float* out_score, int B, int frames, int k, int beam, int nbest, const PbArgs<MODE>& cx, const PbTimeArgs<TIMES>& tx) {
    if (!vals || !ids || !blank_lp || !ws || !out_tok || !out_len || !out_score) ASR_FAIL(ASR_EINVAL, "%s: null pointer", what);
    if (const char* why = pb_args_check(cx)) ASR_FAIL(ASR_EINVAL, "%s: %s", what, why);
    if (const char* why = pb_time_out_check(tx)) ASR_FAIL(ASR_EINVAL, "%s: %s", what, why);
    if (beam > PB_MAX_BEAM || k > PB_MAX_K || beam * (k + 1) > 64 || nbest > beam)
        ASR_FAIL(ASR_EINVAL, "%s: one wave ranks the beam * (k + 1) candidates of a frame: beam * (k + 1) <= 64, beam <= %d, nbest <= beam (beam=%d k=%d nbest=%d)", what, PB_MAX_BEAM, beam, k, nbest);
    if ((size_t)frames * beam + 1 > (size_t)INT_MAX) ASR_FAIL(ASR_EINVAL, "%s: %d * beam + 1 nodes do not fit an int32 (beam=%d)", what, frames, beam);
    if (((uintptr_t)vals | (uintptr_t)ids | (uintptr_t)blank_lp | (uintptr_t)out_tok | (uintptr_t)out_len | (uintptr_t)out_score) % 4)
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (inputs and outputs: 4 bytes)", what);
    const size_t need = PbHost<MODE, TIMES>::workspace_bytes(B, frames, beam);
    if (ws_bytes < need || ((uintptr_t)ws % PbHost<MODE, TIMES>::ws_align)) ASR_FAIL(ASR_EWORKSPACE, "%s: workspace of %zu bytes needed (got %zu)", what, need, ws_bytes);
    return ASR_OK;
}

// the offline search; in_len == nullptr: every utterance has T frames
template <int MODE, bool TIMES>
int pb_search_launch(const char* what, const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, void* ws, size_t ws_bytes,
                     int32_t* out_tok, int32_t* out_len, float* out_score, int B, int T, int k, int beam, int nbest, int Lcap, int blank, void* stream,
                     const PbArgs<MODE>& cx, const PbTimeArgs<TIMES>& tx) {
    if (B <= 0 || T <= 0 || k <= 0 || beam <= 0 || nbest <= 0 || Lcap <= 0) ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d T=%d k=%d beam=%d nbest=%d Lcap=%d", what, B, T, k, beam, nbest, Lcap);
    if ((uintptr_t)in_len % 4) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (in_len: 4 bytes)", what);
    if constexpr (MODE == PB_CTX) {
        if (!cx.root) ASR_FAIL(ASR_EINVAL, "%s: null pointer", what);
        if ((uintptr_t)cx.root % 4) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (root: 4 bytes)", what);
    }
    if (int rc = pb_check<MODE, TIMES>(what, vals, ids, blank_lp, ws, ws_bytes, out_tok, out_len, out_score, B, T, k, beam, nbest, cx, tx)) return rc;
    ctc_prefix_beam_kernel<MODE, TIMES><<<B, 64, 0, (hipStream_t)stream>>>(vals, ids, blank_lp, in_len, (int32_t*)ws, out_tok, out_len, out_score, T, k, beam, nbest, Lcap, blank, cx, tx);
    ASR_CHECK_LAUNCH(what);
    return ASR_OK;
}

// one chunk of the resumable search
template <int MODE, bool TIMES>
int pb_chunk_launch(const char* what, const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                    size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score, int32_t* out_stable, int B, int C, int k, int beam, int nbest, int Lcap,
                    int T_cap, int blank, void* stream, const PbArgs<MODE>& cx, const PbTimeArgs<TIMES>& tx) {
    if (B <= 0 || C < 1 || T_cap < 1 || k <= 0 || beam <= 0 || nbest <= 0 || Lcap <= 0)
        ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d C=%d T_cap=%d k=%d beam=%d nbest=%d Lcap=%d", what, B, C, T_cap, k, beam, nbest, Lcap);
    if (!n_valid || !state || !out_stable) ASR_FAIL(ASR_EINVAL, "%s: null pointer", what);
    if (((uintptr_t)state % 8) || (((uintptr_t)n_valid | (uintptr_t)out_stable) % 4)) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (state: 8 bytes, the others: 4)", what);
    if constexpr (TIMES) {
        if (!tx.out_final) ASR_FAIL(ASR_EINVAL, "%s: null pointer", what);
        if ((uintptr_t)tx.out_final % 4) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (out_final: 4 bytes)", what);
    }
    if (int rc = pb_check<MODE, TIMES>(what, vals, ids, blank_lp, ws, ws_bytes, out_tok, out_len, out_score, B, T_cap, k, beam, nbest, cx, tx)) return rc;
    ctc_prefix_beam_chunk_kernel<MODE, TIMES><<<B, 64, 0, (hipStream_t)stream>>>(vals, ids, blank_lp, n_valid, (char*)state, (int32_t*)ws, out_tok, out_len, out_score,
                                                                                out_stable, C, k, beam, nbest, Lcap, T_cap, blank, cx, tx);
    ASR_CHECK_LAUNCH(what);
    return ASR_OK;
}

// The empty-prefix state of every utterance (flags == nullptr: init) or of the flagged ones (reset).  cx: the ctx state's roots, the LM
// state's LM (its start state); the outputs of cx are unused.
template <int MODE, bool TIMES>
int pb_state_launch(const char* what, void* state, void* ws, const int32_t* flags, int B, int beam, int T_cap, void* stream, const PbArgs<MODE>& cx) {
    if (!state || !ws) ASR_FAIL(ASR_EINVAL, "%s: null pointer", what);
    if constexpr (MODE == PB_CTX) {
        if (!cx.root) ASR_FAIL(ASR_EINVAL, "%s: null pointer", what);
        if ((uintptr_t)cx.root % 4) ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (root: 4 bytes)", what);
    }
    if constexpr (MODE == PB_LM) {
        if (const char* why = ngram_lm_check(cx.lm)) ASR_FAIL(ASR_EINVAL, "%s: %s", what, why);
    }
    if (B <= 0 || beam <= 0 || beam > PB_MAX_BEAM || T_cap <= 0 || (size_t)T_cap * beam + 1 > (size_t)INT_MAX)
        ASR_FAIL(ASR_EINVAL, "%s: bad shape B=%d beam=%d (<= %d) T_cap=%d", what, B, beam, PB_MAX_BEAM, T_cap);
    if (((uintptr_t)state % 8) || ((uintptr_t)ws % PbHost<MODE, TIMES>::ws_align) || ((uintptr_t)flags % 4))
        ASR_FAIL(ASR_EINVAL, "%s: misaligned pointer (state: 8 bytes, workspace: %d, flags: 4)", what, PbHost<MODE, TIMES>::ws_align);
    const dim3 grid(ceil_div(B, 64));
    const hipStream_t st = (hipStream_t)stream;
    if constexpr (TIMES) ctc_prefix_beam_timed_state_init_kernel<<<grid, 64, 0, st>>>((char*)state, (int32_t*)ws, flags, B, beam, T_cap);
    else if constexpr (MODE == PB_CTX) ctc_prefix_beam_ctx_state_init_kernel<<<grid, 64, 0, st>>>((char*)state, (int32_t*)ws, flags, cx.root, B, beam, T_cap);
    else if constexpr (MODE == PB_LM) ctc_prefix_beam_lm_state_init_kernel<<<grid, 64, 0, st>>>((char*)state, (int32_t*)ws, flags, cx.lm.start, B, beam, T_cap);
    else if (flags) ctc_prefix_beam_state_reset_kernel<<<grid, 64, 0, st>>>((char*)state, (int32_t*)ws, flags, B, beam, T_cap);
    else ctc_prefix_beam_state_init_kernel<<<grid, 64, 0, st>>>((char*)state, (int32_t*)ws, B, beam, T_cap);
    ASR_CHECK_LAUNCH(what);
    return ASR_OK;
}

}  // namespace

// ---- the plain search ---------------------------------------------------------------------------------------------------------------------
extern "C" size_t asr_ctc_prefix_beam_workspace_bytes(int B, int T, int beam) { return PbHost<PB_PLAIN, false>::workspace_bytes(B, T, beam); }
extern "C" size_t asr_ctc_prefix_beam_stream_workspace_bytes(int B, int T_cap, int beam) { return PbHost<PB_PLAIN, false>::workspace_bytes(B, T_cap, beam); }
extern "C" size_t asr_ctc_prefix_beam_state_bytes(int B, int beam) { return PbHost<PB_PLAIN, false>::state_bytes(B, beam); }

extern "C" int asr_ctc_prefix_beam(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, void* ws, size_t ws_bytes,
                                   int32_t* out_tok, int32_t* out_len, float* out_score, int B, int T, int k, int beam, int nbest, int Lcap, int blank,
                                   void* stream) {
    return pb_search_launch<PB_PLAIN, false>("asr_ctc_prefix_beam", vals, ids, blank_lp, in_len, ws, ws_bytes, out_tok, out_len, out_score, B, T, k, beam, nbest, Lcap,
                                             blank, stream, {}, {});
}

extern "C" int asr_ctc_prefix_beam_state_init(void* state, void* ws, int B, int beam, int T_cap, void* stream) {
    return pb_state_launch<PB_PLAIN, false>("asr_ctc_prefix_beam_state_init", state, ws, nullptr, B, beam, T_cap, stream, {});
}

extern "C" int asr_ctc_prefix_beam_state_reset(void* state, void* ws, const int32_t* flags, int B, int beam, int T_cap, void* stream) {
    if (!flags) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_beam_state_reset: null pointer");      // without flags it would be an init
    return pb_state_launch<PB_PLAIN, false>("asr_ctc_prefix_beam_state_reset", state, ws, flags, B, beam, T_cap, stream, {});
}

extern "C" int asr_ctc_prefix_beam_chunk(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                                         size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score, int32_t* out_stable, int B, int C, int k,
                                         int beam, int nbest, int Lcap, int T_cap, int blank, void* stream) {
    return pb_chunk_launch<PB_PLAIN, false>("asr_ctc_prefix_beam_chunk", vals, ids, blank_lp, n_valid, state, ws, ws_bytes, out_tok, out_len, out_score, out_stable, B, C, k,
                                            beam, nbest, Lcap, T_cap, blank, stream, {}, {});
}

// ---- hotword biasing: the same searches with a context graph (additive to ABI 10); the tries are the plain ones --------------------------
extern "C" size_t asr_ctc_prefix_beam_ctx_state_bytes(int B, int beam) { return PbHost<PB_CTX, false>::state_bytes(B, beam); }

extern "C" int asr_ctc_prefix_beam_ctx(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, const int32_t* root,
                                       const asr_context_graph* ctx, void* ws, size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score,
                                       double* out_bias, int32_t* out_state, int B, int T, int k, int beam, int nbest, int Lcap, int blank, void* stream) {
    return pb_search_launch<PB_CTX, false>("asr_ctc_prefix_beam_ctx", vals, ids, blank_lp, in_len, ws, ws_bytes, out_tok, out_len, out_score, B, T, k, beam, nbest, Lcap,
                                           blank, stream, {pb_ctx_of(ctx), root, out_bias, out_state}, {});
}

extern "C" int asr_ctc_prefix_beam_ctx_state_init(void* state, void* ws, const int32_t* root, int B, int beam, int T_cap, void* stream) {
    return pb_state_launch<PB_CTX, false>("asr_ctc_prefix_beam_ctx_state_init", state, ws, nullptr, B, beam, T_cap, stream, {PbCtx{}, root, nullptr, nullptr});
}

extern "C" int asr_ctc_prefix_beam_ctx_state_reset(void* state, void* ws, const int32_t* flags, const int32_t* root, int B, int beam, int T_cap, void* stream) {
    if (!flags) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_beam_ctx_state_reset: null pointer");      // without flags it would be an init
    return pb_state_launch<PB_CTX, false>("asr_ctc_prefix_beam_ctx_state_reset", state, ws, flags, B, beam, T_cap, stream, {PbCtx{}, root, nullptr, nullptr});
}

extern "C" int asr_ctc_prefix_beam_chunk_ctx(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                                             size_t ws_bytes, const asr_context_graph* ctx, int32_t* out_tok, int32_t* out_len, float* out_score,
                                             double* out_bias, int32_t* out_state, int32_t* out_stable, int B, int C, int k, int beam, int nbest, int Lcap,
                                             int T_cap, int blank, void* stream) {
    return pb_chunk_launch<PB_CTX, false>("asr_ctc_prefix_beam_chunk_ctx", vals, ids, blank_lp, n_valid, state, ws, ws_bytes, out_tok, out_len, out_score, out_stable, B, C,
                                          k, beam, nbest, Lcap, T_cap, blank, stream, {pb_ctx_of(ctx), nullptr, out_bias, out_state}, {});
}

// ---- n-gram LM shallow fusion: the same searches with an LM (additive to ABI 10) ------------------------------------------------------
extern "C" size_t asr_ctc_prefix_beam_lm_workspace_bytes(int B, int T, int beam) { return PbHost<PB_LM, false>::workspace_bytes(B, T, beam); }
extern "C" size_t asr_ctc_prefix_beam_lm_state_bytes(int B, int beam) { return PbHost<PB_LM, false>::state_bytes(B, beam); }

extern "C" int asr_ctc_prefix_beam_lm(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, const asr_ngram_lm* lm, void* ws,
                                      size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score, double* out_bias, int32_t* out_state, int B,
                                      int T, int k, int beam, int nbest, int Lcap, int blank, void* stream) {
    return pb_search_launch<PB_LM, false>("asr_ctc_prefix_beam_lm", vals, ids, blank_lp, in_len, ws, ws_bytes, out_tok, out_len, out_score, B, T, k, beam, nbest, Lcap,
                                          blank, stream, {ngram_lm_of(lm), out_bias, out_state}, {});
}

extern "C" int asr_ctc_prefix_beam_lm_state_init(void* state, void* ws, const asr_ngram_lm* lm, int B, int beam, int T_cap, void* stream) {
    return pb_state_launch<PB_LM, false>("asr_ctc_prefix_beam_lm_state_init", state, ws, nullptr, B, beam, T_cap, stream, {ngram_lm_of(lm), nullptr, nullptr});
}

extern "C" int asr_ctc_prefix_beam_lm_state_reset(void* state, void* ws, const int32_t* flags, const asr_ngram_lm* lm, int B, int beam, int T_cap, void* stream) {
    if (!flags) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_beam_lm_state_reset: null pointer");      // without flags it would be an init
    return pb_state_launch<PB_LM, false>("asr_ctc_prefix_beam_lm_state_reset", state, ws, flags, B, beam, T_cap, stream, {ngram_lm_of(lm), nullptr, nullptr});
}

extern "C" int asr_ctc_prefix_beam_chunk_lm(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                                            size_t ws_bytes, const asr_ngram_lm* lm, int32_t* out_tok, int32_t* out_len, float* out_score, double* out_bias,
                                            int32_t* out_state, int32_t* out_stable, int B, int C, int k, int beam, int nbest, int Lcap, int T_cap, int blank,
                                            void* stream) {
    return pb_chunk_launch<PB_LM, false>("asr_ctc_prefix_beam_chunk_lm", vals, ids, blank_lp, n_valid, state, ws, ws_bytes, out_tok, out_len, out_score, out_stable, B, C,
                                         k, beam, nbest, Lcap, T_cap, blank, stream, {ngram_lm_of(lm), out_bias, out_state}, {});
}

// ---- token times: the plain searches with the best single alignment of every prefix riding along (additive to ABI 10) ----------------------
extern "C" size_t asr_ctc_prefix_beam_timed_workspace_bytes(int B, int T, int beam) { return PbHost<PB_PLAIN, true>::workspace_bytes(B, T, beam); }
extern "C" size_t asr_ctc_prefix_beam_timed_state_bytes(int B, int beam) { return PbHost<PB_PLAIN, true>::state_bytes(B, beam); }

extern "C" int asr_ctc_prefix_beam_timed(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, void* ws, size_t ws_bytes,
                                         int32_t* out_tok, int32_t* out_len, float* out_score, double* out_vit, int32_t* out_start, int32_t* out_end,
                                         float* out_mx, float* out_mn, float* out_sm, int B, int T, int k, int beam, int nbest, int Lcap, int blank,
                                         void* stream) {
    return pb_search_launch<PB_PLAIN, true>("asr_ctc_prefix_beam_timed", vals, ids, blank_lp, in_len, ws, ws_bytes, out_tok, out_len, out_score, B, T, k, beam, nbest, Lcap,
                                            blank, stream, {}, {out_vit, out_start, out_end, out_mx, out_mn, out_sm, nullptr});
}

extern "C" int asr_ctc_prefix_beam_timed_state_init(void* state, void* ws, int B, int beam, int T_cap, void* stream) {
    return pb_state_launch<PB_PLAIN, true>("asr_ctc_prefix_beam_timed_state_init", state, ws, nullptr, B, beam, T_cap, stream, {});
}

extern "C" int asr_ctc_prefix_beam_timed_state_reset(void* state, void* ws, const int32_t* flags, int B, int beam, int T_cap, void* stream) {
    if (!flags) ASR_FAIL(ASR_EINVAL, "asr_ctc_prefix_beam_timed_state_reset: null pointer");      // without flags it would be an init
    return pb_state_launch<PB_PLAIN, true>("asr_ctc_prefix_beam_timed_state_reset", state, ws, flags, B, beam, T_cap, stream, {});
}

extern "C" int asr_ctc_prefix_beam_chunk_timed(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                                               size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score, double* out_vit, int32_t* out_start,
                                               int32_t* out_end, float* out_mx, float* out_mn, float* out_sm, int32_t* out_stable, int32_t* out_final, int B,
                                               int C, int k, int beam, int nbest, int Lcap, int T_cap, int blank, void* stream) {
    return pb_chunk_launch<PB_PLAIN, true>("asr_ctc_prefix_beam_chunk_timed", vals, ids, blank_lp, n_valid, state, ws, ws_bytes, out_tok, out_len, out_score, out_stable, B,
                                           C, k, beam, nbest, Lcap, T_cap, blank, stream, {}, {out_vit, out_start, out_end, out_mx, out_mn, out_sm, out_final});
}
