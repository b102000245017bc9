/*
 * asr_hip.h - C ABI of libasr_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the training
 * hot path of the Speech-Transformer of zqs01/ASR_chinese_e2e (+ the CTC branch that
 * BASELINE.json's north_star adds).
 *
 * The reference is pure Python on stock PyTorch ops and has NO native / FFI boundary of its own
 * (SURVEY.md section 8b).  Each entry point below therefore cites the reference op SEQUENCE
 * (file:line under the reference tree) that it replaces; the Python-side binding a maintainer
 * would add is shown in INTEGRATION.md (ctypes, mirrored in asr_chinese_e2e_amd/_lib.py).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  No torch types, no exceptions.
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in _host.
 *   - no allocation, no synchronisation, no host<->device copy inside any entry point: each call
 *     only enqueues kernels on `stream` (a hipStream_t passed as void*), so every entry point can
 *     be captured into a hipGraph.  Scratch memory comes from the caller (`ws`, sized by the
 *     matching asr_*_workspace_bytes query).
 *   - return value: ASR_OK (0) or a negative ASR_E* code; asr_last_error() gives the per-thread
 *     message.  Stateless and re-entrant; ordering is stream order only.
 *   - activations are padded-dense row-major (B, T, d) == (B*T, d); utterance b owns rows
 *     [b*T, (b+1)*T) of which the first len[b] are valid.  All masks are derived in-kernel from
 *     int32 length vectors - the reference's materialised (B,Tq,Tk) bool masks
 *     (Predictor/Models/utils.py:100-144) never exist.
 *   - dtype: ASR_F32 or ASR_BF16 is the STORAGE type of activation tensors; all arithmetic
 *     accumulates in fp32.  Parameters, optimizer state, statistics and losses are fp32.
 */
#ifndef ASR_HIP_H
#define ASR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASR_ABI_VERSION 10

typedef enum { ASR_F32 = 0, ASR_BF16 = 1 } asr_dtype_t;

#define ASR_OK 0
#define ASR_EINVAL (-1)     /* bad shape / null pointer / unsupported size */
#define ASR_EDTYPE (-2)     /* unsupported dtype for this op */
#define ASR_EWORKSPACE (-3) /* workspace too small */
#define ASR_EHIP (-4)       /* HIP runtime reported an error at launch */

#define ASR_ACT_NONE 0
#define ASR_ACT_RELU 1
#define ASR_ACT_RELU_MASK 2 /* C = (A W^T) where res > 0, else 0 (no bias: gradients have none) - the ReLU backward of
                               module.py:70-71 applied in the store tail of the input-gradient GEMM (res = the activations) */

int asr_abi_version(void);
/* copies the calling thread's last error message (NUL-terminated) into buf; returns its length */
int asr_last_error(char* buf, size_t n);
/* Deterministic mode (process-wide; initial value from the environment variable ASR_DETERMINISTIC).  The reference's
 * autograd on CPU sums every gradient in a fixed order (torch.autograd through transformer_official.py:100-103);
 * the default HIP path combines partial weight-gradient tiles, bias-gradient slices and embedding rows with fp32
 * atomics, whose arrival order varies from run to run.  With the mode on, every such reduction runs in a fixed
 * order: asr_gemm_tn_* write one partial slab per M-split into `ws` (asr_gemm_tn_workspace_bytes is then non-zero)
 * and add the slabs in split order, the column-sum finalisers use one workgroup per column group, asr_embed_bwd
 * adds the token rows in order, asr_gemm_tn_grouped_bf16 refuses.  Results are then bit-identical from run to run.
 * asr_set_deterministic returns the previous value. */
/* Stream ordering helper of the host runtime: work queued on `to_stream` after this call runs after the work queued on
 * `from_stream` before it (hipEventRecord + hipStreamWaitEvent on a pooled event).  The reference has one stream and
 * synchronises every step (trainer11.py:73-74); the engine runs weight gradients / the CTC branch / communication on side
 * streams and forks ~50 times per step.  Must not be called while either stream is being captured into a hipGraph. */
int asr_stream_fork(void* from_stream, void* to_stream);
/* Hand-over WITHOUT a marker packet in the producer's queue (ABI 7).  asr_stream_arm(from, to): the next entry point of this library
 * that supports it (asr_gemm_nt_bf16 on the loader / consumer kernel, asr_add_ln_bwd in its partial-sum form, the fused asr_sdpa_bwd,
 * asr_ctc_fwd_bwd with a gradient) launches its LAST kernel on `from` with the completion event bound to the dispatch packet itself
 * (hipExtLaunchKernelGGL) and makes `to` wait for it - hipEventRecord would put a barrier packet behind that kernel, and the next
 * kernel of the queue starts ~3.5 us later.  asr_stream_arm_pending() returns 1 (and clears the arm) when no launch took it: the
 * caller then uses asr_stream_fork.  One arm at a time; host-side state only. */
int asr_stream_arm(void* from_stream, void* to_stream);
int asr_stream_arm_pending(void);
/* A non-blocking stream created by the HIP runtime THIS library is bound to: priority < 0 = the lowest priority the device
 * offers (weight-gradient stream: off the critical path of the step), 0 = default, > 0 = the highest.  Lives as long as the
 * process.  (The reference has one stream, trainer11.py:73-74; torch.cuda.Stream offers no low priority.) */
int asr_stream_create(int priority, void** out_stream);
/* Tuning options: process-wide integer switches under which every value gives correct results, settable at run time.  ABI 8 keeps one:
 * "cu_limit" (> 0: the one-workgroup-per-CU kernels - persistent NT GEMM grid, weight-gradient M-splits - size their launches for this
 * many CUs instead of the device's; the engine sets it around the large launches that run beside the decoder's chain of small kernels;
 * 0 = the whole device).  (Rounds 2 - 3 carried switches between kernel variants here - store policy, tile shape, split plans; the variants
 * that lost their A/B left the library, see DESIGN.md section 4 "Tried".)  Initial value 0.
 * "tn_multi" (round 5; initial value 1): asr_gemm_tn_grouped_bf16 runs a group of problems over the same >= 4096 rows on the 128 x 128-tile
 * code of the single-problem kernel in one launch; 0 = always the 256 x 128-tile grouped kernel (A/B timing).
 * "sdpa_pair" (round 5; initial value 0): 1 = asr_sdpa_fwd without causal / band mask and without dropout on the kernel that takes both 32-query
 * blocks of a wave through one pass over the key tiles (same bits; measured slower, kept for A/B).
 * "sdpa_small" (initial value 1): asr_sdpa_fwd / asr_sdpa_bwd run bf16 heads of at most 64 queries and 64 keys, causal or unmasked, on the kernels
 * that give a head to ONE wave; 0 = on the one-workgroup-per-head kernels as before (results agree to the order of fp32 sums; kept for A/B).
 * "gemm_small_ring" (initial value 1): asr_gemm_small_bf16 keeps four 256-deep k-steps of both operands in flight and requests bias and ReLU mask before
 * the first of them; 0 = two k-steps in flight and bias / mask loaded in the store tail, as before (the same bits; kept for A/B).
 * previous (may be NULL) receives the old value.  Unknown name: ASR_EINVAL. */
int asr_set_option(const char* name, int value, int* previous);
int asr_get_deterministic(void);
int asr_set_deterministic(int on);

/* ---------------------------------------------------------------------------------------------
 * Fused residual-add + LayerNorm (+ positional encoding) (+ pad-row zeroing).
 * Replaces:  layer_norm(fc(x)+residual) ; enc_output *= non_pad_mask
 *              Predictor/Models/attention.py:59-60, module.py:72-75,
 *              transformer_official.py:208, 211, 449, 453, 456
 *            layer_norm_in(linear_in(x)) + positional_encoding   transformer_official.py:175-177
 *   z = x + res (res may be NULL);  xhat = (z - mean) * rstd  (eps 1e-5, biased variance)
 *   y = xhat * gamma + beta  (+ pe[t] if pe != NULL)   ;   y = 0 for rows t >= lens[b] if lens
 * x, res, y, xhat: (B*T, d) `dtype`; xhat may alias x.  gamma, beta: (d) f32; pe: (>=T, d) f32;
 * rstd: (B*T) f32; lens: (B) int32 or NULL.  d <= 2048.
 * Dropout (drop_p > 0; reference sites attention.py:59, module.py:73, transformer_official.py:175):
 *   drop_mode ASR_DROP_PRE : x is dropped (x * keep / (1-p)) before the residual add;
 *   drop_mode ASR_DROP_POST: the output (after the PE add, before pad zeroing) is dropped.
 * The keep mask of element (row, col) is a counter hash of (row*d + col, drop_seed): forward and
 * backward regenerate it, nothing is stored (asr_dropout_mask materialises it for tests).
 */
#define ASR_DROP_PRE 1
#define ASR_DROP_POST 2
int asr_add_ln_fwd(const void* x, const void* res, const float* gamma, const float* beta,
                   const float* pe, const int32_t* lens, void* y, void* xhat, float* rstd,
                   int B, int T, int d, float drop_p, uint32_t drop_seed, int drop_mode, int dtype,
                   void* stream);

/* asr_add_ln_slots_fwd (additive to ABI 10; independent sessions): the input LayerNorm of one tick of `slots` sessions, each at its
 * own frame offset.  y[b, t] = LN(x[b, t]) * gamma + beta + pe[pe_off[b] + t]; rows t >= lens[b] are zeroed.  Inference only: no
 * residual, no dropout.  x: (slots*T, d) `dtype`, overwritten with the normalised rows (asr_add_ln_fwd's xhat, in place); y:
 * (slots*T, d), not x; rstd: (slots*T) f32 scratch; gamma, beta: (d) f32; pe: (pe_rows, d) f32; pe_off, lens: (slots) int32 on the
 * device (wave-uniform loads).  It launches asr_add_ln_fwd's own kernel with one more argument, so a row has the bits asr_add_ln_fwd
 * gives it with pe + pe_off[b] * d as its table.  The caller checks pe_off[b] + T <= pe_rows on the host before the call (the
 * offsets are device data here); the kernel clamps the table row to [0, pe_rows) so that a wrong offset reads nothing outside.
 * ASR_EINVAL: a null pointer, slots, T or d < 1, d > 2048, pe_rows < T, y == x, a misaligned pointer. */
int asr_add_ln_slots_fwd(void* x, const float* gamma, const float* beta, const float* pe, const int32_t* pe_off,
                         const int32_t* lens, void* y, float* rstd, int slots, int T, int d, int pe_rows, int dtype, void* stream);

/* Backward of the above.  dy (+ dy2 if not NULL) is the gradient wrt y.
 *   g = (dy + dy2) * mask * gamma ;  dz = rstd * (g - mean(g) - xhat * mean(g * xhat))
 * dz: (B*T, d) `dtype` (gradient wrt x and wrt res).  Column sums over all rows are ACCUMULATED
 * (+=) into f32 vectors: dgamma += sum (dy*mask*xhat), dbeta += sum (dy*mask), and, if dbias is
 * not NULL, dbias += sum dz (bias gradient of the GEMM that produced x).
 * With ASR_DROP_PRE dropout the gradient wrt x differs from the residual gradient: dz stays the
 * residual gradient and dx (required then, (B*T, d) `dtype`) receives dz * keep / (1-p); dbias sums
 * dx.  With ASR_DROP_POST the mask is applied to (dy + dy2) first.  dx may be NULL otherwise.
 * ws: asr_add_ln_bwd_workspace_bytes(B*T, d) bytes of scratch.
 */
size_t asr_add_ln_bwd_workspace_bytes(int rows, int d);
int asr_add_ln_bwd(const void* dy, const void* dy2, const void* xhat, const float* rstd,
                   const float* gamma, const int32_t* lens, void* dz, void* dx, float* dgamma,
                   float* dbeta, float* dbias, void* ws, size_t ws_bytes, int B, int T, int d,
                   float drop_p, uint32_t drop_seed, int drop_mode, int dtype, void* stream);
/* With dgamma == dbeta == NULL asr_add_ln_bwd leaves the per-workgroup partial sums of the parameter gradients in
 * `ws` (which the caller then keeps); this call adds the partial sums of up to ASR_LN_REDUCE_MAX such sites into
 * their dgamma / dbeta / dbias in ONE launch (the 13 LayerNorm sites of an encoder backward would otherwise cost
 * 13 small launches).  `items` is a host array, read during the call; rows = B*T of the site's asr_add_ln_bwd. */
#define ASR_LN_REDUCE_MAX 16
typedef struct asr_ln_reduce_item {
    const void* ws;
    float* dgamma;
    float* dbeta;
    float* dbias; /* or NULL */
    int rows;
} asr_ln_reduce_item;
int asr_add_ln_bwd_reduce_batched(const asr_ln_reduce_item* items, int n, int d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Masked scaled-dot-product attention, flash style (scores never materialised).
 * Replaces:  bmm(q,k^T)/temperature -> masked_fill(mask,-inf) -> softmax -> bmm(attn,v)
 *              Predictor/Models/attention.py:76-84, with the head split/merge permutes of
 *              attention.py:43-57 folded into strided addressing, and the masks of
 *              utils.py:100-144 / transformer_official.py:292-303 computed from lengths.
 * q: rows b*Tq+t, k/v: rows b*Tk+t; head h lives at columns [h*dk, (h+1)*dk) of a row whose
 * stride is ldq / ldk / ldv / ldo ELEMENTS (so q,k,v can point into one fused QKV buffer).
 * Key j is visible to query i of utterance b iff  j < k_len[b]  and (!causal or j <= i)
 * and (window < 0 or |i - j| <= window).  lse: (B, H, Tq) f32 = log sum exp of scaled scores.
 * ASR_BF16 runs on MFMA (dk must be 64); ASR_F32 is an exact-fp32 VALU path (dk <= 128).
 * drop_p > 0: dropout on the attention probabilities after the softmax (attention.py:83): the
 * output uses p * keep / (1-p), the normaliser does not.  Mask of (b,h,q,k) = counter hash of
 * (((b*H+h)*Tq+q)*Tk_even + k, drop_seed), Tk_even = Tk rounded up to even.
 * o_lo (ABI 10; ASR_BF16 only, may be NULL): a second buffer of o's layout that receives the LOW-ORDER piece of the output,
 * bf16(x - float(bf16(x))) of the fp32 value x whose bf16 rounding is stored in o.  Nothing but asr_sdpa_bwd reads it: with o alone
 * delta = rowsum(do * o) carries 2^-9 |o| of rounding per coordinate, which dq = sum_j p_j (dp_j - delta) k_j multiplies by the MEAN key
 * (the reference's fp32 softmax backward has no such term): measured 0.989 instead of >= 0.9995 gradient cosine of the top encoder
 * layer's Q / K projections at the full-size configuration.  The single-pass backward kernel (Tk <= 512) has its own remedy (centred keys,
 * dK's mean over the keys removed) and ignores the piece; the band form (Tk > 512 inside a window) and the two-kernel path read it.
 * The forward pass WRITES the piece on the tiled path (Tk > 512) and clears it everywhere else.
 */
int asr_sdpa_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                 const int32_t* k_len, int B, int H, int Tq, int Tk, int dk, int ldq, int ldk,
                 int ldv, int ldo, int causal, int window, float scale, float drop_p,
                 uint32_t drop_seed, void* o_lo, int dtype, void* stream);

/* Backward: given do (same layout as o) computes dq, dk, dv (layouts/strides of q, k, v).
 * delta: f32 scratch of delta_bytes >= asr_sdpa_bwd_workspace_bytes(...) bytes, written by the call: (B, H, Tq) row sums
 * rowsum(do*o) for the two-kernel paths, or - bf16 self-attention inside a +-window band over more than 512 keys (the long-form
 * configuration, T = 2000: the band precedent is Predictor/Models/transformer_new.py:53) - the fp32 dQ partials of the query tiles
 * that straddle a 512-key block boundary of the single-pass band kernel.  With a smaller scratch (>= B*H*Tq floats) the band shapes
 * run on the two-kernel path. */
size_t asr_sdpa_bwd_workspace_bytes(int B, int H, int Tq, int Tk, int dk, int causal, int window, int dtype);
int asr_sdpa_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                 const float* lse, float* delta, size_t delta_bytes, void* dq, void* dk_, void* dv,
                 const int32_t* k_len, int B, int H, int Tq, int Tk, int dk, int ldq, int ldk,
                 int ldv, int ldo, int causal, int window, float scale, float drop_p,
                 uint32_t drop_seed, const void* o_lo, int dtype, void* stream);      /* o_lo: what asr_sdpa_fwd wrote there, or NULL */

/* Chunk-masked attention (streaming encoders; WeNet's subsequent_chunk_mask with num_left_chunks, plus the key-length mask).
 * Same arguments as asr_sdpa_fwd / asr_sdpa_bwd with (causal, window) replaced by (chunk, left_chunks), in key / query frames:
 * key j is visible to query i of utterance b iff
 *     j < k_len[b]  and  j < (i / chunk + 1) * chunk  and  (left_chunks < 0  or  j >= (i / chunk - left_chunks) * chunk)
 * (integer division).  chunk >= Tk with left_chunks = -1 is full attention; chunk = 1, left_chunks = -1 is causal attention.  A query that sees no key (a padded frame of a chunk past the left context of
 * every valid key, any query of an utterance with k_len = 0) gets o = 0 and lse = 0 (finite) and adds nothing to dk / dv.
 * chunk < 1 or left_chunks < -1: ASR_EINVAL before anything is launched.  Dropout masks: the counters of asr_sdpa_fwd.
 * Every path of asr_sdpa_fwd / _bwd has a chunk form except the band kernel (no window here); o_lo as there.
 * The backward scratch needs asr_sdpa_chunk_bwd_workspace_bytes(...) = B*H*Tq floats. */
int asr_sdpa_chunk_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                       const int32_t* k_len, int B, int H, int Tq, int Tk, int dk, int ldq, int ldk,
                       int ldv, int ldo, int chunk, int left_chunks, float scale, float drop_p,
                       uint32_t drop_seed, void* o_lo, int dtype, void* stream);
size_t asr_sdpa_chunk_bwd_workspace_bytes(int B, int H, int Tq, int Tk, int dk, int chunk, int left_chunks, int dtype);
int asr_sdpa_chunk_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                       const float* lse, float* delta, size_t delta_bytes, void* dq, void* dk_, void* dv,
                       const int32_t* k_len, int B, int H, int Tq, int Tk, int dk, int ldq, int ldk,
                       int ldv, int ldo, int chunk, int left_chunks, float scale, float drop_p,
                       uint32_t drop_seed, const void* o_lo, int dtype, void* stream);

/* Test helpers: materialise the keep masks the kernels regenerate (1 = kept), uint8.
 * asr_dropout_mask: (rows, cols) mask of the LayerNorm / embedding sites;
 * asr_sdpa_dropout_mask: (B, H, Tq, Tk) mask of the attention-probability site. */
int asr_dropout_mask(uint8_t* mask, int rows, int cols, float drop_p, uint32_t drop_seed, void* stream);
int asr_sdpa_dropout_mask(uint8_t* mask, int B, int H, int Tq, int Tk, float drop_p, uint32_t drop_seed, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CTC loss, forward-backward, fused with log-softmax over the vocabulary.
 * NOT in the reference (it has only cross-entropy, Predictor/Utils/loss.py:26-51); required by
 * BASELINE.json north_star.  Semantics = torch.nn.functional.ctc_loss(log_softmax(logits), ...,
 * blank, reduction='none') and its gradient wrt logits (ATen native/LossCTC.cpp).
 * logits: (B, T, V) `dtype`, rows `ld` elements apart (ABI 6: ld = V for a dense tensor; the training engine pads rows to a
 * multiple of 64 elements so that every row starts on a 128-byte line - with V = 4232 the head GEMM that writes them is 14 %
 * faster; columns V .. ld are never read or written);  in_len: (B) int32 frames per utterance (<= T);
 * labels: (B, Lmax) int32 padded; lab_len: (B) int32 (<= Lmax <= 255).
 * nll: (B) f32 = -log p(labels | x) (+inf when infeasible, i.e. in_len < L + number of adjacent repeats; 0 if zero_infinity).
 * The lattice runs in a scaled linear domain; an utterance that leaves its fp64 range (long labels under blank-dominated
 * posteriors) is redone in the log domain, so a feasible utterance never reads as infeasible.
 * dlogits: (B, T, V) `dtype`, same row stride (may alias logits) = scale * d(sum_b nll_b)/dlogits,
 * rows t >= in_len[b] are 0.  If dlogits is NULL only nll is computed.
 * scale = grad_scale, or grad_scale / *grad_scale_div when grad_scale_div (a DEVICE f32 scalar) is not NULL: under data
 * parallelism the CTC term is normalised by the GLOBAL batch, which arrives from an all-reduce on the device - the
 * host never waits for it (ABI 3; the cross-entropy kernel takes its token count the same way).
 * best_path (ABI 9; may be NULL): (B, T) int32, the frame-wise argmax of the logits (first index on ties, `blank` for frames
 * t >= in_len[b]) - the greedy CTC path, taken by the kernel that holds the row anyway.  With dlogits aliasing logits the
 * logits are gone after the call; the training step's per-batch CER (the reference's trainer reads metrics.cer every step,
 * Trainer/trainer11.py:73-75, computed by transformer_official.py:83-94) collapses this path with asr_ctc_collapse.
 */
size_t asr_ctc_workspace_bytes(int B, int T, int Lmax);
int asr_ctc_fwd_bwd(const void* logits, void* dlogits, const int32_t* in_len,
                    const int32_t* labels, const int32_t* lab_len, float* nll, int B, int T, int V, int ld,
                    int Lmax, int blank, float grad_scale, const float* grad_scale_div, int zero_infinity,
                    int32_t* best_path, void* ws, size_t ws_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CTC forced alignment (Viterbi): the single best path through the same lattice, i.e. the max-product form of
 * torch.nn.functional.ctc_loss.  Additive to ABI 10 (no version change).  Inputs as asr_ctc_fwd_bwd.
 * States: the blank-augmented sequence l' (blanks at even s, labels at odd s, S = 2L + 1);
 *   delta_0(0) = log y_0(blank), delta_0(1) = log y_0(l_1),
 *   delta_t(s) = log y_t(l'_s) + max(delta_{t-1}(s), delta_{t-1}(s-1), delta_{t-1}(s-2)), the s-2 term only where l'_s is a label
 *   different from l'_{s-2}; y = softmax of the logits row.  The path ends in 2L or 2L-1 at t = in_len[b] - 1.
 *   Ties: the predecessor s before s-1 before s-2; at the end 2L before 2L-1.
 * path: (B, T) int32 token id of the aligned state per frame (`blank` on blank frames, -1 for t >= in_len[b]).
 * spans: (B, Lmax, 2) int32 first and last frame (inclusive) of each label token, -1 for i >= lab_len[b].
 * token_logp: (B, Lmax) f32 sum of log y_t(l_i) over the frames of token i (0 for i >= lab_len[b]).
 * score: (B) f32 log-probability of the best path.
 * Infeasible utterances (in_len < L + number of adjacent repeats): score = -inf, spans -1, token_logp -inf, path `blank` on the
 * utterance's frames.  L = 0 aligns every frame to the blank; in_len = 0 gives score 0 when L = 0 (else -inf) and a path of -1.
 * ws: asr_ctc_align_workspace_bytes(B, T, Lmax) bytes.  Lmax <= 255.
 */
size_t asr_ctc_align_workspace_bytes(int B, int T, int Lmax);
int asr_ctc_align(const void* logits, const int32_t* in_len, const int32_t* labels, const int32_t* lab_len, int32_t* path,
                  int32_t* spans, float* token_logp, float* score, int B, int T, int V, int ld, int Lmax, int blank, void* ws,
                  size_t ws_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Greedy CTC decoding: per-frame argmax over the vocabulary (first index wins ties, as
 * torch.argmax), frames t >= in_len[b] count as blank, then the CTC collapse (merge repeats, drop
 * blanks).  NOT in the reference (no CTC there; its decoder-side search is the Python beam loop
 * transformer_official.py:331-434) - SURVEY.md 8(f) rank 1.
 * logits: (B, T, V) `dtype`, rows `ld` elements apart (ABI 6; V for a dense tensor); out_ids: (B, T) int32 = collapsed label ids,
 * 0-padded; out_len: (B).
 * ABI 9: the two halves are entry points of their own - asr_ctc_frame_argmax writes the frame-wise best path (B, T), asr_ctc_collapse
 * collapses a path in place (ids: (B, T) -> collapsed ids, 0-padded; out_len) - so that the training step can collapse the path
 * asr_ctc_fwd_bwd hands out (best_path) without a second pass over the logits.
 */
int asr_ctc_greedy_decode(const void* logits, const int32_t* in_len, int32_t* out_ids,
                          int32_t* out_len, int B, int T, int V, int ld, int blank, int dtype, void* stream);
int asr_ctc_frame_argmax(const void* logits, const int32_t* in_len, int32_t* path, int B, int T, int V, int ld, int blank,
                         int dtype, void* stream);
int asr_ctc_collapse(int32_t* ids, const int32_t* in_len, int32_t* out_len, int B, int T, int blank, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Beam search of the attention decoder, batched over utterances x beams
 * with key/value caches.  Replaces Decoder.recognize_beam, transformer_official.py:331-434, which
 * re-runs the whole decoder over the growing prefix for every hypothesis at every step in a
 * Python loop, one utterance at a time.  Same search: every live hypothesis is extended by its
 * `beam` best tokens (log_softmax scores, no length normalisation), the best `beam` extensions
 * survive (stable order on ties), hypotheses that emit eos leave the beam, at step maxlen-1 eos is
 * appended to every survivor.
 *
 * asr_decode_attn: single-query attention.  q: (R, H*dk) rows of stride ldq; keys/values of row r
 *   are rows (r / kv_div) * Tk_cap + t, t < len, of k / v (strides ldk / ldv, head h at columns
 *   [h*dk, (h+1)*dk)); len = k_len[r / len_div] if k_len else k_len_uniform.  No mask other than the
 *   length (recognize_beam passes dec_enc_attn_mask=None and a causal mask that only hides the
 *   future, which a cache never contains).  o: (R, H*dk), stride ldo.
 * asr_logsoftmax_topk: vals/ids (R, beam) = the `beam` largest log_softmax(logits[r]) entries,
 *   descending, ties by ascending index (transformer_official.py:381-384).
 * asr_beam_step: one search step for B utterances (beam <= 8).  In/out state score, alive,
 *   last_tok, parent: (B, beam).  Records of step `step` at [(step*B + b)*beam + slot]: rec_tok,
 *   rec_par (slot of the parent at the previous step), rec_end (0 live, 1 ended by its own eos,
 *   2 eos appended at the last step), rec_score.  maxlen: (B) int32 steps allowed per utterance.
 *   *alive_total += number of hypotheses still live after the step.
 * asr_cache_gather: dst[l][r][t] = src[l][(r / beam) * beam + parent[r]][t] for t < n_pos, with
 *   L caches of R rows x Lcap positions x row_bytes bytes (multiple of 16).
 */
/* asr_ctc_frame_topk: per frame (row) of the CTC head's logits, the k largest log_softmax entries (as asr_logsoftmax_topk) and the
 *   log_softmax of the blank class: the per-frame candidates of CTC prefix beam search (the reference has
 *   no CTC and leaves greedy_search / beam_search as empty stubs, transformer_official.py:106-110).  The prefix bookkeeping
 *   (merging paths that spell the same prefix) runs over these k candidates per frame.
 * asr_ctc_prefix_beam (ABI 4): that bookkeeping on the device - CTC prefix beam search (Hannun et al. 2014, algorithm 1 without a
 *   language model) for B utterances, one wave per utterance.  vals / ids: (B*T, k) from asr_ctc_frame_topk, blank_lp: (B*T),
 *   in_len: (B) frames per utterance (NULL = T).  The beam's prefixes are nodes of a trie in `ws`
 *   (asr_ctc_prefix_beam_workspace_bytes); beam * (k + 1) <= 64 (one wave ranks a frame's candidates), nbest <= beam.
 *   Out, per utterance and rank r < nbest, best first: out_tok[(b*nbest + r)*Lcap ..] the prefix (its first Lcap tokens),
 *   out_len its length (-1: fewer than nbest prefixes have non-zero probability), out_score log p(prefix | x) summed over
 *   alignments (fp64 inside).  Same results as the host restatement oracle/decode_ref.py::ctc_prefix_beam_search with the same
 *   per-frame candidates. */
int asr_ctc_frame_topk(const void* logits, float* vals, int32_t* ids, float* blank_lp, int R, int V, int ld, int k,
                       int blank, int dtype, void* stream);
size_t asr_ctc_prefix_beam_workspace_bytes(int B, int T, int beam);
int asr_ctc_prefix_beam(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, void* ws, size_t ws_bytes,
                        int32_t* out_tok, int32_t* out_len, float* out_score, int B, int T, int k, int beam, int nbest, int Lcap,
                        int blank, void* stream);
/* The same search, resumable (additive to ABI 10): the beam leaves the kernel between launches, so the frames may arrive in chunks.
 *   state: asr_ctc_prefix_beam_state_bytes(B, beam) bytes, 8-aligned; per utterance int32 {nb, next_node, frames consumed, 0}, int32
 *   node / token / parent / depth [beam], fp64 pb / pnb [beam].  ws: asr_ctc_prefix_beam_stream_workspace_bytes(B, T_cap, beam) bytes, the
 *   trie ([parent | token] x (T_cap * beam + 1) nodes per utterance, numbered as asr_ctc_prefix_beam numbers them).
 * asr_ctc_prefix_beam_state_init: the empty-prefix beam asr_ctc_prefix_beam starts from, and the trie's root.
 * asr_ctc_prefix_beam_chunk: vals / ids (B*C, k), blank_lp (B*C) = one chunk's rows of asr_ctc_frame_topk; consumes the first
 *   n_valid[b] in [0, C] frames of utterance b (clamped to what T_cap still admits: nothing is ever written outside ws), stores the state
 *   back and writes out_tok / out_len / out_score as asr_ctc_prefix_beam does - after any cutting of the frames into chunks bit for bit what
 *   asr_ctc_prefix_beam gives on the frames consumed so far (both run one frame-step body).  n_valid[b] == 0: the state keeps every byte,
 *   the outputs are spelled from it.  out_stable[b] = the length of the longest common prefix of all beam entries (the depth of their
 *   lowest common ancestor in the trie): every later entry descends from a current one, so these tokens are never retracted and the
 *   length never decreases.  Limits as asr_ctc_prefix_beam, and C >= 1, T_cap >= 1; one wave per utterance. */
size_t asr_ctc_prefix_beam_state_bytes(int B, int beam);
size_t asr_ctc_prefix_beam_stream_workspace_bytes(int B, int T_cap, int beam);
int asr_ctc_prefix_beam_state_init(void* state, void* ws, int B, int beam, int T_cap, void* stream);
int asr_ctc_prefix_beam_chunk(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                              size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score, int32_t* out_stable, int B, int C, int k,
                              int beam, int nbest, int Lcap, int T_cap, int blank, void* stream);
/* asr_ctc_prefix_beam_state_reset (additive to ABI 10; independent sessions): re-initialises the utterances b with flags[b] != 0
 *   (flags: (B) int32 on the device) - their beam and their trie's root, byte for byte what asr_ctc_prefix_beam_state_init leaves
 *   for them (one device function writes both); every other utterance keeps every byte.  Arguments and limits as state_init. */
int asr_ctc_prefix_beam_state_reset(void* state, void* ws, const int32_t* flags, int B, int beam, int T_cap, void* stream);
/* Hotword (context) biasing of the CTC prefix beam search (additive to ABI 10; the definition: asr_chinese_e2e_amd/context.py, restated in
 *   fp64 by tests/context_ref.py).  asr_context_graph: the phrase lists of one or more graphs as one flat automaton on the device - arcs of
 *   state s = [st_off[s], st_off[s + 1]) with ascending arc_tok, arc_next the state an arc leads to (an arc onto a final leaf leads to its
 *   graph's root), st_held[s] = w * (depth(s) - depth of the deepest final state on its path), w the bonus per matched token.  A beam entry
 *   carries (state, bias) from (root, 0.0); appending token c: an arc (state, c) -> bias += w and the state follows it; otherwise bias -=
 *   st_held[state], the state is the root and the arc (root, c) is tried once.  Candidates of a frame are ranked by log p + bias; nothing
 *   else of the search changes, and out_score stays log p.
 *   THE WRAPPERS CHECK pointers, alignment (8 bytes for anything fp64), S >= 1, A >= 0 and the searches' limits; THEY CANNOT CHECK THE
 *   TABLES' CONTENTS, which live on the device: ContextGraph is their only producer and validates them (tokens in [1, V), every arc_next <
 *   S, arcs sorted and unique, offsets ascending within [0, A]).  The kernels still clamp every table index they form.
 * asr_ctc_prefix_beam_ctx: asr_ctc_prefix_beam with a graph.  root: (B) int32 on the device, the root state of each utterance's graph, -1
 *   (or anything outside [0, S)) = this utterance is not biased and gets asr_ctc_prefix_beam's outputs bit for bit.  Two more outputs per
 *   n-best entry: out_bias (B, nbest) fp64, 8-aligned - the entry's RAW bias, st_held[out_state] is not yet taken off (the caller reports
 *   bias - held, so that a phrase begun and not finished earns nothing) - and out_state (B, nbest) int32 (-1: no entry / not biased).  The
 *   entries are in the beam's rank order (log p + raw bias); the caller sorts by log p + bias - held (stable).
 * asr_ctc_prefix_beam_ctx_state_bytes / _ctx_state_init / _ctx_state_reset / asr_ctc_prefix_beam_chunk_ctx: the resumable form.  The state
 *   of one utterance is asr_ctc_prefix_beam_chunk's, followed by fp64 bias[beam], int32 ctx[beam], int32 root, padded to 8 bytes; init and
 *   reset take root (B) int32 on the device (reset reads it for the flagged utterances only: a reopened session may bring another list).  A
 *   context state is only ever passed to the _ctx entry points and a plain state to the plain ones.  Cutting the frames into chunks changes
 *   no bit of any output, and a chunk that consumes nothing changes no byte of the state, as for the plain search. */
typedef struct asr_context_graph {
    const int32_t* st_off;    /* device, (S + 1) */
    const int32_t* arc_tok;   /* device, (A) */
    const int32_t* arc_next;  /* device, (A) */
    const double* st_held;    /* device, (S), 8-aligned */
    int S, A;
    double w;
} asr_context_graph;
int asr_ctc_prefix_beam_ctx(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, const int32_t* root,
                            const asr_context_graph* ctx, void* ws, size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score,
                            double* out_bias, int32_t* out_state, int B, int T, int k, int beam, int nbest, int Lcap, int blank, void* stream);
size_t asr_ctc_prefix_beam_ctx_state_bytes(int B, int beam);
int asr_ctc_prefix_beam_ctx_state_init(void* state, void* ws, const int32_t* root, int B, int beam, int T_cap, void* stream);
int asr_ctc_prefix_beam_ctx_state_reset(void* state, void* ws, const int32_t* flags, const int32_t* root, int B, int beam, int T_cap, void* stream);
int asr_ctc_prefix_beam_chunk_ctx(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                                  size_t ws_bytes, const asr_context_graph* ctx, int32_t* out_tok, int32_t* out_len, float* out_score,
                                  double* out_bias, int32_t* out_state, int32_t* out_stable, int B, int C, int k, int beam, int nbest, int Lcap,
                                  int T_cap, int blank, void* stream);
/* N-gram LM shallow fusion in the CTC prefix beam search (additive to ABI 10; the definition: asr_chinese_e2e_amd/lm.py, restated in fp64 by
 *   tests/lm_ref.py).  asr_ngram_lm: a back-off n-gram model (ARPA semantics, orders 1 to 5) as one flat automaton on the device.  State 0
 *   is the empty history and has no arcs; a state s >= 1 is a context of 1 .. order - 1 tokens with the arcs [st_off[s], st_off[s + 1]),
 *   ascending arc_tok.  An arc (s, c) carries arc_term, the term of the listed n-gram s.c, and arc_next >= 0, the state after c; arc_next =
 *   ~state marks an arc whose n-gram is not listed itself (only longer ones are): it fixes the next state and the chain goes on.  st_back[s] =
 *   the state of the longest proper suffix of s that is a state, st_bow[s] = the back-off term (0.0: none).  uni_term[c] / uni_next[c]: the
 *   unigram level, dense over the V tokens (the unk term and state 0 where there is no unigram), so every chain ends in one indexed load.
 *   Every term is fp64 weight * ln p, folded on the host.  A beam entry carries (state, bias) from (start, 0.0); appending token c walks
 *   the chain from its state: bias += st_bow per state left, bias += the term of the n-gram found, bias += ins; the state becomes that of the
 *   first arc met (uni_next at the end of the chain).  Candidates of a frame are ranked by log p + bias; nothing else of the search changes,
 *   and out_score stays log p.  An LM and a context graph are not combined: each has its own entry points and its own state layout.
 *   THE WRAPPERS CHECK pointers, alignment (8 bytes for anything fp64), S >= 1, A >= 0, V >= 1, 1 <= order <= 5, 0 <= start < S, a finite ins
 *   and the searches' limits; THEY CANNOT CHECK THE TABLES' CONTENTS, which live on the device: NgramLM is their only producer and validates
 *   them.  The kernels still clamp every table index they form and bound the chain by `order`.
 * asr_ctc_prefix_beam_lm: asr_ctc_prefix_beam with an LM.  Two more outputs per n-best entry: out_bias (B, nbest) fp64, 8-aligned - the
 *   entry's bias WITHOUT the end-of-sentence term (the caller adds term(</s> | out_state) and sorts by log p + that, stable) - and out_state
 *   (B, nbest) int32 (-1: no entry).  The entries are in the beam's rank order (log p + bias).
 * asr_ctc_prefix_beam_lm_workspace_bytes: the LM searches' trie, offline (T frames) and resumable (T = T_cap): twice the plain search's,
 *   int32 [parent | token | first child | sibling] x (T * beam + 1) nodes per utterance.  The child lists make a prefix that left the beam
 *   and comes back take the node it had, so that a longer prefix that stayed is still recognised as its extension (with an insertion bonus
 *   that happens; the plain search would hold the same string twice and split its probability).
 * asr_ctc_prefix_beam_lm_state_bytes / _lm_state_init / _lm_state_reset / asr_ctc_prefix_beam_chunk_lm: the resumable form.  The state of one
 *   utterance is asr_ctc_prefix_beam_chunk's, followed by fp64 bias[beam], int32 st[beam], padded to 8 bytes; init puts every utterance on
 *   lm->start, reset the flagged ones, every other utterance keeps every byte; their workspace is asr_ctc_prefix_beam_lm_workspace_bytes(B, T_cap, beam).  An LM state is only ever passed to the _lm entry points.
 *   Cutting the frames into chunks changes no bit of any output, and a chunk that consumes nothing changes no byte of the state. */
typedef struct asr_ngram_lm {
    const int32_t* st_off;    /* device, (S + 1) */
    const int32_t* arc_tok;   /* device, (A) */
    const int32_t* arc_next;  /* device, (A) */
    const double* arc_term;   /* device, (A), 8-aligned */
    const int32_t* st_back;   /* device, (S) */
    const double* st_bow;     /* device, (S), 8-aligned */
    const double* uni_term;   /* device, (V), 8-aligned */
    const int32_t* uni_next;  /* device, (V) */
    int S, A, V, order, start;
    double ins;
} asr_ngram_lm;
int asr_ctc_prefix_beam_lm(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, const asr_ngram_lm* lm, void* ws,
                           size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score, double* out_bias, int32_t* out_state, int B,
                           int T, int k, int beam, int nbest, int Lcap, int blank, void* stream);
size_t asr_ctc_prefix_beam_lm_workspace_bytes(int B, int T, int beam);
size_t asr_ctc_prefix_beam_lm_state_bytes(int B, int beam);
int asr_ctc_prefix_beam_lm_state_init(void* state, void* ws, const asr_ngram_lm* lm, int B, int beam, int T_cap, void* stream);
int asr_ctc_prefix_beam_lm_state_reset(void* state, void* ws, const int32_t* flags, const asr_ngram_lm* lm, int B, int beam, int T_cap, void* stream);
int asr_ctc_prefix_beam_chunk_lm(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                                 size_t ws_bytes, const asr_ngram_lm* lm, int32_t* out_tok, int32_t* out_len, float* out_score, double* out_bias,
                                 int32_t* out_state, int32_t* out_stable, int B, int C, int k, int beam, int nbest, int Lcap, int T_cap, int blank,
                                 void* stream);
/* Token times and confidence for the plain prefix beam search (additive to ABI 10; the definition the tests check against, bit for bit, is
 * tests/beam_times_ref.py).  Beside pb / pnb every beam entry carries the best single alignment of its prefix that ends in blank and in
 * non-blank: its fp64 log-probability (every sum is v + (double)lp in that order) and one record per token {start, end, mx, mn, sm} = the
 * first and last absolute frame of the token's run in that alignment, the largest and smallest log-posterior of the token over the run and
 * their float32 sum in ascending frame order.  An extension that is merged into an entry of the beam competes with that entry's own repeat:
 * the larger alignment wins, the repeat on equality.  The records are persistent lists in a second trie behind the B prefix tries: per
 * utterance (T * beam + 1) nodes of 8 words {parent, depth, start, end, mx, mn, sm, 0}; a kept entry with a finite non-blank alignment takes
 * one node per frame.  out_tok / out_len / out_score (and out_stable) are bit for bit the plain entry points'.
 * asr_ctc_prefix_beam_timed: asr_ctc_prefix_beam with, per n-best entry, out_vit (B, nbest) fp64, 8-aligned = the log-probability of the better
 *   of its two alignments (the blank one on equality; -inf: no entry) and that alignment's records out_start / out_end (B, nbest, Lcap) int32,
 *   out_mx / out_mn / out_sm (B, nbest, Lcap) float.  Only the first min(out_len, Lcap) positions of a row are written.
 * asr_ctc_prefix_beam_timed_workspace_bytes: both tries, offline (T frames) and resumable (T = T_cap): B * 10 * (T * beam + 1) * 4 bytes, 8-aligned.
 * asr_ctc_prefix_beam_timed_state_bytes / _timed_state_init / _timed_state_reset / asr_ctc_prefix_beam_chunk_timed: the resumable form.  The
 *   state of one utterance is asr_ctc_prefix_beam_chunk's, followed by fp64 vb[beam], vnb[beam], int32 hb[beam], hnb[beam] (list heads) and the
 *   time trie's nodes in use, padded to 8 bytes.  Reset touches the flagged utterances only; a chunk that consumes nothing changes no byte of
 *   state or workspace; cutting the frames into chunks changes no bit of any output.  out_final (B) int32: how many leading records of every
 *   reported list are final - the depth of the lowest common ancestor of the lists without their last record, over every non-empty list of
 *   a finite alignment in the beam (0 when one of those lists is empty).  It never decreases and final records never change.  A timed state is
 *   only ever passed to the _timed entry points.
 *   THE WRAPPERS CHECK pointers, alignment (8 bytes for the state, the workspace and out_vit) and the plain searches' limits; the kernels keep every index
 *   they form inside the workspace of T_cap frames. */
size_t asr_ctc_prefix_beam_timed_workspace_bytes(int B, int T, int beam);
int asr_ctc_prefix_beam_timed(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* in_len, void* ws, size_t ws_bytes,
                              int32_t* out_tok, int32_t* out_len, float* out_score, double* out_vit, int32_t* out_start, int32_t* out_end,
                              float* out_mx, float* out_mn, float* out_sm, int B, int T, int k, int beam, int nbest, int Lcap, int blank,
                              void* stream);
size_t asr_ctc_prefix_beam_timed_state_bytes(int B, int beam);
int asr_ctc_prefix_beam_timed_state_init(void* state, void* ws, int B, int beam, int T_cap, void* stream);
int asr_ctc_prefix_beam_timed_state_reset(void* state, void* ws, const int32_t* flags, int B, int beam, int T_cap, void* stream);
int asr_ctc_prefix_beam_chunk_timed(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* n_valid, void* state, void* ws,
                                    size_t ws_bytes, int32_t* out_tok, int32_t* out_len, float* out_score, double* out_vit, int32_t* out_start,
                                    int32_t* out_end, float* out_mx, float* out_mn, float* out_sm, int32_t* out_stable, int32_t* out_final, int B,
                                    int C, int k, int beam, int nbest, int Lcap, int T_cap, int blank, void* stream);
int asr_decode_attn(const void* q, const void* k, const void* v, void* o, const int32_t* k_len,
                    int k_len_uniform, int len_div, int R, int H, int dk, int Tk_cap, int kv_div,
                    int ldq, int ldk, int ldv, int ldo, float scale, int dtype, void* stream);
int asr_logsoftmax_topk(const void* logits, float* vals, int32_t* ids, int R, int V, int ld,
                        int beam, int dtype, void* stream);
int asr_beam_step(const float* top_vals, const int32_t* top_ids, float* score, int32_t* alive,
                  int32_t* last_tok, int32_t* parent, int32_t* rec_tok, int32_t* rec_par,
                  int32_t* rec_end, float* rec_score, const int32_t* maxlen, int32_t* alive_total,
                  int B, int beam, int step, int eos, void* stream);
int asr_cache_gather(const void* src, void* dst, const int32_t* parent, int L, int R, int beam,
                     int Lcap, int n_pos, int row_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CTC prefix scoring for one-pass joint CTC / attention beam search (Watanabe et al. 2017, section 3.2 and algorithm 2).  NOT in
 * the reference (no CTC there).  Additive to ABI 10 (no version change).  The search (asr_chinese_e2e_amd/decode.py::
 * one_pass_beam_search) runs, per step, asr_logsoftmax_topk with k = C (the attention candidates), asr_ctc_prefix_score,
 * asr_joint_beam_step, then asr_ctc_prefix_gather beside asr_cache_gather.  R = B * beam hypotheses, slot r of utterance r / beam.
 *
 * asr_ctc_prefix_logprobs: lpT (B, V, T) f32 = log_softmax of each frame of logits ((B, T, V) `dtype`, rows `ld` apart), transposed.
 * asr_ctc_prefix_score: the state of hypothesis r is st_rb / st_rt (T, R) f64 (frame-major, element [t * R + r]): log r^b_t(g) (paths
 *   of frames 0..t whose collapse is g and that end in a blank) and log (r^n_t(g) + r^b_t(g)), for t < in_len[b]; hyp_psi (R) f32 =
 *   log psi(g).  At step 0 every hypothesis is [sos] (r^n = -inf, r^b_t = sum_{tau <= t} log y_tau(blank), psi = 0) and st_rb,
 *   st_rt, hyp_psi, last_tok are not read (may be NULL).  att_vals / att_ids (R, C): the attention candidates (beam <= C <= 16).
 *   Per (r, j), c = att_ids[r, j], h = g + c: cand_rb / cand_rt (T, R * C) f64, element [t * R * C + r * C + j], the state of h;
 *   log psi(h) = logsumexp_t (phi_{t-1} + log y_t(c)) with phi = r^b(g) + [c != last(g)] r^n(g), the t = 0 term only for g = [sos];
 *   c == eos: psi = log p_ctc(g) = log (r^n + r^b)_{in_len-1}(g); c == blank: -inf; h longer than the frames can spell: -inf.
 *   Joint score (1 - ctc_weight) * att + ctc_weight * (log psi(h) - log psi(g)), -inf for dead hypotheses (alive[r] == 0).
 *   Out (R, beam), per hypothesis best first (ties: lower j): out_vals the joint score, out_ids the token, out_att the attention
 *   log-probability, out_psi log psi(h), out_full log p_ctc(h) (the full-sequence probability; -inf for eos / blank).
 *   0 < ctc_weight <= 1.  fp64 log domain inside (the log1p(exp) correction in fp32).
 * asr_ctc_prefix_gather: for every r with alive[r] != 0, st_rb / st_rt[., r] = cand_rb / cand_rt[., p * C + j] where p = b * beam +
 *   parent[r] and j the candidate of p with token last_tok[r] (att_ids[p, j]; the ids of a row are distinct).
 * asr_joint_beam_step: asr_beam_step on the joint scores of asr_ctc_prefix_score (score + out_vals), with three differences:
 *   candidates of score -inf are dropped (an utterance whose every extension is -inf ends with no hypothesis); per slot
 *   att_score (sum of the attention log-probabilities) and ctc_score (log psi, or log p_ctc once ended) go along, with records
 *   rec_att / rec_ctc; a hypothesis that emits eos ends with it also at the last step (rec_end 1), every other survivor of the last
 *   step gets eos appended (rec_end 2) and its CTC part replaced by log p_ctc(h): score += ctc_weight * (full - psi).
 */
int asr_ctc_prefix_logprobs(const void* logits, float* lpT, int B, int T, int V, int ld, int dtype, void* stream);
int asr_ctc_prefix_score(const float* lpT, const int32_t* in_len, const double* st_rb, const double* st_rt, const float* hyp_psi,
                         const int32_t* last_tok, const int32_t* alive, const float* att_vals, const int32_t* att_ids, double* cand_rb,
                         double* cand_rt, float* out_vals, int32_t* out_ids, float* out_att, float* out_psi, float* out_full, int B, int T,
                         int V, int beam, int C, int step, float ctc_weight, int eos, int blank, void* stream);
int asr_ctc_prefix_gather(const double* cand_rb, const double* cand_rt, double* st_rb, double* st_rt, const int32_t* parent,
                          const int32_t* last_tok, const int32_t* alive, const int32_t* att_ids, const int32_t* in_len, int B, int T,
                          int beam, int C, void* stream);
int asr_joint_beam_step(const float* top_vals, const int32_t* top_ids, const float* top_att, const float* top_psi, const float* top_full,
                        float* score, float* att_score, float* ctc_score, int32_t* alive, int32_t* last_tok, int32_t* parent, int32_t* rec_tok,
                        int32_t* rec_par, int32_t* rec_end, float* rec_score, float* rec_att, float* rec_ctc, const int32_t* maxlen,
                        int32_t* alive_total, int B, int beam, int step, int eos, float ctc_weight, void* stream);

/* Character error rate per utterance on the device.
 * Replaces: calculate_cer (Predictor/Utils/score.py:4-13) over Vocab.convert_id2str strings
 *           (data_handler/vocab.py:75-79), called per step from cal_metrics
 *           (transformer_official.py:87-91) after a device-to-host copy of the greedy ids.
 * Convention kept: ids equal to pad_id are dropped, the token strings are joined by ONE space, the edit
 * distance runs over code points (spaces included) and is divided by (spaces in the reference string + 1).
 * hyp (B, Lh) ldh, ref (B, Lr) ldr: int32 ids; hyp_len / ref_len (B) or NULL = whole rows.
 * tok_cp: code points of all V token strings back to back; tok_off (V + 1): start of each;
 * max_tok_len: longest token string.  per_utt (B) f32 = distance / words of each utterance. */
int asr_cer(const int32_t* hyp, const int32_t* hyp_len, int Lh, int ldh, const int32_t* ref,
            const int32_t* ref_len, int Lr, int ldr, const int32_t* tok_cp, const int32_t* tok_off,
            int V, int max_tok_len, int pad_id, int B, float* per_utt, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Softmax cross-entropy with ignore_index, forward + gradient in one pass over the logits.
 * Replaces:  F.cross_entropy(pred, gold, ignore_index=0, reduction='mean')  Utils/loss.py:47-49
 *            (+ label smoothing branch Utils/loss.py:30-45 when smoothing > 0)
 * logits: (M, V) `dtype`; gold: (M) int32.  row_nll: (M) f32 per-row loss (0 for ignored rows).
 * dlogits (may alias logits, may be NULL) = grad_scale / n_valid * d(sum row_nll)/dlogits where
 * n_valid is read from device memory (*n_valid, f32, e.g. written by asr_dec_preprocess).
 * argmax_out (ABI 9; may be NULL): (M) int32, the greedy class of EVERY row (ignored ones included; first index on ties) - the ids of
 * cal_metrics' pred.topk(1) (transformer_official.py:87-91), taken by the pass that reads the row anyway (with dlogits aliasing logits
 * the logits are gone after the call).
 */
int asr_xent_fwd_bwd(const void* logits, const int32_t* gold, const float* n_valid,
                     float* row_nll, void* dlogits, int M, int V, int ignore_index,
                     float smoothing, float grad_scale, int32_t* argmax_out, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Decoder target preparation on device.
 * Replaces:  Decoder.preprocess (python list loop) transformer_official.py:260-275
 * tgt: (B, Lmax) int64 zero-padded label ids.  Writes (B, Lmax+1) int32:
 *   ys_in  = [sos, y..., eos-padding],  ys_out = [y..., eos, 0-padding]
 * dec_len[b] = 1 + #nonzero(tgt[b]) (rows of ys_in that are not eos padding),
 * lab_len[b] = #nonzero(tgt[b]), labels32 = compacted labels (B, Lmax) int32 (for CTC),
 * *n_valid = number of non-zero entries of ys_out (f32).
 * len_a / len_b (ABI 8, each may be NULL): (B) int64 length vectors of the batch contract (wave_len, tgt_len: collat.__call__
 * ai_shell_1.py:75-88 hands them over as int64) copied to len32_a / len32_b as the int32 the kernels take, in the same launch.
 */
int asr_dec_preprocess(const int64_t* tgt, int32_t* ys_in, int32_t* ys_out, int32_t* labels32,
                       int32_t* dec_len, int32_t* lab_len, float* n_valid, int B, int Lmax, int sos, int eos,
                       const int64_t* len_a, int32_t* len32_a, const int64_t* len_b, int32_t* len32_b, void* stream);

/* Embedding gather * scale + positional encoding.
 * Replaces:  tgt_word_emb(ys_in) * x_logit_scale + positional_encoding
 *              transformer_official.py:306-307
 * ids: (B*To) int32; emb: (V, d) f32 master embedding; pe: (>=To, d) f32; y: (B*To, d) `dtype`.
 * drop_p > 0: dropout on the output (transformer_official.py:306), mask as in asr_dropout_mask. */
int asr_embed_pe_fwd(const int32_t* ids, const void* emb, const float* pe, void* y, float scale,
                     int B, int To, int d, int V, float drop_p, uint32_t drop_seed, int dtype,
                     void* stream);
/* demb (V, d) f32 += scale * scatter-add over rows of ((dy + dy2) * keep / (1-p)) ((B*To, d) `dtype`; dy2 may be NULL: ABI 9 - the
 * gradient wrt the first decoder layer's input arrives as a (projection path, residual path) pair, added here in fp32). */
int asr_embed_bwd(const int32_t* ids, const void* dy, const void* dy2, float* demb, float scale, int rows, int d,
                  int V, float drop_p, uint32_t drop_seed, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Elementwise / reductions used between GEMMs.
 */
/* x = relu(x) in place, (n) `dtype`.  Replaces F.relu in module.py:70. */
int asr_relu_fwd(void* x, size_t n, int dtype, void* stream);
/* da = da * (a > 0) in place over (rows, cols); if dbias != NULL also dbias (cols) f32 +=
 * column sums of the masked da.  ws: asr_colsum_workspace_bytes(rows, cols). */
int asr_relu_bwd(void* da, const void* a, float* dbias, void* ws, size_t ws_bytes, int rows,
                 int cols, int dtype, void* stream);
/* out (cols) f32 (+)= column sums of x (rows, cols) with row stride ld elements. */
size_t asr_colsum_workspace_bytes(int rows, int cols);
int asr_colsum(const void* x, float* out, void* ws, size_t ws_bytes, int rows, int cols, int ld,
               int accumulate, int dtype, void* stream);
/* The first Tk of every T rows of a (B*T, d) `dtype` matrix and a compact (B*Tk, d) one (Tk <= T): the encoder frames the decoder's
 * cross-attention can see under the reference's text-length mask (transformer_official.py:78).
 *   asr_rows_gather:       dst (B*Tk, d) = src rows b*T + t, t < Tk
 *   asr_rows_scatter_add:  dst rows b*T + t += src (B*Tk, d) row b*Tk + t  (fp32 add, one rounding)
 * B*Tk == 0 is a no-op, and then src / dst may be NULL (empty allocations); T < Tk is refused. */
int asr_rows_gather(const void* src, void* dst, int B, int T, int Tk, int d, int dtype, void* stream);
int asr_rows_scatter_add(const void* src, void* dst, int B, int T, int Tk, int d, int dtype, void* stream);
/* dst (n) `dst_dtype` = src (n) `src_dtype`  (f32 <-> bf16 conversion / copy) */
int asr_cast(const void* src, void* dst, size_t n, int src_dtype, int dst_dtype, void* stream);
/* Transposed copies of many matrices that live in one flat bf16 buffer, one launch: for tile t,
 * tiles[6t..6t+5] = {element offset of its matrix in src, rows N, cols K, (tile row << 16) | tile col (64 x 64 tiles),
 * element offset of the copy in dst, row stride ldd >= N of the copy} (ABI 6: the copy has its own offset and stride, so that
 * the CTC head's W^T - rows of V = 4232 elements - can be padded to whole 128-byte lines);
 * dst[dst_off + k * ldd + n] = src[src_off + n * K + k].  Used for the W^T copies the input-gradient GEMMs
 * (dX = dY W as an NT product, replacing autograd's mm backward of nn.Linear, attention.py:43-59, module.py:70-71) read. */
int asr_transpose_batched_bf16(const void* src, void* dst, const int32_t* tiles, int ntiles, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused optimizer over the flat parameter / gradient buffers.
 * Replaces:  clip_grad_norm_(params, 5.0) ; NoamOpt.step() -> Adam.step()
 *              transformer_official.py:102-103, Trainer/optimizer.py:15-28, main.py:81-83
 * asr_grad_sumsq: *sumsq (f32) = sum g^2 over n f32 elements (ws: asr_sumsq_workspace_bytes(n)).
 * asr_noam_hyper:  step += 1 (device int32); hyper[0] = lr = factor * model_size^-0.5 *
 *   min(step^-0.5, step*warmup^-1.5) (or lr_const if warmup <= 0); hyper[1] = 1 - b1^step;
 *   hyper[2] = sqrt(1 - b2^step).
 * asr_adam_step: coef = min(1, max_norm / (sqrt(*sumsq) + 1e-6)) (no clipping if max_norm <= 0);
 *   g' = g*coef; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 *   p -= lr/bc1 * m / (sqrt(v)/bc2s + eps); if p_lp != NULL the bf16 shadow copy is refreshed.
 *   If write_clipped != 0 the clipped gradient is written back to g (clip_grad_norm_ is in-place).
 */
size_t asr_sumsq_workspace_bytes(size_t n);
int asr_grad_sumsq(const float* g, size_t n, float* sumsq, void* ws, size_t ws_bytes, void* stream);
int asr_noam_hyper(int32_t* step, float* hyper, float model_size, float warmup, float factor,
                   float lr_const, float b1, float b2, void* stream);
/* asr_grad_sumsq followed by asr_noam_hyper in two launches instead of three (ABI 8): the single-workgroup finalizer of the squared norm
 * also advances the device-side step counter and writes the step's hyper-parameters. */
int asr_grad_sumsq_noam(const float* g, size_t n, float* sumsq, void* ws, size_t ws_bytes, int32_t* step, float* hyper, float model_size,
                        float warmup, float factor, float lr_const, float b1, float b2, void* stream);
int asr_adam_step(float* p, float* g, float* m, float* v, void* p_lp, size_t n,
                  const float* hyper, const float* sumsq, float max_norm, float b1, float b2,
                  float eps, int write_clipped, void* stream);
/* Exponential moving average of the parameters (additive to ABI 10).  For optimizer step s >= 1 (the value asr_noam_hyper leaves in
 * hyper[3]), p the parameter AFTER that step's Adam update and e the average before the step:
 *
 *   d   = min(float64(float32(decay)), (1.0 + s) / (10.0 + s))   if warmup else float64(float32(decay))     float64
 *   omd = float32(1.0 - d)                                                                                  one rounding
 *   t   = float32(p - e);   u = float32(omd * t);   e' = float32(e + u)                                     three float32 roundings, no FMA
 *
 * decay lies in (0, 1); p == e is an exact fixed point; numpy float32 restates the three roundings bit for bit (tests/ema_ref.py),
 * and the kernels equal that restatement bit for bit.
 * asr_adam_ema_step: asr_adam_step (the same arithmetic, the same bits in p, g, m, v, p_lp) and the blend of the fresh p into ema (n f32)
 *   in the same pass, s read from hyper[3] on the device (graph-capturable).
 * asr_ema_update: the blend as a pass of its own with s = step given by the host (optimizers that do not run asr_adam_ema_step); p is only read.
 * Both refuse before any launch: null pointers, buffers that are not 16-byte aligned, decay not finite or outside (0, 1), step < 1. */
int asr_adam_ema_step(float* p, float* g, float* m, float* v, void* p_lp, size_t n,
                      const float* hyper, const float* sumsq, float max_norm, float b1, float b2,
                      float eps, int write_clipped, float* ema, float decay, int warmup, void* stream);
int asr_ema_update(const float* p, float* ema, size_t n, float decay, int warmup, float step, void* stream);
/* loss[0] = w_ce * sum(row_nll[0..M)) / *n_valid + w_ctc * sum(nll[0..B)) / B ;
 * loss[1] = the CE term, loss[2] = the CTC term (either input may be NULL with weight 0). */
int asr_loss_combine(const float* row_nll, int M, const float* n_valid, const float* nll, int B,
                     float w_ce, float w_ctc, float* loss, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense projections on MFMA:  C = act(A * W^T + bias)  ("NT": both operands K-contiguous).
 * Replaces:  nn.Linear / Conv1d(k=1) forward  attention.py:43-45, 59; module.py:70;
 *            transformer_official.py:176, 321  (and, with transposed operands, their dgrad).
 * A: (M, K) lda, W: (N, K) ldb, C: (M, N) ldc, all bf16; bias: (N) f32 or NULL;
 * if res != NULL, C += res (M, N) ldc (used to accumulate the residual gradient).
 */
int asr_gemm_nt_bf16(const void* A, const void* W, const float* bias, const void* res, void* C,
                     int M, int N, int K, int lda, int ldb, int ldc, int act, void* stream);
/* Small-M form of the projections (the decoder's B*To ~ 550 rows; transformer_official.py:446-458 through attention.py:43-59 and
 * module.py:70-71): 64 x 64 tiles, many short workgroups instead of a dozen long ones.
 *   trans_b = 0: C (M, N) = act(A (M, K) * Bm (N, K)^T + bias)        forward, Bm = the weight as stored
 *   trans_b = 1: C (M, N) = A (M, K) * Bm (K, N) (+ bias)             input gradient dx = dy W, Bm = the SAME weight (no transposed copy)
 * act: ASR_ACT_NONE / ASR_ACT_RELU / ASR_ACT_RELU_MASK (C = 0 where mask <= 0; mask (M, N) ldc bf16 = the activations of the ReLU whose
 * backward this is).  All bf16, fp32 accumulation; N, K, lda, ldb multiples of 8. */
int asr_gemm_small_bf16(const void* A, const void* Bm, const float* bias, const void* mask, void* C, int M, int N, int K,
                        int lda, int ldb, int ldc, int trans_b, int act, void* stream);
/* fp32 projections on the matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 FMA chains): every GEMM of the PARITY mode (dtype fp32),
 * which is what the tests compare with the reference's own CPU outputs - nn.Linear / Conv1d(k=1) forward, input gradient and weight
 * gradient of attention.py:43-45,59, module.py:70-71, transformer_official.py:176,321 - and the odd shapes the bf16 kernels refuse.
 *   C (M, N) ldc  (+)=  act( opA (M, K) * opB (K, N) + bias (N) )
 *   trans_a = 0: A stored (M, K) lda;  1: A stored (K, M) lda      trans_b = 0: B stored (K, N) ldb;  1: B stored (N, K) ldb
 *   forward y = x W^T + b: (0, 1);  input gradient dx = dy W: (0, 0);  weight gradient dW += dy^T x: (1, 0) with accumulate = 1.
 * act: ASR_ACT_NONE / ASR_ACT_RELU / ASR_ACT_RELU_MASK (C = 0 where mask <= 0; mask (M, N) ldc f32); accumulate != 0: C += result.
 * The reduction is never split across workgroups: results are deterministic (same bits every run) in either mode. */
int asr_gemm_f32(const float* A, const float* B, const float* bias, const float* mask, float* C, int M, int N, int K,
                 int lda, int ldb, int ldc, int trans_a, int trans_b, int act, int accumulate, void* stream);
/* Weight gradient  dW (N, K) f32 (+)= dY^T (M, N)^T * X (M, K)   ("TN": reduction over rows).
 * ws: NULL / 0 in the default mode; in deterministic mode a 16-byte aligned buffer of
 * asr_gemm_tn_workspace_bytes(M, N, K) bytes (partial slabs, one per M-split). */
size_t asr_gemm_tn_workspace_bytes(int M, int N, int K);
int asr_gemm_tn_bf16(const void* dY, const void* X, float* dW, int M, int N, int K, int ldy,
                     int ldx, int ldw, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* The same, and dbias (N) f32 += column sums of dY (the bias gradient of the projection), taken
 * from the dY tiles the kernel stages anyway - no separate pass over dY.  dbias == NULL: as above. */
int asr_gemm_tn_bias_bf16(const void* dY, const void* X, float* dW, float* dbias, int M, int N, int K,
                          int ldy, int ldx, int ldw, int accumulate, void* ws, size_t ws_bytes,
                          void* stream);
/* Grouped form: nprob (<= 8) independent weight gradients dW_p (+)= dY_p^T X_p (+ bias gradients
 * where dbias != NULL) in ONE launch - e.g. all projections of a Transformer layer, whose
 * autograd weight-gradient GEMMs the reference runs one by one (torch.autograd through
 * attention.py:43-59, module.py:70-71).  Together the problems fill the GPU with larger tiles and
 * fewer splits of the M = B*T reduction than each would alone.  `probs` is a HOST array, read
 * during the call.  Per problem: dY (M, N) ldy, X (M, K) ldx bf16; dW (N, K) ldw f32.
 * Round 5: up to four problems over the SAME M >= 4096 rows whose 128 x 128 tiles fill the device with a few M-splits (the two projections
 * of a feed-forward or attention block: 64 tiles x 4 splits) run on the tile code of asr_gemm_tn_bias_bf16 in one launch - every workgroup
 * of either form ends by adding its fp32 tile to memory with atomics, so one launch for two problems halves that traffic; other groups
 * (different M per problem: a decoder layer's) take the 256 x 128-tile kernel as before. */
typedef struct asr_tn_problem {
    const void* dY;
    const void* X;
    float* dW;
    float* dbias;
    int M, N, K, ldy, ldx, ldw;
} asr_tn_problem;
int asr_gemm_tn_grouped_bf16(const asr_tn_problem* probs, int nprob, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One decoder layer as ONE host call: the fixed launch sequence of DecoderLayer.forward (transformer_official.py:446-458: self-attention,
 * encoder-decoder attention, position-wise FFN; each with post-LayerNorm and pad zeroing, attention.py:33-62, module.py:68-75) and of
 * autograd through it, issued from C++ on caller-owned buffers.  The decoder's ~23 kernels per layer and direction take 4 - 13 us each on
 * its B*To ~ 550 rows: with one foreign call per kernel from Python the host paced that part of the joint step.  Same kernels, same order,
 * same results as calling asr_gemm_small_bf16 / asr_sdpa_* / asr_add_ln_* / asr_gemm_nt_bf16 one by one.  bf16 activations only
 * (M = B*To rows; d, H*dk, ff multiples of 8).  All pointers are device pointers unless stated; the struct itself is HOST memory, read
 * during the call.  Not included (they stay with the caller): weight-gradient GEMMs (the dY / X operands are the buffers below), the
 * reduction of the LayerNorm parameter-gradient partial sums left in part_* (asr_add_ln_bwd_reduce_batched), data-parallel marks. */
typedef struct asr_dec_layer_plan {
    int B, To, T, d, H, dk, ff;           /* utterances, target positions, encoder frames per utterance, model width, heads, head dim, FFN width */
    float drop_p;                          /* dropout of every site of the layer (0 = off) */
    uint32_t seed[5];                      /* per-step mask seeds: self-attn probabilities, after self fc, cross-attn probabilities, after cross fc, after w_2 */
    int ld_kv_c_T;                         /* row stride (elements) of w_kv_c_T */
    const int32_t* dec_len;                /* (B) valid target positions (self-attention keys, pad zeroing) */
    const int32_t* cross_len;              /* (B) visible encoder frames of the encoder-decoder attention */
    /* parameters: bf16 weights as stored (out, in), f32 biases and LayerNorm gains / biases */
    const void *w_qkv_s, *w_fc_s, *w_q_c, *w_fc_c, *w_1, *w_2;
    const float *b_qkv_s, *b_fc_s, *b_q_c, *b_fc_c, *b_1, *b_2;
    const float *g_s, *be_s, *g_c, *be_c, *g_f, *be_f;
    const void* w_kv_c_T;                  /* (d, 2 H dk) bf16: transposed K|V projection weight of the cross attention (backward; may be NULL) */
    /* forward: input, then every activation the backward pass needs */
    const void* x_in;                      /* (M, d) layer input */
    void *qkv_s, *ctx_s, *a_s, *y_s;       /* (M, 3 H dk), (M, H dk), (M, d) = fc output then xhat, (M, d) block output */
    float *lse_s, *rstd_s;                 /* (B, H, To), (M) */
    void* q_c;                             /* (M, H dk) */
    const void* kv_c;                      /* (B*T, 2 H dk) K|V of the encoder frames, projected by the caller (row stride ld_kv_c) */
    void* kv_ready_event;                  /* hipEvent_t after which kv_c is complete, or NULL (HOST handle) */
    void *ctx_c, *a_c, *y_c;
    float *lse_c, *rstd_c;
    void *h, *o, *y_f;                     /* (M, ff) ReLU output, (M, d) w_2 output then xhat, (M, d) layer output */
    float* rstd_f;
    /* backward: gradients wrt activations (bf16), bias gradients (f32, accumulated), scratch */
    void *dz_f, *g_o, *g_h, *dx_f;         /* residual gradient of the FFN block, dY of w_2 (only with dropout, else dz_f is it), dY of w_1, dX of w_1 */
    void *dz_c, *g_ac, *g_qc, *g_kvc, *dx_c;   /* cross block: residual gradient, dY of fc (dropout only), dY of the Q projection (M, H dk), dY of K|V (B*T, 2 H dk), dX of Q */
    void *dz_s, *g_as, *g_qkv, *dx_s;      /* self block: residual gradient, dY of fc (dropout only), dY of Q|K|V (M, 3 H dk), dX of Q|K|V */
    void* dctx;                            /* (M, H dk) scratch: gradient wrt an attention output */
    float *gb_2, *gb_fc_c, *gb_fc_s;       /* bias gradients of w_2 and the two out-projections: come out of the LayerNorm backward (partial sums) */
    void *part_f, *part_c, *part_s;        /* asr_add_ln_bwd_workspace_bytes(M, d) bytes each: partial sums of the LayerNorm parameter gradients */
    float* delta;                          /* scratch of asr_sdpa_bwd */
    size_t delta_bytes;
    void* d_enc;                           /* (B*T, d) bf16 gradient wrt the encoder output, accumulated in place (or NULL) */
    void* wgrad_stream;                    /* backward (ABI 7): stream that will run the layer's weight gradients, or NULL.  The LAST kernel of
                                              asr_decoder_layer_bwd then hands over to it by its own completion event (asr_stream_arm): check
                                              asr_stream_arm_pending() afterwards and fall back to asr_stream_fork when it returns 1 */
    int aux_cus;                           /* backward (ABI 8): > 0 = the (B*T)-row GEMM d_enc += g_kvc W_kv that the layer puts on aux_stream is
                                              sized for this many CUs (tuning option "cu_limit" around that one launch), so that the rest stay free
                                              for the layer's own chain of small kernels; 0 = the whole device */
    /* ABI 9: the K | V projections of ALL decoder layers read the same encoder output (transformer_official.py:309-314, 446-458): the caller may
     * keep them - and the gradients wrt them - side by side in one (B*T, L 2 H dk) buffer and run the encoder-output gradient once per GROUP of
     * layers with the reduction over the group's columns, instead of one read-modify-write of d_enc per layer. */
    int ld_kv_c;                           /* row stride (elements) of kv_c and g_kvc; 0 = 2 H dk (a buffer per layer) */
    int kv_dgrad_cols;                     /* 0: d_enc += g_kvc W_kv over this layer's 2 H dk columns (as before).  > 0: this layer is the LAST of a
                                              group to run its backward pass: d_enc += g_kv_group W_group over kv_dgrad_cols columns, with g_kv_group
                                              (B*T, kv_dgrad_cols) at row stride ld_kv_c and w_kv_c_T = the group's (d, kv_dgrad_cols) slice of the
                                              transposed weight; the other layers of the group pass d_enc = NULL */
    const void* g_kv_group;
    /* ABI 10: the low-order pieces of the two attention outputs (asr_sdpa_fwd's o_lo), (M, H dk) each, or NULL */
    void *ctx_s_lo, *ctx_c_lo;
    /* Compact key rows (still ABI 10, fields appended): when the cross-attention sees only the first T frames of each utterance (T <= T_enc;
     * the reference's mask from text lengths, transformer_official.py:78), kv_c / g_kvc hold the K | V of those B*T rows only.  g_enc_x
     * != NULL: the encoder-output gradient becomes g_enc_x (B*T, d) = g_kv_group W_group on the small-M kernel, with w_kv_c = the group's
     * (kv_dgrad_cols, d) rows of the K|V weight AS STORED, then d_enc (B*T_enc, d) += g_enc_x scattered into rows t < T of each utterance
     * (asr_rows_scatter_add); w_kv_c_T is not read.  g_enc_x == NULL: d_enc += ... over all B*T rows as above. */
    const void* w_kv_c;
    void* g_enc_x;
    int T_enc;                             /* encoder frames per utterance of d_enc (row stride of its utterances); read only with g_enc_x */
} asr_dec_layer_plan;
int asr_decoder_layer_fwd(const asr_dec_layer_plan* plan, void* stream);
/* (dy, dy2): gradient wrt y_f (dy2 may be NULL; the two are added).  Results: plan->dx_s and plan->dz_s = gradient wrt x_in through the
 * projections and along the residual path (to be added by the consumer).  aux_stream: stream for d_enc += g_kvc W_kv (forked behind
 * `stream`), or NULL = on `stream`. */
int asr_decoder_layer_bwd(const asr_dec_layer_plan* plan, const void* dy, const void* dy2, void* stream, void* aux_stream);

/* ---------------------------------------------------------------------------------------------
 * Log-mel front end on device.
 * Replaces:  MelSpectrogram(sr=16000, ws=400, hop=160, n_mels) -> log(x+1e-20)
 *              Predictor/data_handler/processor.py:33-40
 *            (f - mean)/std (scalar, unbiased) and build_LFR_features   processor.py:42-46, 74-100
 * wav: (B, Smax) f32, wav_len: (B) int32 samples, taken as min(max(wav_len[b], 0), Smax): a length past the row
 * never reads the next row.  feat: (B, Tmax, n_mels) f32 log-mel: utterance b has T_b = min(1 + wav_len[b]/160, Tmax)
 * frames (none for wav_len[b] = 0; a smaller Tmax truncates), frames t >= T_b are written as 0.  Frame t, tap n reads
 * sample i = 160 t - 200 + n; i < 0 -> -i; i >= len -> 2 (len - 1) - i; then clamped to [0, len - 1]: reflect padding
 * for len > 200, the same rule for shorter utterances, which reflect padding does not define.
 * melfb: (201, n_mels) f32 filterbank; window: (400) f32.
 * The normalisation entry points below are not given Smax: their frame count is min(1 + wav_len[b]/160, Tmax), 0 for
 * wav_len[b] <= 0, so they stay inside feat whatever the length says.
 *
 * One kernel and one tile.  asr_logmel_fwd, asr_fbank_fwd and their streaming forms run one frame tile (DFT, power,
 * filterbank, log), instantiated per front end behind its own frame preparation.  The six normalise-augment-stack entry
 * points - asr_utt_norm_lfr_fwd, asr_utt_norm_augment_lfr_fwd, asr_global_norm_augment_lfr_fwd, asr_utt_norm_specaug_lfr_fwd,
 * asr_global_norm_specaug_lfr_fwd here and below - launch one kernel (utterance or global normalisation x reference masks or
 * policy row x f32 or bf16) through one launcher, so they refuse the same things in the same order: ASR_EINVAL for a null
 * pointer, then for a shape (B, Tmax, n_mels, m, n, Tlfr_max < 1, or B > 65535), then for Tlfr_max * m * n_mels > INT32_MAX,
 * then for a policy's row arguments; ASR_EDTYPE for a dtype other than f32 / bf16; nothing is launched after a refusal.
 * Two of these refusals are newer than ABI 10's first release, both of calls that could not work: the utterance entry
 * points used to let Tlfr_max * m * n_mels overflow an int inside the kernel, and they did not refuse B > 65535 (utterances
 * are now the grid's y dimension on every path).
 */
int asr_logmel_fwd(const float* wav, const int32_t* wav_len, const float* window,
                   const float* melfb, float* feat, int B, int Smax, int Tmax, int n_mels,
                   void* stream);
/* out: (B, Tlfr_max, m*n_mels) `dtype`, out_len[b] = ceil(T_b / n); padded rows 0. */
int asr_utt_norm_lfr_fwd(const float* feat, const int32_t* wav_len, void* out, int32_t* out_len,
                         int B, int Tmax, int n_mels, int m, int n, int Tlfr_max, int dtype,
                         void* stream);
/* The same with SpecAugment between normalisation and frame stacking, as AudioParser.parse(augment=
 * True) does (processor.py:52-58, 67-69; augments.py:4-42): masks (B, 4) int32 = [t0, t1, f0, f1]
 * per utterance (frames / mel channels of the un-stacked feature, host RNG); frames [t0, t1) are
 * filled with the mean of the normalised feature, then channels [f0, f1) with the mean of the
 * time-masked feature.  masks == NULL: no augmentation. */
int asr_utt_norm_augment_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* masks,
                                 void* out, int32_t* out_len, int B, int Tmax, int n_mels, int m,
                                 int n, int Tlfr_max, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Speed perturbation of a waveform batch (the 0.9 / 1.0 / 1.1 augmentation of the AISHELL-1 recipes), in front of
 * asr_logmel_fwd.
 * Stands in for:  sox / Kaldi `speed` (resampling by p/q, pitch and tempo together).  The reference has no
 *                 waveform-side augmentation: parity unpinned by the reference; the definition (Hann-windowed sinc,
 *                 width 6, roll-off 0.99, as torchaudio's resampler) is restated in float64 in tests/speed_ref.py.
 * wav: (B, Smax) f32, wav_len: (B) int32 samples, factor: (B) int32 index f into pq / taps.  pq: (F, 2) int32 = (p, q)
 * of factor p/q, 1 <= p <= 20, 1 <= q <= qmax <= 20; taps: (F, qmax, ntaps) f32, ntaps = 2 W + 1 odd,
 * taps[f][r][j + W] = h(r/q - j) for r < q, every unused entry 0 (narrower filters are centred).  Per utterance
 *   n_out = ceil(wav_len q / p),   out[b, n] = sum_j wav[b, (n p)/q + j] taps[f][(n p) % q][j + W]   (wav = 0 outside
 * [0, wav_len)),   out[b, n] = 0 for n_out <= n < Smax_out,   out_len[b] = n_out (never more than Smax_out: pass Smax_out
 * >= every n_out).  p == q: out[b, :wav_len] = wav[b, :wav_len] bit for bit, the table is not read.  A factor index
 * outside [0, F) is clamped; a (p, q) outside the ranges above is taken as factor 1.  All index arithmetic is exact
 * (64 bits where n p can pass 2^31).  out must not alias wav.  16-byte loads and stores are used where wav / out are
 * 16-byte aligned; any Smax / Smax_out is accepted.
 */
#define ASR_SPEED_TILE 1024      /* output samples per workgroup (tests cover the tile edges) */
int asr_speed_perturb_fwd(const float* wav, const int32_t* wav_len, const int32_t* factor, const int32_t* pq,
                          const float* taps, float* out, int32_t* out_len, int B, int Smax, int Smax_out, int F,
                          int qmax, int ntaps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sample-rate conversion of a waveform batch to 16 kHz, in front of asr_speed_perturb_fwd and everything behind it.
 * Stands in for:  the "kaiser_best" resamplers of the common toolkits (Kaiser-windowed sinc, 64 zero crossings, roll-off
 *                 0.9476, beta 14.77).  The reference has no resampler: parity unpinned by the reference; the definition is
 *                 in data_handler/resample.py and restated in float64 in tests/resample_ref.py.
 * wav: (B, Smax) f32.  rate_idx: (B) int32 index r into the plans; outside [0, R) (16 kHz itself) the row is copied.
 * pq: (R, 2) int32 = (p, q), source rate = 16000 p / q in lowest terms, q <= ASR_RESAMPLE_Q_MAX; tap_off: (R + 1) int32,
 * ascending; taps: taps_len f32, plan r at taps[tap_off[r] : tap_off[r + 1]] as T[j][m], j < ntaps = 2 W + 1 <=
 * ASR_RESAMPLE_NTAPS_MAX (odd), m < q, T[j][n mod q] = h((n p mod q) / q - (j - W)) - the phase table in the order the
 * kernel reads it.  A plan outside these ranges, or with p == q, is taken as a copy.  R <= ASR_RESAMPLE_PLANS_MAX.
 * win: (B, 5) int32 = {in_base, n_avail, n_total, out_start, n_emit} per utterance: the row holds samples
 * [in_base, in_base + n_avail) of an utterance of n_total samples (in_base may be negative; x[k] = 0 for k < 0, k >= n_total
 * and outside the row), and
 *   out[b, t] = y[out_start + t] = sum_{j = -W .. W} x[((out_start + t) p) / q + j] T[j + W][(out_start + t) mod q]
 * for t < n_emit, exact zeros for n_emit <= t < Smax_out, out_len[b] = n_emit (clamped to Smax_out).  Offline: {0, n_in,
 * n_in, 0, ceil(n_in q / p)}.  Per output acc = 0, then acc = fmaf(x, T, acc) for j ascending, one accumulator: the bits
 * do not depend on the window, so a stream cut anywhere reproduces the offline call.  Index arithmetic is exact (64 bits
 * once per workgroup).  out must not alias wav.  16-byte accesses are used where wav / out are 16-byte aligned; any Smax /
 * Smax_out is accepted.  No atomics, no workspace.
 */
#define ASR_RESAMPLE_TILE 1024        /* output samples per workgroup (tests cover the tile edges) */
#define ASR_RESAMPLE_Q_MAX 640
#define ASR_RESAMPLE_NTAPS_MAX 1023
#define ASR_RESAMPLE_PLANS_MAX 16
int asr_resample_fwd(const float* wav, const int32_t* rate_idx, const int32_t* win, const int32_t* pq,
                     const int32_t* tap_off, const float* taps, float* out, int32_t* out_len, int B, int Smax,
                     int Smax_out, int R, int taps_len, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reverberation and additive noise of a waveform batch (the other two waveform-side augmentations of the Kaldi / WeNet /
 * ESPnet recipes), behind asr_speed_perturb_fwd and in front of asr_logmel_fwd: first the room, then the noise.
 * Stands in for:  Kaldi steps/data/reverberate_data_dir.py (wav-reverberate --shift-output) / WeNet add_reverb and
 *                 add_noise.  The reference has no waveform-side augmentation: parity unpinned by the reference; both
 *                 definitions are restated in float64 in tests/noise_ref.py.
 *
 * asr_reverb_fwd: wav, out (B, Smax) f32 (out must not alias wav), wav_len (B) int32, rir_idx (B) int32, rir (R, Lcap)
 * f32 with rir_len, rir_peak (R) int32; 1 <= Lcap <= ASR_REVERB_MAX_TAPS.  Per utterance r = rir_idx[b],
 * L = clamp(rir_len[r], 1, Lcap), p = clamp(rir_peak[r], 0, L - 1), len = clamp(wav_len[b], 0, Smax) and
 *   out[b, n] = sum_{k < L} rir[r][k] x[n + p - k]   for n < len (x = wav[b], 0 outside [0, len)),   out[b, n] = 0 for
 * len <= n < Smax: the length does not change and the direct path (the response's peak) stays where it was, so
 * lengths and labels are untouched.  r outside [0, R): out[b, :len] = wav[b, :len] bit for bit, the bank is not read.
 * fp32 accumulation; the order of the sum is the kernel's.  16-byte accesses are used only where wav and out are
 * 16-byte aligned; any Smax is accepted.
 *
 * asr_noise_mix_fwd: par (B, 4) int32 = {clip index j, start offset o, scale as fp32 bits, 0} with scale =
 * 10^(-snr_dB / 20) computed by the host.  noise: all clips in one f32 buffer, clip j at [noise_off[j], noise_off[j + 1])
 * (noise_off: N + 1 int32, ascending, inside the buffer: the host's responsibility).  With nlen the clip's length,
 *   v[n] = noise[noise_off[j] + (o + n) mod nlen]   (the clip wraps as often as needed; exact for o + n up to 2^31),
 *   Ex = sum_{n < len} x[n]^2,   Ev = sum_{n < len} v[n]^2   (fp64 sums of fp64 products, per-tile partials in ws added in
 *   tile order: no atomics, the same input gives the same bits),   g = scale sqrt(Ex / Ev) in fp64, rounded once to fp32,
 *   out[b, n] = x[n] + g v[n] for n < len, 0 for len <= n < Smax;   gain_out[b] = g (gain_out may be NULL).
 * j outside [0, N), nlen <= 0, len = 0, Ex = 0 or Ev = 0: out[b, :len] = wav[b, :len] bit for bit and g = 0.  out may
 * alias wav.  ws: asr_noise_mix_workspace_bytes(B, Smax) bytes, 8-byte aligned.
 */
#define ASR_REVERB_TILE 1024         /* output samples per workgroup (tests cover the tile edges) */
#define ASR_REVERB_CHUNK 256         /* taps per staged pass over the input (tests cover the chunk edges) */
#define ASR_REVERB_MAX_TAPS 8192
#define ASR_NOISE_MIX_TILE 4096      /* samples per workgroup and energy partial of asr_noise_mix_fwd (tests cover the tile edges) */
int asr_reverb_fwd(const float* wav, const int32_t* wav_len, const int32_t* rir_idx, const float* rir,
                   const int32_t* rir_len, const int32_t* rir_peak, float* out, int B, int Smax, int R, int Lcap,
                   void* stream);
size_t asr_noise_mix_workspace_bytes(int B, int Smax);
int asr_noise_mix_fwd(const float* wav, const int32_t* wav_len, const int32_t* par, const float* noise,
                      const int32_t* noise_off, float* out, float* gain_out, void* ws, size_t ws_bytes, int B, int Smax,
                      int N, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reverberation with long responses: the definition of asr_reverb_fwd (same arguments, same clamping of len, L and p, same
 * copies for r outside [0, R), zeros from len on, out must not alias wav, any Smax and any alignment of wav / out, nothing
 * at or beyond rir_len[r] is read), evaluated as a uniformly partitioned overlap-save convolution with transforms of
 * ASR_REVERB_FFT_N points, for 1 <= Lcap <= ASR_REVERB_FFT_MAX_TAPS.  With Bk = ASR_REVERB_FFT_N / 2, window j of an utterance
 * x[(j - 1) Bk, (j + 1) Bk) and partition q of its response h[q Bk, (q + 1) Bk):
 *   full[i Bk, (i + 1) Bk) = last Bk samples of IFFT(sum_{q < P_b, q <= i} FFT(partition q) FFT(window i - q)),
 *   out[b, m - p] = full[m],   P_b = ceil(L / Bk) per utterance (a short response does not pay for the bank's longest).
 * fp32 throughout, the products summed over q in ascending order, no atomics: the same input gives the same bits.  The
 * rounding error scales with S_i = sum_q ||partition q||_2 ||window i - q||_2 per output block (tests/reverb_fft_ref.py).
 * twiddle: ASR_REVERB_FFT_N pairs (cos, -sin)(2 pi t / ASR_REVERB_FFT_N), t = 0 .. N - 1, computed in float64 and rounded
 * once (kernels.reverb_fft_twiddle), 8-byte aligned.
 * ws: asr_reverb_fft_workspace_bytes(B, Smax, Lcap) bytes, 16-byte aligned; need not be initialised:
 *   B * (ceil(Smax / Bk) + 1 + ceil(Lcap / Bk)) * Bk * 8
 * - the spectra (Bk complex words each) of the ceil(Smax / Bk) + 1 windows of every utterance and of the ceil(Lcap / Bk)
 * partitions of the response it drew; spectra are computed per batch, never kept for the bank.  0 for B, Smax or Lcap < 1.
 */
#define ASR_REVERB_FFT_N 4096             /* transform points; N / 2 = 2048 new samples per block */
#define ASR_REVERB_FFT_MAX_TAPS 65536     /* 32 partitions of 2048 taps */
size_t asr_reverb_fft_workspace_bytes(int B, int Smax, int Lcap);
int asr_reverb_fft_fwd(const float* wav, const int32_t* wav_len, const int32_t* rir_idx, const float* rir,
                       const int32_t* rir_len, const int32_t* rir_peak, const float* twiddle, float* out, void* ws,
                       size_t ws_bytes, int B, int Smax, int R, int Lcap, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Global CMVN: one mean and one inverse standard deviation per mel bin, fixed for a corpus (WeNet / ESPnet / Kaldi
 * global_cmvn), as the alternative to the per-utterance scalar normalisation above - the one that can stream.
 * Stands in for:  nothing in the reference (it has no global CMVN): parity unpinned by the reference; the definition is
 *                 restated in float64 in tests/cmvn_ref.py.
 *
 * asr_cmvn_accumulate: feat (B, Tmax, n_mels) f32 as asr_logmel_fwd writes it.  acc: 2 n_mels + 1 doubles that persist
 * across calls (zero them once): acc[m] += sum x, acc[n_mels + m] += sum x^2 over every valid frame (t < Tb,
 * Tb = min(1 + wav_len / 160, Tmax), 0 for wav_len = 0), acc[2 n_mels] += the number of such frames.  n_mels <= 256.
 * The host then takes mean = sum / N, var = sumsq / N - mean^2 (population variance), istd = 1 / sqrt(max(var, 1e-20)).
 *
 * asr_global_norm_augment_lfr_fwd: asr_utt_norm_augment_lfr_fwd with (x - mean[bin]) * istd[bin] - one fp32
 * subtraction, one fp32 multiplication - in place of the utterance's scalar statistics; mean, istd: (n_mels) f32.
 * Same masks (may be NULL: then no reduction runs at all), same stacking rule, same outputs.
 */
int asr_cmvn_accumulate(const float* feat, const int32_t* wav_len, double* acc, int B, int Tmax, int n_mels,
                        void* stream);
int asr_global_norm_augment_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* masks,
                                    const float* mean, const float* istd, void* out, int32_t* out_len, int B,
                                    int Tmax, int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SpecAugment policies: several time and mel masks with zero fill, a linear time warp and spectral substitution, between
 * normalisation and frame stacking.  Additive to ABI 10; the augment entry points above are untouched.
 * Stands in for:  the masking of the WeNet / ESPnet AISHELL recipes (spec_aug, spec_sub, time_warp).  The reference has one
 *                 mask per axis with mean fill (the augment entry points): parity unpinned by the reference; the definition,
 *                 in Python integers and numpy float32, is tests/specaug_ref.py, and the outputs equal it bit for bit.
 *
 * asr_utt_norm_specaug_lfr_fwd / asr_global_norm_specaug_lfr_fwd: the arguments of asr_utt_norm_augment_lfr_fwd /
 * asr_global_norm_augment_lfr_fwd with `masks` replaced by
 *   ranges: (B, ld) int32, rows ld >= 2 + 2 n_t + 2 n_f + 3 n_s words apart; never NULL.  Row b, for the T_b frames and
 *           n_mels bins of utterance b (un-stacked frames, resolved on the host: data_handler/specaug.py):
 *             [wc, ww | (t0, t1) x n_t | (f0, f1) x n_f | (s, e, p) x n_s]
 *   n_t, n_f, n_s: 0 .. ASR_SPECAUG_MAX_RANGES each.
 * The kernels clamp a row before use - t0 into [0, T_b], t1 into [t0, T_b]; f likewise against n_mels; s into [0, T_b], e into
 * [s, T_b], p into [0, s]; the warp is on iff 0 < wc < T_b and 0 < ww < T_b - so no row reaches outside its utterance.
 * With x the normalised frames (for the utterance normalisation: the statistics of the un-augmented frames), output frame t,
 * bin f is
 *   1. u = t - p_i for the last i with s_i <= t < e_i, else u = t           (substitution: reads augmented frames, never chains)
 *   2. +0.0f if u lies in a [t0, t1) or f in a [f0, f1)                     (zero is the mean under both normalisations)
 *   3. x[u][f] without a warp; with it, output frames [0, ww) resample input frames [0, wc) and [ww, T_b) resample [wc, T_b):
 *      (o, n_out, base, n_in) = (u, ww, 0, wc) or (u - ww, T_b - ww, wc, T_b - wc); in 64-bit integers num =
 *      max((2 o + 1) n_in - n_out, 0), den = 2 n_out, i0 = num / den, i1 = min(i0 + 1, n_in - 1), w = f32(num % den) / f32(den),
 *      value = v0 + w * (v1 - v0) with v = x[base + i][f]: one fp32 division, subtraction, multiplication and addition, each
 *      rounded on its own (never contracted).
 * Frame stacking, out and out_len as the augment entry points (the same kernel); an all-zero row gives the bits of the call
 * without masks.  No reduction runs for the augmentation: the global variant keeps the tiled grid of the no-mask call.
 * ASR_EINVAL before any launch: a null pointer, n_* outside 0 .. 8, ld too small, the shared shape checks (asr_logmel_fwd above).
 */
#define ASR_SPECAUG_MAX_RANGES 8
int asr_utt_norm_specaug_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* ranges, int ld, int n_t, int n_f,
                                 int n_s, void* out, int32_t* out_len, int B, int Tmax, int n_mels, int m, int n,
                                 int Tlfr_max, int dtype, void* stream);
int asr_global_norm_specaug_lfr_fwd(const float* feat, const int32_t* wav_len, const int32_t* ranges, int ld, int n_t, int n_f,
                                    int n_s, const float* mean, const float* istd, void* out, int32_t* out_len, int B,
                                    int Tmax, int n_mels, int m, int n, int Tlfr_max, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Streaming front end: samples in, encoder chunks out, with the state on the device and the counters on the host.
 * Each utterance owns a ring of its most recent samples, wav_ring (B, scap) f32 with sample s at [b][s & (scap - 1)],
 * and a ring of its most recent log-mel frames, feat_ring (B, fcap, n_mels) f32 with frame t at [b][t & (fcap - 1)];
 * scap and fcap are powers of two, and the host asks only for what the rings still hold.  Every `par` is a small int32
 * device array the host fills per call.  ASR_STREAM_OPEN stands for "length not known yet".
 *
 * asr_stream_append:   par (B, 2) = {received, n_new}: pcm[b][pcm_off .. pcm_off + n_new) becomes samples
 *                      received .. received + n_new - 1 of utterance b.  pcm (B, S) f32; n_new <= max_new <= scap.
 * asr_stream_logmel:   par (B, 3) = {t_begin, n_new, total}: frames t_begin .. t_begin + n_new - 1 (n_new <= max_new <=
 *                      fcap) computed by the tile body of asr_logmel_fwd - bit for bit the frames it gives for the
 *                      whole utterance.  total = the length in samples of a closed utterance (reflection and clamping at
 *                      the end as offline), ASR_STREAM_OPEN otherwise; the ring must hold samples
 *                      max(0, 160 t_begin - 200) .. the last one the frames touch.
 * asr_stream_norm_lfr: par (B, 3) = {r_begin, n_rows, Tb}: LFR rows r_begin .. r_begin + n_rows - 1 (n_rows <= C) under
 *                      global CMVN, by the source rule and the expression asr_global_norm_augment_lfr_fwd's kernel uses
 *                      (neither is written twice), into out (B, C, m n_mels) f32 or
 *                      bf16; rows past n_rows are zero.  Tb = the frame count of a closed utterance (tail rows repeat
 *                      frame Tb - 1), ASR_STREAM_OPEN otherwise.
 */
#define ASR_STREAM_OPEN 0x3fffffff
int asr_stream_append(const float* pcm, const int32_t* par, float* wav_ring, int B, int S, int pcm_off, int max_new,
                      int scap, void* stream);
int asr_stream_logmel(const float* wav_ring, const int32_t* par, const float* window, const float* melfb,
                      float* feat_ring, int B, int max_new, int scap, int fcap, int n_mels, void* stream);
int asr_stream_norm_lfr(const float* feat_ring, const int32_t* par, const float* mean, const float* istd, void* out,
                        int B, int C, int fcap, int n_mels, int m, int n, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kaldi fbank front end: the features of compute-fbank-feats / torchaudio.compliance.kaldi.fbank / kaldi-native-fbank
 * with WeNet's settings (25 ms / 10 ms at 16 kHz, dither 0, snip_edges, remove_dc_offset, Povey window, no energy column),
 * as the alternative to asr_logmel_fwd.
 * Stands in for:  nothing in the reference (its features are asr_logmel_fwd's): parity unpinned by Kaldi's binaries;
 *                 the definition is restated in float64 in tests/fbank_ref.py.
 *
 * asr_fbank_fwd: wav (B, Smax) f32, wav_len (B) int32 samples, taken as min(max(wav_len[b], 0), Smax).  Utterance b has
 * T_b = min(1 + (len - 400) / 160, Tmax) frames, none for len < 400 (a smaller Tmax truncates); frame t is samples
 * 160 t .. 160 t + 399 and nothing else: no padding at either end, trailing samples that fill no frame are dropped.
 * Per frame: x = wav_scale * sample; subtract the frame's mean; y[n] = x[n] - preemph x[n - 1] (y[0] = x[0] - preemph x[0]);
 * times window[n]; zero-padded 512-point power spectrum, bins 0 .. 255; feat = log(max(power x melfb, FLT_EPSILON)).
 * feat: (B, Tmax, n_mels) f32, frames t >= T_b written as 0.  window: (400) f32; melfb: (256, n_mels) f32.
 * A frame's bits depend on its 400 samples only, not on the batch, tile or row it is computed in.
 * The normalisation entry points above count frames as 1 + wav_len / 160: hand them 160 (T_b - 1) + 1 (0 for T_b = 0).
 *
 * asr_stream_fbank: the streaming twin on the rings of the streaming front end above.  par (B, 2) = {t_begin, n_new}: frames
 * t_begin .. t_begin + n_new - 1 (n_new <= max_new <= fcap) by the same tile body - bit for bit the offline frames - and
 * behind the same host check as asr_stream_logmel.  No
 * length is passed: the ring must hold samples 160 t_begin .. 160 (t_begin + n_new - 1) + 399.  wav_ring (B, scap) f32 and
 * feat_ring (B, fcap, n_mels) f32 as above; refused with ASR_EINVAL unless scap is a power of two of at least 1024, fcap a
 * power of two, 1 <= max_new <= fcap, n_mels >= 1 and 1 <= B <= 65535.
 */
int asr_fbank_fwd(const float* wav, const int32_t* wav_len, const float* window, const float* melfb, float* feat,
                  int B, int Smax, int Tmax, int n_mels, float wav_scale, float preemph, void* stream);
int asr_stream_fbank(const float* wav_ring, const int32_t* par, const float* window, const float* melfb,
                     float* feat_ring, int B, int max_new, int scap, int fcap, int n_mels, float wav_scale,
                     float preemph, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Independent streaming sessions (additive to ABI 10; csrc/session.hip, asr_chinese_e2e_amd/sessions.py): `slots` sessions share one
 * batch, each at its own frame offset and cache length.  The per-slot parameters are (slots) int32 device arrays - rows of the one
 * parameter block a tick uploads - and no kernel lets a slot's result depend on another slot's parameters.
 *
 * asr_slot_rows_put: dst[b, start[b] + t, :] = src[b * C + t, :] for t < min(n[b], C).  src: (slots*C) rows of `cols` elements, row
 *   stride ld_src elements (a column slice of a wider matrix: the K | V columns of qkv); dst: (slots, cap, cols) dense.  Appends a
 *   layer's new keys to its cache, and the encoder's output rows to the per-slot output buffer.  Only valid rows are written; a row
 *   that would land outside [0, cap) is dropped.  16-byte vectors: cols and ld_src times the element size are multiples of 16, src and
 *   dst 16-byte aligned; 1 <= C <= cap, slots <= 65535 (ASR_EINVAL otherwise, before any launch).
 * asr_slot_rows_slide: dst[b, t, :] = src[b, from[b] + t, :] for t < count[b] <= max_count; src and dst are two different
 *   (slots, cap, cols) buffers (the ping-pong of the fixed-window cache: never in place - overlapping buffers are refused).  Rows
 *   read outside [0, cap) are dropped.  Alignment as above; 1 <= max_count <= cap.
 * asr_ctc_frame_best_blank: one pass per frame of the CTC head's logits (B, T, V) (row stride ld): path = the best class, the first
 *   maximum winning, as asr_ctc_frame_argmax (same 16-byte bf16 path and scalar tail); blank_lp = log_softmax of class `blank`, bit
 *   for bit asr_ctc_frame_topk's (the maximum is order-free, the sum of exponentials is taken in that kernel's order).  Frames
 *   t >= in_len[b] (in_len may be NULL) get path = blank and blank_lp = 0.
 * asr_session_ctc_step: one wave per slot over its n_valid[b] <= C frames in order.  state (slots, 4) int32 = {last class, trailing
 *   silent frames, frames consumed, decoded}; reset[b] != 0: the slot starts from {blank, 0, 0, 0} instead of its stored state.
 *   A class c of frame t is emitted when c != blank and c != the class of the frame before (the carried last class at t = 0): the
 *   CTC collapse across chunk boundaries.  A frame is silent iff blank_lp > silence_lp (the caller passes log(blank_threshold));
 *   trailing = the current run of silent frames, frames += n_valid[b], decoded = 1 once anything was emitted.  path == NULL (beam
 *   sessions): nothing is emitted, last and decoded keep their values.  out (slots, 4 + C) int32 = {ids emitted, trailing, frames,
 *   decoded, the ids, 0-padded}: one buffer, one copy to the host.  n_valid[b] == 0 without reset leaves the slot's state as it is.
 */
int asr_slot_rows_put(const void* src, void* dst, const int32_t* start, const int32_t* n, int slots, int C, int cap, int cols,
                      int ld_src, int dtype, void* stream);
int asr_slot_rows_slide(const void* src, void* dst, const int32_t* from, const int32_t* count, int slots, int max_count, int cap,
                        int cols, int dtype, void* stream);
int asr_ctc_frame_best_blank(const void* logits, const int32_t* in_len, int32_t* path, float* blank_lp, int B, int T, int V,
                             int ld, int blank, int dtype, void* stream);
int asr_session_ctc_step(const int32_t* path, const float* blank_lp, const int32_t* n_valid, const int32_t* reset, int32_t* state,
                         int32_t* out, int slots, int C, int blank, float silence_lp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token confidence and streamed token times from the CTC posteriors (additive to ABI 10; csrc/confidence.hip,
 * asr_chinese_e2e_amd/confidence.py; the definitions in float64: tests/confidence_ref.py).  p = softmax of a frame's logits over V >= 2 classes.
 *
 * asr_ctc_frame_stats: one wave per frame of logits (B, T, V) f32 / bf16 (row stride ld).  path = the best class, the first maximum
 *   winning, bit for bit asr_ctc_frame_argmax's; blank_lp = log p[blank], bit for bit asr_ctc_frame_best_blank's (same passes, same
 *   order of the sum of exponentials); lse = m + logf(s) with m the maximum and s = sum e^(x - m); best_lp = m - lse = log p[path];
 *   ent = 1 - H / ln V clamped to [0, 1], H = ln s - u / s with u = sum (x - m) e^(x - m), a class whose exponential is 0 (a -inf
 *   logit, an underflow) adding exactly 0 - a one-hot row gives 1, a constant row 0, no row with a finite maximum gives NaN.  All
 *   outputs (B, T); frames t >= in_len[b] (in_len may be NULL) get path = blank and 0 in the four float outputs.
 * asr_ctc_token_conf: one wave per utterance, a lane per token.  labels (B, Lmax), lab_len (B), spans (B, Lmax, 2) as asr_ctc_align
 *   takes and writes them, lse / ent (B, T) from asr_ctc_frame_stats over the same logits.  For token l < lab_len[b] with class y on
 *   frames s..e (n = e - s + 1), lp_t = logits[b, t, y] - lse[b, t]: out (B, Lmax, 5) f32 = {post_max = exp(max lp_t), post_min =
 *   exp(min lp_t), post_mean = exp(sum lp_t / n), ent_mean = sum ent_t / n, ent_min = min ent_t}.  The sums are fp32, start at 0.f
 *   and take the frames one at a time in ascending t.  Entries l >= lab_len[b] hold 0; a token whose span is -1 (asr_ctc_align found
 *   no alignment), or is no span of [0, T), holds NaN in all five.  1 <= Lmax <= 255.
 * asr_session_ctc_step_tokens: asr_session_ctc_step with path required, plus the greedy path's runs.  best_lp, ent (slots, C) from
 *   asr_ctc_frame_stats.  A run is a maximal sequence of frames of one non-blank class (it continues across ticks); the token
 *   asr_session_ctc_step emits when a run opens gets its record when the run closes, i.e. at the first frame of another class.
 *   run (slots, 8) int32, the open run between ticks = {class (blank: none), first frame, frames, then as float bits: sum, max, min of
 *   lp = best_lp, sum, min of ent}, the sums in the order above; reset[b] != 0 clears it with state; n_valid[b] == 0 without reset
 *   leaves both untouched.  out (slots, 13 + 9 C) int32, one copy to the host:
 *     [0, 4 + C)           asr_session_ctc_step's out, the same values
 *     [4 + C]              runs closed in this tick (<= C)
 *     [5 + C, 5 + 9 C)     a record of 8 words per closed run, in order, 0 behind the last: {id, first frame, last frame, post_max,
 *                          post_min, post_mean, ent_mean, ent_min} (floats as their bits), frames counted from the session's frame 0
 *     [5 + 9 C, 13 + 9 C)  the record of the run still open after this tick (id -1 and zeros: none); the host closes it when the
 *                          session's input ends
 */
int asr_ctc_frame_stats(const void* logits, const int32_t* in_len, int32_t* path, float* best_lp, float* blank_lp, float* lse,
                        float* ent, int B, int T, int V, int ld, int blank, int dtype, void* stream);
int asr_ctc_token_conf(const void* logits, const int32_t* labels, const int32_t* lab_len, const int32_t* spans, const float* lse,
                       const float* ent, float* out, int B, int T, int V, int ld, int Lmax, int dtype, void* stream);
int asr_session_ctc_step_tokens(const int32_t* path, const float* blank_lp, const float* best_lp, const float* ent,
                                const int32_t* n_valid, const int32_t* reset, int32_t* state, int32_t* run, int32_t* out, int slots,
                                int C, int blank, float silence_lp, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Energy voice-activity detection and segment gather for long recordings (additive to ABI 10; csrc/vad.hip,
 * asr_chinese_e2e_amd/vad.py, longform.py).
 * Stands in for:  nothing in the reference (it has no segmenter); Kaldi's compute-vad-energy restated - parity unpinned by Kaldi's
 *                 binaries; the definition in float64 is tests/vad_ref.py.
 *
 * asr_vad_energy: wav (B, S) f32, wav_len (B) int32 samples, taken as min(max(wav_len[b], 0), S).  Recording b has
 *   T_b = min(1 + (len - 400) / 160, Tmax) frames, none for len < 400; frame t is samples 160 t .. 160 t + 399 (asr_fbank_fwd's
 *   frames).  E (B, Tmax) f32: E[b][t] = logf(max(sum_i (x_i - mean)^2, FLT_EPSILON)) with x = 32768 * sample and mean = the frame's
 *   mean (Kaldi's raw log-energy, dither 0); frames t >= T_b hold 0.  One fixed summation order (csrc/vad.hip): a frame's bits depend
 *   on its 400 samples only, not on the batch, the tile or the recording's length; an all-zero frame gives logf(FLT_EPSILON).
 *   16-byte loads when S is a multiple of 4 and wav is 16-byte aligned, else a scalar path with the same bits.  1 <= B <= 65535.
 * asr_vad_decide: E as above (Tmax the same; wav_len should not pass S), params (3) f64 on the device = {energy_threshold,
 *   energy_mean_scale, proportion_threshold}.  thr_out[b] = params[0] + params[1] * (sum_t E[b][t]) / T_b in fp64, the sum by
 *   per-workgroup partials in ws and a final pass, both in a fixed order and without atomics: bit-reproducible.  speech (B, Tmax)
 *   uint8: frame t < T_b is 1 iff num >= den * params[2] in fp64, den = the frames of [t - ctx, t + ctx] inside [0, T_b), num = those
 *   of them with (double)E > thr; frames t >= T_b hold 0.  T_b = 0: the row is zeros, thr_out[b] = params[0], nothing is divided.
 *   ws: asr_vad_decide_workspace_bytes(B, Tmax) bytes, 8-byte aligned.  0 <= ctx <= ASR_VAD_CTX_MAX.  Two launches.
 * asr_segment_gather: out (N, Smax) f32 row n = samples [seg_start[n], seg_start[n] + seg_len[n]) of row seg_rec[n] of wav (rows of
 *   S samples), bit for bit, zeros behind.  The window is clamped to its row (an empty row for a negative seg_rec or a start outside
 *   [0, S); at most min(Smax, S - start) samples); seg_rec must be below the number of rows, which the caller guarantees.  16-byte
 *   pieces when S and Smax are multiples of 4, wav and out are 16-byte aligned and the start is a multiple of 4; else scalar.
 *   1 <= N <= 65535.
 */
#define ASR_VAD_CTX_MAX 1024
int asr_vad_energy(const float* wav, const int32_t* wav_len, float* E, int B, int S, int Tmax, void* stream);
size_t asr_vad_decide_workspace_bytes(int B, int Tmax);
int asr_vad_decide(const float* E, const int32_t* wav_len, const double* params, uint8_t* speech, double* thr_out, void* ws,
                   int B, int Tmax, int ctx, void* stream);
int asr_segment_gather(const float* wav, int S, const int32_t* seg_rec, const int32_t* seg_start, const int32_t* seg_len,
                       float* out, int N, int Smax, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CTC forced alignment of whole recordings (csrc/align_long.hip).  Additive to ABI 10.  The definition, in float64 and plain numpy, is
 * tests/align_long_ref.py; the kernel agrees with it bit for bit.
 * R recordings share one call.  Recording r owns rows [row_off[r], row_off[r+1]) of rows (sum T, ld) `dtype` (f32 / bf16, ld >= V) and of
 * lse (sum T) f32 (asr_ctc_frame_stats' log-sum-exp of the same rows), and labels [lab_off[r], lab_off[r+1]) of labels (sum L) int32,
 * classes in [0, V) other than `blank`.  The emission is lp(t, c) = (float)rows[t][c] - lse[t], one f32 subtraction.
 * States s = 0 .. 2L, blanks at even s, label (s - 1) / 2 at odd s:
 *   v_0(0) = lp(0, blank), v_0(1) = lp(0, l_0), v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)) + (double)lp(t, sym(s)) in fp64,
 *   the s-2 term for odd s >= 3 whose label differs from the one before.  Ties: s before s-1 before s-2; the end 2L before 2L-1.
 * path (sum T) int32: the index (within the recording) of the token frame t belongs to, -1 on blank frames.
 * spans (sum L, 2) int32: first and last frame (inclusive, within the recording) of each token.
 * tok (sum L, 3) f32: over the token's frames in ascending t, the f32 sum from 0.f of lp(t, l_i), its largest and its smallest value.
 * score (R) f64: v_{T-1} of the end state.  T = 0 is feasible iff L = 0 (score 0).  An infeasible recording has score -inf, spans -1,
 *   tok -inf and a path of -1.
 * L <= ASR_ALIGN_LONG_MAX_LABELS per recording (a longer one is reported as infeasible); T is bounded by the workspace alone, which
 * holds one back-pointer byte per label (rows of L rounded up to 64) and frame: asr_ctc_align_long_workspace_bytes(R, sum T, max L) is
 * enough for any split of the frames and labels among R recordings; a recording whose rows pass ws_bytes is reported as infeasible.
 * The offsets are device data: the kernel clamps what it forms from them and from the labels, the caller checks them on the host
 * (kernels.ctc_align_long).  ws 16-byte aligned.  Four launches (one per workgroup size; a workgroup of another size leaves at once).
 */
#define ASR_ALIGN_LONG_MAX_LABELS 8192
size_t asr_ctc_align_long_workspace_bytes(int R, int T_total, int Lmax);
int asr_ctc_align_long(const void* rows, const float* lse, const int32_t* row_off, const int32_t* labels, const int32_t* lab_off,
                       int32_t* path, int32_t* spans, float* tok, double* score, void* ws, size_t ws_bytes, int R, int V, int ld,
                       int dtype, int blank, void* stream);

/* asr_ctc_align_long with filler frames for audio the transcript does not cover.  Additive to ABI 10.  The definition is
 * tests/align_filler_ref.py; the kernel agrees with it bit for bit.
 * No state is added and the topology does not change: some blank states are WIDE.  gap (sum L) uint8, indexed like labels: gap[i] != 0
 * marks the blank state 2i in front of label i; gap_tail (R) uint8: gap_tail[r] != 0 marks the last state 2L of recording r.  star
 * (sum T) f32, indexed like lse: the log-probability of "anything" on every frame (no NaN).  With eb = lp(t, blank), a wide blank state
 * emits on frame t
 *   star[t] if star[t] > eb, else eb      (strict: the blank wins ties; the chosen f32 is converted to double as every emission is)
 * at t = 0 too, and in the L = 0 sum.  The recursion, the tie order, the choice of the end state and tok are asr_ctc_align_long's.
 * path gains the value -2: the frame sits in a wide blank state and star[t] > eb (a filler frame); a plain blank frame stays -1.
 * With every flag 0, or with star = -inf everywhere, every output has asr_ctc_align_long's bits.  A wide blank stays optional and
 * skippable, so it never makes an infeasible recording feasible.  Workspace and back-pointer coding are asr_ctc_align_long's (the filler
 * choice is a function of the frame and the state, so nothing more is stored per frame). */
int asr_ctc_align_long_filler(const void* rows, const float* lse, const float* star, const int32_t* row_off, const int32_t* labels,
                              const int32_t* lab_off, const uint8_t* gap, const uint8_t* gap_tail, int32_t* path, int32_t* spans,
                              float* tok, double* score, void* ws, size_t ws_bytes, int R, int V, int ld, int dtype, int blank,
                              void* stream);

/* Blank-frame skipping in front of the CTC prefix beam search.  Additive to ABI 10.  The definition is tests/blank_skip_ref.py.
 * asr_ctc_blank_skip_compact: vals / ids (B*T, k), blank_lp (B*T) = the per-frame candidates of asr_ctc_frame_topk; count (B) int32 on
 *   the device = the frames of each utterance (in_len offline, n_valid per chunk; NULL = T; clamped to [0, T]).  Frame t < count[b] is
 *   high iff blank_lp[b, t] > thr (float32 against float32, strict: a NaN is not high; thr = log p <= 0) and dropped iff it is high and
 *   its predecessor exists and is high: the head of every run of high frames stays.  The kept rows are copied in order to the front of
 *   the utterance's rows of out_vals / out_ids / out_blank_lp (the same (B, T) layout, never in place), out_len[b] = their number, and
 *   out_frame[b, i] = the frame the i-th kept row was.  Rows at and past count[b] are neither read nor counted; output rows at and past
 *   out_len[b] keep what they held.  No atomics and one fixed order: two runs write the same bytes.  k <= 63.
 *   state == NULL (offline): out_frame is (B, map_cap) with map_cap >= T (or NULL with map_cap 0).
 *   state (B, 4) int32 {carry = the last consumed frame was high, frames seen, frames kept, 0}, zeros at first (the resumable form, one
 *   launch per chunk): the predecessor of a chunk's frame 0 is the carry bit, out_frame is a per-utterance map (B, map_cap) that the
 *   launch extends at [kept, kept + out_len[b]) with seen + t (entries past map_cap are not written), and the state is advanced; after
 *   any cutting of the frames into chunks (empty ones included: count 0 keeps every word of the state) the kept frames are those of one
 *   launch over all of them.  reset (B) int32 or NULL, with a state only: reset[b] != 0 treats utterance b's state as zeros before the
 *   chunk, with the meaning of asr_ctc_prefix_beam_state_reset's flags.
 * asr_frame_index_remap: idx, out (B, per) int32 (out may be idx): out[b, i] = idx[b, i] < 0 ? idx[b, i] : map[b, idx[b, i]], map
 *   (B, map_cap); an index >= map_cap stays.  Takes the start / end frames of the timed searches run on kept rows back to real frames. */
int asr_ctc_blank_skip_compact(const float* vals, const int32_t* ids, const float* blank_lp, const int32_t* count, float thr,
                               int32_t* state, const int32_t* reset, float* out_vals, int32_t* out_ids, float* out_blank_lp,
                               int32_t* out_len, int32_t* out_frame, int B, int T, int k, int map_cap, void* stream);
int asr_frame_index_remap(const int32_t* idx, const int32_t* map, int32_t* out, int B, int per, int map_cap, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Keyword spotting on the CTC posteriors (additive to ABI 10; csrc/kws.hip, asr_chinese_e2e_amd/keywords.py).
 * Stands in for:  nothing in the reference; a max-path keyword filler-free search in the spirit of wekws' CTC spotter - parity unpinned (none
 *                 of its code or output was on hand); the definition in float32 is tests/kws_ref.py, the kernels agree with it bit for bit.
 *
 * Emission of frame t: lp_t(v) = (float)logits[b, t, v] - lse[b, t], one f32 subtraction; lse from asr_ctc_frame_stats over the same rows.
 * A keyword w_0 .. w_{L-1} (1 <= L <= ASR_KWS_MAX_LEN, ids in [0, V), none the blank) has states s = 0 .. 2L-2: even s = 2i emits
 * lp_t(w_i), odd s emits lp_t(blank), the optional blank between w_i and w_{i+1}.  No leading and no trailing blank.
 *   D_{-1}(s) = -inf, start_{-1}(s) = -1.  Frame t:
 *     s = 0:   best = 0.0f, bs = t                  (a match may begin on any frame: every continued path has D <= 0)
 *     s >= 1:  best = D_{t-1}(s), bs = start_{t-1}(s); those of s-1 iff D_{t-1}(s-1) > best; then, for even s >= 2 with
 *              w_{s/2} != w_{s/2-1}, those of s-2 iff D_{t-1}(s-2) > best      (both strict; compare-and-select, never fmaxf)
 *     D_t(s) = best + e_t(s) (one f32 addition), start_t(s) = best > -inf ? bs : -1
 *   H_t = D_t(2L-2), hs_t = start_t(2L-2): the largest log-probability of a CTC alignment of the keyword that ends on frame t, over every
 *   start, and that alignment's first frame.  State 0 is entered afresh on every frame (a longer stay in w_0 never scores more), so a
 *   hit's start is the LAST frame of the audio's run of w_0, not its first: the hit brackets the keyword from the inside.
 * Frame t is a candidate of keyword k iff H_t >= thr[k] (a NaN is none) and hs_t >= 0 and t - hs_t + 1 <= span[k].  Each maximal run of
 * candidate frames of one (utterance, keyword) is one hit {start = hs of the run's best frame, end = that frame, score = its H}, the
 * best frame being the one of largest H, the first on ties.  A run closes on the first frame that is no candidate; offline also behind
 * the utterance's last frame, streamed when the slot is pushed with `final`.  The logits must hold no NaN and no +inf (-inf is fine).
 *
 * asr_kws_list: the tables of K keywords.  Row j: tok[j, 0 .. len[j]) of tok (K, ASR_KWS_MAX_LEN), thr[j] f32, span[j], and index[j] =
 *   the keyword's own number, the row of every output it writes (a permutation of [0, K): the rows may be sorted by length so that the
 *   64 keywords of a wave share a length bucket, L <= 4 / 8 / 16, at no change to any output).  host_tok / host_len / host_index are host
 *   copies of tok / len / index, which every launcher checks before any launch (K, the lengths, the ids against V and blank, the
 *   permutation); the kernels clamp what they read from the device tables all the same.
 * asr_kws_search: logits (B, T, V) f32 / bf16 (row stride ld), lse (B, T), in_len (B) or NULL (= T; clamped to [0, T]).  cnt (B, K):
 *   the hits of keyword k in utterance b (it keeps counting past cap); rec (B, K, cap, 3) int32 {start, end, score as f32 bits}: the
 *   first cap of them in order of their end, zeros behind.  One wave per (utterance, 64 table rows), one launch.
 * asr_kws_chunk: the resumable form, one call per chunk: logits (slots, C, V), lse (slots, C), n_valid / reset / final (slots) int32 in
 *   the sense of asr_session_ctc_step.  state: asr_kws_state_bytes(slots, K) bytes, initialised by asr_kws_state_init; per (slot, keyword)
 *   the column D, start (in frames of the session) and the open run {open, start, end, H}, per slot the frames consumed.  reset[b] != 0:
 *   the slot starts from the initial state; n_valid[b] == 0 without reset or final leaves every word of the slot's state as it is.
 *   final[b] != 0 closes the open runs behind the chunk's frames.  cnt / rec as above, for the runs closed in this call.  After any
 *   cutting of the frames into chunks the hits of all calls are those of asr_kws_search over all of them, bit for bit.
 * asr_kws_compact: cnt / rec as written above -> hits (B, max_hits, 4) int32 {keyword, start, end, score bits} in one fixed order, keyword
 *   ascending, then end ascending, zeros behind; count[b] = the rows written, dropped[b] = the hits found and not written (past cap,
 *   or past max_hits).  Offsets by ballot and popcount; no atomics: two runs write the same bytes.
 * asr_kws_state_reset: flags (slots) int32 on the device, flags[b] != 0 puts slot b back to the initial state.
 * Limits: K <= ASR_KWS_MAX_KEYWORDS, cap <= ASR_KWS_MAX_CAP, B / slots <= 65535; 4-byte aligned pointers.
 */
#define ASR_KWS_MAX_LEN 16
#define ASR_KWS_MAX_KEYWORDS 65536
#define ASR_KWS_MAX_CAP 64
typedef struct asr_kws_list {
    const int32_t* tok;        /* device, (K, ASR_KWS_MAX_LEN) */
    const int32_t* len;        /* device, (K) */
    const float* thr;          /* device, (K) */
    const int32_t* span;       /* device, (K) */
    const int32_t* index;      /* device, (K) */
    const int32_t* host_tok;   /* host copies, read by the launchers' checks */
    const int32_t* host_len;
    const int32_t* host_index;
    int K;
} asr_kws_list;
size_t asr_kws_state_bytes(int slots, int K);
size_t asr_kws_records_bytes(int B, int K, int cap);
int asr_kws_search(const void* logits, const float* lse, const int32_t* in_len, const asr_kws_list* kw, int32_t* cnt, int32_t* rec, int B,
                   int T, int V, int ld, int blank, int cap, int dtype, void* stream);
int asr_kws_chunk(const void* logits, const float* lse, const int32_t* n_valid, const int32_t* reset, const int32_t* final,
                  const asr_kws_list* kw, int32_t* state, int32_t* cnt, int32_t* rec, int slots, int C, int V, int ld, int blank, int cap,
                  int dtype, void* stream);
int asr_kws_compact(const int32_t* cnt, const int32_t* rec, int32_t* count, int32_t* dropped, int32_t* hits, int B, int K, int cap,
                    int max_hits, void* stream);
int asr_kws_state_init(int32_t* state, int slots, int K, void* stream);
int asr_kws_state_reset(int32_t* state, const int32_t* flags, int slots, int K, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token-level scoring: Levenshtein alignment of hypotheses against references with its split into correct tokens, substitutions,
 * deletions and insertions (additive to ABI 10; csrc/score.hip, asr_chinese_e2e_amd/scoring.py).
 * Stands in for:  nothing in the reference, whose only scorer is the string convention of asr_cer (untouched).  The definition, in
 *                 integers, is tests/score_ref.py; the kernel agrees with it integer for integer, ties included.
 *
 * For a reference r[0..m) and a hypothesis h[0..n):  D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (r[i-1] != h[j-1]),
 * D[i-1][j] + 1, D[i][j-1] + 1).  The direction of a cell is the FIRST that applies of DIAG (D[i-1][j-1] + (r[i-1] != h[j-1]) ==
 * D[i][j]), UP (D[i-1][j] + 1 == D[i][j]: r[i-1] is deleted), LEFT (h[j-1] is inserted); row 0 is LEFT, column 0 is UP.  The alignment
 * is the walk from (m, n) to (0, 0) along the directions, reported from (0, 0) on.  Ids are compared, never used as indices.
 *
 * asr_edit_align: P pairs, one wave each, one launch.  hyp (P, Lh) int32 rows ldh apart, hyp_len (P); ref (R, Lr) rows ldr apart, ref_len
 *   (R); ref_of (P): pair p scores hyp row p against ref row ref_of[p], so an n-best list shares its reference.  All of these on the
 *   device; host_hyp_len / host_ref_len / host_ref_of are host copies of the three small arrays, by which the launcher checks ref_of
 *   against [0, R) and sizes LDS and workspace without reading the device.  The kernel clamps lengths to [0, Lh] / [0, Lr] and ref_of to
 *   [0, R) all the same (the host sizes by the same clamped lengths).
 *   counts (P, 5) int32 = {distance, cor, sub, del, ins}.
 *   ops == NULL: counts only; no direction is stored, no workspace is needed and n_ops is not written.
 *   ops (P, 3, ldo) int32, ldo >= max(Lh + Lr, 1), n_ops (P): plane 0 holds the n_ops[p] codes ASR_EDIT_COR / SUB / DEL / INS in forward
 *   order, plane 1 the op's reference position (-1 for an insertion), plane 2 its hypothesis position (-1 for a deletion).  Words at and
 *   past n_ops[p] are scratch of the kernel.
 *   The two direction bits of a cell are kept for the walk, 16 bytes per (reference token, 64 hypothesis tokens): in LDS for a pair with
 *   m * ceil(n / 64) * 16 <= ASR_EDIT_LDS_DIR_BYTES, else in ws, of at least asr_edit_align_workspace_bytes(...) bytes (0 when every pair
 *   fits LDS; ws may then be NULL), 16-byte aligned.  Should the device lengths ask for more than the host copies provided, the pair gets
 *   its distance, -1 for the four counts and n_ops = -1; nothing is written out of bounds.
 *   The launch's dynamic LDS is sized by its largest pair (at most 150 KB, as asr_cer).  Limits: ASR_EDIT_MAX_REF tokens per reference
 *   (hypotheses have none); 4-byte aligned pointers.  No atomics: two runs write the same bytes.
 *   Refused before any launch (ASR_EINVAL; ASR_EWORKSPACE for the last): null or misaligned pointers, P <= 0, R <= 0, negative Lh / Lr,
 *   ldh < Lh, ldr < Lr, ldo too small, ref_of[p] outside [0, R), a reference above the limit, a workspace below the size query's answer.
 */
#define ASR_EDIT_LDS_DIR_BYTES 98304
#define ASR_EDIT_MAX_REF 16384
#define ASR_EDIT_COR 0
#define ASR_EDIT_SUB 1
#define ASR_EDIT_DEL 2
#define ASR_EDIT_INS 3
size_t asr_edit_align_workspace_bytes(const int32_t* host_hyp_len, const int32_t* host_ref_len, const int32_t* host_ref_of, int P, int R,
                                      int Lh, int Lr);
int asr_edit_align(const int32_t* hyp, const int32_t* hyp_len, int Lh, int ldh, const int32_t* ref, const int32_t* ref_len, int Lr,
                   int ldr, const int32_t* ref_of, const int32_t* host_hyp_len, const int32_t* host_ref_len, const int32_t* host_ref_of,
                   int P, int R, int32_t* counts, int32_t* ops, int32_t* n_ops, int ldo, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Consensus decoding of n-best lists: the minimum-Bayes-risk entry, a pivot-based confusion network with the posterior mass of its
 * alternatives, the consensus string and a token confidence from the votes (additive to ABI 10; csrc/consensus.hip,
 * asr_chinese_e2e_amd/consensus.py).
 * Stands in for:  nothing in the reference.  The definition, in integers, is tests/consensus_ref.py; the kernels agree with it integer
 *                 for integer, ties included.  Parity with SRILM's nbest-lattice or with ROVER is not pinned.
 *
 * Inputs, in the layout the prefix beam search produces: tok (U, N, L) int32 ids, entry rows ldn apart and utterances ldu apart; len
 * (U, N) int32, -1 = absent (the entry keeps its index and takes part in nothing); weights (U, N) int32 >= 0, at most 2^30 per
 * utterance over its present entries.  All three on the device; host_len / host_weights are host copies of the two small arrays, by which
 * the launcher refuses.  The kernels clamp a length to [-1, L] and a weight to >= 0 all the same, and never use an id as an index.  The
 * device sees no float: weights come from the caller (consensus.nbest_weights: floor(softmax * 2^20 + 0.5) in float64 on the host).
 *
 * With d[i][k] the edit distance of entries i and k (asr_edit_align's recurrence), risk[i] = sum_k w_k d[i][k] (int64), pivot = the
 * present i of least risk (lowest i on ties), m = len[pivot] and S = 2 L + 1: the pivot's slots are 0 .. 2 m, slot 2 i + 1 pivot position
 * i and slot 2 g the gap in front of position g.  Entry k, aligned to the pivot as asr_edit_align aligns a hypothesis to a reference (the
 * pivot is the reference), votes its COR / SUB token at 2 i + 1, ASR_NBEST_EPS for a DEL, the FIRST token it inserts in gap g at 2 g
 * (ASR_NBEST_EPS if none); later tokens of an insertion run vote nowhere and are counted in extra.  The alternatives of a slot are its
 * distinct votes, ordered by weight (descending), then by their lowest voter (ascending).
 *
 * Output: one buffer `out` of asr_nbest_out_bytes(U, N, L, A) bytes, 8-byte aligned, of these arrays back to back (int32 but the first):
 *   risk (U, N) int64 | d (U, N, N) | pivot (U) | W (U) | extra (U, N) | n_alts (U, S) | pivot_w (U, S) | votes (U, N, S) |
 *   alts (U, S, A, 2) = (token, weight), the top A; entries past n_alts are (ASR_NBEST_EPS, 0).
 *   pivot_w = the weight of the pivot's own vote; slots past 2 m hold n_alts = 0, pivot_w = 0, votes ASR_NBEST_EPS; an absent entry has
 *   risk 0, d 0, extra 0 and votes ASR_NBEST_EPS.  Every word is written by exactly one lane: no atomics, two runs write the same bytes.
 *
 * asr_nbest_pair_dist (d), asr_nbest_pivot_votes (risk, pivot, W, votes, extra; reads d) and asr_nbest_slot_vote (alts, n_alts, pivot_w;
 * reads pivot and votes) are the three stages, one launch each; asr_nbest_consensus is the three in order on `stream`.  All four take
 * the same arguments and make the same checks.
 * Refused before any launch (ASR_EINVAL; ASR_EWORKSPACE for the last): null or misaligned pointers, U <= 0 or above 65535, N outside
 * [1, ASR_NBEST_MAX_N], L outside [0, ASR_NBEST_MAX_LEN], a host length above ASR_NBEST_MAX_LEN, ldn < L, ldu < (N - 1) ldn + L, A
 * outside [1, ASR_NBEST_MAX_ALTS], a negative weight, a weight sum above 2^30, an utterance with no present entry, out_bytes below
 * the size query's answer.
 */
#define ASR_NBEST_MAX_N 64
#define ASR_NBEST_MAX_LEN 256
#define ASR_NBEST_MAX_ALTS 8
#define ASR_NBEST_EPS (-1)
size_t asr_nbest_out_bytes(int U, int N, int L, int A);
int asr_nbest_pair_dist(const int32_t* tok, const int32_t* len, const int32_t* weights, int L, int ldn, int ldu, const int32_t* host_len,
                        const int32_t* host_weights, int U, int N, int A, int32_t* out, size_t out_bytes, void* stream);
int asr_nbest_pivot_votes(const int32_t* tok, const int32_t* len, const int32_t* weights, int L, int ldn, int ldu, const int32_t* host_len,
                          const int32_t* host_weights, int U, int N, int A, int32_t* out, size_t out_bytes, void* stream);
int asr_nbest_slot_vote(const int32_t* tok, const int32_t* len, const int32_t* weights, int L, int ldn, int ldu, const int32_t* host_len,
                        const int32_t* host_weights, int U, int N, int A, int32_t* out, size_t out_bytes, void* stream);
int asr_nbest_consensus(const int32_t* tok, const int32_t* len, const int32_t* weights, int L, int ldn, int ldu, const int32_t* host_len,
                        const int32_t* host_weights, int U, int N, int A, int32_t* out, size_t out_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Rescoring of n-best lists: the n-gram LM score of many finished strings in one launch, and the sweep of a grid of weight vectors over
 * lists of feature vectors (additive to ABI 10; csrc/rescore.hip, asr_chinese_e2e_amd/rescore.py).
 * Stands in for:  nothing in the reference.  The definition is tests/rescore_ref.py on top of lm.py::NgramLM's host methods; the kernels
 *                 agree with it in integers and float bits, with no tolerance.
 *
 * asr_lm_score_nbest: P hypotheses, tok (P rows, ld apart) int32 ids and len (P) int32 on the device, -1 = absent; host_len is a host copy
 *   of len, by which the launcher refuses.  One lane per hypothesis walks its tokens from (lm->start, 0.0) with the statements of the
 *   prefix beam search's LM step (bias += st_bow per state left, += the term found, += ins; asr_ngram_lm above), then adds the
 *   end-of-sentence chain for token `eos` without ins if has_eos != 0 (NgramLM.final; has_eos / eos are arguments, not fields of
 *   asr_ngram_lm).  out_score (P) fp64 = NgramLM.score, out_bias (P) fp64 and out_state (P) = NgramLM.walk, out_ntok (P) = the token
 *   count, bit for bit: the device only adds fp64 table terms in the host's order.  An absent entry gives (0.0, 0.0, -1, 0).  A token id
 *   is an index only into the V-sized unigram tables, clamped to [0, V) there as the host clamps it; every other table index is clamped too.
 *   Refused before any launch (ASR_EINVAL): null or misaligned pointers (fp64: 8 bytes), P <= 0, ld < 0, a host length below -1 or
 *   above ld, and what the LM searches refuse of an asr_ngram_lm.
 *
 * asr_nbest_sweep: U lists of N entries with K features each, G weight vectors.  feat (K, N, U) fp64 planes, len (N, U) int32 (-1 =
 *   absent), err (3, N, U) int32 = every entry's (sub, del, ins) against its reference, grid (G, K) fp64, all on the device with the
 *   utterance as the unit-stride index; host_feat / host_len / host_grid are host copies in the same layouts, by which the launcher refuses.
 *   The total of an entry under w: total = 0.0; for k ascending, if w[k] != 0.0: total = total + (w[k] * f[k]) - the product rounded,
 *   then the sum, never fused; a term of weight 0.0 is skipped, so 0 * -inf never happens.  An entry is unscorable under w if some f[k]
 *   with w[k] != 0.0 is not finite.  The pick of (g, u) is the present, scorable entry of greatest total, the lowest index on ties; the
 *   present entry of lowest index if none is scorable.
 *   out_pick (G, U) int32; out_tot (G, 4) int64 = the picks' summed sub, del, ins and the number of utterances whose pick has
 *   sub + del + ins > 0; out_total (G, U, N) fp64 or NULL: every present, scorable entry's total, -inf for the others.
 *   One wave per (grid point, 64 utterances) writes its partial counts into ws (asr_nbest_sweep_workspace_bytes(U, N, K, G) bytes,
 *   8-aligned); a second launch sums them.  Integers and no atomics: two runs write the same bytes.
 *   Refused before any launch (ASR_EINVAL; ASR_EWORKSPACE for the last): null or misaligned pointers, U outside [1, ASR_RESCORE_MAX_U],
 *   N outside [1, ASR_RESCORE_MAX_N], K outside [1, ASR_RESCORE_MAX_K], G outside [1, ASR_RESCORE_MAX_G], a non-finite weight, a NaN or
 *   +inf feature, an utterance with no present entry, a workspace below the size query's answer.  The kernel treats a non-finite
 *   feature as unscorable and clamps the pick all the same.
 */
#define ASR_RESCORE_MAX_N 64
#define ASR_RESCORE_MAX_K 8
#define ASR_RESCORE_MAX_G 65536
#define ASR_RESCORE_MAX_U 1048576
int asr_lm_score_nbest(const int32_t* tok, const int32_t* len, const int32_t* host_len, int P, int ld, const asr_ngram_lm* lm, int has_eos, int eos,
                       double* out_score, double* out_bias, int32_t* out_state, int32_t* out_ntok, void* stream);
size_t asr_nbest_sweep_workspace_bytes(int U, int N, int K, int G);
int asr_nbest_sweep(const double* feat, const int32_t* len, const int32_t* err, const double* grid, const double* host_feat,
                    const int32_t* host_len, const double* host_grid, int U, int N, int K, int G, int32_t* out_pick, int64_t* out_tot,
                    double* out_total, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MWER training of the CTC head: the expected number of errors over an n-best list, and its gradient with respect to the logits
 * (additive to ABI 10; csrc/mwer.hip, kernels.ctc_mwer, engine.ctc_fwd_bwd).
 * Stands in for:  nothing in the reference.  The definition is tests/mwer_ref.py (float64, torch on the CPU).
 *
 * The list: hyp (B, N, Lh) int32 ids, entry rows ldn apart and utterances ldb apart, hyp_len (B, N) int32 with -1 = absent - the layout
 * asr_ctc_prefix_beam writes.  Lengths are read ON THE DEVICE only (there are no host mirrors: the training step never waits for the
 * search) and clamped to the shapes stated here.  Ids are compared, never used as indices, except as a column < V of the frames.
 * An entry TAKES PART iff 0 <= len <= Lh (the search reports the true length of an entry it had to truncate: such an entry is dropped),
 * every id is in [0, V) and differs from `blank`, len + adjacent repeats <= in_len[b], and in_len[b] > 0.
 *
 *   y_t = softmax(x_t);  ll_i = log p(h_i | x) (the CTC likelihood, as asr_ctc_fwd_bwd's -nll);  e_i = Levenshtein(h_i, r_b)
 *   P_i = exp(ll_i - logsumexp over the entries taking part);  risk_b = sum_i P_i e_i;  c_i = P_i (e_i - risk_b)
 *   G[b,t,v] = scale * sum_i c_i gamma_i(t, v),  gamma_i(t, v) = sum_{s: l'_s = v} alpha_t(s) beta_t(s) / (y_t(v) p(h_i | x))
 * G is the gradient of scale * sum_b risk_b with respect to the logits: d ll_i / d x_t = gamma_i(t, .) - y_t and sum_i c_i = 0, so the
 * dense softmax terms cancel and G is exactly 0 outside the blank column and the columns of the list's tokens, and on rows t >= in_len[b].
 * An utterance with in_len = 0 or no entry taking part has risk 0, posteriors 0 and gradient 0.
 *
 * asr_mwer_errors: err (B, N) int32 = the distance of every entry to ref[b] (ref (B, Lr) int32 rows ldr apart, ref_len (B) int32 clamped
 *   to [0, Lr]); one wave per pair.  flags (B, N) int32: 0, ASR_MWER_ABSENT (len < 0) or ASR_MWER_LONG (len > Lh); a flagged entry gets err 0.
 * asr_ctc_mwer_lattice: logits (B, T, V) `dtype`, rows ld >= V apart, as asr_ctc_fwd_bwd takes them (only read).  Writes ll (B, N) fp64
 *   (-inf for an entry that does not take part), post (B, N) f32 = P, coef (B, N) f32 = c, risk (B) f32, present (B, N) int32 (1 = takes
 *   part), and leaves in ws (asr_ctc_mwer_workspace_bytes(B, N, T, Lh) bytes, 16-byte aligned) what the gradient needs: the state
 *   posteriors of every entry (f32) and the chains that link equal tokens of a list.  The lattice runs in the log domain in fp64, so no
 *   entry leaves the range: a long entry under blank-dominated posteriors never reads as infeasible.
 * asr_ctc_mwer_grad: NEVER reads the logits - only ws, the list, in_len and coef.  dlogits (B, T, V) `dtype`, rows ld apart (it may be
 *   the buffer asr_ctc_fwd_bwd wrote its gradient into: run the lattice before that call, this one after it).
 *   scale = grad_scale, or grad_scale / *grad_scale_div (a DEVICE f32 scalar), as asr_ctc_fwd_bwd.
 *   accumulate = 0: the whole (B, T, V) block is written, zeros where the gradient is zero; columns V .. ld are not touched.
 *   accumulate = 1: only the touched cells (rows t < in_len[b]; the blank and the tokens of the entries taking part) are read, added to in
 *   f32 and stored; every other byte stays.  No atomics; one summation order (entries ascending, states ascending) in f32: two runs
 *   write the same bytes.
 * Refused before any launch (ASR_EINVAL; ASR_EDTYPE; ASR_EWORKSPACE): null or misaligned pointers (fp64: 8 bytes, ws: 16), B outside
 *   [1, 65535], N outside [1, ASR_MWER_MAX_N], Lh or Lr outside [1, ASR_MWER_MAX_LEN], ldn < Lh, ldb < (N - 1) ldn + Lh, ldr < Lr,
 *   T <= 0, V <= 1, blank outside [0, V), ld < V, a dtype other than f32 / bf16, a workspace below the size query's answer (the query
 *   itself returns 0 for a bad shape), a non-finite grad_scale, accumulate other than 0 / 1.
 */
#define ASR_MWER_MAX_N 16
#define ASR_MWER_MAX_LEN 255
#define ASR_MWER_ABSENT 1
#define ASR_MWER_LONG 2
size_t asr_ctc_mwer_workspace_bytes(int B, int N, int T, int Lh);
int asr_mwer_errors(const int32_t* hyp, const int32_t* hyp_len, const int32_t* ref, const int32_t* ref_len, int32_t* err, int32_t* flags,
                    int B, int N, int Lh, int ldn, int ldb, int Lr, int ldr, void* stream);
int asr_ctc_mwer_lattice(const void* logits, const int32_t* in_len, const int32_t* hyp, const int32_t* hyp_len, const int32_t* err,
                         double* ll, float* post, float* coef, float* risk, int32_t* present, int B, int T, int V, int ld, int N, int Lh,
                         int ldn, int ldb, int blank, void* ws, size_t ws_bytes, int dtype, void* stream);
int asr_ctc_mwer_grad(void* dlogits, const int32_t* in_len, const int32_t* hyp, const int32_t* hyp_len, const float* coef, int B, int T,
                      int V, int ld, int N, int Lh, int ldn, int ldb, int blank, float grad_scale, const float* grad_scale_div,
                      int accumulate, const void* ws, size_t ws_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CR-CTC: consistency between the frame posteriors of two augmented views of an utterance, and its gradient with respect to the logits
 * (additive to ABI 10; csrc/cr_ctc.hip, kernels.cr_ctc, engine.ctc_fwd_bwd).
 * Stands in for:  nothing in the reference.  The definition is tests/cr_ctc_ref.py (float64, torch on the CPU).
 *
 * logits (2P, T, V) `dtype`, rows ld >= V apart (only read): rows p and p + P are the two views of utterance p.  in_len (2P) int32 ON
 * THE DEVICE, clamped to [0, T]; n_p = min(in_len[p], in_len[p + P]).  For t < n_p, with y = softmax(x[., t]) of each view:
 *   J[p, t] = 1/2 (KL(sg(y_b) || y_a) + KL(sg(y_a) || y_b)) = 1/2 sum_v (y_a - y_b)(log y_a - log y_b)     (sg: the target is a constant)
 *   pair_loss[p] = sum_{t < n_p} J[p, t];   d pair_loss[p] / d x[p, t] = 1/2 (y_a - y_b),  d pair_loss[p] / d x[p + P, t] = 1/2 (y_b - y_a)
 * frame_loss (P, T) f32 = J (0 for t >= n_p), pair_loss (P) f32 = its sum in frame order.  No atomics: two runs write the same bytes.
 * Both rows go through one instruction sequence: identical views give exactly 0, swapped views swapped bytes, and an f32 gradient
 * of view b is the exact negation of view a's.
 * grad (optional; 2P, T, V, laid out like the logits, NOT overlapping them): scale = grad_scale, or grad_scale / *grad_scale_div (a
 *   DEVICE f32 scalar), as asr_ctc_fwd_bwd.
 *   accumulate = 0: every cell [.., :V] is written, zeros for frames t >= n_p.
 *   accumulate = 1: the cells of frames t < n_p are read, added to in f32 and rounded once to `dtype`; frames t >= n_p are not touched.
 *   Columns V .. ld are never touched.
 * One workgroup per (pair, frame).  V <= ASR_CR_CTC_RESIDENT_MAX_V: both rows stay in registers from the load to the gradient store;
 * above it they are read three times.  16-byte accesses when V and ld are multiples of 16 / sizeof(element) and both blocks are
 * 16-byte aligned, element accesses otherwise.  The exponentials are f32; their sums, the probabilities and J are carried in fp64 and
 * rounded once (with peaked posteriors one f32 rounding of a sum moves J by more than its f32 spacing).  A -inf logit is outside the
 * contract.
 * Refused before any launch (ASR_EINVAL; ASR_EDTYPE): null logits / in_len / frame_loss / pair_loss, pointers not aligned to their
 *   element, P outside [1, 65535], T <= 0, V < 2, ld < V, a dtype other than f32 / bf16, a gradient block that overlaps the logits,
 *   accumulate other than 0 / 1 or without a gradient block, a non-finite grad_scale.
 */
#define ASR_CR_CTC_RESIDENT_MAX_V 6144
int asr_cr_ctc_fwd_bwd(const void* logits, const int32_t* in_len, void* grad, float* frame_loss, float* pair_loss, int P, int T, int V,
                       int ld, float grad_scale, const float* grad_scale_div, int accumulate, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Intermediate CTC with self-conditioning: the frame posteriors of a middle layer and the backward pass of their softmax
 * (additive to ABI 10; csrc/interctc.hip, kernels.softmax_rows / softmax_bwd_add, engine.encoder_fwd / encoder_bwd).
 * Stands in for:  nothing in the reference.  The definition is tests/interctc_ref.py (float64, torch on the CPU).
 *
 * Both work on (B, T, V) frames of `dtype` in rows ld >= V elements apart, every block of a call laid out alike, and on in_len (B) int32
 * ON THE DEVICE, clamped to [0, T].  One workgroup per frame; V <= ASR_INTERCTC_RESIDENT_MAX_V: the row (for the backward both rows)
 * stays in registers from the load to the store, above it the rows are read once per pass.  16-byte accesses when V and ld are
 * multiples of 16 / sizeof(element) and every block is 16-byte aligned, element accesses otherwise.  Exponentials and products are
 * f32, the row sums fp64, one rounding to `dtype`.  No atomics: two runs write the same bytes.  Columns V .. ld are never touched.
 *
 * asr_softmax_rows:  out[b, t, :V] = softmax(logits[b, t, :V]) for t < in_len[b], zeros for t >= in_len[b].  A -inf logit gives
 *   exactly 0; a row whose maximum is not finite gets zeros.  `out` must not overlap the logits.
 * asr_softmax_bwd_add:  for t < in_len[b]:  grad[b, t, v] = (accumulate ? grad[b, t, v] : 0) + p[v] (dp[v] - sum_u p[u] dp[u]);
 *   frames t >= in_len[b] are not touched under accumulate = 1 and get zeros under accumulate = 0.  Where p is 0 the term is exactly 0.
 *   `grad` must overlap neither p nor dp.
 * Refused before any launch (ASR_EINVAL; ASR_EDTYPE): a null pointer, pointers not aligned to their element, B outside [1, 65535],
 *   T <= 0, V <= 0, ld < V, a dtype other than f32 / bf16, accumulate other than 0 / 1, overlapping blocks as stated.
 */
#define ASR_INTERCTC_RESIDENT_MAX_V 6144
int asr_softmax_rows(const void* logits, const int32_t* in_len, void* out, int B, int T, int V, int ld, int dtype, void* stream);
int asr_softmax_bwd_add(const void* p, const void* dp, const int32_t* in_len, void* grad, int B, int T, int V, int ld, int accumulate,
                        int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H */
