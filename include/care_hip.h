/*
 * care_hip.h - C ABI of libcare_hip.so: hand-written gfx950 (MI355X) kernels for the
 * captioning forward path of yangbang18/CARE.
 *
 * The reference has NO native/FFI boundary on this path (it is pure PyTorch, SURVEY.md
 * 8(b)); its seam is the two Python factories `get_framework` / `get_translator`
 * (models/Framework.py:14-51, models/Translator.py:14-19).  The host mirror of that seam
 * lives in care_amd/framework.py and care_amd/translator.py and calls the entry points
 * below through ctypes.  Each entry point names the reference code it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers are DEVICE pointers; sizes/strides are in ELEMENTS unless noted;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - returns 0 on success, a negative CARE_E* code for a rejected argument, or a
 *     positive hipError_t from the launch;
 *   - never allocates, frees or synchronises; no host-visible global state; safe to
 *     capture into a hipGraph;
 *   - activations are fp32; `wdtype` selects the storage type of weights and of the
 *     K/V caches: CARE_F32 (exact f32 MFMA, parity mode) or CARE_BF16 (bf16 MFMA with
 *     fp32 accumulation, throughput mode).  LayerNorm / softmax statistics, the concept
 *     head and all accumulators are always fp32.
 */
#ifndef CARE_HIP_H
#define CARE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CARE_ABI_VERSION 25

enum { CARE_F32 = 0, CARE_BF16 = 1 };
enum { CARE_ACT_NONE = 0, CARE_ACT_RELU = 1, CARE_ACT_GELU = 2 };
enum {
  CARE_EINVAL = -1,      /* null pointer / non-positive size */
  CARE_EALIGN = -2,      /* pointer or leading dimension not 16-byte aligned */
  CARE_ESHAPE = -3,      /* shape outside what the kernels support (stated per function) */
  CARE_EDTYPE = -4       /* unknown dtype / activation code */
};

/* ABI version of the loaded library (== CARE_ABI_VERSION). */
int care_version(void);

/* Name of the code-object architecture the library was built for ("gfx950"). */
const char* care_arch(void);

/*
 * What the library was built from (care_amd/build.py; csrc/version.hip):
 *   care_source_hash: 32 hex digits of the SHA-256 over csrc/ (.hip and .h), this header and the compile flags - the host
 *     side (care_amd/_lib.py) compares it with the hash of the tree it runs from and rebuilds or refuses a stale library;
 *   care_build_flags: the extra compile flags of the build ("" for the default library, "-DCARE_H16_FP16" for the fp16 one);
 *   care_h16: the 16-bit storage / MFMA operand type the kernels were compiled for, "bf16" (libcare_hip.so) or "fp16"
 *     (libcare_hip_f16.so).  Wherever this header says CARE_BF16 / "bf16" for a storage type it means THAT type: the two
 *     libraries are one source, and the fp16 one is the compute mode `fp16` (11 significand bits at bf16's bytes and MFMA
 *     rate).  Nothing else differs between them.
 */
const char* care_source_hash(void);
const char* care_build_flags(void);
const char* care_h16(void);

/*
 * care_gemm:  C = act(A * W^T + bias), optionally split over two destinations.
 *   Replaces every nn.Linear on the path: Embedder Linear (models/Encoder.py:167),
 *   SDPA query/key/value (models/components/Attention.py:53-56,63-67), MHA dense
 *   (SubLayers.py:35,69), FFN dense1/dense2 (SubLayers.py:129-130,143-145), concept
 *   prj / semantic2hidden (models/Predictor/pred_attribute.py:62-65,260) and the vocab
 *   projection when all logits are needed (models/Head.py:26-32, Framework.py:258-259).
 *   A [M,K] fp32 row-major, leading dim lda.  W [N,K] row-major (nn.Linear layout,
 *   leading dim K) of type wdtype.  bias [N] fp32 or NULL.
 *   Columns [0,n_split) go to C0 (leading dim ldc0, type c0_dtype), columns
 *   [n_split,N) go to C1 at column (col - n_split) (ldc1, c1_dtype); pass n_split = N
 *   and C1 = NULL for a single destination.  n_split must be a multiple of 16.
 *   Requires K % 32 == 0 (f32) or K % 64 == 0 (bf16), lda % 4 == 0, 16-byte aligned A, W.
 */
int care_gemm(const float* A, int64_t lda, const void* W, int wdtype, const float* bias,
              void* C0, int64_t ldc0, int c0_dtype, void* C1, int64_t ldc1, int c1_dtype,
              int n_split, int M, int N, int K, int act, void* stream);

/*
 * care_gemm_argmax: per-row (max, argmax, sum exp) of A * W^T without writing the logits.
 *   Replaces NaiveHead + log_softmax + the top-1 of Beam.advance for greedy decoding
 *   (models/Head.py:26-32, models/Translator.py:127, misc/Decoding/Beam.py:58-70).
 *   Writes partial results for `care_argmax_parts(N)` column groups per row:
 *   pmax/psum fp32 [M, parts], pidx int32 [M, parts]; psum = sum exp(x - pmax) over the
 *   group's columns.  Ties resolve to the lowest column index.
 */
int care_argmax_parts(int N);
int care_gemm_argmax(const float* A, int64_t lda, const void* W, int wdtype,
                     float* pmax, int32_t* pidx, float* psum, int M, int N, int K, void* stream);

/*
 * care_split3_weight / care_gemm_split3: C = A W^T + bias for fp32 A and an fp32 weight with fp32-GRADE products at a
 *   third of the 16-bit MFMA rate (the exact-f32 MFMA of care_gemm runs at 1/16): operands split into fp16 pieces,
 *   A_hi W_hi + A_hi W_lo + A_lo W_hi as one product over 3K (the dropped term is ~2^-22 of a product).  The
 *   feature embedder (models/Encoder.py:167) of concept models whose d_model the fused care_gemm_ln_split does not
 *   cover.  W3: [N, 3K] 16-bit (W_hi | W_lo | W_hi), made once by care_split3_weight; C fp32; K % 64 == 0; |A| < 65504.
 */
int care_split3_weight(const float* W, void* W3, int N, int K, void* stream);
int care_gemm_split3(const float* A, int64_t lda, const void* W3, const float* bias, float* C,
                     int64_t ldc, int M, int N, int K, void* stream);

/*
 * care_gemm_bf16 / care_gemm_argmax_bf16: the same contracts as care_gemm /
 *   care_gemm_argmax for bf16 weights, implemented by the A-stationary kernel
 *   (csrc/gemm_as.hip: A panel resident in registers, W streamed through LDS by LDS-DMA).
 *   A may be fp32 (rounded to bf16 on load) or bf16 (a_dtype); lda in elements of A.
 *   Requires K % 128 == 0 and lda % 8 == 0; care_gemm_argmax_bf16 additionally K <= 512.
 *   The number of partial column groups of the argmax variant depends on M as well:
 *   care_argmax_parts_bf16(M, N).
 */
int care_gemm_bf16(const void* A, int64_t lda, int a_dtype, const void* W, const float* bias,
                   void* C0, int64_t ldc0, int c0_dtype, void* C1, int64_t ldc1, int c1_dtype,
                   int n_split, int M, int N, int K, int act, void* stream);
int care_argmax_parts_bf16(int M, int N);
/*
 * care_gemm_bf16_splitk: K > 512 at small M (the decode-step FFN dense2, SubLayers.py:143-145):
 *   K/512 slices; slice s writes A[:, 512s:512s+512] * W[:, 512s:512s+512]^T (+ bias when
 *   s == 0) to the fp32 slab C + s * slab_stride.  The slabs are summed by the consumer,
 *   care_add_ln(nslab = K / 512, slab_stride), so no reduction pass exists.  K % 512 == 0.
 */
int care_gemm_bf16_splitk(const void* A, int64_t lda, int a_dtype, const void* W,
                          const float* bias, float* C, int64_t ldc, int64_t slab_stride,
                          int M, int N, int K, void* stream);
int care_gemm_argmax_bf16(const void* A, int64_t lda, int a_dtype, const void* W, float* pmax,
                          int32_t* pidx, float* psum, const int32_t* labels, float* plab,
                          int M, int N, int K, void* stream);

/*
 * care_gemm_tile / care_gemm_tile_argmax: the contracts of care_gemm_bf16 / care_gemm_argmax_bf16 for bf16 A
 *   and ANY K % 64 == 0 (csrc/gemm_tile.hip: both operands streamed through an LDS ring by LDS-DMA in K steps of
 *   64, 64 x 64 output tiles per wave) - the nn.Linear layers of the d_model = 768 / 1024 architectures
 *   (config/archs.yaml:15-26: K = 768, 1024, 3072, 4096; the same reference lines as care_gemm), and the
 *   vocabulary projection of greedy decoding / teacher-forced scoring there (models/Head.py:26-32,
 *   Translator.py:127, misc/Crit/crit_lang.py:75-103).  A bf16 [M, lda], W bf16 [N, K], lda % 8 == 0.
 *   care_gemm_tile_argmax writes care_argmax_parts_tile(N) partials per row (one per 64 columns); labels / plab
 *   (optional, both or neither) as in care_gemm_argmax_bf16.
 */
/* care_split2_act / care_gemm_tile_split3: the contract of care_gemm_split3 (fp32 A, fp32-GRADE products
 *   a_hi w_hi + a_hi w_lo + a_lo w_hi in fp16 pieces: the feature embedder of concept models, models/Encoder.py:167)
 *   on the LDS-tiled kernel: A2 = care_split2_act(A) fp16 [M, 2K] (hi | lo), W3 = care_split3_weight(W) [N, 3K];
 *   destinations, split and activation as care_gemm.  K % 64 == 0, |A| < 65504. */
int care_split2_act(const float* A, int64_t lda, void* A2, int M, int K, void* stream);
int care_gemm_tile_split3(const void* A2, const void* W3, const float* bias, void* C0, int64_t ldc0, int c0_dtype,
                          void* C1, int64_t ldc1, int c1_dtype, int n_split, int M, int N, int K, int act,
                          void* stream);
/* Split products of PRE-SCALED operands - the GEMMs of training mode (models/Wrapper.py:423-435 -> Framework.py:215-237 under
 *   autograd: every nn.Linear's forward, dx = dy W and dW = dy^T x; care_amd/training.py).  Gradients are 1e-6 .. 1e-3: the low
 *   piece of an unscaled hi / lo split would be an fp16 denormal.  care_absmax: *slot (4 bytes, device) = bit pattern of max |A|
 *   (the function zeroes it first; NaNs skipped).  care_split_pieces: the fp16 pieces of src * 2^e, e chosen from *amax so that
 *   the largest magnitude lies in [2^14, 2^15) (exact in fp32; zero / non-finite maxima: e = 0), read from the operand as it
 *   lies - [rows, K], or transposed [K, rows] - and written slab-major: [slabs][rows][pieces ks], pieces = 2 (hi | lo: the A
 *   operand, care_split2_act's layout per slab) or 3 (hi | lo | hi: the W operand, care_split3_weight's); slab s = columns
 *   s ks .. of the operand, zeros past K; ks % 64 == 0.  care_gemm_tile_split3_scaled: C [M, ldc] fp32 =
 *   (A2 W3^T) / (2^ea 2^eb) + bias, the exponents re-derived from the same two slots.  No host synchronisation anywhere:
 *   the scales never leave the device.  K % 64 == 0, lda % 4 == 0.  slabs > 1: split-K for products with few output tiles
 *   (dW = dy^T x): A2 / W3 hold `slabs` matrices of K columns each (consecutive K ranges of the product), slab s goes to
 *   C + s M ldc, the caller adds them in order (care_strided_sum); bias == NULL then. */
int care_absmax(const float* A, int64_t lda, int M, int K, void* slot, void* stream);
int care_split_pieces(const float* src, int64_t ld, int rows, int K, int transposed, int slabs, int ks, void* out,
                      int pieces, const void* amax, void* stream);
int care_gemm_tile_split3_scaled(const void* A2, const void* W3, const float* bias, float* C, int64_t ldc, int M, int N,
                                 int K, const void* amax_a, const void* amax_b, int slabs, void* stream);
/* ... and the fused vocabulary arg-max (care_gemm_tile_argmax's partials) on the same split products: the `fp16x3`
 *   compute mode (fp32 storage, every GEMM as three fp16 MFMA passes) of care_amd/engine.py. */
int care_gemm_tile_split3_argmax(const void* A2, const void* W3, float* pmax, int32_t* pidx, float* psum, int M,
                                 int N, int K, void* stream);
int care_gemm_tile(const void* A, int64_t lda, const void* W, const float* bias, void* C0, int64_t ldc0,
                   int c0_dtype, void* C1, int64_t ldc1, int c1_dtype, int n_split, int M, int N, int K,
                   int act, void* stream);
int care_argmax_parts_tile(int N);
/* care_gemm_tile_batched: `batch` independent products C_b = A_b W_b^T + bias_b in one launch (element offsets a_bs,
 *   w_bs, c_bs, bias_bs per batch; W rows of leading dimension ldw): the per-head projections on either side of the
 *   absorbed cross-attention for d_model = 1024 - the roles of care_head_expand / care_head_reduce
 *   (models/components/Attention.py:63-67 moved to the query / context side). */
int care_gemm_tile_batched(const void* A, int64_t lda, int64_t a_bs, const void* W, int64_t ldw, int64_t w_bs,
                           const float* bias, int bias_bs, void* C, int64_t ldc, int64_t c_bs, int c_dtype, int batch,
                           int M, int N, int K, void* stream);
int care_gemm_tile_argmax(const void* A, int64_t lda, const void* W, float* pmax, int32_t* pidx, float* psum,
                          const int32_t* labels, float* plab, int M, int N, int K, void* stream);

/*
 * Teacher-forced scoring (the metrics step): log-probability of the label token and the arg-max
 *   token of every row.  Replaces log_softmax + gather / max of LanguageGeneration
 *   (misc/Crit/crit_lang.py:75-103: word accuracy, perplexity) for the eval metrics step
 *   (models/Wrapper.py:182-184).
 *   care_gemm_argmax_bf16 with labels/plab non-NULL also records, per column group, the logit
 *   of column labels[row] (-inf where the group does not contain it);
 *   care_score_partials reduces the groups: logp[r] = x[label] - max - log(sum exp(x - max)),
 *   pred[r] = arg-max column.  The [rows, V] logits are never written.
 *   care_score_logits does the same from materialised logits [rows, ld] (fp32 mode / checker).
 */
int care_score_partials(const float* pmax, const int32_t* pidx, const float* psum,
                        const float* plab, int parts, float* logp, int32_t* pred, int rows,
                        void* stream);
/* The label logit on its own (so that the arg-max statistics can come from the fastest kernel, which keeps none):
 *   care_label_logits: out[r] = A[r, :] . W[col[r], :], bf16 A [rows, lda] and W [N, K], fp32 accumulation;
 *   care_score_partials_lab: care_score_partials with that one logit per row instead of per-group label partials. */
int care_label_logits(const void* A, int64_t lda, const void* W, const int32_t* col, float* out, int rows, int N,
                      int K, void* stream);
int care_score_partials_lab(const float* pmax, const int32_t* pidx, const float* psum, int parts,
                            const float* lab_logit, float* logp, int32_t* pred, int rows, void* stream);
int care_score_logits(const float* logits, int64_t ld, int V, const int32_t* labels, float* logp,
                      int32_t* pred, int rows, void* stream);

/*
 * care_greedy_update: finish the argmax over the partials and advance the greedy state.
 *   Replaces Beam.advance / Beam.done for beam_size == 1 (misc/Decoding/Beam.py:45-85)
 *   and the bookkeeping of Translator_ARFormer.beam_decode_step
 *   (models/Translator.py:91-109,135-143) without the per-step host sync.
 *   For every row r: tok = argmax, logp = -log(sum exp(x - max)).  If the row is not
 *   finished: fed[r, t] = tok, score[r] += logp, length[r] = t, and the row finishes
 *   when tok == eos_id or t == max_steps.  `fed` is int32 [rows, fed_stride]; column 0
 *   holds BOS.  Finished rows keep running (rows are independent) but are frozen.
 */
int care_greedy_update(const float* pmax, const int32_t* pidx, const float* psum, int parts,
                       int32_t* fed, int fed_stride, float* score, int32_t* length,
                       int32_t* finished, int t, int max_steps, int eos_id, int rows,
                       void* stream);

/*
 * care_greedy_update_embed: care_greedy_update for step t, and in the same launch the embedding of
 *   the chosen token at position t - word[token] + pos[t] (+ sem[r / sem_div]) -> LayerNorm ->
 *   out / out_bf16 - i.e. the care_embed_ln call of decode step t + 1 (Embeddings.forward,
 *   models/components/Embeddings.py) fused behind Beam.advance's token choice.  One launch per
 *   decoder step less.  word fp32 [V, d], pos fp32 [>= t + 1, d], sem (optional) fp32.
 */
int care_greedy_update_embed(const float* pmax, const int32_t* pidx, const float* psum, int parts,
                             int32_t* fed, int fed_stride, float* score, int32_t* length,
                             int32_t* finished, int t, int max_steps, int eos_id, int rows,
                             const float* word, const float* pos, const float* sem, int sem_div,
                             const float* gamma, const float* beta, float eps, float* out,
                             void* out_bf16, int64_t ldo, int d, void* stream);

/*
 * care_sample_logits: draw one token per row from the row's logits - temperature, top-k, nucleus (top-p) - and hand it to
 *   care_greedy_update / care_greedy_update_embed through their parts = 1 contract (csrc/sample.hip).  No reference
 *   counterpart: the reference decodes by beam search only.
 *   logits fp32 [rows, ld], columns V .. ld - 1 are never read; -inf entries carry probability 0 and are never chosen.
 *   params: a 24-byte DEVICE block, 16-byte aligned, read by the kernel - so a captured hipGraph replays with a new seed or
 *   new settings: { uint64 seed; float inv_temperature; float top_p; int32 top_k; int32 reserved }.
 *   Per row, x = logits[row, 0 : V]:
 *     1. s_i = x_i * inv_temperature;
 *     2. top-k (off for top_k <= 0 or >= V): the top_k first entries by (s descending, index ascending);
 *     3. top-p (off for top_p >= 1): of those, in that order, with q_i = exp(s_i - m) / Z over them, entry j stays when the
 *        summed q of the entries before it is < top_p - the smallest prefix whose mass reaches top_p, never empty;
 *     4. tok = argmax over the kept set of s_i + g_i, ties to the lower index (Gumbel-max: stateless, a row is checkable on
 *        its own): g_i = -logf(-logf(u_i)), u_i = (2 k + 1) 2^-24 with k the top 23 bits of h(h(seed, (key << 16) | t), i),
 *        h(a, n) = fin(a + 0x9E3779B97F4A7C15 (n + 1)), fin the splitmix64 finaliser, key = row_key[row] (NULL: the row
 *        index), t the decoder step (1-based).  u lies in (0, 1) and is exact in fp32; g <= 16.64, so a Gumbel tail of
 *        probability 6e-8 per entry is cut off.
 *   Out, all [rows]: pmax = x[tok], pidx = tok, psum = sum over ALL V columns of exp(x_i - x[tok]) (so -log psum is the
 *   MODEL's log-probability of tok at temperature 1); logq (optional) = s_tok - logsumexp over the kept set of s, the
 *   log-probability under the distribution sampled from; nkept (optional) = the size of the kept set.
 *   Deterministic (fixed reduction orders, no floating-point atomics); a row's result depends on its logits, key, t and
 *   params alone.  rows == 0 is a no-op.  CARE_EINVAL: rows < 0, V < 1, ld < V, t < 1, a NULL logits / params / pmax / pidx /
 *   psum; CARE_EALIGN: params not 16-byte aligned.
 * care_sample_accum: score_q[r] += logq[r] for every row with finished[r] == 0 - the running sum of logq of a sampled
 *   decode, issued in front of the step's care_greedy_update, which sets `finished`.
 */
int care_sample_logits(const float* logits, int64_t ld, int V, int rows, const int32_t* row_key, int t,
                       const void* params, float* pmax, int32_t* pidx, float* psum, float* logq, int32_t* nkept,
                       void* stream);
int care_sample_accum(const float* logq, const int32_t* finished, float* score_q, int rows, void* stream);

/*
 * care_add_ln: out = LayerNorm(x + res) * gamma + beta, row-wise over d columns.
 *   Replaces nn.LayerNorm after the Embedder Linear (models/Encoder.py:167) and the
 *   post-LN residual epilogues of MultiHeadAttention / PositionwiseFeedForward
 *   (SubLayers.py:73-79,147-150).  res may be NULL.  If pos is non-NULL, pos[(r % grp), :]
 *   is added as well (TransformerEncoderBase position embedding, Encoder.py:265-279).
 *   Output row of input row r: (r / grp) * out_grp_rows + out_row_off + (r % grp), so an
 *   encoder stream lands directly inside the [B, Lk, d] cross-attention memory
 *   (the torch.cat of Encoder.py:148-149 and Framework.py:184-185 becomes an offset).
 *   out_bf16 (optional, same layout and ldo as out): a bf16 mirror of the result, the A
 *   operand of the next bf16 GEMM (the same rounding that GEMM would apply on load).
 *   nslab > 1: x is the sum of nslab fp32 slabs spaced slab_stride elements apart (the
 *   split-K partial products of care_gemm_bf16_splitk); nslab = 1 otherwise.
 *   gamma == beta == NULL: NO LayerNorm - out = x + res (+ pos): the sub-blocks of a pre-LN decoder
 *   (`transformer_pre_ln`, opts.py:68; SubLayers.py:55,78,140,149: LayerNorm BEFORE the sub-block, the residual sum left
 *   as it is); care_embed_ln likewise (Embeddings.py:130: no LayerNorm after the embedding sum).
 *   d % 4 == 0, d <= 2048.
 */
int care_add_ln(const float* x, int64_t ldx, const float* res, int64_t ldres,
                const float* pos, const float* gamma, const float* beta, float eps,
                float* out, void* out_bf16, int64_t ldo, int rows, int d, int grp,
                int out_grp_rows, int out_row_off, int nslab, int64_t slab_stride, void* stream);

/*
 * care_gemm_ln: out = LayerNorm(A W^T + bias + res + pos) * gamma + beta with N = d_model = 512,
 *   one workgroup owning full output rows (csrc/gemm_ln.hip).  Fuses the Linear -> LayerNorm of
 *   the Embedder (models/Encoder.py:167) and the dense -> dropout -> +residual -> LayerNorm
 *   epilogues of MultiHeadAttention / PositionwiseFeedForward (SubLayers.py:69-79,143-150).
 *   A [M, K] fp32 (raw features; rounded to bf16 when multiplied) or bf16; W bf16 [512, K];
 *   bias/gamma/beta fp32 [512]; res (optional) fp32 [M, ldres]; pos (optional) fp32 [grp, 512]
 *   added per row r as pos[r % grp].  Output rows are remapped exactly like care_add_ln
 *   (grp / out_grp_rows / out_row_off); out fp32 and the bf16 mirror share ldo; either may be
 *   NULL (not both): a caller that only feeds bf16 GEMMs / the absorbed cross-attention needs no
 *   fp32 copy.  Requires N == 512, K % 32 == 0.
 */
int care_gemm_ln(const void* A, int64_t lda, int a_dtype, const void* W, const float* bias,
                 const float* res, int64_t ldres, const float* pos, const float* gamma,
                 const float* beta, float eps, float* out, void* out_bf16, int64_t ldo, int M,
                 int N, int K, int grp, int out_grp_rows, int out_row_off, void* stream);

/*
 * care_pack_ln_weight / care_gemm_ln_packed: the same fused Linear -> (+residual) -> LayerNorm with
 *   the [512, K] bf16 weight re-laid-out ONCE (at weight-load time) into the order the kernel streams
 *   it: for every K step of 32 the 32-KB LDS image of that step (rows in order, 16-byte chunks at
 *   their bank-swizzled positions), so every DMA instruction reads 1 KB of full cache lines instead
 *   of sixteen 64-byte row pieces.  Same arithmetic, bit for bit, as care_gemm_ln on the plain
 *   weight.  K % 64 (fp32 A) / K % 128 (bf16 A) == 0; no position table.  W_packed: K * 1024 bytes.
 */
int care_pack_ln_weight(const void* W, void* W_packed, int N, int K, void* stream);
int care_gemm_ln_packed(const void* A, int64_t lda, int a_dtype, const void* W_packed,
                        const float* bias, const float* res, int64_t ldres, const float* gamma,
                        const float* beta, float eps, float* out, void* out_bf16, int64_t ldo,
                        int M, int N, int K, int grp, int out_grp_rows, int out_row_off,
                        void* stream);

/*
 * care_pack_ln_weight_split / care_gemm_ln_split: the Embedder's Linear -> LayerNorm
 *   (models/Encoder.py:167) for models whose memory feeds the DISCRETE concept choice
 *   (pred_attribute.py:88-125,262-264): fp32 A and an fp32 [512, K] weight, multiplied as
 *   a_hi w_hi + a_hi w_lo + a_lo w_hi with x_hi = fp16(x), x_lo = fp16(x - x_hi) - three fp16 MFMA
 *   passes accumulated in fp32 (11 bits per piece: the dropped a_lo w_lo term is ~2^-22 of a product,
 *   fp32-grade, against bf16's 2^-9 per operand).  |x| < 65504.  W_split: 3 * K * 1024 bytes (per K
 *   step of 32 the LDS images of w_hi, w_lo, w_hi).  K % 64 == 0; no residual, no position table.
 */
int care_pack_ln_weight_split(const float* W, void* W_split, int N, int K, void* stream);
int care_gemm_ln_split(const void* A, int64_t lda, const void* W_split, const float* bias,
                       const float* gamma, const float* beta, float eps, float* out,
                       void* out_bf16, int64_t ldo, int M, int N, int K, int grp,
                       int out_grp_rows, int out_row_off, void* stream);

/*
 * care_group_mean: out[g, col_off + c] = mean over the grp rows of group g of x[., c].
 *   Replaces `item.mean(1)` per modality (models/Encoder.py:106); with ldo = n_mod * d and
 *   col_off = m * d it also performs the channel concat of pred_attribute.py:88-89.
 *   Input row of (g, i): g * in_grp_rows + in_row_off + i.
 */
int care_group_mean(const float* x, int64_t ldx, int in_grp_rows, int in_row_off, int grp,
                    float* out, int64_t ldo, int col_off, int groups, int d, void* stream);

/*
 * care_concept_finish: concept probabilities from concept scores.
 *   Replaces prepare_merged_probs for seq_len == 1, restated literally
 *   (models/Predictor/pred_attribute.py:17-46): p = sigmoid(s);
 *   preds = 1 - exp(log(clamp(1 - p, 1e-12, 1))); avg = mean_k p.
 *   scores [B, lds] fp32 (k valid columns) -> preds [B, ldp] (columns >= k zeroed up to
 *   ldp so the buffer can feed care_gemm with K = ldp), avg [B].
 */
int care_concept_finish(const float* scores, int64_t lds, float* preds, int64_t ldp,
                        float* avg, int B, int k, void* stream);

/*
 * care_concept_topk_embed: top-`topk` concepts -> embedded concept rows in the memory.
 *   Replaces SemanticContainer.forward's topk + NaiveEmbeddings
 *   (models/Predictor/pred_attribute.py:262-270, models/components/Embeddings.py:53-87):
 *   labels[b, j] = index of the j-th largest preds[b, :] (order: value desc, index asc;
 *   torch leaves the order of exact ties unspecified);
 *   out[b * out_grp_rows + out_row_off + j, :] = LN(word[labels[b,j]] + pos[j]).
 *   word == NULL: the labels alone - a model without local guidance (`use_attr_flags` G1L0:
 *   pred_attribute.py:252 builds no `attr_embs`, :276-277 leaves `semantic_embs` None).
 *   k <= 1024, topk <= 64, d % 4 == 0, d <= 2048.
 */
int care_concept_topk_embed(const float* preds, int64_t ldp, int k, int topk,
                            const float* word, const float* pos, const float* gamma,
                            const float* beta, float eps, int64_t* labels, float* out,
                            void* out_bf16, int64_t ldo, int out_grp_rows, int out_row_off,
                            int B, int d, void* stream);

/*
 * care_embed_ln: decoder input embedding.
 *   Replaces Embeddings.forward (models/components/Embeddings.py:134-188):
 *   out[r] = LN(word[tok(r)] + pos[pos0 + r % seq] + sem[r / sem_div]) with
 *   tok(r) = tokens[(r / seq) * tok_stride + tok_off + r % seq] (int32).  sem may be NULL
 *   (no global semantic guidance).  seq = 1 for an incremental decode step.
 *   If anc is non-NULL (beam search) the token row is anc[(r / seq) * anc_stride + col]
 *   instead of (r / seq), col = tok_off + r % seq.
 */
int care_embed_ln(const int32_t* tokens, int tok_stride, int tok_off, const int32_t* anc,
                  int anc_stride, const float* word, const float* pos, int pos0,
                  const float* sem, int sem_div, const float* gamma, const float* beta,
                  float eps, float* out, void* out_bf16, int64_t ldo, int rows, int seq, int d,
                  void* stream);

/*
 * care_attention: scaled-dot-product attention for single query rows, head dim 64.
 *   Replaces ScaledDotProductAttention.forward after the projections
 *   (models/components/Attention.py:83-131): scores = q.k / 8 -> masked_fill(-1e9) ->
 *   + hybrid_bias[h, j] -> softmax -> P.V, for every (row, head).
 *   Q [rows, ldq] fp32 (head h at columns h*64..).  K and V of type kv_dtype; key j of
 *   query row r lives at  base + kvb * kv_batch_stride + j * kv_row_stride + h * 64  with
 *   kvb = anc ? anc[r * anc_stride + j] : r / rows_per_kv.
 *   Number of keys of row r: causal ? min(nkeys, r % seq + 1 + causal_off) : nkeys.
 *   pad_tok (int32, optional): key j of row r is masked when
 *   pad_tok[ptb * pad_stride + j] == pad_id, ptb = anc ? anc[r*anc_stride + j] : r / rows_per_kv
 *   (the key-pad mask of models/Decoder/Transformer.py:15-28,169-174).
 *   bias (optional) fp32 [H, bias_ld].  ctx [rows, ldctx] of type ctx_dtype (bf16 when the
 *   context only feeds a bf16 GEMM).  nkeys <= 128.
 */
int care_attention(const float* Q, int64_t ldq, const void* K, const void* V, int kv_dtype,
                   int64_t kv_batch_stride, int64_t kv_row_stride, int rows_per_kv,
                   const int32_t* anc, int anc_stride, int nkeys, int causal, int seq,
                   int causal_off, const int32_t* pad_tok, int pad_stride, int pad_id,
                   const float* bias, int bias_ld, void* ctx, int64_t ldctx, int ctx_dtype,
                   int rows, int heads, void* stream);

/*
 * care_attention_seq: the same attention (models/components/Attention.py:83-131) for WHOLE query sequences of
 *   seq <= 32 positions with bf16 operands - the teacher-forced forward (models/Framework.py:215-237,
 *   Decoder/Transformer.py:161-268) - one wave per (sequence, head), K and V read once for all positions,
 *   QK^T and PV on the matrix cores (csrc/attention_seq.hip).
 *   Q bf16 [nseq * seq, ldq] (head h at columns h*64..); key j of sequence s at
 *   base + (s / seqs_per_kv) * kv_batch_stride + j * kv_row_stride + h * 64 (elements, bf16) for K and V.
 *   causal: query position i sees keys j <= i.  pad_tok (int32, optional): key j is masked (-1e9, before the
 *   bias) when pad_tok[(s / seqs_per_kv) * pad_stride + j] == pad_id.  bias fp32 [heads, bias_ld] or NULL.
 *   ctx bf16 [nseq * seq, ldctx].  nkeys <= 128.
 */
int care_attention_seq(const void* Q, int64_t ldq, const void* K, const void* V, int64_t kv_batch_stride,
                       int64_t kv_row_stride, int seqs_per_kv, int nkeys, int causal, int seq,
                       const int32_t* pad_tok, int pad_stride, int pad_id, const float* bias, int bias_ld,
                       void* ctx, int64_t ldctx, int nseq, int heads, void* stream);

/*
 * care_attention_latent: the cross-attention of a decoder step with W_k / W_v absorbed into
 *   the query / context side (bf16 mode, d_model = 512).  Same reference lines as
 *   care_attention (models/components/Attention.py:63-67,83-131), re-associated:
 *     scores[h][j] = (W_k,h^T q_h / 8) . mem_j   (+ a per-head constant the softmax cancels)
 *     ct[h]        = sum_j softmax_j(scores[h][j] + bias[h][j]) mem_j
 *   so every step reads ONE bf16 copy of the memory row instead of projected K and V.
 *   qt  bf16 [rows, heads, d] (row stride ldq): the expanded, pre-scaled queries.
 *   mem bf16: key j of row r at  mem + (r / rows_per_kv) * mem_batch_stride + j * mem_row_stride.
 *   bias fp32 [heads, bias_ld] or NULL.  ct bf16 [rows, heads, d] (row stride ldc); the caller
 *   finishes ctx_h = W_v,h ct[h] + b_v,h.  nkeys <= 128, heads <= 16, d == 512 (one wave per row) or d == 1024
 *   (two waves per row, each owning 512 dims; the partial scores cross through LDS).
 */
int care_attention_latent(const void* qt, int64_t ldq, const void* mem, int64_t mem_batch_stride,
                          int64_t mem_row_stride, int rows_per_kv, int nkeys, const float* bias,
                          int bias_ld, void* ct, int64_t ldc, int rows, int heads, int d,
                          void* stream);

/*
 * care_head_expand / care_head_reduce: the per-head projections on either side of
 *   care_attention_latent (the key / value halves of models/components/Attention.py:63-67 moved
 *   from the memory to the query / context):
 *     qt[r][h][c]     = sum_e q[r][h*64+e] * wkt[h][c][e]        wkt = W_k,h^T / 8, bf16 [H][512][64]
 *     ctx[r][h*64+e]  = sum_c ct[r][h][c] * wv[h*64+e][c] + bv   wv = W_v bf16 [512][512], bv fp32 or NULL
 *   q bf16 [rows, ldq], qt / ct bf16 [rows, heads, 512] (row strides ldo / ldc), ctx bf16 [rows, ldo].
 *   d_model = 512, head dim 64.
 */
int care_head_expand(const void* q, int64_t ldq, const void* wkt, void* qt, int64_t ldo, int rows,
                     int heads, void* stream);
int care_head_reduce(const void* ct, int64_t ldc, const void* wv, const float* bv, void* ctx,
                     int64_t ldo, int rows, int heads, void* stream);

/*
 * care_beam_select: per row of logits [rows, ldl] (V valid columns): the beam_size best
 *   columns as log-probabilities.  Replaces torch.log_softmax(logits, dim=1)
 *   (models/Translator.py:127) plus the per-row part of the flattened topk of
 *   Beam.advance (misc/Decoding/Beam.py:60): cand_val[r, k] = (x - max) - log(sum exp(x - max))
 *   of the k-th best column (value desc, index asc), cand_idx[r, k] its column.  bm <= 8.
 *   waves_per_row: 1 (a 64-lane wave walks a row), or 4 for few rows (a workgroup per row, four partial lists merged:
 *   the same columns in the same order, the log-sum-exp added in another order).
 */
int care_beam_select(const float* logits, int64_t ldl, int V, int bm, float* cand_val,
                     int32_t* cand_idx, int rows, int waves_per_row, void* stream);

/*
 * care_ensemble_select: care_beam_select for a LIST of models (model ensembling, models/Translator.py:112-133): per row the
 *   beam_size best columns of the members' log_softmax rows AVERAGED equally - torch.stack(word_probs).mean(0), :130-131 - as they
 *   are (an average of log-probabilities is not renormalised; the reference's Beam.advance adds it to the beam's score as it is).
 *   logits: HOST array of n_models (<= 8) device pointers, each fp32 [rows, ldl] with V valid columns; cand_val / cand_idx
 *   [rows, bm] in the format care_beam_advance reads (value desc, column asc); bm <= 8.  The averaged array never exists.
 */
int care_ensemble_select(const float* const* logits, int n_models, int64_t ldl, int V, int bm, float* cand_val,
                         int32_t* cand_idx, int rows, void* stream);

/*
 * Fused beam selection (bf16 mode): the per-row top beam_size of log_softmax(x W^T) without the
 *   [rows, V] logits in memory.  Replaces torch.log_softmax (models/Translator.py:127) + the per-row
 *   part of Beam.advance's top-k (misc/Decoding/Beam.py:60) exactly like care_beam_select does:
 *     1. care_gemm_argmax_bf16_min : care_gemm_argmax_bf16 with at least `min_parts` column ranges
 *        (care_argmax_parts_bf16_min, called with the same M, N, K, a_dtype and min_parts, gives the
 *        count: at large row counts the kernel balances its column ranges over whole launch rounds)
 *        -> pmax / pidx / psum [M, parts];
 *     2. care_beam_threshold      : thr[r] = bm-th largest range maximum of row r (a lower bound of
 *        the row's bm-th best logit); cnt[r] = 0;
 *     3. care_gemm_collect_bf16   : the same product; every logit >= thr[r] is appended to row r's
 *        candidate list cval / cidx [M, cap] (cnt[r] counts them, also past cap);
 *     4. care_beam_pick           : cand_val / cand_idx [rows, bm] = the bm best candidates (value
 *        desc, column asc) as log-probabilities; a row with cnt > cap is recomputed exactly from
 *        A and W inside the kernel.
 */
int care_argmax_parts_bf16_min(int M, int N, int K, int a_dtype, int min_parts);
int care_gemm_argmax_bf16_min(const void* A, int64_t lda, int a_dtype, const void* W, float* pmax,
                              int32_t* pidx, float* psum, int M, int N, int K, int min_parts,
                              void* stream);
int care_beam_threshold(const float* pmax, int parts, int bm, float* thr, int32_t* cnt, int rows,
                        void* stream);
int care_gemm_collect_bf16(const void* A, int64_t lda, int a_dtype, const void* W, const float* thr,
                           int32_t* cnt, float* cval, int32_t* cidx, int cap, int M, int N, int K,
                           void* stream);
/*
 * The SPARSE second pass (large row counts, K = 512, bf16 rows: care_beam_sparse_applies): step 1 as
 *   care_gemm_argmax_bf16_tiles, which also writes tile_max [ceil(N / 32), M] fp32 - the maximum of every
 *   (32-column tile, row); step 3 as care_beam_sparse_collect, which lists per tile the rows whose tile
 *   maximum reaches thr[row] (tcount [2 tiles + 1], tlist [tiles, M] int32 scratch: counts, then the
 *   prefix sums of the 128-entry work units) and recomputes ONLY those
 *   (tile, row) products - the same MFMA chain as the first pass, bit-identical logits - appending the
 *   logits >= thr[row] to cval / cidx exactly like care_gemm_collect_bf16 (~2 % of its arithmetic).
 */
int care_beam_sparse_applies(int M, int N, int K, int a_dtype);
int care_gemm_argmax_bf16_tiles(const void* A, int64_t lda, int a_dtype, const void* W, float* pmax,
                                int32_t* pidx, float* psum, float* tile_max, int M, int N, int K,
                                int min_parts, void* stream);
int care_beam_sparse_collect(const void* A, int64_t lda, const void* W, const float* tile_max,
                             const float* thr, int32_t* cnt, float* cval, int32_t* cidx, int cap,
                             int32_t* tcount, int32_t* tlist, int M, int N, int K, void* stream);
int care_beam_pick(const float* pmax, const float* psum, int parts, const int32_t* cnt,
                   const float* cval, const int32_t* cidx, int cap, int bm, const void* A, int64_t lda,
                   int a_dtype, const void* W, int V, int K, float* cand_val, int32_t* cand_idx,
                   int rows, void* stream);

/*
 * Beam selection from GROUP MAXIMA of the LDS-tiled vocabulary product (16-bit modes, a few hundred to a few thousand
 *   rows; replaces the same reference lines as care_beam_select: models/Translator.py:127, misc/Decoding/Beam.py:60):
 *     1. care_gemm_tile_beam   : x W^T on csrc/gemm_tile.hip without writing logits - per (row, 64-column part)
 *        pmax / psum [M, parts] (maximum, sum exp(x - max)) and gmax [M, parts, 16]: the maxima of the part's sixteen
 *        4-column groups (-inf for groups past N); parts = care_argmax_parts_tile(N);
 *     2. care_beam_pick_groups : one wave per row - log-sum-exp from the parts; the bm parts with the largest maxima; the
 *        bm best of their 16 bm groups (a row's bm best logits lie in its bm best groups); those 4 bm logits recomputed
 *        from A and W (the tile kernel's MFMA, operand roles and K order: the same bits); cand_val / cand_idx [rows, bm]
 *        = the bm best as log-probabilities (value desc, column asc), the format care_beam_advance reads.
 *   A bf16 [M, lda] (lda % 8 == 0), W bf16 [N, K], K % 64 == 0, bm <= 8, 128 <= N <= 16384; gmax 16-byte aligned.
 */
int care_gemm_tile_beam(const void* A, int64_t lda, const void* W, float* pmax, float* psum, float* gmax, int M,
                        int N, int K, void* stream);
int care_beam_pick_groups(const float* pmax, const float* psum, const float* gmax, int parts, int bm, const void* A,
                          int64_t lda, const void* W, int V, int K, float* cand_val, int32_t* cand_idx, int rows,
                          void* stream);

/*
 * care_beam_advance: one beam-search step for every clip (B clips x bm beams), on device.
 *   Replaces Beam.advance / Beam.done (misc/Decoding/Beam.py:38-85), the re-ordering of the
 *   beams' prefixes (Beam.get_tentative_hypothesis, :112-117) and the removal of finished
 *   clips (models/Translator.py:145-209; clips are frozen instead, rows are independent).
 *   State, all device arrays: scores fp32 [B*bm]; tokphys int32 [B*bm, stride] physical
 *   token store (column 0 = BOS); anc_old -> anc_new int32 [B*bm, stride] ancestor tables
 *   (anc[row, j] = physical row holding position j of the hypothesis in beam slot `row`;
 *   initialise anc[row, 0] = row); done / n_fin int32 [B]; finished hypotheses
 *   fin_score fp32, fin_len int32 [B, fin_cap], fin_hyp int32 [B, fin_cap, stride]
 *   (tokens without BOS), recorded in the reference's order.  t = 1-based step,
 *   max_steps = max_len - 1, need = max(beam_size, topk) <= fin_cap, V = vocabulary size
 *   (ties between equal candidates resolve to the lower flattened index beam*V + column).
 *   One wave per clip: stride (= max_len) <= 64, bm <= 8.
 */
int care_beam_advance(const float* cand_val, const int32_t* cand_idx, float* scores, int bm,
                      int32_t* tokphys, const int32_t* anc_old, int32_t* anc_new,
                      int32_t* done, int32_t* n_fin, int fin_cap, float* fin_score,
                      int32_t* fin_len, int32_t* fin_hyp, int t, int max_steps, int need,
                      int eos_id, int V, int stride, int B, void* stream);

/*
 * care_attention_probs: the attention probabilities [rows, heads, nkeys] fp32 of one attention
 *   (scale 1/8, key-padding mask -> -1e9, then the optional per-head/per-key bias, softmax) - the
 *   `attention_probs` entries of the dict TransformerDecoder.forward returns
 *   (models/Decoder/Transformer.py:239-252, Attention.py:104-118).  Off the decode path: the fused
 *   kernels never materialise them; this is for the teacher-forced forward's auxiliary outputs.
 *   Q fp32 [rows, heads * 64]; K as in care_attention (no ancestor table); causal as there.
 */
int care_attention_probs(const float* Q, int64_t ldq, const void* K, int kv_dtype,
                         int64_t kv_batch_stride, int64_t kv_row_stride, int rows_per_kv, int nkeys,
                         int causal, int seq, const int32_t* pad_tok, int pad_stride, int pad_id,
                         const float* bias, int bias_ld, float* probs, int rows, int heads,
                         void* stream);

/*
 * Active-set compaction of the decode loop (csrc/compact.hip).  The reference ends a batch when every
 * instance is done and removes finished instances from every cached tensor at each step
 * (models/Translator.py:77-81,194-209); here the loop runs in segments and compacts between them.
 *   care_active_slots: idx[0 .. cnt) = the slots with finished == 0 in ascending order, idx[cnt .. n)
 *     = the finished ones in ascending order (a stable partition), count[0] = cnt.  n <= 2^30.
 *   care_gather_rows:  dst row i = src row idx[i], i < n.
 *   care_scatter_rows: dst row idx[i] = src row i, i < n; rows with idx[i] < 0 are skipped.
 *   row_bytes and the strides are multiples of 4 (16-byte vectors are used when everything allows).
 */
int care_active_slots(const int32_t* finished, int n, int32_t* idx, int32_t* count, void* stream);
int care_gather_rows(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes,
                     const int32_t* idx, int n, int64_t row_bytes, void* stream);
int care_scatter_rows(const void* src, int64_t src_stride_bytes, void* dst, int64_t dst_stride_bytes,
                      const int32_t* idx, int n, int64_t row_bytes, void* stream);
/* Beam search keeps bm consecutive rows per clip and ancestor tables that name physical rows:
 *   care_expand_index: idx_r[k * bm + j] = idx_c[k] * bm + j  (clip slots -> row slots), k < m;
 *   care_remap_rows:   anc[i] = cmap[anc[i] / bm] * bm + anc[i] % bm for the n entries of a table, after
 *     the rows of clip c have moved to clip cmap[c]. */
int care_expand_index(const int32_t* idx_c, int m, int bm, int32_t* idx_r, void* stream);
int care_remap_rows(int32_t* anc, int64_t n, const int32_t* cmap, int bm, void* stream);

/*
 * Training mode (models/Wrapper.py:423-435 -> models/Framework.py:215-237 under autograd; care_amd/training.py):
 *   everything of a backward pass that is not a GEMM (those re-use care_gemm on transposed operands).  fp32.
 *   care_ln_bwd: backward of care_add_ln (y = LN(x + res) gamma + beta): ds = dx = dres; dgamma / dbeta are
 *     ACCUMULATED (atomics) into zero-initialised [d] buffers.  d <= 2048.  (nn.LayerNorm of Encoder.py:167,
 *     SubLayers.py:73-79,147-150, Embeddings.py:84,185.)
 *   care_act: dy == NULL: out = act(z); else out = dy * act'(z)  (activations.py:3-16; exact-erf GELU).
 *   care_dropout: out = x * keep / (1 - p), keep = [u(seed, i) >= p] from a counter-based generator - the same call
 *     with the same seed is nn.Dropout's backward (RNG parity with torch is not a goal).
 *   care_strided_sum: out[r] = scale * sum_{k < terms} x[r * row_stride + k * term_stride]  (bias gradients, the
 *     backward of broadcast adds);  care_bcast_rows: dst[i] = scale * src[i / grp]  (backward of mean(1), Encoder.py:106).
 *   care_add_pos_sem: out[r] = x[r] + pos[r % seq] + sem[r / sem_div]  (Embeddings.py:170-176 before its LayerNorm).
 *   care_scatter_add_rows: table[idx[i]] += src[i]  (nn.Embedding backward; rows idx == skip_idx (padding_idx) skipped).
 *   care_concept_bwd: backward of care_concept_finish (pred_attribute.py:17-46) to the concept scores.
 *   care_attn_pv: ctx = dropout(P) V per (sequence, head); P [nseq * seq, heads, nkeys] from care_attention_probs.
 *   care_attn_bwd: backward of softmax(Q K^T / 8 + mask + bias) -> dropout -> . V  (Attention.py:83-131): dQ, dK, dV
 *     (written) and dbias [heads, bias_ld] (accumulated, optional).  nkeys <= 128, head dim 64; key / value block s of
 *     sequence s (no sharing between sequences: rows_per_kv = seq).
 */
int care_ln_bwd(const float* x, int64_t ldx, const float* res, int64_t ldres, const float* gamma, const float* dy,
                int64_t lddy, float eps, float* ds, int64_t ldds, float* dgamma, float* dbeta, int rows, int d,
                void* stream);
int care_act(const float* z, const float* dy, float* out, int64_t n, int act, void* stream);
int care_dropout(const float* x, float* out, int64_t n, float p, uint64_t seed, void* stream);
int care_strided_sum(const float* x, int64_t ldx, float* out, int64_t ldo, int rows, int d, int terms,
                     int64_t row_stride, int64_t term_stride, float scale, void* stream);
int care_bcast_rows(const float* src, int64_t lds, float* dst, int64_t ldd, int rows, int d, int grp, float scale,
                    void* stream);
int care_add_pos_sem(const float* x, const float* pos, const float* sem, float* out, int rows, int d, int seq,
                     int sem_div, void* stream);
int care_scatter_add_rows(const float* src, int64_t lds, const int32_t* idx, float* table, int64_t ldt, int rows,
                          int d, int skip_idx, void* stream);
int care_concept_bwd(const float* scores, int64_t lds, const float* dpreds, int64_t ldp, const float* davg, float* ds,
                     int64_t ldo, int B, int k, void* stream);
int care_attn_pv(const float* P, const float* V, int64_t kv_bs, int64_t kv_rs, float* ctx, int64_t ldc, int nseq,
                 int seq, int nkeys, int heads, float p_drop, uint64_t seed, void* stream);
int care_attn_bwd(const float* Q, int64_t ldq, const float* K, const float* V, int64_t kv_bs, int64_t kv_rs,
                  const float* P, const float* dctx, int64_t ldd, float* dQ, int64_t lddq, float* dK, float* dV,
                  int64_t dkv_bs, int64_t dkv_rs, float* dbias, int bias_ld, int nseq, int seq, int nkeys, int heads,
                  float p_drop, uint64_t seed, void* stream);

/*
 * care_gemm_kn: C [M, N] = op(A) B in exact f32 (v_mfma_f32_16x16x4_f32), B [K, N] row-major (ldb); a_is_km == 0: A is
 *   [M, K] row-major (lda), a_is_km != 0: A is stored [K, M] (the reduction index is its row).  The two products of an
 *   nn.Linear's backward as the operands lie in memory (training mode, models/Wrapper.py:423-435 under autograd):
 *   dx = dy W (a_is_km = 0, B = the [out, in] weight) and dW = dy^T x (a_is_km = 1, A = dy, B = x).  Any sizes and
 *   leading dimensions.
 */
int care_gemm_kn(const float* A, int64_t lda, int a_is_km, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N,
                 int K, void* stream);
/* The same product with K cut into `ksplit` ranges, range s multiplied into slab s of C (C + s * c_slab floats, each
 * [M, ldc]); the caller adds the slabs in order (care_strided_sum: terms = ksplit, row_stride = 1, term_stride = M rows:
 * deterministic).  For few output tiles
 * and a long K (dx = dlogits W: M = 1856, N = 512, K = 10547).  care_gemm_kn_splits(M, N, K) -> the ksplit to use (1: do
 * not split); any other ksplit must give every slab a range (ceil(K / ksplit) rounded up to 16) or CARE_ESHAPE.
 * Reference: the backward of nn.Linear under autograd (models/Wrapper.py:423-435 trains through it). */
int care_gemm_kn_splitk(const float* A, int64_t lda, int a_is_km, const float* B, int64_t ldb, float* C, int64_t ldc,
                        int64_t c_slab, int M, int N, int K, int ksplit, void* stream);
int care_gemm_kn_splits(int M, int N, int K);

/*
 * Training criteria (misc/Crit/base.py:20-47 CritBase.__call__ around the two `_step`s below; driven by Criterion.get_loss
 * from models/Wrapper.py:423-435; care_amd/criterion.py).  fp32 arithmetic in both libraries; no floating-point atomics:
 * row results go to per-row arrays and the sums over rows are added in a fixed order by a one-workgroup reduce that the
 * forward entry points enqueue behind the row kernel - two calls give identical bits.
 *
 * care_lang_loss_fwd: LanguageGeneration._step (misc/Crit/crit_lang.py:27-73: log_softmax, NLLLoss, the label-smoothing
 *   mean, the PAD mask) with calculate_word_acc / calculate_perplexity (:75-103) for `rows` label positions.  Row r reads the
 *   V fp32 logits at logits + (r / rows_per_seq) * seq_stride + (r % rows_per_seq) * ld - with seq_stride = (rows_per_seq + 1) * ld
 *   the `logits[:, :-1, :]` case of crit_lang.py:49-50 runs without a copy - and writes
 *     rmax[r] = max x, lsum[r] = log sum exp(x - max), lse[r] = rmax + lsum, logp[r] = x[y] - lse,
 *     pred[r] = arg-max column (lowest index on ties, as care_score_logits),
 *     row_loss[r] = (1 - eps) (lse - x[y]) + eps (lse - mean(x)).
 *   One workgroup per row; the row is read ONCE while V <= 16384 (kept in registers: 16 float4 per lane of 256; 16-byte loads
 *   after peeling to alignment, any ld and any 4-byte-aligned base) and twice beyond (the re-reading form).  Rows whose label
 *   is PAD (0) are not read: lse = rmax = lsum = logp = row_loss = 0, pred = 0.  A label outside [0, V) is never dereferenced: the row is
 *   treated like a PAD row and counted.  Behind the row kernel:
 *     sums[0] = sum row_loss, sums[1] = sum -logp (fp32, fixed order);
 *     counts[0] = rows with pred == label, counts[1] = non-PAD rows, counts[2] = rows with a label outside [0, V) (n_bad);
 *     acc (optional, 5 doubles): acc[0..1] += sums, acc[2..4] += counts - the recorders of Criterion.get_loss
 *     (base.py:95) and crit_lang.py:83-103 without a host synchronisation; one thread adds, in stream order.
 * care_lang_loss_bwd: the autograd backward of the above to the logits: for live rows
 *     dlogits[r, c] = g (exp(x[c] - lse[r]) - (1 - eps) [c == y] - eps / V),   g = *g (a DEVICE scalar: the upstream
 *   gradient is not known to the host), one read and one write per live row; the exponent is taken as (x - rmax) - lsum, the
 *   forward's two parts of lse (exact where the probability is; x - lse rounds at an ulp of |lse|); PAD rows, rows with a bad label and the positions
 *   rows_per_seq .. seq_rows - 1 of every sequence (the dropped last position) are zero-filled - dlogits arrives uninitialised.
 *   dlogits row (s, p), p < seq_rows, lies at dlogits + s * dseq_stride + p * ldd; rows must be a multiple of rows_per_seq.
 * care_noisy_or_bce_fwd / _bwd: NoisyOrMIL._step (misc/Crit/crit_attribute.py:38-48) and its backward: p = clamp(preds, 0.01,
 *   0.99), row_loss[b] = -sum_{c < K} (y log p + (1 - y) log(1 - p)) / denom[b], denom[b] = max(1, sum_{c < K} y); labels fp32
 *   [B, ldl >= K], the first K columns used.  dpreds[b, c] = -g (y / p - (1 - y) / (1 - p)) / denom[b] where 0.01 <= preds <= 0.99
 *   and 0 elsewhere (torch.clamp's rule).  One wave per clip.  sums[0] = sum row_loss (fixed order), acc (optional, 1 double) +=.
 */
int care_lang_loss_fwd(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V, const int32_t* labels,
                       float eps, float* lse, float* rmax, float* lsum, float* logp, int32_t* pred, float* row_loss, float* sums,
                       int32_t* counts, double* acc, int rows, void* stream);
int care_lang_loss_bwd(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V, const int32_t* labels,
                       const float* rmax, const float* lsum, float eps, const float* g, float* dlogits, int64_t ldd,
                       int64_t dseq_stride, int seq_rows, int rows, void* stream);
int care_noisy_or_bce_fwd(const float* preds, int64_t ldp, const float* labels, int64_t ldl, float* row_loss, float* denom,
                          float* sums, double* acc, int B, int K, void* stream);
int care_noisy_or_bce_bwd(const float* preds, int64_t ldp, const float* labels, int64_t ldl, const float* denom, const float* g,
                          float* dpreds, int64_t ldd, int B, int K, void* stream);

/*
 * The training head fused with the language loss (models/Head.py:26-32: logits = hidden tgt_word_prj^T; misc/Crit/crit_lang.py:49-71:
 * the [N, t + 1] against [N, t] rule, log_softmax, NLLLoss, the label-smoothing mean, the PAD mask; care_amd/criterion.py,
 * _HeadLoss).  The vocabulary projection, the loss and its backward over the LIVE label positions only (label in [1, V)); no
 * [rows, V] fp32 tensor is written at any point.  The head's products are split products of pre-scaled fp16 hi / lo pieces
 * (care_absmax -> care_split_pieces -> the LDS-tiled kernel with F16 operands), whatever the other layers use.
 *
 * care_head_live_rows (Head.py:26-32 is applied to these rows only; crit_lang.py:49-52,63-66): the ordered (ascending)
 *   compaction of the n_seq * t label positions with 0 < label < V: for the i-th live position r = s * t + p
 *     idx_h[i] = s * seq_rows + p (its row of the hidden states [n_seq, seq_rows >= t, d]), idx_l[i] = r, lab_c[i] = label;
 *   counts[0] = live positions, counts[1] = labels outside [0, V).  The three index arrays hold n_seq * t entries (the
 *   entries from counts[0] on are left as they are).  One workgroup; PAD and out-of-range labels are never used as an index.
 * care_gemm_tile_split3_head_stats (Head.py:26-32 + crit_lang.py:57-60): x = (A2 W3^T) / (scale_a scale_b) as
 *   care_gemm_tile_split3_scaled computes it (the accumulators times the exact power of two BEFORE any statistic), never
 *   stored; per (row, 64-column part) - parts = care_argmax_parts_tile(N), arrays [M, parts] -
 *     pmax = max x, pidx = FIRST arg-max column, psum = sum exp(x - pmax), plab = x[labels[row]] (-inf when the label is not
 *     in the part), psx = sum x over the part's columns < N.  labels [M]: the live rows' labels (lab_c).
 * care_head_loss_finish (crit_lang.py:57-71): merges the parts of live row i < R into rmax = max x, lsum = log sum exp(x - max)
 *   (kept apart for the backward, as care_lang_loss_fwd keeps them), lse, logp = (x[y] - rmax) - lsum, pred (lowest index on
 *   ties) and row_loss = (1 - eps) (-logp) + eps (lse - sum x / V); written at position idx_l[i] of the per-position arrays
 *   of care_lang_loss_fwd's layout, rmax / lsum also at i of rmax_c / lsum_c [R].  One wave per row, a fixed order.
 * care_lang_loss_reduce (crit_lang.py:63-71,83-103): care_lang_loss_fwd's ordered one-workgroup reduction on its own - sums,
 *   counts and acc as described there, over per-position arrays filled by care_head_loss_finish (dead positions are
 *   skipped by their label).  No floating-point atomics: two calls give the same bits.
 * care_head_grad_scale: *slot = the bit pattern of |*g| (one thread).  |dl| <= |g| for every element of the gradient of
 *   the logits, so the power-of-two scale of its pieces comes from the device scalar g - there is no |max| sweep.
 * care_gemm_tile_split3_head_grad (the backward of crit_lang.py:57-71 to the logits of Head.py:26-32): recomputes x from the
 *   same pieces in the same K order and writes, for row r < M and column c < ks = ceil64(N),
 *     dl = g (exp((x - rmax[r]) - lsum[r]) - eps / N - (1 - eps) [c == labels[r]])   (0 for N <= c < ks)
 *   as the fp16 pieces hi | lo of dl * 2^e(gbits) into out [M, 2 ks] - the A operand of care_gemm_tile_split3_scaled with
 *   amax_a = gbits.  rmax / lsum / labels [M] (compact).  out 16-byte aligned.
 * care_pieces_transpose: fp16 pieces [R, 2 ks_v] (hi | lo of [R, ks_v]) -> slab-major pieces of the transpose,
 *   out [slabs][V, 2 ks_r]: out[s][v][q ks_r + k] = src[s ks_r + k][q ks_v + v] (zero for s ks_r + k >= R), q = 0, 1 - the A
 *   operand of dW = dl^T h (Head.py:26-32 backward).  fp16 to fp16 through 64 x 64 LDS tiles; ks_v, ks_r multiples of 64,
 *   V <= ks_v, slabs ks_r >= R.
 */
int care_head_live_rows(const int32_t* labels, int n_seq, int t, int seq_rows, int V, int32_t* idx_h, int32_t* idx_l,
                        int32_t* lab_c, int32_t* counts, void* stream);
int care_gemm_tile_split3_head_stats(const void* A2, const void* W3, const void* amax_a, const void* amax_b, const int32_t* labels,
                                     float* pmax, int32_t* pidx, float* psum, float* plab, float* psx, int M, int N, int K,
                                     void* stream);
int care_head_loss_finish(const float* pmax, const int32_t* pidx, const float* psum, const float* plab, const float* psx, int parts,
                          const int32_t* lab_c, const int32_t* idx_l, int V, float eps, int R, float* lse, float* rmax,
                          float* lsum, float* logp, int32_t* pred, float* row_loss, float* rmax_c, float* lsum_c, void* stream);
int care_lang_loss_reduce(const float* row_loss, const float* logp, const int32_t* pred, const int32_t* labels, int V, int rows,
                          float* sums, int32_t* counts, double* acc, void* stream);
int care_head_grad_scale(const float* g, void* slot, void* stream);
int care_gemm_tile_split3_head_grad(const void* A2, const void* W3, const void* amax_a, const void* amax_b, const int32_t* labels,
                                    const float* rmax, const float* lsum, const float* g, const void* gbits, float eps, void* out,
                                    int M, int N, int K, void* stream);
int care_pieces_transpose(const void* src, int R, int V, int ks_v, int slabs, int ks_r, void* out, void* stream);

/*
 * The training head fused with the self-critical loss (models/Head.py:26-32: logits = hidden tgt_word_prj^T; the loss of
 * care_reward_loss_fwd - misc/Crit/crit_lang.py:57-60's log_softmax at the label, weighted per caption, no label smoothing;
 * care_amd/reward.py, _HeadRewardLoss):
 *     loss = -(1 / n_live) sum over live rows i of w[i] logp[i],   w[i] = adv[caption of row i].
 * The forward is care_head_live_rows, care_gather_rows, care_split_pieces and care_gemm_tile_split3_head_stats as they are.  The
 * gradient of the logits of live row i is (g w[i] / n_live) (softmax - onehot): care_gemm_tile_split3_head_grad with eps = 0 and
 * the device scalar g / n_live writes dl WITHOUT the weight, which is linear and goes onto the d-wide sides:
 *     dh[i] = w[i] (dl[i] W),   dW = dl^T (w (.) h_live)   (Head.py:26-32 backward).
 *
 * care_head_reward_finish (crit_lang.py:57-60): merges the parts (pmax, psum, plab of care_gemm_tile_split3_head_stats,
 *   arrays [R, parts], parts = care_argmax_parts_tile(V)) of live row i < R into rmax_c[i] = max x, lsum_c[i] =
 *   log sum exp(x - max), logp_c[i] = (x[y] - rmax) - lsum - care_head_loss_finish's bits - and writes the row's weight
 *   w_c[i] = adv[idx_l[i] / t] (idx_l: the label positions of care_head_live_rows, t positions per caption).  One wave per
 *   row, a fixed order.  R == 0 launches nothing.
 * care_head_reward_reduce: the outputs of care_reward_loss_fwd, with the same meaning, from the compact rows: totals[0] =
 *   sum w_c logp_c (a weight of exactly 0 adds nothing), totals[1] = R, *loss (DEVICE float) = -(totals[0] / R), 0 for R == 0;
 *   seq_logp (optional) [n_seq]: each caption's sum of logp over its live rows, 0 without one; acc (optional): += (loss, R).
 *   One workgroup, every sum in double and in one order, no floating-point atomics: two calls give the same bits.
 * care_head_reward_gscale: *gs = (float)(*g / totals[1]) (0 for totals[1] == 0), *slot = the bit pattern of |*gs| (one
 *   thread) - care_head_grad_scale's role: |dl| <= |gs| because the weight is not in dl.
 * care_rows_scale: dst[i, :] = w[i] src[i, :], fp32 [rows, cols] with row strides ld_src, ld_dst >= cols (elements); dst may
 *   be src.  16-byte accesses when cols, both strides and both pointers allow them.  rows == 0 launches nothing.
 * All four: a NULL pointer (but the optional ones) or a negative size -> CARE_EINVAL; totals / acc not 8-byte aligned ->
 *   CARE_EALIGN; parts != care_argmax_parts_tile(V), R > n_seq t or a stride below cols -> CARE_ESHAPE; all before anything is
 *   launched.
 */
int care_head_reward_finish(const float* pmax, const float* psum, const float* plab, int parts, const int32_t* idx_l,
                            const float* adv, int t, int V, int R, float* rmax_c, float* lsum_c, float* logp_c, float* w_c,
                            void* stream);
int care_head_reward_reduce(const float* logp_c, const float* w_c, const int32_t* idx_l, int R, int t, int n_seq, double* totals,
                            float* loss, float* seq_logp, double* acc, void* stream);
int care_head_reward_gscale(const float* g, const double* totals, float* gs, void* slot, void* stream);
int care_rows_scale(const float* src, int64_t ld_src, const float* w, float* dst, int64_t ld_dst, int rows, int cols,
                    void* stream);

/*
 * The optimiser step (models/Wrapper.py:316-386: configure_optimizers builds torch.optim.Adam; train.py:128 / opts.py:145:
 * Lightning's gradient_clip_val runs clip_grad_norm_ before it; misc/utils.py:282-304: the weight-decay groups; care_amd/optim.py).
 * One sweep for the norm of all gradients and one for the update of all parameters, whatever the number of tensors.  fp32 in
 * both library variants.
 *
 * care_opt_tensor: one parameter tensor - p, g, m (exp_avg), v (exp_avg_sq): fp32, contiguous, n elements each, 4-byte
 *   aligned; step_size = lr / (1 - beta1^t) and weight_decay are the tensor's parameter group's (0 = no decay).  `tensors`
 *   is a HOST array: the descriptors travel in the kernel arguments, CARE_OPT_PACK tensors per launch, so a step uploads
 *   nothing and a list of any length is ceil(count / CARE_OPT_PACK) launches.
 * care_grad_sqnorm (torch.nn.utils.clip_grad_norm_, norm type 2, as Lightning's gradient_clip_val calls it, train.py:128):
 *   *norm (DEVICE float) = the L2 norm of all g together.  Every tensor is cut into chunks of 1024 elements; workgroup b of
 *   care_grad_sqnorm_partials(total) takes a contiguous range of the chunks, adds squares in fp32 per lane and the lanes in
 *   double in a fixed order into partials[b] (DEVICE doubles, 8-byte aligned, care_grad_sqnorm_partials(total) of them,
 *   total = sum n); one workgroup adds the partials in index order and takes the square root.  No floating-point atomics:
 *   the same inputs give the same bits.  p, m, v are not touched (and may be anything non-NULL).  count == 0: *norm = 0.
 * care_adam_step (torch.optim.Adam's single-tensor arithmetic, torch 2.10 optim/adam.py _single_tensor_adam with amsgrad =
 *   maximize = False, as Wrapper.py:316-386 builds it, with clip_grad_norm_'s coefficient folded in): per element, in fp32,
 *     c  = norm ? min(1, max_norm / (*norm + 1e-6)) : 1      (read from the DEVICE scalar; a NaN norm gives a NaN c)
 *     g' = c g;  if (weight_decay != 0) g' += weight_decay p
 *     m += (g' - m) (1 - beta1);   v = beta2 v + (1 - beta2) g' g'
 *     p -= step_size m / (sqrt(v) / bias2_sqrt + eps)         (bias2_sqrt = sqrt(1 - beta2^t), by the host in double)
 *   g is read and never written: .grad stays unscaled after a clipped step (clip_grad_norm_ scales it in place).  beta1,
 *   beta2, eps, bias2_sqrt and max_norm are doubles: 1 - beta is taken in double before it is rounded to fp32, as torch
 *   takes it.  One pass: 16-byte loads and stores in every chunk whose four pointers are 16-byte aligned (a 0..3-element
 *   scalar tail in a tensor's last chunk), scalar ones in the others; nothing at or beyond element n is written.
 *   count == 0 is a no-op that returns 0.
 * Both: a NULL pointer in a descriptor, NULL tensors with count > 0, count < 0 or n < 0 -> CARE_EINVAL; a pointer that is
 *   not 4-byte aligned (partials: 8-byte) -> CARE_EALIGN; more than 2^31 - 1 chunks in one launch -> CARE_ESHAPE; all before
 *   anything is launched.
 */
#define CARE_OPT_PACK 64
typedef struct care_opt_tensor {
  float* p; const float* g; float* m; float* v;
  int64_t n;
  float step_size;
  float weight_decay;
} care_opt_tensor;
int care_grad_sqnorm_partials(int64_t total);
int care_grad_sqnorm(const care_opt_tensor* tensors, int count, double* partials, float* norm, void* stream);
int care_adam_step(const care_opt_tensor* tensors, int count, double beta1, double beta2, double eps, double bias2_sqrt,
                   const float* norm, double max_norm, void* stream);

/*
 * The mean-teacher step (models/Wrapper.py:550-614: InterplayModel - a student trained by the criterion plus a
 * distillation term towards a teacher that is the exponential moving average of the student; opts.py:253-255: ema_weight,
 * distillation_weight, eval_model; care_amd/interplay.py).  fp32 in both library variants.
 *
 * care_ema_tensor: one parameter pair - t (the teacher's, written) and s (the student's, read and never written): fp32,
 *   contiguous, n elements each, 4-byte aligned.  `tensors` is a HOST array: the descriptors travel in the kernel arguments,
 *   CARE_EMA_PACK tensors per launch, so an update uploads nothing and a list of any length is ceil(count / CARE_EMA_PACK)
 *   launches.
 * care_ema_step (Wrapper.py:574-581: torch._foreach_mul_(teacher, w); torch._foreach_add_(teacher, torch._foreach_mul(student,
 *   1 - w))): per element, in fp32 with every operation rounded on its own (no fused multiply-add),
 *     t = fl(fl(t (float)w) + fl(s (float)one_minus_w))
 *   - the bits of the three torch calls.  one_minus_w is the caller's double 1 - w; both are narrowed to float by the host.
 *   One pass: 16-byte loads and stores in every 1024-element chunk whose two pointers are 16-byte aligned (a 0..3-element
 *   scalar tail in a tensor's last chunk), scalar ones in the others; nothing at or beyond element n is written.  An empty
 *   tensor owns no chunk; count == 0 is a no-op that returns 0.  A NULL pointer in a descriptor, NULL tensors with
 *   count > 0, count < 0, n < 0 or t == s -> CARE_EINVAL; a pointer that is not 4-byte aligned -> CARE_EALIGN; more than
 *   2^31 - 1 chunks in one launch -> CARE_ESHAPE; all before anything is launched.
 * care_mse_fwd (Wrapper.py:565:((student_logits - teacher_logits) ** 2).mean()): *loss (DEVICE float) =
 *   (float)(sum (a_i - b_i)^2 / n) - the difference in fp32 as torch takes it, its square and every sum in double.  a and b
 *   are cut into chunks of 1024 elements; workgroup w of care_mse_partials(n) takes a contiguous range of the chunks and
 *   writes partials[w] (DEVICE doubles, 8-byte aligned, care_mse_partials(n) of them), one workgroup adds the partials in
 *   index order.  No floating-point atomics: the same inputs give the same bits; grid and partial count depend on n only.
 *   a and b may start at any 4-byte phase: 0..3 scalars are peeled up to the 16-byte boundary when both have the same
 *   phase, everything moves as scalars when they differ.
 * care_mse_bwd: da_i = fl(fl(a_i - b_i) c), c = (float)(2 (double)*g / (double)n) with g the upstream gradient, a DEVICE
 *   scalar read by the kernel.  The difference is recomputed from the operands; da (n floats) may be a or b itself.
 * Both: a NULL pointer or n <= 0 -> CARE_EINVAL; a pointer that is not 4-byte aligned (partials: 8-byte) -> CARE_EALIGN.
 */
#define CARE_EMA_PACK 128
typedef struct care_ema_tensor {
  float* t; const float* s;
  int64_t n;
} care_ema_tensor;
int care_ema_step(const care_ema_tensor* tensors, int count, double w, double one_minus_w, void* stream);
int care_mse_partials(int64_t n);
int care_mse_fwd(const float* a, const float* b, int64_t n, double* partials, float* loss, void* stream);
int care_mse_bwd(const float* a, const float* b, int64_t n, const float* g, float* da, void* stream);

/*
 * Caption retrieval (pretreatment/clip_retrieval.py:47-83 `run`, :175-176 the two normalisations of `load`, :305-321 the
 * per-video call and the rows that are stored; dataloader.py:808-814 takes the first `retrieval_topk` of them as the `r`
 * modality; care_amd/retrieval.py).  Builds that modality on device from a bank of caption embeddings.  fp32 in both
 * library variants; nothing here synchronises with the host.
 *
 * care_l2_normalize_rows (:176): y [M, D] = x [M, D] with every row divided by its L2 norm (sum of squares in a fixed order).
 * care_retrieval_query (:105-110, :175): q [B, D] = the mean over the n frames of frames [B, n, D] (summed in frame order,
 *   divided by n), divided by its L2 norm.
 * care_retrieval_topk (:47-83): per row b of q [B, D] the topk columns j of bank [M, D] (unit rows) with the largest
 *   q_b . bank_j among the ELIGIBLE ones, ordered by (score descending, j ascending).  Scores are exact f32
 *   (v_mfma_f32_16x16x4_f32) with ONE summation order for every (row, column) - k in blocks of 16, within a block
 *   k = 4 g + i taken i-major - whatever B, the row's place in the batch or the column's place in a tile, so bit-identical
 *   bank rows score bit-identically against a query and the tie rule decides.  The [B, M] scores never exist: a scan keeps
 *   the maximum over the eligible columns of every 16-column group, the topk groups of a row are re-scored with the same
 *   summation order and ranked.
 *   Eligibility of column j for row b, with [start_b, end_b) the row's own range (`info`; start == end == NULL: none):
 *   j outside [start_b, end_b) and - when first / prev are given (`unique`: first[j] the lowest member of j's group of equal
 *   captions, prev[j] the previous member or -1) - prev[j] < 0 or (first[j] >= start_b and prev[j] < end_b): j is the lowest
 *   member of its group outside the own range.  All of these are in the numbering of the scanned bank; orig (optional, [M],
 *   ascending: the `sampled_indices` of --ratio) only renames the ids that are written.
 *   Out: ids int64 [B, topk] (-1 past count), scores fp32 [B, topk] (-inf past count), count int32 [B] = min(topk,
 *   eligible columns).  scratch: care_retrieval_scratch(B, M, topk) bytes (< 0: unsupported shape), 16-byte aligned.
 * care_retrieval_gather (:318-321): out [n, De] = table[ids[i]] (the UN-normalised embeddings, possibly of another width:
 *   --arch_f); a row of zeros where ids[i] is negative or not below `rows`.
 * All: D / De a multiple of 16 up to 1024, 1 <= topk <= 128, 1 <= M <= 2^31 - 64, B >= 1 (n >= 1) or CARE_ESHAPE; a NULL
 *   pointer, one of start / end or of first / prev without the other, or a scratch that is too small -> CARE_EINVAL; a
 *   pointer that is not 16-byte aligned (the int32 / int64 arrays and count: their element size) -> CARE_EALIGN; all before
 *   anything is launched.
 */
int care_l2_normalize_rows(const float* x, float* y, int M, int D, void* stream);
int care_retrieval_query(const float* frames, float* q, int B, int n, int D, void* stream);
int64_t care_retrieval_scratch(int B, int M, int topk);
int care_retrieval_topk(const float* q, const float* bank, int B, int M, int D, int topk, const int32_t* start,
                        const int32_t* end, const int32_t* first, const int32_t* prev, const int32_t* orig,
                        int64_t* ids, float* scores, int32_t* count, void* scratch, int64_t scratch_bytes, void* stream);
int care_retrieval_gather(const float* table, int rows, int De, const int64_t* ids, int n, float* out, void* stream);

/*
 * care_decode_resident: the whole greedy decode of a SMALL batch (1 .. a few hundred caption rows) as ONE launch.
 *   Replaces the step loop of Translator.translate_batch with beam_size 1 (models/Translator.py:77-143: embedding,
 *   models/Decoder.py + models/components/Layers.py:157-228 per layer, Head.py:26-32, the top-1 of Beam.advance, and
 *   the `no active instance` exit of Translator.py:77-81) for batches whose step is bound by launch latency: a grid of
 *   at most one workgroup per CU stays resident and walks the phases of every step, handed on through producer counters
 *   (csrc/decode_resident.hip).  bf16 weights / caches, fp32 accumulation and statistics - the rounding points of the
 *   multi-launch path with projected cross K/V.
 *   care_resident_attn: one post-LN attention block over STATIC keys (inter_attention / attr_attention): q_w [d, d],
 *   o_w [d, d] bf16, biases / LayerNorm fp32, kv bf16 [batches, nkeys, 2 d] (K | V, as care_gemm writes cross K/V) with
 *   kv_batch_stride elements between batches, row r reads batch r / rows_per_kv; bias (optional) fp32 [heads, bias_ld].
 *   care_resident_layer: qkv_w [3 d, d], o_w [d, d], w1 [ff, d], w2 [d, ff] bf16; self_kv bf16 [rows, T, 2 d] (written).
 *   word fp32 [V, d], pos fp32 [>= T, d], sem (optional) fp32 [rows / sem_div, d]; vocab_w bf16 [V, d].
 *   Outputs: fed int32 [rows, fed_stride >= T + 1] (column 0 = bos; columns after a row's end: the tokens it kept
 *   choosing while frozen, or 0 once every row had ended), score fp32 [rows] (sum of chosen log-probs), length int32
 *   [rows], finished int32 [rows].  All four are initialised by the kernel.
 *   early_exit != 0: stop after the step at which the last row ended (else all `steps` steps run).  The number of
 *   steps run is left in ((int32_t*)scratch)[2].
 *   scratch: care_decode_resident_scratch(rows, d, ff, V) bytes, 16-byte aligned.  blocks: workgroups (0 = as many as
 *   the widest phase has items, at most one per CU; every workgroup must be resident).
 *   Requires heads == d / 64, T <= 128, nkeys <= 128, n_layers <= 4, n_att <= 2, V <= 16384 and either d == 512 with ff in
 *   {512, 1024, 2048} (any row count one workgroup per 16-row tile fits) or d in {768, 1024} with ff == 4 d and
 *   rows <= 128 (config/archs.yaml:15-26: the `median` / `large` architectures, K-split forms in every phase).
 *   Every workgroup must be resident at the same time (they wait for one another): the grid is at most one workgroup
 *   per CU and the entry point refuses (CARE_ESHAPE, nothing enqueued) unless hipOccupancyMaxActiveBlocksPerMultiprocessor
 *   admits a workgroup of the kernel per CU; do not run two of these launches concurrently on different streams.  A
 *   workgroup that waits ~2 s for a phase's producers aborts the launch: EVERY row's length = -1.
 *   Tuning knobs, read from the environment ONCE per process: CARE_RESIDENT_RB, CARE_RESIDENT_SMALL,
 *   CARE_RESIDENT_HALF_ROWS (forms of three phases), CARE_RESIDENT_BEAM_CFG (the beam launch's form).
 *   care_decode_resident_debug(prof_step, ghost): tools / tests only - phase clocks of step `prof_step` into the scratch
 *   (tools/resident_prof.py); ghost != 0: phases that can never complete (the watchdog test).  Process-wide, default 0 / 0.
 *   The entry points that issue two operations: a 52-KB memset node (hand-off counters) and the kernel.
 */
typedef struct care_resident_attn {
  const void* q_w; const float* q_b; const void* o_w; const float* o_b; const float* ln_g; const float* ln_b;
  const void* kv; int64_t kv_batch_stride; int32_t nkeys; int32_t rows_per_kv; const float* bias; int32_t bias_ld;
  int32_t reserved;
} care_resident_attn;
typedef struct care_resident_layer {
  const void* qkv_w; const float* qkv_b; const void* o_w; const float* o_b; const float* ln_g; const float* ln_b;
  void* self_kv;
  care_resident_attn att[2]; int32_t n_att; int32_t reserved;
  const void* w1; const float* b1; const void* w2; const float* b2; const float* ffn_g; const float* ffn_b;
} care_resident_layer;
int64_t care_decode_resident_scratch(int rows, int d, int ff, int V);
int care_decode_resident(const care_resident_layer* layers, int n_layers, const float* word, const float* pos,
                         const float* sem, int sem_div, const float* emb_g, const float* emb_b, float eps,
                         const void* vocab_w, int V, int d, int heads, int ff, int act, int rows, int T, int steps,
                         int bos, int eos, int pad, int32_t* fed, int fed_stride, float* score, int32_t* length,
                         int32_t* finished, void* scratch, int64_t scratch_bytes, int early_exit, int blocks, void* stream);

void care_decode_resident_debug(int prof_step, int ghost);

/*
 * The hand-off between the phases of a resident launch (care_decode_resident, care_decode_resident_beam): by default
 * (mode -1) fence-free - sc1 write-through stores, a drained vmcnt, one relaxed atomic add; sc1 polls and loads - on the
 * configuration that form was validated on (a gfx950 device with all 256 CUs in one partition), and with an agent-scope
 * release before the add / acquire after the poll on any other device or partition mode (+ 1 .. 4 us per hand-off).
 * care_resident_set_fenced(1 / 0) forces one form for the process (also CARE_RESIDENT_FENCED in the environment, read
 * once); care_resident_fenced() = the form a launch on the current device would take.
 */
void care_resident_set_fenced(int mode);
int care_resident_fenced(void);

/*
 * care_decode_resident_beam: BEAM SEARCH over a small batch (clips x beam <= a few hundred rows) as ONE launch.
 *   Replaces the step loop of Translator.translate_batch for beam_size > 1 (models/Translator.py:77-143 with
 *   predict_word's log_softmax :127, Beam.advance misc/Decoding/Beam.py:45-85 incl. its quirks - first step row 0 only,
 *   ended beams offer nothing, hypotheses collected in beam order until `need` = max(beam_size, topk) have ended, forced
 *   finish at max_len - and the `no active instance` exit of Translator.py:77-81): translate.py's default decode (beam 5,
 *   batch 128; --latency: batch 1).  Same machinery and rounding points as care_decode_resident; the vocabulary phase
 *   keeps every row's best 4-column groups and the advance phase recomputes their logits bit for bit
 *   (csrc/decode_resident_beam.hip), so the [rows, V] logits never exist.
 *   layers as for care_decode_resident with self_kv bf16 [clips * beam, T, 2 d] and rows_per_kv = beam in every
 *   attention block; sem (optional) fp32 [clips, d].
 *   State and outputs (all initialised by the kernel), as care_beam_advance: tok / anc0 / anc1 int32 [clips * beam, stride
 *   >= T + 1] (token table and the two ancestor tables), scores fp32 [clips * beam], done / nfin int32 [clips], fscore fp32 /
 *   flen int32 [clips, fin_cap], fhyp int32 [clips, fin_cap, stride]; fin_cap >= need + beam.  Steps run:
 *   ((int32_t*)scratch)[2].  Aborted launch (see care_decode_resident): EVERY nfin = -1.
 *   Requires heads == d / 64, T <= 63, beam <= 8 (beam 6 .. 8: a second instance of the launch with 8 groups kept per list), V <= 16384
 *   and either d == 512 with ff in {512, 1024, 2048} or d in {768, 1024}
 *   with ff == 4 d and clips * beam <= 128 (config/archs.yaml:15-26: the `median` / `large` architectures - VATEX runs
 *   translate.py with its default beam 5 - in the K-split forms of every phase).
 *   scratch: care_decode_resident_beam_scratch(clips, beam, d, ff, V) bytes, 16-byte aligned.
 */
int64_t care_decode_resident_beam_scratch(int clips, int beam, int d, int ff, int V);
int care_decode_resident_beam(const care_resident_layer* layers, int n_layers, const float* word, const float* pos,
                              const float* sem, const float* emb_g, const float* emb_b, float eps, const void* vocab_w,
                              int V, int d, int heads, int ff, int act, int clips, int beam, int need, int T, int steps,
                              int bos, int eos, int pad, int32_t* tok, int stride, int32_t* anc0, int32_t* anc1,
                              float* scores, int32_t* done, int32_t* nfin, float* fscore, int32_t* flen, int32_t* fhyp,
                              int fin_cap, void* scratch, int64_t scratch_bytes, int early_exit, int blocks, void* stream);

/* care_timestamp: out[0] (uint64) = the device wall clock (constant 100 MHz) when the one-thread kernel runs.
 *   Measurement only (bench.py: the duration of a kernel inside a replayed hipGraph); no reference counterpart. */
int care_timestamp(void* out, void* stream);

/*
 * care_decode_chain_beam: steps t0 .. t1 of a BEAM SEARCH as a chain of kernels - the phases of care_decode_resident_beam,
 *   each a launch of its own (10 per step for a one-layer decoder) with a grid sized by the phase's items; for batches
 *   beyond what one resident launch serves well (a few hundred rows) up to thousands of rows.  Replaces the same reference
 *   code as care_decode_resident_beam (models/Translator.py:77-143, misc/Decoding/Beam.py:45-85) with the SAME arithmetic
 *   per row (the device code is shared; plain loads / stores instead of agent-scope ones): hypotheses and scores are
 *   bit-identical to the resident launch's.  Arguments as care_decode_resident_beam; [t0, t1] the steps to run (1-based;
 *   t0 == 1 initialises the beam state and zeroes the `clips done` counter ((uint32_t*)scratch)[1]; later calls continue
 *   on the same state and scratch); the caller decides between calls whether any clip is still live (`done`).  There is
 *   no residency condition and no hand-off protocol: any grid, any number of concurrent streams.  form: -1 = by row
 *   count (<= 64 rows K-split items; <= 256 one row tile per workgroup; beyond, 2 / 2 / 2 / 4 row tiles per weight fetch
 *   in QKV / the d x d products / FFN dense1 / the vocabulary), 0 / 1 / 3 force one - a row's bits are the same in all.
 *   scratch: care_decode_chain_beam_scratch(clips, beam, d, ff, V) bytes, 16-byte aligned.
 *   Requires d == 512, heads == 8, ff in {512, 1024, 2048}, beam <= 5, T <= 63, V <= 16384, nkeys <= 128, n_att <= 2.
 */
int64_t care_decode_chain_beam_scratch(int clips, int beam, int d, int ff, int V);
int care_decode_chain_beam(const care_resident_layer* layers, int n_layers, const float* word, const float* pos,
                           const float* sem, const float* emb_g, const float* emb_b, float eps, const void* vocab_w,
                           int V, int d, int heads, int ff, int act, int clips, int beam, int need, int T, int t0, int t1,
                           int bos, int eos, int pad, int32_t* tok, int stride, int32_t* anc0, int32_t* anc1,
                           float* scores, int32_t* done, int32_t* nfin, float* fscore, int32_t* flen, int32_t* fhyp,
                           int fin_cap, void* scratch, int64_t scratch_bytes, int form, void* stream);

/*
 * Self-critical sequence training (care_amd/reward.py, care_amd/scst.py; csrc/reward.hip): the CIDEr-D of sampled captions
 * as a reward, advantages against a baseline, and the advantage-weighted log-likelihood of the teacher-forced samples.  The
 * reference only monitors the metric (opts.py `lr_monitor_metric` "CIDEr", computed by the Java / Python coco-caption
 * tools on words); here it is the coco-caption CIDEr-D over integer token ids, restated in float64 in
 * tests/cider_reference.py.  fp32 / double arithmetic in both libraries, no floating-point atomics, nothing synchronises.
 *
 * care_cider_score: out[r] (fp32) = the CIDEr-D of candidate r against the references of video[r].  Candidate r is
 *   tokens[r * ld + col0 .. + min(length[r], width)) with ONE trailing `eos` dropped unless with_eos != 0; token ids are
 *   taken modulo 2^16 and PAD (0) must not occur inside a caption.  An n-gram (n = 1..4) is one uint64 key, 16 bits a token,
 *   the first token lowest, the orders below 4 zero-filled.  With tf the count of a key in a caption, df the number of videos
 *   whose references hold it and N = n_videos:  w(g) = tf(g) (ln N - ln max(1, df(g)));  norm_n = sqrt(sum w^2) over a
 *   caption's keys of order n;  for candidate h and reference r
 *     sim_n = sum_{g in h, order n} min(w_h(g), w_r(g)) w_r(g),  divided by norm_n(h) norm_n(r) when both are non-zero,
 *             times exp(-(len_h - len_r)^2 / 72);
 *   out = 10 * (1 / 4) sum_n (1 / R) sum_{r < R} sim_n over the R references of the video.
 *   The bank (a HOST struct of DEVICE arrays, built once by care_amd.reward.CiderBank):
 *     corpus_keys [n_corpus] ascending (as uint64), corpus_lndf [n_corpus] = ln max(1, df) - a key that is absent has df 0;
 *     ref_start [n_refs + 1]: reference i owns ref_keys / ref_w [ref_start[i], ref_start[i + 1]) - its unique keys ascending
 *     and their weights; ref_norm [n_refs, 4]; ref_len [n_refs] (tokens, after the EOS rule); vid_start [n_videos + 1]:
 *     video v owns the references [vid_start[v], vid_start[v + 1]); ln_n = ln N.
 *   One workgroup of 256 per candidate: keys, tf and first-occurrence flags in LDS (all pairs), ln df by binary search in
 *   corpus_keys, the references of the video dealt to the four waves round-robin, the lanes of a wave over the candidate's
 *   unique keys with a binary search in the reference's keys.  Every sum is in double and in ONE order - the norms in key
 *   order, a reference's sim_n by a scan in lane order, a wave's references in bank order, the waves in wave order - so a
 *   row's bits do not depend on `rows` or on the row's place; rounded once to fp32.  Rows with length <= 0, an empty caption
 *   or a video without references score 0.  A video[r] outside [0, n_videos) is never dereferenced: the row scores 0 and
 *   *bad (optional, int32, ASSIGNED) counts such rows.
 *   NULL tokens / length / video / out / bank or a NULL array in the bank, rows < 0, width < 1, width > 64, col0 < 0,
 *   ld < col0 + width, n_videos < 1 -> CARE_EINVAL; a double / uint64 / int64 array that is not 8-byte aligned ->
 *   CARE_EALIGN; before anything is launched.  rows == 0 is a no-op that returns 0.
 * care_reward_advantage: adv [B, n] from reward [B, n] (fp32, every operation rounded on its own).  baseline [B] given
 *   (the greedy caption's reward): adv = reward - baseline[b].  baseline NULL (leave-one-out, n >= 2 or CARE_EINVAL):
 *     s = ((r_0 + r_1) + r_2) + ...,  base_j = (s - r_j) / (float)(n - 1),  adv_j = r_j - base_j.
 *   stats (2 doubles, ASSIGNED): the mean over all B n entries of the reward and of the baseline that was subtracted, summed
 *   in double in a fixed order (one workgroup).  NULL reward / adv / stats, B < 1 or n < 1 -> CARE_EINVAL; stats not 8-byte
 *   aligned -> CARE_EALIGN.
 * care_reward_loss_fwd: the logits and labels of care_lang_loss_fwd (same addressing: ld, seq_stride, rows_per_seq; label
 *   PAD (0) or outside [0, V) = a dead row that is not read), adv fp32 [rows / rows_per_seq] one per sequence.  Per live row
 *   rmax, lsum (kept apart for the backward) and logp = (x[y] - rmax) - lsum in fp32, 0 on dead rows; then ONE workgroup,
 *   in double and a fixed order:  totals[0] = sum over live rows of adv logp, totals[1] = n_live,
 *     *loss (DEVICE float) = -(totals[0] / n_live), 0 when n_live == 0;
 *   seq_logp (optional, [rows / rows_per_seq]) = each sequence's sum of logp; acc (optional, 2 doubles) += loss, n_live.
 * care_reward_loss_bwd: dlogits[s, p, c] = (float)(g adv[s] / n_live) (exp((x[c] - rmax) - lsum) - [c == y]) on live rows,
 *   g = *g a DEVICE scalar, n_live = totals[1]; one read and one write per live row.  Dead rows, the positions rows_per_seq ..
 *   seq_rows - 1 of every sequence and every row of a sequence whose adv is exactly 0 are zero-filled without reading their
 *   logits.  dlogits is addressed as in care_lang_loss_bwd.
 *   Both: the return codes of care_lang_loss_fwd / _bwd (eps apart); totals / acc not 8-byte aligned -> CARE_EALIGN.
 */
typedef struct care_cider_bank {
  const uint64_t* corpus_keys; const double* corpus_lndf; int64_t n_corpus;
  const uint64_t* ref_keys; const double* ref_w; const int64_t* ref_start; const double* ref_norm; const int32_t* ref_len;
  const int32_t* vid_start; int32_t n_videos; int32_t n_refs;
  double ln_n;
} care_cider_bank;
int care_cider_score(const int32_t* tokens, int ld, int col0, int width, const int32_t* length, const int32_t* video,
                     int rows, int with_eos, int eos, const care_cider_bank* bank, float* out, int32_t* bad, void* stream);
int care_reward_advantage(const float* reward, const float* baseline, int B, int n, float* adv, double* stats, void* stream);
int care_reward_loss_fwd(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V, const int32_t* labels,
                         const float* adv, float* rmax, float* lsum, float* logp, double* totals, float* loss, float* seq_logp,
                         double* acc, int rows, void* stream);
int care_reward_loss_bwd(const float* logits, int64_t ld, int64_t seq_stride, int rows_per_seq, int V, const int32_t* labels,
                         const float* adv, const float* rmax, const float* lsum, const double* totals, const float* g,
                         float* dlogits, int64_t ldd, int64_t dseq_stride, int seq_rows, int rows, void* stream);

/*
 * Consensus captions (care_amd/consensus.py, Translator_ARFormer.consensus_batch; csrc/consensus.hip): of the n candidate
 * captions of a clip - the samples of care_sample_logits - the one that agrees most with the others under CIDEr-D (minimum
 * Bayes risk with the task's metric as the gain).  No references of the clip are read: the bank gives ln N and ln df only.
 * Restated in float64 in tests/consensus_reference.py.  fp32 / double arithmetic in both libraries, no atomics, nothing
 * synchronises, nothing is allocated.
 *
 * care_consensus_score: clip b owns the candidate rows b n + j, j = 0 .. n - 1, of which the first m = count[b] (clamped
 *   into [0, n]; count NULL: m = n) are valid.  A candidate is the caption of care_cider_score: tokens[r * ld + col0 .. +
 *   min(length[r], width)) with ONE trailing `eos` dropped unless with_eos != 0, its keys and weights w(g) = tf(g) (ln N -
 *   ln max(1, df(g))) those of care_cider_score (df = 0 for a key that is absent from corpus_keys).  For j != i, both < m:
 *     sim_o(j -> i) = sum_{g in j, order o} min(w_j(g), w_i(g)) w_i(g),  divided by norm_o(j) norm_o(i) when both are non-zero;
 *     t_o(j, i)     = sim_o(j -> i) exp(-(len_j - len_i)^2 / 72);
 *     pairs[b, j, i] = 10 (((t_1 + t_2) + t_3) + t_4) / 4;
 *     score[b, j]    = 10 (((a_1 / (m - 1) + a_2 / (m - 1)) + a_3 / (m - 1)) + a_4 / (m - 1)) / 4,
 *                      a_o = the sum of t_o(j, i) over i != j, i < m, in ascending i
 *   - the CIDEr-D of candidate j with the clip's other valid candidates as its reference set; duplicates each count as a
 *   reference; an empty candidate scores 0 and, as a reference, adds 0 and still counts in m - 1.  pairs[b, j, j] = 0, every
 *   pairs / score entry with j >= m or i >= m is 0, and with m <= 1 every score is 0.  winner[b] = the j < m with the largest
 *   score[b, j] AS WRITTEN (the double rounded to fp32), the lower j among equals - the first arg-max of the row the caller
 *   reads; -1 when m == 0.  (Copies of one caption get the same terms in another order of i, so their doubles may differ in
 *   the last bit: compared as doubles, that bit and not the index would choose among them.)  winner_row[b] = b n + winner[b],
 *   or -1.
 *   Every sum is in double and in ONE order - the norms in key order, sim_o by a scan in lane order (a lane per key of j, key
 *   l + 64 q on lane l), a_o in ascending i - so a clip's bits depend on the clip alone; score and pairs are rounded once to
 *   fp32.  pairs [clips, n, n] and winner_row [clips] are optional.
 *   One workgroup of 256 per clip; per candidate 256 keys, 256 weights, 4 norms, 64 tokens in LDS: 4400 n + 8 bytes, 137.5 KB
 *   at CARE_CONSENSUS_MAX_N.
 *   NULL tokens / length / bank / score / winner, a NULL corpus_keys / corpus_lndf, clips < 0, n < 1, width < 1, col0 < 0,
 *   ld < col0 + width, n_videos < 1 -> CARE_EINVAL; n > CARE_CONSENSUS_MAX_N, width > 64, clips n > 2^31 - 1 -> CARE_ESHAPE;
 *   corpus_keys / corpus_lndf not 8-byte aligned -> CARE_EALIGN; before anything is launched.  clips == 0 is a no-op that
 *   returns 0.
 */
#define CARE_CONSENSUS_MAX_N 32
int care_consensus_score(const int32_t* tokens, int ld, int col0, int width, const int32_t* length, const int32_t* count,
                         int clips, int n, int with_eos, int eos, const care_cider_bank* bank, float* score, float* pairs,
                         int32_t* winner, int32_t* winner_row, void* stream);

/*
 * Validation metrics (care_amd/capmetrics.py, care_amd/validation.py; csrc/capmetrics.hip): what the reference's validation
 * epoch reports besides METEOR (models/Wrapper.py:214-273, misc/cocoeval.py) - corpus BLEU-1..4, ROUGE-L and CIDEr - over
 * integer token ids, from sufficient statistics that stay on the device for a whole epoch.  The definitions are coco-caption's,
 * restated in float64 in tests/capmetrics_reference.py.  int / fp32 / double arithmetic in both libraries, no floating-point
 * atomics, nothing synchronises.
 *
 * care_caption_stats: per candidate r - the caption of care_cider_score: tokens[r * ld + col0 .. + min(length[r], width)) with
 *   ONE trailing `eos` dropped unless with_eos != 0, L tokens - against the references of video[r]:
 *     rec [r, 12] (int32) = (valid, testlen = L, reflen, guess_1..4, correct_1..4, 0) with
 *       guess_n   = max(0, L - n + 1),
 *       correct_n = sum over the caption's distinct n-grams g of min(count in the caption, max over the references of count),
 *       reflen    = the reference length closest to L, the smaller one of two equally close (min of (|l - L|, l));
 *     rouge [r] (double) = (1 + b^2) P R / (R + b^2 P) with b = 1.2, P = max_ref lcs / L, R = max_ref (lcs / len(ref)) - the two
 *       maxima independent of each other - and 0 unless both are non-zero; a reference without tokens has lcs 0 and adds to
 *       neither.
 *   The bank (a HOST struct of DEVICE arrays, built once by care_amd.capmetrics.MetricBank) embeds the care_cider_bank of the
 *   same references (vid_start / n_videos are read from it) and adds
 *     clip_start [n_videos + 1]: video v owns clip_keys / clip_max [clip_start[v], clip_start[v + 1]) - the unique n-gram keys
 *     (n = 1..4, the keys of care_cider_score) of its references ascending and each one's largest count in ONE reference;
 *     ref_tok_start [n_refs + 1]: reference i owns the tokens ref_tok [ref_tok_start[i], ref_tok_start[i + 1]) (after the EOS
 *     rule, any length).
 *   One workgroup of 256 per candidate: keys and counts in LDS, the clip table by binary search, integer sums; the references
 *   dealt to the four waves round-robin, the LCS of a reference by the bit-parallel recurrence on one 64-bit word (lane j holds
 *   candidate token j; per reference token t: M = ballot(cand == t), U = V & M, V = (V + U) | (V & ~M), V = ~0 at the start;
 *   lcs = the zero bits among the low L).  A row's bits do not depend on `rows` or on the row's place.
 *   L == 0 after the EOS rule is an empty caption: valid = 1, the counts 0, reflen the shortest reference, rouge 0.  length[r]
 *   <= 0, a video[r] outside [0, n_videos) (never dereferenced) or a video without references: an INVALID row, all 12 ints
 *   and rouge 0.
 *   NULL tokens / length / video / rec / rouge / bank or a NULL array of the five (or vid_start), rows < 0, width < 1,
 *   width > 64, col0 < 0, ld < col0 + width, n_videos < 1 -> CARE_EINVAL; clip_keys, clip_start, ref_tok_start or rouge not
 *   8-byte aligned -> CARE_EALIGN; before anything is launched.  rows == 0 is a no-op that returns 0.
 * care_caption_totals: ADDS a batch to the running totals  totals_i [12] (int64) = (n_valid, n_invalid, testlen, reflen,
 *   guess_1..4, correct_1..4),  totals_d [2] (double) = (sum rouge, sum cider); cider (optional, fp32 [rows]) is
 *   care_cider_score's output.  Invalid rows count in n_invalid and add nothing else.  One workgroup of 1024 in ONE order: a
 *   thread's rows t, t + 1024, .., a scan in lane order, the waves in wave order.  The integers are exact for any split of an
 *   epoch into batches; the two doubles depend on the split in their last bits.  The caller zeroes the totals once.
 *   NULL rec / rouge / totals, rows < 0 -> CARE_EINVAL; rouge / totals not 8-byte aligned -> CARE_EALIGN; rows == 0: a no-op.
 * care_beam_winner: the caption Translator.translate_batch returns first for each clip of a beam result block (nfin [B],
 *   fscore / flen [B, cap], fhyp [B, cap, w]): the arg-max of (double)fscore / len_pow[clamp(flen, 0, n_pow - 1)] over the
 *   first min(nfin, cap) hypotheses, the earliest among equals (a stable sort).  len_pow [n_pow] (double) is the host's table of
 *   length ** beam_alpha: the division is IEEE's, no pow on the device, so the choice is the host's.  tokens [B, w] = the
 *   winner's tokens, 0 behind its length; length [B] = its length, 0 (and a row of zeros) when nfin <= 0.
 *   NULL pointers, B < 0, cap < 1, cap > 64, w < 1, n_pow < 1 -> CARE_EINVAL; len_pow not 8-byte aligned -> CARE_EALIGN;
 *   B == 0: a no-op.
 */
typedef struct care_metric_bank {
  care_cider_bank cider;
  const uint64_t* clip_keys; const int32_t* clip_max; const int64_t* clip_start;
  const int32_t* ref_tok; const int64_t* ref_tok_start;
} care_metric_bank;
int care_caption_stats(const int32_t* tokens, int ld, int col0, int width, const int32_t* length, const int32_t* video,
                       int rows, int with_eos, int eos, const care_metric_bank* bank, int32_t* rec, double* rouge, void* stream);
int care_caption_totals(const int32_t* rec, const double* rouge, const float* cider, int rows, int64_t* totals_i,
                        double* totals_d, void* stream);
int care_beam_winner(const int32_t* nfin, const float* fscore, const int32_t* flen, const int32_t* fhyp, int B, int cap, int w,
                     const double* len_pow, int n_pow, int32_t* tokens, int32_t* length, void* stream);

/*
 * Concept metrics (care_amd/metrics.py, care_amd/criterion.py, care_amd/validation.py; csrc/concept_metrics.hip): the metric
 * half of NoisyOrMIL._step (misc/Crit/crit_attribute.py:58-89) - F1@k and average precision of the concept probabilities
 * against multi-hot labels - without a sort, and their sums over an epoch in totals that stay on the device: what the
 * reference's eval criterion (models/Wrapper.py:182-184, :421: calculate_mAP) feeds into `mAP` / `best_mAP` (:59-71, :245-248).
 * int, fp32 compares and double arithmetic in both libraries, no floating-point atomics, nothing synchronises.
 *
 * care_concept_metrics: preds fp32 [B, ldp >= K], labels fp32 [B, ldl >= K] read in place (as care_noisy_or_bce_fwd reads
 *   them); a POSITIVE of clip b is a column j < K with labels[b, j] != 0, P of them.  ONE total order of the columns of a clip:
 *   by p = clamp(preds, 0.01, 0.99) in fp32 (torch.clamp: NaN stays NaN) descending, NaN before every number (torch's
 *   descending order); among equal values, or among NaNs, the lower column first (sort(stable=True)).  With
 *     rank_j = the number of columns i < K before j,  posrank_j = the number of positives before j:
 *     hits [b, t] (int32 [B, n_topk], optional) = #{positive j : rank_j < topk[t]}       (crit_attribute.py:59-64),
 *     n_pos [b]   (int32 [B], optional)         = P                                      (:60),
 *     ap [b]      (double [B], optional)        = (sum over the positives of (posrank_j + 1) / (rank_j + 1)) / P   (:73-84),
 *   the terms added in ascending posrank - the reference's order - grouped one fixed way; every division and sum in double: the
 *   operands are integers, so this is the exact value up to its own rounding.  P == 0: ap = 0 / 0 = NaN, from the same
 *   expression.  topk is a HOST array of n_topk <= CARE_CONCEPT_MAX_TOPK positive ints; it travels in the kernel arguments.
 *   One workgroup of 256 per clip: keys and a bitmap of the positives in LDS, the positives compacted by ballot and prefix
 *   count and dealt to the four waves, per positive one sweep of the K columns by 64 lanes that counts both integers.  A
 *   clip's bits do not depend on B or on the clip's place.  K <= CARE_CONCEPT_MAX_K (the LDS form).
 *   totals_d (double [n_topk + 1]) / totals_i (int64 [2]), optional but only together: a second launch of ONE workgroup of
 *   1024 ADDS the batch, in one order (a thread's clips t, t + 1024, .., a scan in lane order, the waves in wave order, as
 *   care_caption_totals):  totals_d[t] += sum_b F1@topk[t],  totals_d[n_topk] += sum_b ap[b],  totals_i = (clips, clips with
 *   P == 0), with  hit = hits == 0 ? 1e-3 : hits,  precision = hit / k,  recall = hit / P,  F1 = 2 precision recall /
 *   (precision + recall)  in double (:65-68); P == 0 makes recall infinite and F1 NaN as in the reference - and the clip is
 *   counted in totals_i[1], so a caller can tell.  The totals are sums of the per-clip outputs: with totals, ap, n_pos and
 *   (for n_topk > 0) hits must be given.  The integers are exact for any split of an epoch into batches; the doubles depend
 *   on the split in their last bits.  The caller zeroes the totals once.
 *   NULL preds / labels, B < 0, K < 1, n_topk outside [0, CARE_CONCEPT_MAX_TOPK], NULL topk with n_topk > 0, a topk[t] < 1,
 *   ldp or ldl < K, one of totals_d / totals_i without the other, totals without the per-clip outputs -> CARE_EINVAL;
 *   K > CARE_CONCEPT_MAX_K, a topk[t] > K (the reference's topk(50) raises there) -> CARE_ESHAPE; ap / totals_d / totals_i not
 *   8-byte, another array not 4-byte aligned -> CARE_EALIGN; all before anything is launched.  B == 0: a no-op that returns 0.
 */
#define CARE_CONCEPT_MAX_K 4096
#define CARE_CONCEPT_MAX_TOPK 8
int care_concept_metrics(const float* preds, int64_t ldp, const float* labels, int64_t ldl, int B, int K, const int32_t* topk,
                         int n_topk, double* ap, int32_t* hits, int32_t* n_pos, double* totals_d, int64_t* totals_i,
                         void* stream);

/*
 * Training and validation batches built on the device (care_amd/clipstore.py; csrc/batch.hip): the per-video feature tables
 * and the caption table stay in HBM, a batch is three launches over a list of item indices.  Replaces the reference's
 * Dataset.__getitem__ + default_collate + H2D copy (dataloader.py:142-190, :232-262, :352-384, :777-814).  Integer and byte
 * arithmetic only: the same in both library variants; nothing synchronises; plain vector stores throughout.
 *
 * The counter-based generator is csrc/care_common.h's care_mix64:  h(a, n) = fin(a + 0x9E3779B97F4A7C15 (n + 1)), fin = the
 * splitmix64 finaliser, all in uint64 with wrap-around.  Item key k1 = h(h(seed, epoch), item), `item` = items[b] - the item's index in
 * the store's infoset, NOT its place b in the batch: an item gets the same frames in whatever batch it lies.
 *
 * care_batch_frame_ids (dataloader.py:23-31 get_frame_ids): frame_ids int32 [B, n_frames], ascending per item.  `bounds` is a
 *   HOST array of n_frames + 1 snippet bounds, int(np.linspace(0, n_total, n_frames + 1)[i]) as the reference computes them
 *   (misc/utils.py:313); it travels in the kernel arguments.
 *     CARE_FRAMES_EQUAL   (misc/utils.py:311-317): id_i = (bounds[i] + bounds[i + 1]) / 2 - items, seed, epoch are not read;
 *     CARE_FRAMES_SEGMENT (:320-326): id_i = bounds[i] + mulhi32((uint32)(h(k1, i) >> 32), bounds[i + 1] - bounds[i]) with
 *       mulhi32(a, w) = (uint64 a w) >> 32 - uniform over the snippet up to 2^-32, integers only;
 *     CARE_FRAMES_ALL     (:329-332, a sorted random.sample): frame f has the key h(k1, f); the n_frames frames with the
 *       smallest (key, f) are chosen and written in ascending f.  One wave per item, the frame on the lane: rank = the number
 *       of smaller (key, f), a ballot of rank < n_frames, a prefix popcount for the slot.  n_total <= 64 or CARE_ESHAPE.
 *   The reference draws from Python's / numpy's global generators: its streams cannot be reproduced, the distribution and
 *   every deterministic rule are.
 *   NULL frame_ids / bounds (items: for the two random types), B < 0, n_total < 1, n_frames < 1, bounds that do not start at 0,
 *   end at n_total and ascend -> CARE_EINVAL; an unknown type -> CARE_EDTYPE; n_frames > CARE_BATCH_MAX_FRAMES, or for the two
 *   random types n_frames > n_total (an empty snippet: the reference's randint / sample raise) -> CARE_ESHAPE; a pointer that
 *   is not 4-byte aligned -> CARE_EALIGN; all before anything is launched.  B == 0 is a no-op that returns 0.
 *
 * care_batch_gather (dataloader.py:232-262 _load_feats with load_feats_type 0, :808-814 load_r_feats, default_collate):
 *   every modality of the batch in ONE launch.  care_batch_table (a HOST array, `count` <= CARE_BATCH_MAX_TABLES of them, in
 *   the kernel arguments): table [n_videos, n_total, pitch bytes] - `pitch` a multiple of 16, >= row_bytes, the table 16-byte
 *   aligned, so every source row is; out [B, n_out, row_bytes] dense.  Row (b, j) of a table is row_bytes BYTES copied from
 *   source row (video_ids[b], n_total == 1 ? 0 : frame_ids[b * n_frames + j]): n_total == 1 is a per-video vector that every
 *   frame id reads (dataloader.py:247-251) - or, with n_out == 1, one whole block per video such as the first retrieval_topk
 *   rows of `r`; n_total > 1 needs n_out == n_frames.  A video id outside [0, n_videos) or a frame id outside [0, n_total)
 *   is never dereferenced: the row is zeros.  row_bytes a multiple of 16 and out 16-byte aligned: 16-byte loads and stores;
 *   else a multiple of 4 and out 4-byte aligned: 16-byte loads, 4-byte stores; else (a multiple of 2) 2-byte stores - never
 *   a byte at or beyond row_bytes of a destination row.  The source is read once an epoch (non-temporal loads), the
 *   destination is read next by the embedder (plain stores).
 *   NULL pointers (frame_ids: only when a table has n_total > 1), count < 1, B < 0, n_videos < 1, n_frames < 1, n_total < 1,
 *   n_out < 1, row_bytes < 2 or odd, pitch < row_bytes -> CARE_EINVAL; count > CARE_BATCH_MAX_TABLES, n_total > 1 with
 *   n_out != n_frames, more than 2^31 - 1 KiB-pieces of rows in one table's output -> CARE_ESHAPE; a table or pitch that is not 16-byte aligned, an out that is not 2-byte aligned, an id
 *   array that is not 4-byte aligned -> CARE_EALIGN; all before anything is launched.  B == 0: a no-op.
 *
 * care_batch_text (dataloader.py:352-384 _getitem_text_only, :524-571 _prepare_input_ids / _make_source_target, :661-675
 *   _padding; misc/utils_corpora.py:424-441 get_vid2attribute_mappings): one workgroup per item.  The caption table: tokens
 *   int32 flat, cap_start int32 [n_caps + 1] (caption c owns tokens [cap_start[c], cap_start[c + 1])), cap_video int32
 *   [n_caps], vid_first int32 [n_videos + 1] (video v owns the captions [vid_first[v], vid_first[v + 1])).  item_cap int32
 *   [n_items]: the caption of infoset item i; c = item_cap[items[b]], v = cap_video[c].  Written:
 *     video_ids [b] = v, caption_ids [b] = c - vid_first[v] (the reference's cap_id), both int32;
 *     with P = the caption cut to max_len, its last place EOS when it was longer, PAD behind a shorter one:
 *     input_ids [b, 0 .. max_len - 2] = P[0 ..], labels [b, 0 .. max_len - 2] = P[1 ..], both int64;
 *     labels_attr [b, a] fp32 (optional, with n_attributes) = 1.0 when a token attribute_start + a stands in ANY caption of v,
 *     its first and last token (BOS, EOS) apart, else 0.0 - a bitmap in LDS set by atomic or, then read out.
 *   An items[b] outside [0, n_items) is never dereferenced: video_ids = caption_ids = -1, PAD rows and zeros.
 *   NULL pointers (labels_attr apart), B < 0, n_items < 1, n_caps < 1, n_videos < 1, max_len < 2 -> CARE_EINVAL; labels_attr
 *   with n_attributes outside [1, CARE_BATCH_MAX_ATTR] -> CARE_ESHAPE; input_ids / labels not 8-byte, another array not
 *   4-byte aligned -> CARE_EALIGN; all before anything is launched.  B == 0: a no-op.
 */
#define CARE_FRAMES_EQUAL 0
#define CARE_FRAMES_SEGMENT 1
#define CARE_FRAMES_ALL 2
#define CARE_BATCH_MAX_FRAMES 128
#define CARE_BATCH_MAX_TABLES 8
#define CARE_BATCH_MAX_ATTR 3000
typedef struct care_batch_table {
  const void* table; void* out;
  int64_t pitch;
  int32_t n_total; int32_t row_bytes; int32_t n_out; int32_t reserved;
} care_batch_table;
int care_batch_frame_ids(const int32_t* items, int B, int n_total, int n_frames, int random_type, const int32_t* bounds,
                         uint64_t seed, uint64_t epoch, int32_t* frame_ids, void* stream);
int care_batch_gather(const care_batch_table* tables, int count, const int32_t* video_ids, const int32_t* frame_ids,
                      int n_videos, int B, int n_frames, void* stream);
int care_batch_text(const int32_t* items, int B, const int32_t* item_cap, int n_items, const int32_t* tokens,
                    const int32_t* cap_start, const int32_t* cap_video, const int32_t* vid_first, int n_caps, int n_videos,
                    int max_len, int pad, int eos, int attribute_start, int n_attributes, int32_t* video_ids,
                    int32_t* caption_ids, int64_t* input_ids, int64_t* labels, float* labels_attr, void* stream);

/*
 * Test epoch (care_amd/corpusstats.py, care_amd/testepoch.py; csrc/corpus_stats.hip): what the reference's test run reports on
 * top of the corpus scores - Wrapper.test_epoch_end (models/Wrapper.py:75-149): the caption analysis `ave_length`, `novel`,
 * `unique`, `usage` of analyze_length_novel_unique (misc/utils.py:406-419 over cal_n_gram :390-403 and cal_gt_n_gram :375-387)
 * and the `score` of a prediction (Wrapper.py:206-210) - as integers and doubles that stay on the device for a whole epoch.
 * Integer and double arithmetic only: the same in both libraries; ordinary 32- / 64-bit integer atomics, no floating-point
 * atomics; nothing synchronises.
 *
 * A CAPTION is tokens[r * ld + col0 .. + min(max(length[r], 0), width)) (each token & 0xFFFF, as care_caption_stats reads it)
 * cut at the first `eos` or `pad`: the words to_sentence yields (misc/utils.py:117-137), n <= 64 of them.  Its KEY:
 *     key = (h(n, 64) + sum_j h(token_j, j)) & key_mask,  h(a, i) = fin(a + 0x9E3779B97F4A7C15 (i + 1)),
 *   fin the splitmix64 finaliser, all in uint64 with wrap-around (care_amd.corpusstats.caption_key is the same function in
 *   numpy).  A key only says where to look: equality is always decided token by token, so every count below is exact.
 * care_corpus_bank (a HOST struct of DEVICE arrays, care_amd.corpusstats.CorpusBank): the DISTINCT training captions -
 *   cal_gt_n_gram's `gt_sents`, the ids tmp[1:-1] of every training caption - with keys [n] ascending, caption i owning
 *   tokens [start[i], start[i + 1]) (any length; one of more than 64 tokens equals no caption).  key_mask (all ones by
 *   default, the same in the bank and in the set) is ANDed onto every key: a small mask makes long runs of equal keys and long
 *   probe chains out of a handful of captions, for the tests.
 * care_epoch_set (a HOST struct of DEVICE arrays, care_amd.corpusstats.EpochCaptions): the captions of the epoch so far.
 *   tokens [capacity, 64] / length [capacity] / keys [capacity]: the epoch store, row g the g-th caption inserted (zeros behind
 *   its length); slots [capacity]: the open-addressing table, -1 = empty, else the store row of the FIRST caption of its kind;
 *   bitmap [CARE_CORPUS_BITMAP_WORDS]: bit t set when token t stands in a caption; totals [CARE_CORPUS_TOTALS] (uint64):
 *     N_CAPTIONS, LENGTH_SUM (an empty caption counts 1: ''.split(' ') is ['']), N_DISTINCT, N_NOVEL (distinct captions no
 *     training caption equals; the empty caption is novel unless a training caption is empty), N_EMPTY, USAGE (written by
 *     care_corpus_totals), N_OVERFLOW (captions that found no slot: 0 unless the caller broke the rules below), 0.
 *   The caller zeroes tokens / bitmap / totals and sets every slot to -1 once an epoch.  `capacity` is a power of two.
 * care_corpus_insert: ADDS the `rows` captions of a batch as store rows [cursor, cursor + rows).  Two launches behind one
 *   another, one wave per caption with a token per lane: the first cuts the captions and writes their store rows and keys
 *   (keys_out [rows], optional, gets the keys too); the second sets the tokens' bits (atomic or), adds to the totals and
 *   probes the table from slot key & (capacity - 1) onwards with wrap-around: an empty slot is taken by a 32-bit atomicCAS - the
 *   caption is the first of its kind, and is looked up in the bank (binary search for the first equal key, then along the run
 *   of equal keys); a slot that names a row with other tokens is passed; one that names an equal row ends the probe - a
 *   duplicate.  A slot only ever names a row written by an EARLIER launch, so no fence is needed; which of several equal
 *   captions of one launch wins is a race that no total depends on.  The totals are integers: exact for any split of an epoch
 *   into batches.  The caller advances `cursor` by `rows` (a host integer); the same cursor twice counts the batch twice.
 *   NULL tokens / length / bank / set or a NULL array of either struct, rows < 0, cursor < 0, width < 1, col0 < 0,
 *   ld < col0 + width, bank n < 0, a bank whose key_mask is not the set's -> CARE_EINVAL; a capacity that is not a power of two, width > 64, cursor + rows > capacity
 *   -> CARE_ESHAPE; a uint64 / int64 array that is not 8-byte aligned -> CARE_EALIGN; all before anything is launched.
 *   rows == 0: a no-op that returns 0.
 * care_corpus_totals: totals[USAGE] = the set bits of the bitmap + (N_EMPTY != 0): the `usage` of the epoch so far (len of
 *   cal_n_gram's gram_count with n = 1, the empty word included).  One workgroup; WRITES, so it may run at any time.
 * care_caption_model_score: out [B] (double) = the `score` translate_batch returns with a clip's first caption: the value
 *   (double)fscore / len_pow[clamp(flen, 0, n_pow - 1)] of care_beam_winner's choice among the first min(nfin, cap)
 *   hypotheses of fscore / flen [B, cap] - the largest, a number before NaN.  nfin NULL: every clip has one hypothesis - the
 *   greedy decode with cap = 1, fscore = its scores, flen = its lengths.  nfin <= 0: 0.  The division Translator_ARFormer._norm
 *   does on the host, bit for bit.  NULL fscore / flen / len_pow / out, B < 0, cap < 1, cap > 64, n_pow < 1 -> CARE_EINVAL;
 *   len_pow / out not 8-byte aligned -> CARE_EALIGN; B == 0: a no-op.
 */
#define CARE_CORPUS_MAX_CAPTION 64
#define CARE_CORPUS_BITMAP_WORDS 2048
#define CARE_CORPUS_TOTALS 8
#define CARE_CORPUS_N_CAPTIONS 0
#define CARE_CORPUS_LENGTH_SUM 1
#define CARE_CORPUS_N_DISTINCT 2
#define CARE_CORPUS_N_NOVEL 3
#define CARE_CORPUS_N_EMPTY 4
#define CARE_CORPUS_USAGE 5
#define CARE_CORPUS_N_OVERFLOW 6
typedef struct care_corpus_bank {
  const uint64_t* keys; const int64_t* start; const int32_t* tokens;
  int64_t n;
  uint64_t key_mask;
} care_corpus_bank;
typedef struct care_epoch_set {
  int32_t* slots; int32_t* tokens; int32_t* length; uint64_t* keys;
  uint32_t* bitmap; uint64_t* totals;
  int32_t capacity; int32_t reserved;
  uint64_t key_mask;
} care_epoch_set;
int care_corpus_insert(const int32_t* tokens, int ld, int col0, int width, const int32_t* length, int rows, int cursor, int eos,
                       int pad, const care_corpus_bank* bank, const care_epoch_set* set, uint64_t* keys_out, void* stream);
int care_corpus_totals(const care_epoch_set* set, void* stream);
int care_caption_model_score(const int32_t* nfin, const float* fscore, const int32_t* flen, int B, int cap, const double* len_pow,
                             int n_pow, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CARE_HIP_H */
