/* rlaifv_hip.h - C ABI of librlaifv_hip.so, the MI355X (gfx950) kernels behind the RLAIF-V LLaVA-1.5
 * DPO training step.
 *
 * Boundary: the reference has no FFI/plugin layer - its hot path is Python
 * calling HuggingFace/torch modules.  Each entry point below replaces the third-party / reference
 * arithmetic named in its comment (paths relative to the reference checkout).  The Python host
 * (rlaif_v_amd.hip) binds these with ctypes; INTEGRATION.md shows the stub a reference maintainer adds.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller and borrowed for the call;
 *    bf16 tensors are raw uint16 bit patterns (`void*`), statistics are fp32, indices are int32;
 *  - `ld*` are row strides in ELEMENTS; bf16 rows must be 16-byte aligned;
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*); nothing synchronises;
 *  - return 0 = ok, 1 = argument error, 2 = launch error; text via rv_last_error() (thread local);
 *  - containment (pinned by tests/test_containment_gpu.py): an entry point reads and writes only the logical [rows][cols] of its
 *    operands - never the ld-padding columns behind a row, never a row past M / N / R (edge tiles of the GEMMs re-read the last
 *    row, contraction rows past R of the TN forms come from an internal zero row), never a row that row_idx / idx / row_off +
 *    row_len do not name - and no result depends on anything else; a workspace is written inside its documented size only;
 *  - accuracy (pinned per element against float64 by tests/test_accuracy_gpu.py, bound and derivations in tests/accuracy.py): every
 *    output is the documented formula evaluated in fp32 (any summation order; __expf / exp2, division, rsqrt, erff to a few fp32
 *    ulps) and stored with ONE round-to-nearest-even; an operand is rounded to bf16 inside a kernel only where the entry point's
 *    comment names that rounding ("ROUNDING:");
 *  - no exceptions cross the ABI, no internal threads, no allocation.
 */
#ifndef RLAIFV_HIP_H
#define RLAIFV_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RV_ABI_VERSION 7

const char* rv_last_error(void);
int rv_abi_version(void);
/* ---- TEST-ONLY knobs (the four rv_set_* below).  They write process-global state without synchronisation: call them from ONE
 * thread, with no launch of this library in flight on another thread, and never from production code - the product path
 * (the rlaif-v_amd Python modules) does not call them; tests use them to run two kernel generations against each other inside one process.
 * Everything else in this library is stateless (per-call arguments only).
 * A/B and test knob: 1 (default, also RV_GEMM_MI16) = the NN-A64 / fused-LoRA NN / TN main loops issue 16x16x32 MFMAs
 * (more flops per joule under the package power cap, profiles/r02_mfma_shape_power_probe.log); 0 = the 32x32x16 loops.
 * Same results to fp32 accumulation order. */
int rv_set_gemm_mi16(int on);
/* dK/dV kernel of rv_attn_bwd: 5 = the round-4 kernel (default), 3 = the round-2/3 kernel, 0 = back to the default / RV_ATTN_DKV.
 * A/B and test knob (both kernels against each other in one process); replaces nothing in the reference. */
int rv_set_attn_dkv_version(int version);
/* forward kernel of rv_attn_fwd at head dim 128: 3 = the round-6 kernel (one wave per SIMD, two 32-query blocks per wave
 * software-pipelined across key tiles, lazy rescale; csrc/attn_fwd3.inc), 2 = the round-2..5 kernel, 0 = back to the default /
 * RV_ATTN_FWD.  A/B and test knob; replaces nothing in the reference. */
int rv_set_attn_fwd_version(int version);
/* GEMM kernel selection: -1 = auto (default), 0 = 128x128x64 register-staged, 1 = 128x128x64 global_load_lds,
 * 2 = 256x256x32 ping-pong (two wave groups alternating MFMA / load segments). */
int rv_set_gemm_variant(int variant);

/* ---- dense contractions (replace torch.nn.Linear inside HF LlamaForCausalLM / CLIPVisionModel /
 *      mm_projector: llava/model/language_model/llava_llama.py:91-102,
 *      llava/model/multimodal_encoder/clip_encoder.py:55, llava/model/multimodal_projector/builder.py:39-46)
 *   C[m][n] = act(alpha * sum_k A[m][k] * B[n][k] + bias[n]) + R[m][n]        (bf16 in, fp32 accumulate)
 *   act: 0 none, 1 quick_gelu (CLIP MLP), 2 gelu(erf) (projector).  K % 64 == 0, N % 4 == 0.
 *   variant: -1 = process default, else as rv_set_gemm_variant. */
int rv_gemm_nt_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                    const void* bias, const void* residual, long ldr, int act, float alpha, int variant,
                    void* stream);
/* C[m][n] = alpha * sum_k A[m][k] * B[k][n] (+ residual): NN form - B is [K][N] row-major (N contiguous).  The same
 * nn.Linear forward / input-gradient products as rv_gemm_nt_bf16, fed with the other orientation of the weight
 * (forward: B = W^T copy [in][out]; input gradient: B = W [out][in]) so that the weight tile is fetched in full
 * 512-byte row segments.  Large problems only (256x256 tiles); K % 32 == 0, N % 8 == 0. */
int rv_gemm_nn_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                    const void* residual, long ldr, float alpha, void* stream);
/* The same with the bias / activation epilogue of rv_gemm_nt_bf16: C = act(alpha * A B + bias[n]) + residual (ABI 7).  For frozen,
 * forward-only towers whose nn.Linear weights (with bias; fc1 + GELU) are kept ONLY in the [in][out] orientation: the EVA02 blocks
 * behind omnilmm/model/omnilmm.py:31-43 (timm Attention.qkv / proj, Mlp.fc1 / fc2). */
int rv_gemm_nn_bias_act_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                             const void* bias, const void* residual, long ldr, int act, float alpha, void* stream);

/* q|k|v projection with RoPE in the epilogue (ABI 7; HF apply_rotary_pos_emb on the outputs of q_proj / k_proj, reached through
 * llava/model/language_model/llava_llama.py:91-102): C = A B with B the W^T copy [K][N] of the fused q|k|v weight; the first
 * rope_cols columns (the q and k heads, head dim hd = 128) leave rotated - y1 = x1 cos - x2 sin, y2 = x2 cos + x1 sin for the
 * half-split pairs (i, i + 64), tables [position][64] fp32 as rv_rope_inplace takes them, position = pos[token] or token % L - from
 * the fp32 accumulators (one rounding; replaces rv_gemm_nn_bf16 + rv_rope_inplace).  N, rope_cols multiples of 256, K % 64 == 0,
 * K >= 512. */
int rv_gemm_nn_rope_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                         const float* cos_tab, const float* sin_tab, const int* pos, int L, int rope_cols, int hd, void* stream);

/* The two fused SwiGLU GEMMs for ADAPTER models (ABI 7; peft lora.Linear.forward of gate_proj / up_proj + LlamaMLP's act_fn(gate) * up,
 * muffin/train/train_llava15_lora.py:304-318).  Forward: GU = [A | A2] [B | B2]^T with interleaved gate / up columns, ACT = silu(g) u,
 * optionally ACTD = rv_dropout(ACT; p, seed) (the dropped adapter input of the down projection).  B2 = the expanded adapter matrix
 * [K2 = 2 r][N]: rows 0..r-1 = lora_B(gate)^T on the even columns (zeros on the odd ones), rows r..2r-1 = lora_B(up)^T on the odd
 * columns; A2 = t = (alpha / r) dropout(x) [lora_A(gate); lora_A(up)]^T [M][2 r].
 * Backward: d(gate|up) = SwiGLU'(GU) o (A B + mask_{p,seed}(A2 B2) / (1 - p)) - the down projection's input gradient with the
 * adapter term (A = dy, B = W_down [d][f], A2 = dt [M][r], B2 = lora_A(down) [r][f]; p = 0: no mask). */
int rv_gemm_nn_lora_swiglu_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                                long ldb2, int K2, void* GU, long ldgu, void* ACT, long ldact, void* ACTD, float p, int seed,
                                int M, int N, int K, void* stream);
int rv_gemm_nn_lora_swiglu_bwd_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                                    long ldb2, int K2, float p, int seed, const void* GU, long ldgu, void* DGU, long lddgu,
                                    int M, int N, int K, void* stream);

/* gate|up projection with SwiGLU in the epilogue (HF LlamaMLP.forward: down_proj(act_fn(gate_proj(x)) * up_proj(x)),
 * reached through llava_llama.py:91-102).  B = the W^T copy [K][N] of the fused weight whose rows are INTERLEAVED
 * (row 2j = gate_j, row 2j+1 = up_j), N = 2 x ffn.  Writes GU [M][N] (kept for backward) and ACT [M][N/2] = silu(g) * u. */
int rv_gemm_nn_swiglu_bf16(const void* A, long lda, const void* B, long ldb, void* GU, long ldgu, void* ACT, long ldact,
                           int M, int N, int K, void* stream);
/* Input gradient of down_proj with the SwiGLU backward in the epilogue: d act = A [M][K] x B [K][N] (B = W_down, N = ffn)
 * never reaches memory; DGU [M][2N] = d(gate|up) interleaved like GU [M][2N].
 * ROUNDING (this and rv_gemm_nn_lora_swiglu_bwd_bf16): d act is rounded to bf16 before SwiGLU' is applied (what the unfused path
 * stores); the forward forms compute ACT from the fp32 accumulators (one rounding) and ACTD = rv_dropout of the ROUNDED ACT. */
int rv_gemm_nn_swiglu_bwd_bf16(const void* A, long lda, const void* B, long ldb, const void* GU, long ldgu, void* DGU,
                               long lddgu, int M, int N, int K, void* stream);

/* Fused LoRA GEMM (peft LoraLayer.forward as used by muffin/train/train_llava15_lora.py:304-318):
 *   C[m][n] = sum_{k<K} A[m][k] B[n][k] + sum_{q<K2} A2[m][c0(n)+q] B2[n][q] (+ residual[m][n]),
 *   c0(n) = group_cols ? group(n) * K2 : 0,  group(n) = n < group0 ? 0 : 1 + (n - group0) / group_cols  (group0 = 0: = group_cols;
 *   grouped-query attention: group0 = hidden (q), group_cols = kv_dim (k, v)).
 * The adapter contribution is two extra steps of the SAME K loop (operand tiles fetched from A2/B2), so
 * the base output is never re-read.  Forward: A = x, B = W, A2 = t = (alpha/r) x A_lora^T [M, G*r], B2 = stacked
 * lora_B [N, r], group_cols = rows of one fused projection (q|k|v, gate|up).  Input gradient: A = dy, B = W^T,
 * A2 = dt [M, G*r], B2 = stacked lora_A^T [N, G*r], group_cols = 0.  K2 multiple of 64; group_cols multiple of 128. */
int rv_gemm_nt_lora_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                         long ldb2, int K2, int group_cols, int group0, void* C, long ldc, int M, int N, int K,
                         const void* residual, long ldr, void* stream);

/* NN form of rv_gemm_nt_lora_bf16: B is [K][N], B2 is [K2][N] (both row-major); A2 as there.  Forward: B = W^T copy,
 * B2 = stacked lora_B^T [r][N]; input gradient: B = W, B2 = stacked lora_A [G*r][N], group_cols = 0.  K, K2 % 32 == 0;
 * group_cols a multiple of 256. */
int rv_gemm_nn_lora_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                         long ldb2, int K2, int group_cols, int group0, void* C, long ldc, int M, int N, int K,
                         const void* residual, long ldr, void* stream);

/* C = dropout_{p,seed}(alpha * A B^T) + residual: rv_gemm_nt_bf16 whose result is masked with exactly the mask
 * rv_dropout(p, seed) draws for a contiguous [M][N] tensor, before the residual is added.  Backward of the LoRA branch
 * dropout: dx = dy W + mask * (dt A) / (1 - p) without materialising dt A.  N % 8 == 0. */
int rv_gemm_nt_dropout_bf16(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                            const void* residual, long ldr, float alpha, float p, int seed, void* stream);

/* C = A B + dropout_{p,seed}(A2 B2) (+ residual) in ONE pass over C: the LoRA input gradient under adapter dropout
 * (peft lora.Linear: result += lora_B(lora_A(dropout(x))) * scaling, so dx = dy W + mask * (dt A) / (1 - p); replaces
 * rv_gemm_nn_bf16 followed by rv_gemm_nt_dropout_bf16 with C as its own residual - two more passes over [M][N]).  A [M][K],
 * B [K][N], A2 = dt [M][K2], B2 = stacked lora_A [K2][N], all row-major; the adapter segment runs FIRST, the mask rv_dropout(p,
 * seed) draws for a contiguous [M][N] tensor is applied to the fp32 accumulators, the main segment accumulates on top (one
 * rounding to bf16 instead of two).  K % 64 == 0, K >= 512, K2 % 64 == 0, N % 8 == 0.  group_cols / group0 as in
 * rv_gemm_nn_lora_bf16 (A2 then has one K2-wide column block per group); with p = 0 this is the adapter-first form of that
 * function (the forward of a fused projection: one 64-deep adapter step per column tile instead of seam phases in the ring). */
int rv_gemm_nn_lora_pre_bf16(const void* A, long lda, const void* B, long ldb, const void* A2, long lda2, const void* B2,
                             long ldb2, int K2, int group_cols, int group0, float p, int seed, void* C, long ldc, int M, int N,
                             int K, const void* residual, long ldr, void* stream);

/* Split-K form of rv_gemm_tn_bf16 for skinny outputs (LoRA weight gradients: I or J = r): `splits` chunks of the
 * contraction rows are reduced by separate workgroups into fp32 slabs (workspace: splits*I*J floats, caller owned)
 * which a second pass sums in a fixed order: C = bf16(alpha * sum).  Deterministic. */
int rv_gemm_tn_bf16_splitk(const void* P, long ldp, const void* Q, long ldq, void* C, long ldc, int R, int I, int J,
                           float alpha, int splits, float* workspace, void* stream);

/* LoRA adapter dropout with ONE MASK PER peft MODULE (peft gives every wrapped nn.Linear its own nn.Dropout, so the G modules of a
 * fused projection - q | k | v, gate | up - drop the same input with independent masks).  Module g uses the mask rv_dropout(p,
 * seed_g) draws for the contiguous [rows][width] adapter input (element index row * width + col, whatever leading dimension is
 * passed); the three functions regenerate it on the operand they hold, no dropped copy exists in memory.  G in {1, 2, 3} (seeds
 * beyond G are ignored), rank block 64 per module, 0 <= p < 1; additive in ABI 7.
 *
 * Adapter down-projection: T[:, 64 g .. 64 g + 63] = alpha * dropout_{p, seed_g}(X) A_g^T, X [M][K], A [64 G][K] (stacked lora_A),
 * T [M][64 G].  X is read once for all G modules; the kept values are scaled by 1.f / (1.f - p) and rounded to bf16 before the MFMA
 * (rv_dropout's arithmetic); any M >= 1, K % 64 == 0; p = 0 is the plain product (K order of rv_gemm_nt_bf16). */
int rv_gemm_nt_lora_masks_bf16(const void* X, long ldx, const void* A, long lda, void* T, long ldt, int M, int K, int G,
                               float alpha, float p, int seed0, int seed1, int seed2, void* stream);

/* Adapter term of the input gradient: C = residual + sum_g mask_{p, seed_g} o (dT_g AT_g^T) / (1 - p), dT [M][64 G], AT [N][64 G]
 * (transposed stacked lora_A), C / residual [M][N] (residual may be NULL or C itself), masks those of the [M][N] adapter input.
 * One read and one write of [M][N] for all modules; module g's term is added with its own rounding to bf16, i.e. the result is
 * bit for bit that of G calls of rv_gemm_nt_dropout_bf16 with C as its own residual (G = 1 is that function).  N % 64 == 0. */
int rv_gemm_nt_dropout_masks_bf16(const void* dT, long lddt, const void* AT, long ldat, void* C, long ldc, int M, int N, int G,
                                  const void* residual, long ldr, float p, int seed0, int seed1, int seed2, void* stream);

/* Adapter weight gradient: dA[64 g .. 64 g + 63][:] = dT_g^T dropout_{p, seed_g}(X), dT [R][64 G], X [R][K], dA [64 G][K], from
 * one pass over X: `splits` chunks of the token rows are reduced into fp32 slabs (workspace: splits * 64 G * K floats, caller
 * owned) which a second pass sums in a fixed order.  Deterministic.  K % 64 == 0; p = 0 is rv_gemm_tn_bf16_splitk.
 * ROUNDING: as in the down-projection, the kept values of X are scaled by 1.f / (1.f - p) and rounded to bf16 before the MFMA. */
int rv_gemm_tn_lora_masks_bf16(const void* dT, long lddt, const void* X, long ldx, void* dA, long ldda, int R, int K, int G, float p,
                               int seed0, int seed1, int seed2, int splits, float* workspace, void* stream);

/* Weight-gradient contraction over the ROW index of both operands (no transposed copies in HBM):
 *   C[i][j] = alpha * sum_r P[r][i] * Q[r][j] + residual[i][j]      P [R][I], Q [R][J], C [I][J]; I, J % 8 == 0
 * e.g. dW = dY^T X (autograd of nn.Linear); operands are transposed on the fly by ds_read_b64_tr_b16. */
int rv_gemm_tn_bf16(const void* P, long ldp, const void* Q, long ldq, void* C, long ldc, int R, int I, int J,
                    const void* residual, long ldr, float alpha, void* stream);
/* rv_gemm_tn_bf16 (no residual, alpha 1) with a TAIL SPLIT: all output tiles of a weight gradient cost the same, so the last,
 * partly filled round of 256 tiles takes as long as a full one; with a workspace the tiles of that round are split over the
 * token axis into fp32 slabs and summed in fixed order (deterministic), e.g. wgu 1376 tiles: 6 -> 5.5 rounds.
 * rv_gemm_tn_workspace_floats: floats the plan for (R, I, J) needs (0: no split pays - then rv_gemm_tn_bf16_ws is
 * rv_gemm_tn_bf16).  A NULL / too small workspace also falls back to the plain launch. */
int rv_gemm_tn_workspace_floats(int R, int I, int J);
int rv_gemm_tn_bf16_ws(const void* P, long ldp, const void* Q, long ldq, void* C, long ldc, int R, int I, int J,
                       float* workspace, long workspace_floats, void* stream);
int rv_gemm_nt_bf16_f32out(const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M, int N, int K,
                           int variant, void* stream);
/* C (fp32) = sum_k A[m][k] B[n][k] + bias[n] + residual[m][n] (fp32; may alias C): the out_proj / fc2 products of the frozen CLIP
 * tower (llava/model/multimodal_encoder/clip_encoder.py:46-58, HF CLIPEncoderLayer) with the tower's residual stream carried in fp32
 * (RV_CLIP_FP32_RESID).  bias / residual may be NULL. */
int rv_gemm_nt_bf16_f32res(const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M, int N, int K,
                           const void* bias, const float* residual, long ldr, int variant, void* stream);

/* ---- fused LM head + log-softmax + label gather (replaces lm_head + get_batch_logps,
 *      muffin/eval/muffin_inference_logp.py:82-115; logits [rows, V] never reach HBM).
 *   fwd : per selected row m and 64-column block j:  pmax[m][j], psum[m][j] = max / sum exp(x - max);
 *         tgt_logit[m] = logit of tgt[m].   V = rows of W = a multiple of 64; columns [V_valid, V) are vocabulary
 *         padding (a tokenizer with added tokens, e.g. OmniLMM's 32000 + 9): left out of the softmax, zero in dlogits.
 *   finish: lse[m], logp[m] = tgt_logit[m] - lse[m].
 *   bwd : dlogits[m][n] = coef[m] * ((n == tgt[m]) - exp(logit - lse[m]))  (bf16, recomputed logits).
 *   Sizes and padding: pmax / psum are [M][V / 64], written completely.  tgt_logit[m] is written only when 0 <= tgt[m] < V (-inf for
 *   a target among the padding columns): the CALLER pre-fills it (ops.lmhead_logp_fwd: zeros), so a row whose target is no
 *   vocabulary id (-100) gets logp = fill - lse and, in bwd, no one-hot term.  Rows of h past M are never read (h needs no padding rows for these calls) and rows
 *   [V_valid, V) of W never reach a result.  bwd writes rows m < M of dlogits over all V columns (the padding columns as zeros)
 *   and leaves rows >= M alone: a caller that feeds a row-padded dlogits to a GEMM zeroes those rows itself
 *   (ops.lmhead_logp_bwd does). */
int rv_lmhead_logp_fwd(const void* h, long ldh, const void* W, long ldw, const int* tgt, int M, int V, int V_valid, int K,
                       float* pmax, float* psum, float* tgt_logit, int variant, void* stream);
int rv_logp_finish(const float* pmax, const float* psum, const float* tgt_logit, int nblk, int M, float* lse,
                   float* logp, void* stream);
/* finish + unpack (the packed log-prob precompute): the lse / logp of rv_logp_finish (same device code, bit-equal), then row
 * m's logp is written to per_token[dst_a[m]], per_token[dst_b[m]] and compact[dst_c[m]]; a negative index is skipped, one
 * out of range too.  Every destination must have one writer (plain stores, no atomics); slots no row names keep the
 * caller's fill. */
int rv_logp_finish_unpack(const float* pmax, const float* psum, const float* tgt_logit, int nblk, int M, const int* dst_a,
                          const int* dst_b, const int* dst_c, float* per_token, long n_per_token, float* compact, int n_compact,
                          void* stream);
int rv_lmhead_logp_bwd(const void* h, long ldh, const void* W, long ldw, const int* tgt, const float* lse,
                       const float* coef, void* dlogits, long ldd, int M, int V, int V_valid, int K, int variant,
                       void* stream);
/* Next-token scores of the yes / no feedback stage (muffin/llava15_gen_data.py:266-333, omnilmm/omnilmm_gen_data.py:245-300:
 * generate(max_new_tokens=1, output_scores=True), softmax of scores[0] read at a few ids).  logits: fp32 [M][ldl], READ ONLY;
 * the softmax runs over the columns [0, V_valid) - the columns behind them are vocabulary padding.  Repetition penalty (HF
 * RepetitionPenaltyLogitsProcessor; penalty == 1 or seen_off == NULL: off): seen_ids[seen_off[m] .. seen_off[m+1]) are the
 * token ids of row m's prompt, a logit l at such an id becomes l / penalty if l > 0, else l * penalty.
 *   probs / logp [M][K]: softmax / log-softmax at want_ids[k] (an id outside [0, V_valid): 0 / -inf);  lse [M];
 *   argmax [M]: greedy next token, the LOWEST index among equal maxima.  One workgroup per row, fixed reduction order. */
int rv_next_token_scores(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids,
                         float penalty, const int* want_ids, int K, float* probs, float* logp, int* argmax, float* lse,
                         void* stream);
/* (per_token_logps * loss_mask).sum(-1) and loss_mask.sum(-1) of get_batch_logps (:103-104); rows of
 * sequence s are seq_off[s] .. seq_off[s+1]; optional per-row weight (compute_weighted_logp,
 * muffin/train/trainers.py:128-137). Fixed summation order. */
int rv_seq_sum(const float* logp, const float* weight, const int* seq_off, int n_seq, float* out_sum, float* out_cnt,
               void* stream);
/* dpo_loss + loss mix + metrics (muffin/train/trainers.py:91-126, :292-309) and its closed-form gradient.
 *   per_pair[5][B] = losses, chosen_rewards, rejected_rewards, policy_win_logp, policy_rej_logp
 *   scalars[8]     = loss, mean chosen reward, mean rejected reward, accuracy, margin, mean win logp, mean rej logp, 0
 *   coef[2B]       = d loss / d (sequence log-prob sum) */
int rv_dpo_loss(const float* seq_sum, const float* seq_cnt, const float* ref_win, const float* ref_rej, int B,
                float beta, int use_average, float sft_weight, float dpo_weight, float* per_pair, float* scalars,
                float* coef, void* stream);
int rv_row_coef(const float* coef, const int* seq_of_row, const float* weight, float* out, int n, void* stream);

/* ---- attention (replaces HF LlamaAttention eager/SDPA math and CLIPAttention).
 *   qkv: [S*L][ld] with q heads at q_col0 + h*hd, k heads at k_col0 + h*hd, v heads at v_col0 + h*hd.
 *   out: [S*L][ldo] (head h at column h*hd); lse: [S][H][L] natural-log of sum exp(scale * q.k).
 *   causal=1: pure causal mask, no padding mask (muffin/train/trainers.py:199). hd in {64,128}.
 *   K/V tiles are staged by LDS-DMA and transposed on the fly (ds_read_b64_tr_b16): no side copies. */
/*   seg_sh / seg_e1 (int32 [S], both NULL = plain causal): packed preference pairs.  Row s holds
 *   [shared prefix | chosen branch | rejected branch]; queries at index >= seg_e1[s] (rejected branch) do not attend
 *   keys in [seg_sh[s], seg_e1[s]) (the chosen branch): the image / prompt prefix is computed ONCE per pair.
 *   With causal = 0 the window still applies: queries at index >= seg_e1[s] do not see the keys [seg_sh[s], seg_e1[s]), every other
 *   (query, key) pair of the row is visible (tests/test_accuracy_gpu.py, layout full-window-L200, forward and backward). */
/*   row_off / row_len (int32 [S], both NULL = S rectangular rows of L tokens; ABI 6): PAD-FREE rows.  Sequence s occupies token
 *   rows [row_off[s], row_off[s] + row_len[s]) of qkv / out (1 <= row_len[s] <= L); the reference right-pads every row to the batch
 *   maximum (llava/model/llava_arch.py:305-313) and SURVEY 8a property (i) makes skipping those pads exact.  L stays the MAXIMUM row
 *   length: it sizes the grid and the [S][H][L] stride of lse (and of the backward's delta planes); seg_sh / seg_e1 are per-row
 *   offsets as before.  Results of a row do not depend on where it starts (tiles are laid relative to the row's first token).
 *   What is touched: of qkv only the H (q) and H / kv_group (k, v) heads at the three column offsets, in the token rows of the S
 *   sequences; of out (and of the backward's dqkv) only those rows and head columns - token rows between or behind pad-free
 *   sequences and columns outside the heads are neither read nor written.  lse[s][h][l] is written for l < row_len[s] only; the
 *   entries at l >= row_len[s] keep the caller's bytes and rv_attn_bwd does not read them; the per-token tables (q_lo, rope_pos)
 *   are read at the sequences' token rows only. */
/*   ROUNDING (rv_attn_fwd, rv_attn_fwd_branches): the probabilities p = exp2(scale log2e s - m) are rounded to bf16 for the P V MFMA;
 *   the row sum (the denominator of out, and lse) is taken from the unrounded fp32 p.  rv_attn_bwd: P (for dV) and dS = P (dP - delta)
 *   (for dQ, dK) are rounded to bf16 once, for their MFMAs; with rope_cos / rope_sin, dQ and dK are rounded to bf16 (what the
 *   separate rv_rope_inplace pass read back) and then rotated in fp32, so they carry a second rounding at the store. */
int rv_attn_fwd(const void* qkv, long ld, int q_col0, int k_col0, int v_col0, void* out, long ldo, float* lse, int S,
                int L, int H, int hd, int causal, float scale, const int* seg_sh, const int* seg_e1, int kv_group,
                const int* row_off, const int* row_len, void* stream);
/* N-branch packed rows (the yes / no feedback stage: many short questions about one image).  Row s holds
 *   [shared prefix | branch 0 | branch 1 | ... | branch N-1]; seg_sh[s] is the prefix length and q_lo (int32, one entry per TOKEN
 *   row of the buffer, indexed like rv_attn_bwd's rope_pos: row_off[s] + i under pad-free rows, s * L + i otherwise) gives, for
 *   query i, the first key - relative to the row's first token - of its own branch.  Always causal:
 *       query i attends key j  <=>  j <= i  &&  (j < seg_sh[s]  ||  j >= q_lo[i]).
 *   q_lo[i] is ignored for i < seg_sh[s]; for the other queries seg_sh[s] <= q_lo[i] <= i, and q_lo does not decrease inside a
 *   row.  The CALLER guarantees these conditions (rlaif-v_amd/splice.py check_branch_rows); the kernel does not check them.
 *   Everything else (lse, out, kv_group, row_off / row_len, hd in {64, 128}) as in rv_attn_fwd, whose main loop this is: with two
 *   branches it gives rv_attn_fwd(seg_sh, seg_e1)'s bits, with one branch plain causal rv_attn_fwd's.  Forward only. */
int rv_attn_fwd_branches(const void* qkv, long ld, int q_col0, int k_col0, int v_col0, void* out, long ldo, float* lse,
                         int S, int L, int H, int hd, float scale, const int* seg_sh, const int* q_lo, int kv_group,
                         const int* row_off, const int* row_len, void* stream);
/* kv_group (both calls): grouped-query attention as in HF Mistral / Llama-3 (`repeat_kv`): H query heads share
 * H / kv_group key/value heads, query head h reads kv head h / kv_group (K at k_col0 + (h / kv_group) * hd); 1 = MHA.
 * backward (hd = 128): O = the forward output (rv_attn_fwd's `out`), delta = [3][S, H, L] fp32 WORKSPACE (ABI 5; it was [S, H, L]): the dQ
 * kernel fills it with rowsum(dO * O) (what rv_attn_delta computes), its negative and -lse / scale on the fly and the dK/dV kernel
 * reads them.  Writes dQ, dK, dV into
 * dqkv at the column offsets of qkv.  Deterministic (no atomics): one kernel per 128-query block for dQ, one per 128-key
 * block for dK/dV.  Packed rows: key tiles / query tiles that a whole block cannot see are never fetched.
 * rope_cos / rope_sin (fp32 [positions][64], both NULL = off) + rope_pos (int32 [S * L] position of every row, NULL = row
 * index inside its sequence): dQ and dK are written ALREADY rotated back (apply_rotary_pos_emb's autograd, HF
 * modeling_llama.py) - the separate rv_rope_inplace(backward) pass over dqkv is not needed.  rope_pos is indexed by the token's row
 * in the buffer (row_off[s] + i under pad-free rows, where it is required).
 * The delta workspace needs no initialisation: each of its three [S][H][L] planes is written at l < row_len[s] (all l without
 * pad-free rows) before the dK/dV kernel reads it there, the rest is neither written nor read, and nothing past
 * rv_attn_bwd_workspace_floats(S, H, L) floats is touched.  dO and O are read like out is written (sequence rows, head columns). */
int rv_attn_bwd(const void* qkv, long ld, int q_col0, int k_col0, int v_col0, const void* dO, long lddo,
                const void* O, long ldo, const float* lse, float* delta, void* dqkv, long lddq, int S, int L, int H,
                int hd, int causal, float scale, const int* seg_sh, const int* seg_e1, int kv_group,
                const float* rope_cos, const float* rope_sin, const int* rope_pos, const int* row_off, const int* row_len,
                void* stream);
/* Number of fp32 elements rv_attn_bwd's `delta` workspace must hold for (S, H, L) under THIS library's ABI (3 * S * H * L since
 * ABI 5).  Callers size the buffer with this query instead of hard-coding the plane count (the signature of rv_attn_bwd carries
 * no size argument). */
long rv_attn_bwd_workspace_floats(int S, int H, int L);
int rv_attn_delta(const void* dO, long lddo, const void* O, long ldo, float* delta, int S, int L, int H, int hd,
                  void* stream);

/* ---- norms / rotary / activations (replace HF LlamaRMSNorm, apply_rotary_pos_emb, LlamaMLP, CLIP LayerNorm)
 * row_idx (int32 [rows], NULL = identity) names the x row of output row r: x, and every operand that carries the residual stream
 * (add / xout of rv_rmsnorm_fwd_f32, dres / dx of the backward forms), is indexed by row_idx[r]; y, yd, rstd and dy by r.  Rows of x
 * that row_idx does not name are not read, rows of dx / xout it does not name are not written.  dw_partial is fp32 scratch
 * [rv_rmsnorm_bwd_nblocks(rows)][d], written completely; dw is bf16 [d], written (dw_accumulate = 0) or read and added to. */
int rv_rmsnorm_fwd(const void* x, long ldx, const int* row_idx, const void* w, void* y, long ldy, float* rstd,
                   int rows, int d, float eps, void* stream);
int rv_rmsnorm_bwd_nblocks(int rows);   /* rows of the fp32 dw_partial scratch [nblocks][d] */
int rv_rmsnorm_bwd(const void* dy, long lddy, const void* x, long ldx, const int* row_idx, const void* w,
                   const float* rstd, const void* dres, long lddres, void* dx, long lddx, float* dw_partial,
                   void* dw, int dw_accumulate, int rows, int d, void* stream);
/* Opt-in fp32 RESIDUAL STREAM of the decoder (RV_RESID_FP32=1, round 5; HF's LlamaDecoderLayer keeps hidden_states in the model dtype,
 * llava_llama.py:91-102).  The projection GEMMs write their branch in bf16 WITHOUT the residual operand; these kernels carry the stream:
 *   rv_rmsnorm_fwd_f32:  add != NULL: xout = x + add (fp32 rows, same row indexing), y = rmsnorm(xout) * w (bf16), rstd;
 *                        add == NULL: y = rmsnorm(x) * w on the fp32 rows (row_idx gathers rows like rv_rmsnorm_fwd);
 *                        y == NULL with add: only the sum is written (no norm).
 *   rv_rmsnorm_bwd_f32x: rv_rmsnorm_bwd reading an fp32 x (gradients stay bf16);
 *   rv_add_f32_bf16:     out = x + b for the last branch of the stack. */
int rv_rmsnorm_fwd_f32(const float* x, long ldx, const int* row_idx, const void* add, long ldadd, float* xout, long ldxout,
                       const void* w, void* y, long ldy, float* rstd, int rows, int d, float eps, void* stream);
int rv_rmsnorm_bwd_f32x(const void* dy, long lddy, const float* x, long ldx, const int* row_idx, const void* w,
                        const float* rstd, const void* dres, long lddres, void* dx, long lddx, float* dw_partial,
                        void* dw, int dw_accumulate, int rows, int d, void* stream);
int rv_add_f32_bf16(const float* x, const void* b, float* out, long n, void* stream);
int rv_layernorm_fwd(const void* x, long ldx, const void* w, const void* b, void* y, long ldy, int rows, int d,
                     float eps, void* stream);
/* the same LayerNorm reading an fp32 input (the fp32 residual stream above); output bf16 (it feeds a bf16 MFMA operand) */
int rv_layernorm_fwd_f32in(const float* x, long ldx, const void* w, const void* b, void* y, long ldy, int rows, int d,
                           float eps, void* stream);
/* LayerNorm backward for the OmniLMM Resampler's trainable ln_q / ln_kv / ln_post (omnilmm/model/resampler.py:127-129,
 * autograd of F.layer_norm): dx (NULL = not wanted), dw / db written or accumulated.  x_period > 0: rows r and r + x_period
 * share the x row r % x_period (the learned queries, identical for every image).  partial: fp32 scratch
 * [rv_rmsnorm_bwd_nblocks(rows)][2 d].  Any d % 8 == 0 up to 8192: exactly d elements of dw and of db are written (or, with
 * accumulate, read and written) - the two may be neighbours in one flat gradient buffer. */
int rv_layernorm_bwd(const void* dy, long lddy, const void* x, long ldx, int x_period, const void* w, void* dx, long lddx,
                     float* partial, void* dw, void* db, int accumulate, int rows, int d, float eps, void* stream);
/* y[r] = x[r] + p[r % period]: the Resampler's position tables added per image (resampler.py:150-155) */
int rv_add_rows(const void* x, long ldx, const void* p, long ldp, int period, void* y, long ldy, long rows, int d,
                void* stream);
/* y[q] = sum_b x[b * period + q]: gradient of a row block that was broadcast over the batch (resampler.py:166-167 _repeat) */
int rv_sum_rows_periodic(const void* x, long ldx, int period, int reps, void* y, long ldy, int d, void* stream);
/* in-place half-split RoPE over n_heads_total adjacent heads (q then k); position = pos[token] when pos != NULL
 * (packed pairs), else token % L (position_ids are dropped: llava/model/language_model/llava_llama.py:94);
 * backward = inverse rotation. */
int rv_rope_inplace(void* x, long ld, const float* cos_tab, const float* sin_tab, const int* pos, long n_tok, int L,
                    int n_heads_total, int hd, int backward, void* stream);
/* SwiGLU on a stored gate|up tensor [rows][2f] and its backward.  interleaved = 0: columns [gate | up];  1: column 2j = gate_j,
 * 2j+1 = up_j (the layout of the fused weight whose GEMM epilogues do this work - rv_gemm_nn_swiglu_bf16 - so the standalone
 * kernels then only serve the recompute paths). */
int rv_swiglu_fwd(const void* gu, long ldgu, void* act, long lda, long rows, int f, int interleaved, void* stream);
int rv_swiglu_bwd(const void* dact, long ldd, const void* gu, long ldgu, void* dgu, long lddgu, long rows, int f,
                  int interleaved, void* stream);
int rv_gelu_fwd(const void* x, void* y, long n, void* stream);
int rv_gelu_bwd(const void* dy, const void* x, void* dx, long n, void* stream);
/* Dropout of the LoRA branch input (peft lora_dropout, muffin/train/train_llava15_lora.py:114,309): element e is kept
 * iff hash16(seed, e) >= p * 2^16 and scaled by 1/(1-p); the same (seed, n) regenerates the same mask in backward.
 * y = dropped x (may alias x, may be NULL); acc (optional) += dropped x (gradient accumulation).  Contiguous, n % 8 == 0. */
int rv_dropout(const void* x, void* y, void* acc, long n, float p, int seed, void* stream);
/* Producer-side forms: rv_rmsnorm_fwd / rv_swiglu_fwd (block layout) that ALSO write yd = rv_dropout(y; p, seed) as a contiguous
 * [rows][d] / [rows][f] tensor, bit-identical to running rv_dropout on the output - the LoRA branch input of the projection that
 * follows (q|k|v, gate|up after the norms; down after SwiGLU) without re-reading the activation. */
int rv_rmsnorm_fwd_dropout(const void* x, long ldx, const int* row_idx, const void* w, void* y, long ldy, float* rstd,
                           int rows, int d, float eps, void* yd, float p, int seed, void* stream);
int rv_swiglu_fwd_dropout(const void* gu, long ldgu, void* act, long lda, long rows, int f, void* actd, float p, int seed,
                          void* stream);

/* ---- CLIP image preprocessing: CLIPImageProcessor of openai/clip-vit-large-patch14-336 as the reference applies it in
 * its DataLoader workers (muffin/train/train_llava15.py:244, muffin/train/train_utils.py:208) - PIL BICUBIC resize
 * (Pillow Resample.c: 22-bit fixed-point taps, uint8 after each pass), center crop, x 1/255, (x - mean) / std.
 * Two passes over the CROPPED window only; tap tables (bounds [n][2] = first source index, tap count; kk [n][ksize])
 * are built on the host exactly as Pillow's precompute_coeffs does.
 *   rv_resize_h_u8      : tmp[r][x][c] (uint8, rows x out_w x 3) from src [H][W][3] rows y0 .. y0+rows-1
 *   rv_resize_v_norm_u8 : out[c][y][x] (float32, 3 x out_h x out_w) = table[c][vertical pass], table = [3][256] */
int rv_resize_h_u8(const void* src, int H, int W, int y0, int rows, const int* bounds, const int* kk, int ksize, int out_w,
                   void* tmp, void* stream);
int rv_resize_v_norm_u8(const void* tmp, int rows, int out_w, const int* bounds, const int* kk, int ksize, int out_h,
                        const float* table, float* out, void* stream);

/* ---- data movement
 * rv_transpose: out [C][ldo] = in [R][C] transposed, ldo >= roundup(R, 64), C % 8 == 0: row c of out holds in[:, c] in its columns
 * [0, R) and ZEROS in the columns [R, roundup(R, 64)) (a K-padded GEMM operand); columns from roundup(R, 64) on are not written. */
int rv_transpose(const void* in, long ld_in, void* out, long ldo, int R, int C, void* stream);
/* prepare_inputs_labels_for_multimodal (llava/model/llava_arch.py:237-315): out row n = embed[src[n]] if
 * src[n] >= 0, zero if -1, image feature row (-2 - src[n]) otherwise. */
int rv_splice_fwd(const int* src, const void* embed, const void* feats, void* out, long n_rows, int d, void* stream);
/* rv_embed_bwd: row uniq_ids[u] of dW = the fp32 sum of the dx rows pos_sorted[seg_off[u] .. seg_off[u + 1]) (written, not added
 * to); rows of dW that uniq_ids does not name are left alone (the caller zeroes dW).  rv_feat_grad: dfeat[r] = dx[src_a[r]] +
 * dx[src_b[r]], an index of -1 = no such row.  rv_gather_rows: scatter = 0: out[r] = in[idx[r]]; 1: out[idx[r]] = in[r], rows of
 * out that idx does not name are left alone. */
int rv_embed_bwd(const int* uniq_ids, const int* seg_off, const int* pos_sorted, int n_uniq, const void* dx, void* dW,
                 int d, void* stream);
int rv_feat_grad(const int* src_a, const int* src_b, const void* dx, void* dfeat, long n_rows, int d, void* stream);
int rv_gather_rows(const void* in, long ld_in, const int* idx, void* out, long ld_out, long n_rows, int d, int scatter,
                   void* stream);
int rv_colsum(const void* dy, long ld, void* db, int M, int N, void* stream);
/* CLIPVisionEmbeddings (patch conv as GEMM): fp32 pixels -> bf16 patch rows [B*P][Kp], then CLS + pos-emb */
int rv_im2col_patches(const float* pixels, void* out, int B, int image_size, int patch, int Kp, void* stream);
int rv_clip_assemble(const void* patch, const void* cls, const void* pos, void* x, int B, int P, int d, void* stream);
int rv_cast_f32_to_bf16(const float* in, void* out, long n, void* stream);
int rv_cast_bf16_to_f32(const void* in, float* out, long n, void* stream);

/* ---- optimizer (replaces torch.optim.AdamW + clip_grad_norm_ selected by optim="adamw_torch",
 *      muffin/train/train_llava15.py:75).  The buffer may hold a SUM over ranks: pre_scale = 1/world.
 *      out2[0] = ||pre_scale*g||, out2[1] = pre_scale * min(1, max_norm/(out2[0]+1e-6)) = the factor
 *      rv_adamw_step multiplies raw gradients by (pass out2 as `clip`; NULL = 1). */
int rv_sumsq_nblocks(void);
int rv_grad_norm(const void* g, long n, float* partial, float max_norm, float pre_scale, float* out2,
                 void* stream);
int rv_adamw_step(void* p, float* master, float* m, float* v, const void* g, long n, float lr, float beta1, float beta2,
                  float eps, float wd, int step, const float* clip, void* stream);
/* The two halves of rv_grad_norm for a SHARDED optimizer (opt-in ZeRO-1, rlaif-v_amd/dist.py ShardedGradReducer; the reference
 * shards its optimizer the same way under DeepSpeed ZeRO-2, script/zero2.json:16-22): each rank holds the reduced gradient of its
 * shard only.  rv_grad_sumsq: out1[0] (+)= sum g^2 over a bf16 slice (partial: rv_sumsq_nblocks floats of scratch); the caller
 * all-reduces out1 over the ranks; rv_clip_from_sumsq: out2 = [pre_scale * sqrt(sumsq), pre_scale * min(1, max_norm / (that + 1e-6))],
 * the pair rv_grad_norm produces. */
int rv_grad_sumsq(const void* g, long n, float* partial, float* out1, int accumulate, void* stream);
int rv_clip_from_sumsq(const float* sumsq, float max_norm, float pre_scale, float* out2, void* stream);
/* --gradient_accumulation_steps (HF Trainer, script/train/llava15_train.sh:23): fp32 accumulation of the bf16 micro-batch
 * gradients.  mode 0: acc = g;  1: acc += g;  2: g = bf16((acc + g) * scale)  (scale = 1 / accumulation steps). */
int rv_grad_accum(float* acc, void* g, long n, int mode, float scale, void* stream);

/* ---- measurement helper (bench.py's single-GPU data-parallel probe; replaces nothing in the reference): dst = a + b
 *      (bf16, n elements) streamed by n_wg persistent 256-thread workgroups - the CU footprint of n_wg RCCL channels
 *      doing the receive-reduce-send of a ring all-reduce step (script/zero2.json:16-22 is what the real exchange replaces). */
int rv_reduce_copy_persistent(const void* a, const void* b, void* dst, long n, int n_wg, void* stream);

/* ---- KV-cached candidate generation (csrc/decode.hip; additive, ABI stays 7).  Replaces the decode steps of HF
 *      GenerationMixin.sample / greedy_search with use_cache=True behind model.generate(do_sample=True, temperature=, ...) in the
 *      sampling branch of muffin/llava15_gen_data.py:335-357 and omnilmm/omnilmm_gen_data.py:305-323.
 *
 * rv_gemm_nt_skinny_bf16: the nn.Linear products of ONE decode step (q|k|v, o, gate|up, down, LM head), 1 <= M <= 64 rows:
 *   C[m][n] = sum_k A[m][k] W[n][k] (+ residual[m][n]),  W [N][K] with K contiguous (rv_gemm_nt_bf16's orientation), fp32 accumulate.
 *   K % 64 == 0, N % 4 == 0, lda / ldw % 8 == 0, ldc / ldr % 4 == 0.  out_f32: 0 = C is bf16, 1 = C is fp32 (the LM-head logits that
 *   rv_next_token_scores / rv_sample_token read); residual is bf16 in both cases and may be NULL.  Weight-bandwidth bound: one
 *   workgroup owns a 16-column panel and all M rows (256 workgroups at N = 4096), W goes from global memory straight into MFMA
 *   fragments, the workgroup's 8 waves split K and are added in wave order through LDS; no split across workgroups.
 *   PROPERTY (pinned by tests/test_decode_kernels_gpu.py): C[m][n] is a function of row m of A (and of residual) and row n of W
 *   alone - bit-identical for the same row at M = 1 and at M = 64, whatever the other rows hold.
 *   Containment: reads rows < M of A / residual and rows < N of W, columns < K (< N for residual); writes C[m][n] for m < M, n < N
 *   only (edge tiles re-read the last row).  No operand is rounded inside the kernel; one rounding at the bf16 store. */
int rv_gemm_nt_skinny_bf16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K,
                           const void* residual, long ldr, int out_f32, void* stream);
/* rv_attn_decode: attention of ONE query token per sequence against a cache (HF LlamaAttention with past_key_values, q_len = 1).
 *   kv: bf16 [rows][ldkv], the cache of one layer: K head g at columns k_col0 + g*hd (RoPE already applied), V head g at v_col0 + g*hd.
 *   Sequence m attends exactly the cache rows [pre_off[m], pre_off[m] + pre_len[m]) (the prompt; the samples of one prompt name the
 *   same span, so it is stored once) followed by [own_off[m], own_off[m] + own_len[m]) (its own tokens, the current one included:
 *   the caller appends it before the call).  pre_len[m] + own_len[m] >= 1 (CALLER's guarantee); either span may be empty.
 *   q: bf16 [M][ldq], out: bf16 [M][ldo], head h at column h*hd; hd = 128; kv_group in {1, 2, 4, 8} as in rv_attn_fwd (query head h
 *   reads kv head h / kv_group); lse (optional, fp32 [M][H]): natural log of sum exp(scale q.k).
 *   One workgroup per (sequence, kv head, key split) serves the kv_group query heads of its kv head from one read of K / V (global
 *   memory straight to registers); split s takes keys [s c, (s + 1) c), c = ceil((pre_len + own_len) / n_split), and writes
 *   (m, l, partial O) to workspace; a second launch adds the n_split partials in split order - a split without keys has weight 0.
 *   Deterministic for a given n_split; the result of a sequence does not depend on the other sequences of the call.
 *   workspace: fp32, rv_attn_decode_workspace_floats(M, H, n_split) elements (0 for bad arguments), needs no initialisation.
 *   Containment: of kv only the two spans' rows at the K / V head columns are read; q / out rows < M at the head columns.
 *   ROUNDING: none inside - softmax and P V run in fp32 on the vector units (p is NOT rounded to bf16); out is rounded once. */
long rv_attn_decode_workspace_floats(int M, int H, int n_split);
int rv_attn_decode(const void* q, long ldq, const void* kv, long ldkv, int k_col0, int v_col0, const int* pre_off,
                   const int* pre_len, const int* own_off, const int* own_len, void* out, long ldo, float* lse, int M, int H, int hd,
                   int kv_group, float scale, int n_split, float* workspace, long workspace_floats, void* stream);
/* rv_sample_token: one token per row from fp32 logits [M][ldl] over the columns [0, V_valid), V_valid <= 65536 (HF's processor order:
 * RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopPLogitsWarper, softmax, multinomial):
 *   1. repetition penalty over seen_ids[seen_off[m] .. seen_off[m+1]) as in rv_next_token_scores (ids outside [0, V_valid) are
 *      skipped; penalty == 1 or seen_off == NULL: off);   2. l / temperature;
 *   3. top_p < 1: a token of probability v is dropped iff the probability mass of all tokens <= v is <= 1 - top_p (what the
 *      warper's ascending sort + cumsum decides, found here by bisection over v with the row in registers); the top token always
 *      stays; equal probabilities at the edge stay or go TOGETHER (HF's sort splits them arbitrarily); top_p >= 1 keeps all;
 *   4. softmax over the kept set;   5. inverse CDF in vocabulary-index order: the first kept id whose running sum exceeds
 *      u[m] * total, u[m] in [0, 1) supplied by the caller (a seeded torch.Generator on the host: reproducible, and tests plant u).
 *   temperature == 0: greedy - the LOWEST index among equal maxima (rv_next_token_scores' argmax), u may be NULL, top_p is ignored
 *   and logp is the log-softmax of the penalised logits at that token.
 *   token int32 [M]; logp fp32 [M] = log-probability of the token under the final (kept, renormalised) distribution.
 *   The DISTRIBUTION is HF's for the processors named above - no top-k: the reference's sampling calls run behind transformers
 *   4.35's default top_k = 50, which is rv_sample_token_topk below - and the map from random numbers to tokens is this kernel's
 *   own - torch.multinomial's stream cannot be reproduced.  One workgroup per row, fixed reduction order; logits are read only, inside [0, V_valid) of rows < M. */
int rv_sample_token(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids, float penalty,
                    float temperature, float top_p, const float* u, int* token, float* logp, void* stream);
/* rv_sample_token_wide (csrc/sample_wide.hip; additive, ABI stays 7): rv_sample_token for 1 <= V_valid <= 262144 (Llama-3: 128256
 *   ids) - the same steps 1 - 5, greedy rule, token / logp and argument order, followed by a workspace.  The row is not held in
 *   registers but streamed (it is L2 / MALL-resident behind the LM head): one workgroup of 16 waves per row, wave w owns the ids
 *   [w SEG, (w + 1) SEG), SEG = ceil(V_valid / 16) rounded up to a multiple of 256, in tiles of 256 (lane l: ids 4 l .. 4 l + 3), so
 *   vocabulary order is (wave, tile, lane, element).  Passes over the row: max / arg-max, Z, and when sampling with top_p < 1 ONE
 *   pass that writes out, in vocabulary order, the tokens of probability > (1 - top_p) / (2 V_valid) - the others are dropped at
 *   any threshold, their mass is summed - then step 3's bisection over that list, the kept mass, and the draw.  A wave's first 512
 *   candidates stay in LDS, further ones go to its SEG floats of the workspace.
 *   DETERMINISTIC: every sum is lane-accumulate over the tiles, wave butterfly, 16 wave results in wave order; no floating-point
 *   atomic; the running sum of the draw is in vocabulary order.  A row's token and logp are a function of that row, u[m] and its
 *   seen ids alone (not of M).  The sums run in another order than rv_sample_token's, so at V_valid <= 65536 the two agree in
 *   distribution and in every draw farther than the fp32 summation error from a CDF boundary, not bit for bit in logp.
 *   CONTAINED: reads [0, V_valid) of rows < M only, for any ldl >= V_valid and any 4-byte-aligned row start (16-byte loads only
 *   when logits is 16-byte aligned and ldl % 4 == 0); writes token, logp and the workspace only.
 *   workspace: fp32, rv_sample_token_wide_workspace_floats(M, V_valid) = M * 16 * SEG elements (0 for bad arguments), needs no
 *   initialisation, holds nothing between calls. */
long rv_sample_token_wide_workspace_floats(int M, int V_valid);
int rv_sample_token_wide(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids, float penalty,
                         float temperature, float top_p, const float* u, int* token, float* logp, float* workspace,
                         long workspace_floats, void* stream);
/* rv_sample_token_topk / rv_sample_token_wide_topk (additive, ABI stays 7): rv_sample_token / rv_sample_token_wide with HF's
 *   TopKLogitsWarper in its place of the processor order (RepetitionPenalty, Temperature, TopK, TopP, softmax, multinomial) - the
 *   same argument lists with `int top_k` behind top_p, and a new step between 2 and 3:
 *   2b. let s_i be the fp32 score of step 2 and tau_k the largest value with #{i : s_i >= tau_k} >= top_k.  Tokens with
 *      s_i < tau_k are dropped; EVERY token tied with tau_k stays, as in HF (the warper removes scores < the k-th largest), so more
 *      than top_k tokens may survive; the comparison is by float value (-0.0 and +0.0 tie).  Z, step 3's threshold (1 - top_p) Z,
 *      the kept mass, the draw and logp are then taken over the survivors, with the reductions of the base entry in the same
 *      fixed order.  top_k == 0 or top_k >= V_valid: off.  top_k < 0 is refused.  Greedy (temperature == 0) ignores top_k as it
 *      ignores top_p.
 *   tau_k is selected on an order-preserving INTEGER key of s_i, never on exp(s_i - max): distinct scores can share a probability
 *   (or 0), which would keep more than HF does.  rv_sample_token_topk: the row is in registers, the key is built bit by bit from
 *   the top with 32 block-wide integer counts.  rv_sample_token_wide_topk: a radix select of 11 + 11 + 10 key bits, each a
 *   2048-bin histogram in LDS filled with integer atomics (the first during the max pass, two more passes over the row); the
 *   candidate list of step 3 then holds survivors only (at most top_k + ties; a wave's first 512 in LDS, further ones in its
 *   part of the workspace).  No floating-point atomic anywhere.
 *   With top-k off (0, >= V_valid, or greedy) both run the base entry's kernel: token and logp are the SAME BITS as
 *   rv_sample_token / rv_sample_token_wide give.  The base entries' clauses hold unchanged: DETERMINISTIC (fixed reduction order;
 *   the integer counts do not depend on the order of the atomics), a row's token and logp are a function of that row, u[m] and
 *   its seen ids alone (not of M), CONTAINED (reads [0, V_valid) of rows < M only, for any ldl >= V_valid and any 4-byte-aligned
 *   row start; writes token, logp and - the wide entry - the workspace only), and the wide entry's workspace is
 *   rv_sample_token_wide_workspace_floats(M, V_valid) floats, uninitialised, holding nothing between calls.
 *   The DISTRIBUTION is HF's for generate(do_sample=True, top_k=k, top_p=p, temperature=T, repetition_penalty=r); what the
 *   reference's sampling calls leave unsaid comes from the checkpoint's generation_config.json and transformers 4.35's defaults
 *   (top_k = 50): rlaif_v_amd/genconfig.py. */
int rv_sample_token_topk(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids, float penalty,
                         float temperature, float top_p, int top_k, const float* u, int* token, float* logp, void* stream);
int rv_sample_token_wide_topk(const float* logits, long ldl, int M, int V_valid, const int* seen_off, const int* seen_ids,
                              float penalty, float temperature, float top_p, int top_k, const float* u, int* token, float* logp,
                              float* workspace, long workspace_floats, void* stream);

/* ---- Beam-search decoding (csrc/beam.hip, rv_attn_decode_indexed in csrc/decode.hip; additive, ABI stays 7).  Replaces the decode
 *      steps of HF GenerationMixin._beam_search behind model.generate(do_sample=False, num_beams=3) in muffin/eval/muffin_vqa.py,
 *      muffin/eval/llava15_chair.py and chat.py.
 *
 * rv_attn_decode_indexed: rv_attn_decode with the sequence's own span given as a ROW TABLE: key t of sequence m is cache row
 *   pre_off[m] + t for t < pre_len[m], else own_rows[m * ld_rows + (t - pre_len[m])] (int32).  Beams with a common ancestor name the
 *   same rows; nothing in the cache is copied or reordered when beams are reselected.  Everything else - split, online softmax,
 *   merge, combine, workspace (rv_attn_decode_workspace_floats), rounding, determinism - is rv_attn_decode's: with the identity
 *   table own_rows[m][i] = own_off[m] + i the result is the same bits.  cur_own_len: the largest own_len[m] of the call (the
 *   CALLER's statement), ld_rows >= cur_own_len is checked; inside the kernel own_len[m] is clamped to ld_rows and every table
 *   entry to [0, kv_rows), kv_rows = rows of the cache: a bad table reads wrong rows, never memory outside the cache or the table.
 *   The table entries of a batch of four keys are loaded ahead of the K / V loads that depend on them. */
int rv_attn_decode_indexed(const void* q, long ldq, const void* kv, long ldkv, int kv_rows, int k_col0, int v_col0,
                           const int* pre_off, const int* pre_len, const int* own_rows, long ld_rows, int cur_own_len,
                           const int* own_len, void* out, long ldo, float* lse, int M, int H, int hd, int kv_group, float scale,
                           int n_split, float* workspace, long workspace_floats, void* stream);
/* rv_beam_topk: per group g of K beams (rows g K .. g K + K - 1 of fp32 logits [G K][ldl], columns [0, V_valid), V_valid <= 65536)
 *   the 2K best of the K V_valid values  log_softmax(row b)[v] + score[g K + b], sorted descending, as cand_val / cand_parent (b) /
 *   cand_tok (v), [G][2K] each; lse fp32 [G K] = log sum exp of each row.  log_softmax in fp32 as rv_sample_token: max, sum of
 *   exp(x - max), log; value = ((x - max) - log Z) + score, one rounding per operation.  Equal values order by the lower flat index
 *   b * V_valid + v.  Columns >= V_valid are never read.  A beam with score -1e9 (HF's start value of beams 1..K-1) gives finite
 *   values near -1e9 that lose to every live candidate.  2 K <= V_valid.  Two launches: one workgroup per row keeps the row in
 *   registers and finds its own top 2K by 2K block arg-max rounds (wave butterfly, then the 16 wave results in wave order), one
 *   wave per group merges the K lists; every reduction has a fixed order: the same bits on every run.
 *   workspace: fp32, rv_beam_topk_workspace_floats(G, K) elements (0 for bad arguments), needs no initialisation.  1 <= K <= 8. */
long rv_beam_topk_workspace_floats(int G, int K);
int rv_beam_topk(const float* logits, long ldl, const float* score, int G, int K, int V_valid, float* cand_val, int* cand_parent,
                 int* cand_tok, float* lse, float* workspace, long workspace_floats, void* stream);
/* rv_beam_topk_penalty: rv_beam_topk with HF's RepetitionPenaltyLogitsProcessor where beam search runs its logits processors:
 *   between the log-softmax and the score add (omnilmm/omnilmm_gen_data.py:306-314: num_beams with repetition_penalty=1.1).
 *   Per row m = g K + b:  lp[v] = (x[v] - max) - log Z  in fp32 exactly as rv_beam_topk; every DISTINCT id v among
 *   hist[m * ld_h + 0 .. n_hist) (int32) with 0 <= v < V_valid is penalised ONCE:  lp[v] = lp[v] < 0 ? lp[v] * penalty :
 *   lp[v] / penalty  (HF gathers and scatters: a duplicate id is not penalised twice); ids outside [0, V_valid), -1 included, are
 *   ignored; then value = lp[v] + score[m] - one multiply, one add, one rounding each, never fused.  (lp <= +0 always - the row's
 *   maximum gives x - max = 0 and Z >= 1 - so the division is met by lp = +0 alone, where quotient and product are the same +0:
 *   the kernel multiplies.)  Then rv_beam_topk's selection and merge: the same order of equal values, V_valid <= 65536,
 *   1 <= K <= 8, the dead-beam score -1e9, the same workspace (rv_beam_topk_workspace_floats(G, K)), the same determinism.
 *   READ: logits columns [0, V_valid) of rows [0, G K); score [G K]; hist entries [0, n_hist) of rows [0, G K) at row stride ld_h
 *   - entries at column >= n_hist are never read, and hist is not read at all when penalty == 1 or n_hist == 0.
 *   WRITTEN: cand_val / cand_parent / cand_tok [G][2K], lse [G K] - the UN-penalised max + log Z - and the workspace.
 *   hist is the token-history table rv_beam_step writes: at step j row m holds the j tokens of running beam m, so a beam search
 *   passes n_hist = j, ld_h = the table's row length.  The ids of a row become a bit set of ceil(V_valid / 32) words in LDS
 *   (8 KB at 65536 ids), read when the register row is transformed.  With penalty == 1, n_hist == 0 or hist == NULL the plain
 *   kernel is launched: rv_beam_topk's bits on every output.
 *   rc 1: everything rv_beam_topk refuses; penalty <= 0; n_hist < 0 or n_hist > ld_h; hist == NULL with n_hist > 0 and
 *   penalty != 1; hist not 4-byte aligned; G K ld_h beyond int32. */
int rv_beam_topk_penalty(const float* logits, long ldl, const float* score, int G, int K, int V_valid, const int* hist, long ld_h,
                         int n_hist, float penalty, float* cand_val, int* cand_parent, int* cand_tok, float* lse, float* workspace,
                         long workspace_floats, void* stream);
/* rv_beam_step: step j (0-based, of at most T) of GenerationMixin._beam_search (transformers 5.x, do_sample=False,
 *   early_stopping=False, one EOS id, generation from inputs_embeds: the prompt length counts 0) on the 2K candidates of every
 *   group, one wave per group.  A candidate "stops" when its token is eos_token_id (-1: none) or when `last` = (j == T - 1).
 *   - running beams: the K best candidates that do not stop, in order -> run_score / parent / token [G K]; slots left over (every
 *     candidate stops) take the stopping candidates in order at value + (-1e9);
 *   - stopping candidates of rank < K join the group's finished set with score value / len_div, len_div = (j + 1) ** length_penalty
 *     (host-computed); the set keeps the K best (an equal score does not evict); slot s: hyp_tokens [G][K][T] (its j + 1 tokens),
 *     hyp_len, hyp_score [G K]; n_hyp [G] = slots in use (slots are NOT sorted);
 *   - done[g] = every candidate stops, or the set is full and run_score[g K] / len_div <= its worst score (with a free slot the
 *     worst counts -1e9).  A group with done[g] != 0 on entry keeps selecting and advancing but its finished set is frozen;
 *   - tables, buffer A -> buffer B (the caller swaps): row m = g K + b of hist_b / rows_b = row g K + parent[m] of hist_a / rows_a
 *     (entries < j) with entry j appended: token[m], and own_base + j * (G K) + m - the cache row the caller writes this token's
 *     K | V to (step-major).  A and B must not overlap (an in-place gather is a race between beams).  ld_t >= T = the row length.
 *   force_parent / force_token / force_score (int32, int32, fp32 [G K]; all or none, test hook): the running beams are these
 *   instead of the selection (parents clamped to [0, K)), the finished set and done are left alone.
 *   n_hyp and done must be zeroed before step 0.  Everything else is written before it is read. */
int rv_beam_step(const float* cand_val, const int* cand_parent, const int* cand_tok, int G, int K, int T, int j, int eos_token_id,
                 float len_div, int last, int own_base, const int* force_parent, const int* force_token, const float* force_score,
                 float* run_score, int* parent, int* token, const int* hist_a, int* hist_b, const int* rows_a, int* rows_b, long ld_t,
                 int* hyp_tokens, int* hyp_len, float* hyp_score, int* n_hyp, int* done, void* stream);

/* ---- Continuous batching of candidate generation (csrc/decode_state.hip; additive, ABI stays 7).  Replaces nothing in the
 *      reference, whose generate() decodes a fixed batch until its longest answer ends; it replaces the per-step torch
 *      bookkeeping of LlavaDPOModel.generate (tokens[:, j] = tok, seen_ids[:, j] = tok, done |= ..., rows.step(j)), which
 *      assumes every row is at step j, by scatters that let every row - "slot" - be at a step of its own, so that a finished
 *      slot can be given to the next waiting prompt (LlavaDPOModel.generate_continuous, rlaif_v_amd/schedule.py).
 *
 * Per-slot state, int32 [S] each: len (tokens recorded so far), budget (1 <= budget <= T: the most tokens the slot's sequence
 *   may have), done (0 = live; a slot that was never admitted must hold done != 0), pre_off / pre_len (the cache rows of its
 *   prompt), own_off (first cache row of the slot's own region of >= T rows; constant).  Tables, row s = slot s, row length
 *   ld_t >= T: out_tokens int32 (the generated ids), seen_ids int32 (the same ids for the sampler's repetition penalty, -1 = none:
 *   pass it to rv_sample_token as seen_ids with seen_off[s] = s * ld_t), u_table fp32 (the uniform of each step, read only).
 *   eos_ids: a HOST array of n_eos ids, 0 <= n_eos <= 8 (NULL when 0); it travels by value with the launch.
 *
 * rv_decode_advance: once per step, after the sampler; one thread per slot, any S >= 1.  token int32 [S] = the sampled tokens.
 *   A live slot s (done == 0; a live slot with len outside [0, budget) is marked done and records nothing): writes token[s] to
 *   out_tokens[s][len] and seen_ids[s][len], increments len, and sets done when the token is one of eos_ids or len == budget.
 *   Then, for every slot, what the next decode step and sampler call take:
 *     still live:  tok_in = token[s], pos = pre_len + len - 1 (RoPE position), dst = own_off + len - 1 (the cache row of the token's
 *                  K | V), spans (pre_off, pre_len_eff = pre_len, own_off, own_len = len) for rv_attn_decode, u_next = u_table[s][len];
 *     PARKED (done, now or before; never admitted): tok_in = 0, pos = 0, dst = own_off, pre_len_eff = 0, own_len = 1, u_next = 0.5 -
 *                  the step writes and then attends row 0 of the slot's own region: finite, satisfies rv_attn_decode's
 *                  pre_len + own_len >= 1, touches no other slot's rows, and the token sampled for it is recorded nowhere.
 * rv_decode_admit: gives the n listed slots (1 <= n <= 64 per call, each slot at most once) to new sequences.  slots,
 *   new_pre_off, new_pre_len, new_budget: HOST int32 [n] (checked here, then passed by value); token int32 [n] on the device = the
 *   first token of each, sampled from its prompt's prefill logits.  One workgroup per listed slot: sets the slot's row of
 *   seen_ids to -1 ([0, T)), len = 0, done = 0, pre_off, pre_len, budget, then performs rv_decode_advance's step for the first
 *   token.  Slots not listed are not touched.
 *
 *   CONTAINED: for slot s the kernels write column len[s] (its value on entry) of row s of out_tokens / seen_ids - rv_decode_admit
 *   also columns [0, T) of row s of seen_ids - and entry s of the [S] state and output arrays; nothing else.  Every table index
 *   is derived from values clamped in the kernel (budget to [0, T], len to [0, budget)), and an emitted dst is never outside
 *   [own_off[s], own_off[s] + budget[s]), for parked slots too.  u_table is read at [s][len] with 1 <= len < T only.
 *   REFUSED before any launch (rc 1 and an rv_last_error text that starts with the entry point's name): S < 1, T < 1, ld_t < T,
 *   S * ld_t beyond int32, n_eos outside [0, 8], a NULL or misaligned table / state / output array, and for rv_decode_admit
 *   n outside [1, 64], a NULL list, a slot index outside [0, S), a slot listed twice, a budget outside [1, T], a negative span.
 *   No waiting on the device, no communication between workgroups, plain vector stores only; the result does not depend on the
 *   order in which slots are processed. */
int rv_decode_advance(const int* token, int* len, const int* budget, int* done, const int* pre_off, const int* pre_len,
                      const int* own_off, const int* eos_ids, int n_eos, int* out_tokens, int* seen_ids, const float* u_table,
                      long ld_t, int S, int T, int* tok_in, int* pos, int* dst, int* pre_len_eff, int* own_len, float* u_next,
                      void* stream);
int rv_decode_admit(const int* slots, const int* new_pre_off, const int* new_pre_len, const int* new_budget, int n,
                    const int* token, int* len, int* budget, int* done, int* pre_off, int* pre_len, const int* own_off,
                    const int* eos_ids, int n_eos, int* out_tokens, int* seen_ids, const float* u_table, long ld_t, int S, int T,
                    int* tok_in, int* pos, int* dst, int* pre_len_eff, int* own_len, float* u_next, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RLAIFV_HIP_H */
