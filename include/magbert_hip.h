/* magbert_hip.h -- C ABI of libmagbert_hip.so: the MI355X (gfx950) MAG-BERT training hot path.
 *
 * Drop-in boundary.  The reference (WasifurRahman/BERT_multimodal_transformer) is pure Python: its "FFI" for this
 * path is torch.nn.Module.forward / autograd / optimizer.step.  This library is what sits under those surfaces
 * (INTEGRATION.md shows the ctypes binding a maintainer adds to bert.py / modeling.py / multimodal_driver.py).
 * Every entry point is extern "C", takes plain device pointers + sizes and a hipStream_t (as void*), allocates
 * nothing on the device, never synchronises, and returns 0 on success or a non-zero code (mb_error_string()).
 * Device memory, streams and torch.distributed stay with the caller (PyTorch-ROCm is plumbing only).
 *
 * dtype: 0 = fp32 "parity mode" (exact-fp32 MFMA, logits within 1e-3 of the CPU reference),
 *        1 = bf16 "perf mode" (bf16 activations / MFMA operands, fp32 accumulate, fp32 master weights).
 * All row-major.  T = B*L tokens, H = the hidden size (256 | 512 | 768 | 1024 for the row operators, MAG and both engines), heads
 * of 64.  Reference citations are relative to /root/reference.
 */
#ifndef MAGBERT_HIP_H
#define MAGBERT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MB_DT_F32 0
#define MB_DT_BF16 1

/* dropout site key: mask(idx) = hash32(idx, k0, k1) < thresh ? drop : keep*scale.  thresh = 0 disables. */
typedef struct { uint32_t k0, k1, thresh; float scale; } mb_dropkey;

const char* mb_error_string(int code);
int mb_version(void);
/* fills the key for (seed, step, site) and probability p; p = 0 -> disabled */
void mb_make_dropkey(uint64_t seed, uint64_t step, uint32_t site, float p, mb_dropkey* out);

/* ------------------------------------------------------------------------------------------------ operators */

/* C[M,N] = sum_k A(m,k) B(n,k) with fused epilogue.  Replaces torch.nn.Linear forward/backward (addmm / mm)
 * under BertSelfAttention / BertSelfOutput / BertIntermediate / BertOutput (transformers 3.0.2, reached from
 * bert.py:221-229) and MAG's Linears (modeling.py:15-19).
 * layout 0 (NT): A[M][K], B[N][K]          forward  Y = X W^T
 * layout 1 (NN): A[M][K], B[K][N]          dgrad    dX = dY W
 * layout 2 (TN): A[K][M], B[K][N]          wgrad    dW += dY^T X   (fp32 accumulate, split-K)
 * epilogue: 0 C=alpha*acc+bias | 1 u=acc+bias: C=gelu'(u), C2=gelu(u) | 2 C=dropout(acc+bias)+R | 3 C=acc+R | 4 C=acc*R (R = the gelu'(u) saved by 1)
 *           5 Cf+=acc (fp32) | 6 Cf=alpha*acc+bias (fp32)
 *           7 relu | 8 swish (silu) | 9 gelu_new (tanh form) | 10 mish: epilogue 1 with that activation in the place of erf-GELU --
 *           C = act'(u), C2 = act(u) [* dropout]; layout 0 only (any other layout: MB_ERR_MODE).  What epilogue 4 reads as R is the
 *           derivative plane C of epilogue 1 or of 7 .. 10, whichever the forward ran.
 * With epilogue 4, Cf (fp32 [N], may be NULL) receives += the column sums of C: the bias gradient of the Linear in front.
 * tile: 0 = chosen by shape (what the engines pass) | 64 | 128 | 12864 (128 x 64, four waves) | 256 (256 x 128 eight-wave ping-pong, bf16)
 *       | 12872 (128 x 64 eight-wave ping-pong, bf16: the choice for N = 768 at one tile per CU) | 25672 (256 x 64, the same at T = 4096);
 *       a tile that cannot take the problem
 *       (dtype, epilogue, k range) falls back to the next smaller one.  splits > 1: split-K (layout 2 only). */
enum { MB_EPI_RELU = 7, MB_EPI_SWISH = 8, MB_EPI_GELU_NEW = 9, MB_EPI_MISH = 10 };
/* feed-forward activation of an engine (mb_bert_config.hidden_act, mb_xlnet_config.ff_activation): transformers' ACT2FN names */
enum { MB_ACT_GELU = 0, MB_ACT_RELU = 1, MB_ACT_SWISH = 2, MB_ACT_GELU_NEW = 3, MB_ACT_MISH = 4 };
int mb_gemm(int dtype, int layout, int epilogue, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
            void* C, int ldc, void* C2, float* Cf, const float* bias, const void* R, int ldr, float alpha,
            const mb_dropkey* drop, int splits, int tile, void* stream);

/* Measurement hook (tools/gemm_bench --trace; not used by the product path): with MB_GEMM_TRACE=1 in the environment every
 * block of an mb_gemm launch stamps the 100 MHz wall clock at 0 entry, 1 first operand stage landed, 2 k loop done,
 * 3 epilogue issued, 4 its stores completed.  Copies the [blocks][8] stamps of the LAST launch to host_out (blocks that
 * exited without a tile stay 0) and returns the block count (0 when tracing is off). */
int mb_debug_gemm_trace(unsigned long long* host_out, int max_blocks);
/* same for mb_attention_backward with MB_ATTN_TRACE=1: 0 entry, 1 operands staged, 2 query sweep done, 3 dQ bias flushed,
 * 4 key sweep done, 5 exit */
int mb_debug_attention_trace(unsigned long long* host_out, int max_blocks);

/* TEST HOOKS (tests/test_gemm_edges_gpu.py; no engine code calls them, no product path changes): they only fill the launchers'
 * argument structures with what mb_gemm / mb_gemm_grouped_wgrad cannot set and call the same launchers the engines call.
 *
 * mb_debug_gemm_ex = mb_gemm plus
 *   bseg, bseg_stride  segmented B: B's contiguous dimension is cut into pieces of bseg elements, bseg_stride elements apart (0 = off)
 *   cvalid, overwrite  epilogue 5: store only columns [0, cvalid) dword-wise (0 = all) ; Cf = acc instead of Cf += acc
 *   colsum_shadow      epilogue 4, may be NULL: [N] 64-bit deterministic-mode accumulator parallel to Cf; the column sums go there as
 *                      2^44-scaled integers, and with fold != 0 the engines' fold adds them into Cf and clears the shadow
 *   rp .. zero_grad    an AdamW rider inside the launch (blocks = 0: none): blocks workgroups update 4 * n4 weight-decayed parameters
 *                      (shadow: bf16 copy of the whole range or NULL); lr .. grad_scale as mb_adamw_step, turned into the step's scalars
 *                      by the same host code and written to adam_dev (device memory, 28 bytes) for the rider to read.  layout 1, tile 0.
 *   ride_tiles         may be NULL: the padded tile count of the rider-carrying launch (0 = that launch carries none: MB_ERR_MODE)
 * mb_debug_gemm_grouped_ex = mb_gemm_grouped_wgrad (count <= 8) plus per-problem cvalid / overwrite (arrays or NULL), the ring depth of the
 *   64 x 64 group (stages 0 | 4 | 5) and a rider as above (128 x 128 and ping-pong tiles only).
 * mb_debug_gemm_last_kernel: the (mangled) symbol of the kernel this process's last GEMM launch used -> its length, 0 = none yet. */
int mb_debug_gemm_ex(int dtype, int layout, int epilogue, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                     void* C, int ldc, void* C2, float* Cf, const float* bias, const void* R, int ldr, float alpha,
                     const mb_dropkey* drop, int splits, int tile, int bseg, size_t bseg_stride, int cvalid, int overwrite,
                     long long* colsum_shadow, int fold, float* rp, float* rg, float* rm, float* rv, void* rshadow, size_t n4, int blocks,
                     int zero_grad, float lr, float beta1, float beta2, float eps, float weight_decay, int step, int correct_bias,
                     float grad_scale, void* adam_dev, int* ride_tiles, void* stream);
int mb_debug_gemm_grouped_ex(int dtype, int count, const int* M, const int* N, int K, const void* const* dY, const int* ldy,
                             const void* const* X, const int* ldx, float* const* dW, const int* ldw, const int* cvalid,
                             const int* overwrite, int tile, int stages, float* rp, float* rg, float* rm, float* rv, void* rshadow,
                             size_t n4, int blocks, int zero_grad, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int step, int correct_bias, float grad_scale, void* adam_dev, void* stream);
int mb_debug_gemm_last_kernel(char* out, int cap);
/* mb_debug_gemm_grouped_rows: mb_gemm_grouped_wgrad with a gathered k loop (bf16, tile 256 only; else MB_ERR_MODE): problem g sums over the
 *   rows rows[g][0 .. n) of dY_g and X_g in list order, n = min(K, *nrows[g]) -- a multiple of 64, at least 192; rows[g] (device, 32-byte
 *   aligned uint32) holds at least that many entries < K.  rows[g] == NULL: all K rows.  overwrite as mb_debug_gemm_grouped_ex.
 * mb_debug_live_rows: the step prologue's lists of a [B][L] int64 mask (device): live_rows (max(192, Tp) uint32) and *live_count; cls_rows /
 *   cls_count (both or neither; may be NULL): the [CLS]-row list, same capacity. */
int mb_debug_gemm_grouped_rows(int dtype, int count, const int* M, const int* N, int K, const void* const* dY, const int* ldy,
                               const void* const* X, const int* ldx, float* const* dW, const int* ldw, const int* overwrite, int tile,
                               const void* const* rows, const void* const* nrows, void* stream);
int mb_debug_live_rows(const int64_t* mask, int B, int L, int Tp, void* live_rows, void* live_count, void* cls_rows, void* cls_count,
                       void* stream);
/* mb_debug_adamw_sweep: the end-of-step sweep of mb_bert_train_step over a caller-built table: piece k = quads [begin4[k], begin4[k] + len4[k])
 *   of the flat buffers with the scalars cls[slot[k]] (cls: device, 7 floats per slot: lr, beta1, beta2, eps, weight_decay, step_size,
 *   grad_scale); shadow / keep ranges and the word range [word_begin, word_end) in elements (multiples of 4), rows of row_len elements.
 *   stamp (device uint32 per row; top bit = the row's seen mark, the rest the number of the update that touched it) and state (device, three
 *   uint32: this update's number, the gradient verdict, the moment verdict); stamp == NULL: a plain sweep.  Nothing is checked against
 *   the buffers' sizes.
 * mb_debug_word_moments_scan: sets or clears the seen mark of stamp[row], row < rows, from m and v[begin + row * row_len ...); rows whose
 *   number is keep_no are left alone. */
int mb_debug_adamw_sweep(float* p, float* g, float* m, float* v, void* shadow, int npieces, const uint32_t* begin4, const uint32_t* len4,
                         const uint8_t* slot, size_t sh_begin, size_t sh_end, size_t keep_begin, size_t keep_end, const void* cls,
                         const void* stamp, const void* state, size_t word_begin, size_t word_end, uint32_t row_len, void* stream);
int mb_debug_word_moments_scan(const float* m, const float* v, void* stamp, size_t begin, size_t rows, uint32_t row_len, uint32_t keep_no,
                               void* stream);

/* `count` (<= 4) weight gradients dW_g[M_g][N_g] += dY_g[K][M_g]^T X_g[K][N_g] in ONE launch (fp32 accumulate) -- the
 * four torch.nn.Linear weight gradients autograd produces per BertLayer (mm_backward under loss.backward(),
 * multimodal_driver.py:378).  Every M_g, N_g must be a multiple of `tile` (64 | 128 | 256 = the 256 x 128 ping-pong tile, bf16: M_g % 256, N_g % 128) and K a
 * multiple of 128 bytes. */
int mb_gemm_grouped_wgrad(int dtype, int count, const int* M, const int* N, int K, const void* const* dY, const int* ldy,
                          const void* const* X, const int* ldx, float* const* dW, const int* ldw, int tile, void* stream);

/* dst[i] = (dtype) src[i] and back, n % 4 == 0 -- the gradient wire format of the data-parallel exchange in bf16 perf mode
 * (distributed.GradReducer: fp32 flat gradients -> bf16 staging -> RCCL all-reduce -> fp32).  New relative to the reference. */
int mb_narrow(int dtype, const float* src, void* dst, size_t n, void* stream);
int mb_widen(int dtype, const void* src, float* dst, size_t n, void* stream);

/* LayerNorm (+ dropout on the output) forward / backward -- torch.nn.LayerNorm under BertSelfOutput/BertOutput. */
int mb_layernorm_forward(int dtype, const void* x, const float* gamma, const float* beta, float eps, void* y,
                         float* mean, float* rstd, int rows, int H, const mb_dropkey* drop, void* stream);
int mb_layernorm_backward(int dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                          const float* rstd, void* dx, void* dx_drop, float* dgamma, float* dbeta, float* dbias,
                          int rows, int H, const mb_dropkey* drop_out, const mb_dropkey* drop_in, void* stream);

/* BertEmbeddings (bert.py:81,211-216): LN(word[ids] + pos[0..L) + type[seg]) -> dropout. ids/seg int64 [B][L]. */
int mb_embed_forward(int dtype, const int64_t* ids, const int64_t* seg, const float* word, const float* pos,
                     const float* type, const float* gamma, const float* beta, float eps, void* out, float* mean,
                     float* rstd, int B, int L, int H, const mb_dropkey* drop, void* stream);
int mb_embed_backward(int dtype, const void* dout, const int64_t* ids, const int64_t* seg, const float* word,
                      const float* pos, const float* type, const float* gamma, const float* mean, const float* rstd,
                      float* dsum_ws, float* dword, float* dpos, float* dtype_, float* dgamma, float* dbeta, int B, int L,
                      int H, int pad_id, const mb_dropkey* drop, void* stream);

/* BertSelfAttention core (bert.py:221-229): ctx = dropout(softmax(QK^T/8 + (1-mask)*-1e4)) V.
 * qkv [T][3H] token-major, mask int64 [B][L], ctx/dctx [T][H], dqkv [T][3H].  L <= 128 (MB_ERR_SHAPE above), head dim 64. */
int mb_attention_forward(int dtype, const void* qkv, const int64_t* mask, void* ctx, int B, int L, int nh,
                         const mb_dropkey* drop, void* stream);
int mb_attention_backward(int dtype, const void* qkv, const int64_t* mask, const void* dctx, void* dqkv, int B, int L,
                          int nh, const mb_dropkey* drop, void* stream);
/* The same LDS-resident kernels with every output they have, as the engines call them.  head_scale fp32 [nh] or NULL (head_mask);
 * probs fp32 [B][nh][L][L] or NULL: the probabilities after dropout, times head_scale (output_attentions); dbias fp32 [3H] or NULL:
 * += the column sums of dqkv (the fused QKV bias gradient).  Arguments are checked as by the tiled pair below, except that L > 128
 * is MB_ERR_SHAPE. */
int mb_attention_resident_forward(int dtype, const void* qkv, const int64_t* mask, void* ctx, int B, int L, int nh,
                                  const mb_dropkey* drop, const float* head_scale, float* probs, void* stream);
int mb_attention_resident_backward(int dtype, const void* qkv, const int64_t* mask, const void* dctx, void* dqkv, float* dbias, int B,
                                   int L, int nh, const mb_dropkey* drop, const float* head_scale, void* stream);
/* The tiled kernels the engines run for 128 < L <= 512, usable at any 1 <= L <= 512 (same arithmetic; 64-row blocks streamed through
 * LDS instead of a whole sequence per head).  stats: caller scratch of mb_attention_tiled_stats_bytes(B, L, nh) -- the forward leaves
 * the row statistics of the backward in it (the backward also uses it as scratch).  head_scale fp32 [nh] or NULL (head_mask);
 * probs fp32 [B][nh][L][L] or NULL: the probabilities after dropout, times head_scale (output_attentions).  The backward also
 * needs the forward's ctx; dbias fp32 [3H] or NULL: += the column sums of dqkv.  MB_ERR_SHAPE when dropout is on and
 * B*nh*L*L >= 2^32 (the mask index is 32-bit). */
size_t mb_attention_tiled_stats_bytes(int B, int L, int nh);
int mb_attention_tiled_forward(int dtype, const void* qkv, const int64_t* mask, void* ctx, float* stats, int B, int L, int nh,
                               const mb_dropkey* drop, const float* head_scale, float* probs, void* stream);
int mb_attention_tiled_backward(int dtype, const void* qkv, const int64_t* mask, const void* ctx, const void* dctx, float* stats,
                                void* dqkv, float* dbias, int B, int L, int nh, const mb_dropkey* drop, const float* head_scale,
                                void* stream);

/* The classification head with its fused objective (bert.py:304-322), as the engines launch it: one wave per sample.
 *   pooled = tanh(z) [B][H] fp32; logits = dropout(pooled) Wc^T + bc [B][num_labels] fp32; H = 256 | 512 | 768 | 1024.
 * The objective is a triple: loss_kind (MB_LOSS_*), loss_param (smooth_l1's beta, else ignored) and loss_vec, a DEVICE vector of
 * num_labels floats or NULL (bce: pos_weight; cross_entropy: class weights; ignored by the other kinds).  Mean reduction throughout:
 *   MB_LOSS_DEFAULT        labels [B]: MSE when num_labels == 1, else cross entropy on class indices held as floats
 *   MB_LOSS_MSE | L1 | SMOOTH_L1 | BCE   labels [B][num_labels]; the mean runs over B * num_labels (bce targets lie in [0, 1])
 *   MB_LOSS_CROSS_ENTROPY  labels [B] class indices, num_labels >= 2; with weights sum_b w[y_b] nll_b / sum_b w[y_b]
 * (torch.nn.functional's mse_loss, l1_loss, smooth_l1_loss(beta), binary_cross_entropy_with_logits(pos_weight), cross_entropy(weight)).
 * An unknown kind, or cross_entropy at num_labels == 1: MB_ERR_ARG.
 * forward: labels NULL = no loss.  loss[0] += this batch's loss (the caller clears it), loss_run[0] += it too; either may be NULL.
 * backward: the logit gradient is dlogits [B][num_labels] when given, else that of the objective (logits and labels required) times
 * loss_scale.  dz [B][H] in `dtype` = the gradient of z; dWc [num_labels][H], dbc [num_labels], dbp [H] (+= column sums of dz), each
 * fp32, accumulated, may be NULL; zero_p[0, zero_bytes) (16-byte multiples, may be NULL) is cleared by extra blocks of the launch. */
enum { MB_LOSS_DEFAULT = 0, MB_LOSS_MSE = 1, MB_LOSS_L1 = 2, MB_LOSS_SMOOTH_L1 = 3, MB_LOSS_BCE = 4, MB_LOSS_CROSS_ENTROPY = 5 };
int mb_head_forward(const float* z, const float* Wc, const float* bc, const float* labels, float* pooled, float* logits, float* loss,
                    float* loss_run, int B, int H, int num_labels, const mb_dropkey* drop, int loss_kind, float loss_param,
                    const float* loss_vec, void* stream);
int mb_head_backward(int dtype, const float* dlogits, const float* logits, const float* labels, float loss_scale, const float* pooled,
                     const float* Wc, void* dz, float* dWc, float* dbc, float* dbp, void* zero_p, size_t zero_bytes, int B, int H,
                     int num_labels, const mb_dropkey* drop, int loss_kind, float loss_param, const float* loss_vec, void* stream);
/* The objective with its options: the triple above plus label smoothing, a focal exponent and an ignored label.  All options zero =
 * the triple alone, and the `_ex` entries then launch exactly what the entries above launch.
 *   cross_entropy, q = softmax(x_b), kept = (y_b != ignore_index), W = sum over kept b of w[y_b] (w = 1 without weights: the count):
 *     label_smoothing e in [0, 1):  [ (1-e) sum_kept w[y_b] (-log q_by) + (e/C) sum_kept sum_k w_k (-log q_bk) ] / W
 *     focal_gamma g, 0 or finite and >= 1, not together with smoothing:  sum_kept w[y_b] (1 - q_by)^g (-log q_by) / W
 *     has_ignore_index != 0: a label equal to ignore_index is left out of the loss, of W and of every gradient, even where it names
 *     a class; the dz row of its sample is written as zeros
 *     (torch.nn.functional.cross_entropy(weight, ignore_index, label_smoothing), with ONE deliberate departure: at W == 0 -- every
 *     sample ignored, or every kept sample in a class of weight 0 -- the loss and all gradients are 0 where torch returns NaN, so
 *     that no NaN reaches the AdamW moments)
 *   bce: focal_gamma as above: mean of (1 - p_t)^g l, l = the bce term with its pos_weight, 1 - p_t = y sigmoid(-x) + (1-y) sigmoid(x)
 * MB_ERR_ARG: e outside [0, 1), g not in {0} or [1, inf), both above 0, smoothing or an ignore_index on a kind other than
 * cross_entropy, g on a kind other than cross_entropy or bce, a NULL struct.  Not built: 0 < g < 1, an alpha other than the weights,
 * ignore_index for bce or the default kind, per-sample weights, reductions other than mean, a normaliser across data-parallel ranks
 * (each rank normalises its own batch).
 * vec: a DEVICE pointer for the two operator entries, a HOST pointer (copied) for the engines' setters. */
typedef struct { int kind; float param; const float* vec; float label_smoothing; float focal_gamma; int has_ignore_index; int ignore_index; } mb_head_loss;
int mb_head_forward_ex(const float* z, const float* Wc, const float* bc, const float* labels, float* pooled, float* logits, float* loss,
                       float* loss_run, int B, int H, int num_labels, const mb_dropkey* drop, const mb_head_loss* hl, void* stream);
int mb_head_backward_ex(int dtype, const float* dlogits, const float* logits, const float* labels, float loss_scale, const float* pooled,
                        const float* Wc, void* dz, float* dWc, float* dbc, float* dbp, void* zero_p, size_t zero_bytes, int B, int H,
                        int num_labels, const mb_dropkey* drop, const mb_head_loss* hl, void* stream);

/* Multimodal Adaptation Gate, MAG.forward (modeling.py:25-51) and its adjoint, for T tokens.
 * Parameters in the REFERENCE layout: W_hv [H][V+H], W_ha [H][A+H], W_v [H][V], W_a [H][A], biases [H], LayerNorm [H].
 * text [T][H] in `dtype`; visual [T][V], acoustic [T][A] fp32 (as the DataLoader yields them).
 * ws: caller scratch of mb_mag_workspace_bytes(); it also carries the activations saved for the backward. */
size_t mb_mag_workspace_bytes(int dtype, int T, int H, int V, int A);
int mb_mag_forward(int dtype, const void* text, const float* visual, const float* acoustic, const float* W_hv,
                   const float* b_hv, const float* W_ha, const float* b_ha, const float* W_v, const float* b_v,
                   const float* W_a, const float* b_a, const float* ln_w, const float* ln_b, float beta_shift,
                   const mb_dropkey* drop, void* out, void* ws, int T, int H, int V, int A, void* stream);
/* grads are ACCUMULATED (+=) into dW_*, db_*, dln_*; d_text [T][H] (dtype) is written; d_visual / d_acoustic
 * (fp32 [T][V] / [T][A], may be NULL) are written. */
int mb_mag_backward(int dtype, const void* d_out, const void* text, const float* W_hv, const float* b_hv,
                    const float* W_ha, const float* b_ha, const float* W_v, const float* b_v, const float* W_a,
                    const float* b_a, const float* ln_w, float beta_shift, const mb_dropkey* drop, void* ws,
                    void* d_text, float* d_visual, float* d_acoustic, float* dW_hv, float* db_hv, float* dW_ha,
                    float* db_ha, float* dW_v, float* db_v, float* dW_a, float* db_a, float* dln_w, float* dln_b,
                    int T, int H, int V, int A, void* stream);
/* TEST HOOKS (tests/mag_op_helpers.py; no engine code calls them): the same two implementations with the arguments only the engines set.
 * mb_debug_mag_forward_ex = mb_mag_forward plus
 *   pads_clean    the caller keeps rows [T, align_up(T, 64)) of the workspace's packed modality operands zero itself
 * mb_debug_mag_backward_ex = mb_mag_backward (without the four weights it never reads) plus
 *   text_padded   `text` has align_up(T, 64) rows (rows behind T meet zero rows of the three dZ panels)
 *   pads_clean    the caller keeps the pad rows of the packed modalities and of the three dZ panels zero itself
 *   slabs         the six column sums (db_hv, db_ha, db_v, db_a, dln_w, dln_b) go to per-block slabs in slab_scratch (device memory of
 *                 at least mb_debug_mag_slab_bytes(T, H), else MB_ERR_ARG) and one reduction launch adds them up, as in the engines
 *   dw_zero       the four weight gradients are stored, not accumulated (the caller says they hold zeros)
 *   path          may be NULL: three ints out -- 1 when the weight gradients ran as one grouped launch, 1 when that launch stored
 *                 straight into dW_hv / dW_ha / dW_v / dW_a, and its tile (64 | 128) */
int mb_debug_mag_forward_ex(int dtype, const void* text, const float* visual, const float* acoustic, const float* W_hv,
                            const float* b_hv, const float* W_ha, const float* b_ha, const float* W_v, const float* b_v,
                            const float* W_a, const float* b_a, const float* ln_w, const float* ln_b, float beta_shift,
                            const mb_dropkey* drop, void* out, void* ws, int T, int H, int V, int A, int pads_clean, void* stream);
size_t mb_debug_mag_slab_bytes(int T, int H);
int mb_debug_mag_backward_ex(int dtype, const void* d_out, const void* text, const float* b_hv, const float* b_ha, const float* b_v,
                             const float* b_a, const float* ln_w, float beta_shift, const mb_dropkey* drop, void* ws, void* d_text,
                             float* d_visual, float* d_acoustic, float* dW_hv, float* db_hv, float* dW_ha, float* db_ha,
                             float* dW_v, float* db_v, float* dW_a, float* db_a, float* dln_w, float* dln_b, int T, int H, int V,
                             int A, int text_padded, int pads_clean, int slabs, float* slab_scratch, size_t slab_bytes, int dw_zero,
                             int* path, void* stream);

/* transformers 3.0.2 AdamW.step over flat fp32 buffers (multimodal_driver.py:345,384). [0,n_decay) decays.
 * shadow: optional bf16 copy of p written for [sh_begin, sh_end).  zero_grad != 0 clears g (optimizer.zero_grad). */
int mb_adamw_step(float* p, float* g, float* m, float* v, void* shadow, size_t n, size_t n_decay, size_t sh_begin,
                  size_t sh_end, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  int correct_bias, float grad_scale, int zero_grad, void* stream);

/* Global gradient-norm clipping over a flat fp32 range (torch.nn.utils.clip_grad_norm_, error_if_nonfinite = False), without touching
 * the gradients: out2 (device, two floats) = {norm, coef}, norm = grad_scale * sqrt(sum of g[i]^2) -- the norm of the gradient as
 * mb_adamw_step(..., grad_scale, ...) sees it -- and coef = min(1, max_norm / (norm + 1e-6)); the caller passes grad_scale * coef as
 * the grad_scale of its mb_adamw_step calls.  Every element is widened to double before it is squared and every sum is a double in
 * a fixed order (no atomics): the same bits on every run, squares that would overflow or underflow fp32 included.  g needs 4-byte
 * alignment only, any n.  scratch: caller-owned device memory of mb_grad_clip_scratch_bytes(n) bytes, 8-byte aligned; nothing is
 * assumed about its contents.  Non-finite gradients give what the arithmetic gives (a NaN element: NaN norm and coefficient). */
size_t mb_grad_clip_scratch_bytes(size_t n);
int mb_grad_clip_coef(const float* g, size_t n, float max_norm, float grad_scale, void* scratch, float* out2, void* stream);

/* ------------------------------------------------------------------------------------------------ MAG-BERT engine
 * The whole MAG_BertForSequenceClassification forward / backward (bert.py:240-324 -> :76-237 -> modeling.py) as a
 * native step executor: one call enqueues every kernel of the pass on the stream (no Python between launches).   */
typedef struct {
    /* hidden_size: 256 | 512 | 768 (bert-base) | 1024 (bert-large) with num_heads * 64 == hidden_size; num_layers >= 1;
     * intermediate_size % 128 == 0.  Anything else: mb_bert_create returns MB_ERR_SHAPE.                            */
    int vocab_size, hidden_size, num_layers, num_heads, intermediate_size, max_position, type_vocab, num_labels;
    int visual_dim, acoustic_dim, pad_token_id;
    float layer_norm_eps, mag_layer_norm_eps, beta_shift;
    float hidden_dropout, attn_dropout, mag_dropout;
    int dtype;       /* MB_DT_* */
    int max_batch, max_seq;      /* max_seq <= min(512, max_position); above 128 the attention runs the tiled kernels and the
                                    workspace holds their row statistics (engines of max_seq <= 128 carve exactly what they did) */
    int injection_index;         /* MAG is applied in front of encoder layer `injection_index`: 0 (what a zero-initialised config has always
                                    run, and the reference) = embeddings -> MAG -> layers; j >= 1 = the embeddings feed layers 0 .. j-1 and
                                    MAG(output of layer j-1, visual, acoustic) is what layer j reads.  Parameters, names, flat layout and
                                    dropout sites are the same for every value; the workspace grows by one [T_pad][H] tensor for j >= 1.
                                    Outside [0, num_layers): MB_ERR_ARG.  (Added after hidden_act, which stays the struct's last field:
                                    tests/test_activations_cpu.py pins that; set the fields by name) */
    int hidden_act;              /* MB_ACT_*: the activation of BertIntermediate (config.hidden_act); 0 = erf-GELU, what a zero-initialised
                                    config has always run.  Fixed at create time; any other value: MB_ERR_ARG */
} mb_bert_config;

typedef struct mb_bert_engine mb_bert_engine;

int mb_bert_create(const mb_bert_config* cfg, mb_bert_engine** out);
void mb_bert_destroy(mb_bert_engine* e);
/* flat parameter layout (reference state-dict names).  decay != 0 -> weight_decay group of multimodal_driver.py:329-343 */
int mb_bert_num_tensors(const mb_bert_engine* e);
int mb_bert_tensor_info(const mb_bert_engine* e, int i, char* name, int name_cap, size_t* offset, size_t* numel,
                        int* ndim, int64_t* shape4, int* decay);
size_t mb_bert_param_count(const mb_bert_engine* e);   /* padded flat length (floats) */
size_t mb_bert_decay_count(const mb_bert_engine* e);   /* elements [0, n) are the weight-decay group */
void mb_bert_shadow_range(const mb_bert_engine* e, size_t* begin, size_t* end);   /* bf16 operand shadow range */
size_t mb_bert_workspace_bytes(const mb_bert_engine* e);
/* params / grads: flat fp32 [param_count]; shadow: bf16 [param_count] (dtype bf16) or NULL; ws: workspace. */
int mb_bert_bind(mb_bert_engine* e, float* params, float* grads, void* shadow, void* workspace, size_t ws_bytes);
/* refresh operand copies from the fp32 masters (bf16 shadow + packed MAG weights); call after loading weights. */
int mb_bert_sync_weights(mb_bert_engine* e, void* stream);

/* forward.  labels optional: num_labels == 1: fp32 [B] regression targets, fused MSE; num_labels > 1: fp32 [B] holding the class
 * index of each sample, fused cross entropy (bert.py:318-320) -> loss[0] (device, overwritten), loss_run += (optional).
 * training != 0 enables dropout keyed by (seed, step).  logits: fp32 [B][num_labels] (device, written). */
int mb_bert_forward(mb_bert_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                    const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                    int training, uint64_t seed, uint64_t step, float* logits, float* loss, float* loss_run,
                    void* stream);
/* backward of the last forward.  dlogits fp32 [B][num_labels], or NULL to use the fused MSE gradient
 * 2*(logit-label)/(B*num_labels)*loss_scale.  Gradients are ACCUMULATED into the bound flat grad buffer.
 * stage_begin/stage_end select a sub-range of [0, num_layers+2): 0 = head+pooler, 1..num_layers = encoder layers
 * (last layer first), num_layers+1 = MAG + embeddings -- lets the caller interleave gradient all-reduces.
 * With injection_index = j >= 1 the MAG backward runs at the end of stage num_layers - j (behind layer j's input gradient) and
 * stage num_layers+1 is the embedding backward alone; MAG's gradients are complete when stage num_layers+1 returns, as for
 * j = 0 (mb_bert_stage_grad_ranges does not depend on j).  The input-gradient chain always runs down to the embeddings. */
int mb_bert_backward(mb_bert_engine* e, const float* dlogits, const float* labels, float loss_scale, int stage_begin,
                     int stage_end, void* stream);
/* activations for API parity (device pointers into the workspace, valid until the next forward) */
const void* mb_bert_sequence_output(const mb_bert_engine* e);   /* [B*L][H] in dtype */
const float* mb_bert_pooled_output(const mb_bert_engine* e);    /* [B][H] fp32 (pre-dropout) */
/* Optional outputs of MAG_BertModel.forward (bert.py:147-156, 227-237).
 * hidden_state(i), i in [0, num_layers]: the encoder's all_hidden_states entry i -- i = 0 is the fused embedding MAG returns,
 * i = l + 1 the output of layer l -- [B*L][H] in dtype, valid until the next forward (they are the activations saved for
 * the backward anyway).  For every injection_index entry i < num_layers is THE TENSOR LAYER i READS: with injection_index = j >= 1
 * entry 0 is the plain embedding output and entry j is MAG's output (not the output of layer j-1 that MAG read).  This differs from
 * mb_xlnet_hidden_state, whose list holds the tensor in front of the gate because its reference collects it there.  set_attention_output: the next forwards also write every layer's attention probabilities AFTER
 * dropout (what BertSelfAttention returns with output_attentions) to probs [num_layers][B][nh][L][L] fp32; NULL turns it off. */
const void* mb_bert_hidden_state(const mb_bert_engine* e, int i);
/* test hook: the operands the last backward multiplied for layer `layer`'s weight gradients: which = 0 ffn2, 1 ffn1, 2 out-proj, 3 qkv -> dY,
 * which + 4 -> X (the saved forward activation); *ld = the row pitch in elements.  The dY buffers alternate between even and odd layers:
 * only those of the two layers the backward ran last are still there. */
const void* mb_bert_debug_wgrad_dy(const mb_bert_engine* e, int layer, int which, int* ld);
/* test hook: the weight-gradient launches of the last single-call step that summed over a row list (0: all dense) */
int mb_bert_debug_live_wgrad_launches(const mb_bert_engine* e);
int mb_bert_set_attention_output(mb_bert_engine* e, float* probs);
/* Optional INPUTS of MAG_BertModel.forward (bert.py:160, 185-209).  Both are sticky until reset with NULL, apply to
 * mb_bert_forward / mb_bert_backward only (mb_bert_train_step returns MB_ERR_MODE while one is set), and point at caller-owned
 * device memory that must stay valid through the backward.
 * set_head_mask: fp32 [num_layers][num_heads]; the attention probabilities of head h in layer l are multiplied by
 *   head_mask[l][h] after dropout (BertSelfAttention; what get_head_mask broadcasts a 1-D or 2-D mask to).
 * set_inputs_embeds: fp32 [B*L][H] word embeddings used instead of the word_embeddings[input_ids] gather (input_ids may then
 *   be NULL); the word table receives no gradient, and after the backward inputs_embeds_grad returns the gradient of the
 *   given embeddings, fp32 [B*L][H] (workspace memory, valid until the next backward). */
int mb_bert_set_head_mask(mb_bert_engine* e, const float* head_mask);
/* The objective of every pass that is given labels (mb_head_forward above describes the triple): the explicit forward / backward,
 * the stage-driven passes, mb_bert_train_step and its graph, the data-parallel steps.  vec: HOST pointer to num_labels floats or NULL,
 * copied.  Sticky like head_mask, legal between steps; an engine starts with MB_LOSS_DEFAULT.  Under the per-element kinds `labels`
 * holds B * num_labels floats everywhere, mb_bert_load_batch's staging included.  Checked before any device call -- MB_ERR_ARG for an
 * unknown kind, cross_entropy at num_labels == 1, a beta that is negative or not finite, a weight that is negative or not finite, all
 * weights zero, a vector handed to a kind that takes none.  A change drops the engine's captured graphs (kind and scalar are kernel
 * arguments): the next step captures again and runs the new objective.  The workspace is not involved.
 * get: what is set; vec (num_labels floats, may be NULL) is written only when *has_vec comes back 1. */
int mb_bert_set_head_loss(mb_bert_engine* e, int kind, float param, const float* vec);
int mb_bert_get_head_loss(const mb_bert_engine* e, int* kind, float* param, float* vec, int* has_vec);
/* ... with the options of the mb_head_loss struct above (vec a HOST pointer, copied).  Sticky, legal between steps, checked before any device
 * call (an engine without a device will do); a change drops the captured step and stage graphs.  mb_bert_set_head_loss sets the triple
 * with every option cleared.  get: *hl receives what is set, its vec NULL; the vector goes to `vec` as in mb_bert_get_head_loss. */
int mb_bert_set_head_loss_ex(mb_bert_engine* e, const mb_head_loss* hl);
int mb_bert_get_head_loss_ex(const mb_bert_engine* e, mb_head_loss* hl, float* vec, int* has_vec);
int mb_bert_set_inputs_embeds(mb_bert_engine* e, const float* inputs_embeds);
/* position_ids (bert.py:211-216): int64 [B*L] device tensor of position-table rows for the next forwards / backwards, NULL =
 * BertEmbeddings' default arange(seq_len).  Sticky like head_mask; the single-call step refuses to run while it is set. */
int mb_bert_set_position_ids(mb_bert_engine* e, const int64_t* position_ids);
const float* mb_bert_inputs_embeds_grad(const mb_bert_engine* e);
/* Backward entry of the BASE model, for heads that live outside the engine: replaces stage 0 of mb_bert_backward.
 * d_sequence_output [B*L][H] (dtype; NULL = zero) is the gradient of outputs[0]; d_pooler_preact [B][H] (dtype; NULL = the
 * pooled output is unused) is the gradient of the pooler's PRE-activation, i.e. d_pooled * (1 - pooled^2) (pooled =
 * mb_bert_pooled_output).  Accumulates the pooler's weight / bias gradients; continue with mb_bert_backward(e, NULL, NULL,
 * 1.f, 1, num_layers + 2, stream). */
int mb_bert_backward_outputs(mb_bert_engine* e, const void* d_sequence_output, const void* d_pooler_preact, void* stream);
/* gradient buckets for data parallelism: range r of stage s covers flat elements [off, off+len) */
int mb_bert_stage_grad_ranges(const mb_bert_engine* e, int stage, size_t* offs, size_t* lens, int cap);

/* Known-zero gradients.  A step that runs the fused AdamW leaves the flat gradient buffer zeroed (the reference's
 * optimizer.zero_grad(), multimodal_driver.py:386); the next backward then STORES the layer weight gradients instead of adding
 * to them (no read of 28 MB per layer).  A host that zeroes the bound gradient buffer itself (model.zero_grad(), a stand-alone
 * mb_adamw_step with zero_grad) says so with known_zero = 1; anything else that writes gradients must leave / set it 0.  The
 * flag is consumed by the first stage of the next backward.  MB_WGRAD_OVERWRITE=0 disables the optimisation. */
int mb_bert_mark_grads_zero(mb_bert_engine* e, int known_zero);
/* Untouched word-embedding rows.  The sweep at the end of mb_bert_train_step does not read the gradient of a word row that no batch
 * of this update contained, when the engine can prove it is +0.0f: its own previous single-call step zeroed the table, and every
 * backward since went through a single-call step (gradient-accumulation micro-steps included).  The engine notices its own other
 * backwards and mb_bert_mark_grads_zero(e, 0); a host that writes into the bound gradient buffer by any other way between two
 * single-call steps calls this (or mb_bert_mark_grads_zero(e, 0)) before the next one, whose update then reads every gradient.
 * MB_ADAMW_SKIP_ZERO_ROWS=0 disables the skip; never needed when the host does not touch the buffer. */
int mb_bert_distrust_word_stamps(mb_bert_engine* e);
size_t mb_bert_word_skip_updates(const mb_bert_engine* e);      /* updates whose sweep was allowed to skip, since the engine was created */
/* Zero moments of never-touched word rows.  Such a row's m and v are +0.0f and stay +0.0f, and its parameters change by the decoupled
 * decay alone: under the skip above the sweep also leaves m, v and g of it unread and unwritten (8 instead of 24 bytes per parameter),
 * when the engine can prove the moments zero.  The proof is a one-off scan of the word range of the moment buffers handed to
 * mb_bert_train_step (one read, enqueued on the step's stream in front of a step that could use it); it holds while every update of
 * the word table is a single-call update with the gradient proof above, on the same m and v.  The engine notices its own other
 * updates (data-parallel, stage-driven, failed), new buffers and changed frozen marks; a host that WRITES INTO m OR v of the word
 * table by any other way (loading an optimizer state, an optimizer step of its own, mb_adamw_step over the range) calls
 * mb_bert_distrust_word_moments before the next single-call step, which then scans again.  Steps whose scalars would not leave the
 * bits alone (eps <= 0, a non-finite or negative step size, beta or gradient scale, non-finite lr * weight_decay in a slot that
 * covers the table), clipping steps and a frozen word table run the full path.  MB_ADAMW_SKIP_ZERO_MOMENTS=0 -- or
 * MB_ADAMW_SKIP_ZERO_ROWS=0 -- disables it: no scan, every moment read and written. */
int mb_bert_distrust_word_moments(mb_bert_engine* e);
size_t mb_bert_word_moment_skip_updates(const mb_bert_engine* e);      /* updates enqueued with the moment skip in force */
size_t mb_bert_word_moment_scans(const mb_bert_engine* e);             /* scans enqueued, since the engine was created */
/* Lazy zeroing.  The zeros mb_bert_train_step's AdamW would write over the layers' GEMM weight gradients are only ever
 * overwritten by the next backward, so a step that ends with the optimizer leaves that range "logically zero, physically stale"
 * (the rest of the buffer IS zeroed).  The engine writes the zeros itself before any of its own backwards that accumulates;
 * a host about to READ the bound gradient buffer after such a step (its own optimizer, a gradient exchange, a user looking at
 * .grad) calls mb_bert_materialize_grads first (a no-op when nothing is stale; mb_bert_grads_stale tells).  known_zero = 1
 * above also clears the state.  MB_ADAMW_KEEP=0 disables lazy zeroing: every fused step then really clears the buffer. */
int mb_bert_materialize_grads(mb_bert_engine* e, void* stream);
int mb_bert_grads_stale(const mb_bert_engine* e);

/* One whole optimizer step of train_epoch (multimodal_driver.py:354-388): `batch = tuple(t.to(DEVICE) ...)` staging, forward,
 * MSE (`:372-373`), loss.backward() (`:378`), optimizer.step() + optimizer.zero_grad() (`:384-386`) -- as TWO launches:
 *   1. a step prologue kernel that gathers the six batch tensors (device pointers, e.g. the landing buffer of an asynchronous
 *      H2D prefetch) into the engine's fixed staging buffers and writes this step's dropout keys (seed, step) and AdamW
 *      scalars (lr, bias-corrected step size from opt_step, grad_scale) into device memory;
 *   2. a replayed hipGraph with every other kernel of the step (captured on first use for each (B, L, output pointers)):
 *      one in-order kernel sequence -- the grouped weight-gradient launches run in line on the caller's stream.
 * Same kernels, same arithmetic, same dropout masks as mb_bert_forward + mb_bert_backward + 2 x mb_adamw_step with the same
 * (seed, step).  m, v: Adam moments parallel to the bound parameters; both NULL = no optimizer update (a gradient-accumulation
 * micro-step: gradients are accumulated, nothing is cleared).  With an update the gradient buffer is cleared in the same pass
 * (lazily over the layers' GEMM weights: see mb_bert_materialize_grads).
 * The two parameter groups of multimodal_driver.py:329-343 are [0, decay_count) with `weight_decay` and the rest with 0.
 * loss[0] = this step's MSE, loss_run (optional) += it.  mode: 1 = graph replay, 2 = the same sequence launched kernel by
 * kernel (reference for tests / profiling).  Pass the same logits / loss / m / v pointers every step: they are baked into the
 * captured graph (a new combination is captured again).  Not for data parallel runs: the gradient exchange is interleaved
 * with the backward stages from the host (mb_bert_backward + mb_bert_stage_grad_ranges). */
int mb_bert_train_step(mb_bert_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                       const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                       uint64_t seed, uint64_t step, float* logits, float* loss, float* loss_run, float* m, float* v, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int opt_step, int correct_bias, float grad_scale,
                       float loss_scale, int mode, void* stream);
/* The same step cut at its backward stages, for data-parallel hosts that issue one gradient all-reduce piece per stage between
 * them (mb_bert_stage_grad_ranges says what each stage makes final): mb_bert_stage_forward = step prologue (batch gather from
 * device or pinned host pointers, this step's dropout keys) + forward + MSE as one replayed graph; mb_bert_stage_backward(stage),
 * stage = 0 .. num_layers + 1 in order, = that stage as one replayed graph.  mode 1 = graphs, 2 = the same kernels launched one by
 * one.  The optimizer update stays with the caller (mb_adamw_step).  Same arithmetic and dropout masks as mb_bert_forward +
 * mb_bert_backward with the same (seed, step). */
int mb_bert_stage_forward(mb_bert_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                          const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                          uint64_t seed, uint64_t step, float* logits, float* loss, float* loss_run, int mode, void* stream);
int mb_bert_stage_backward(mb_bert_engine* e, float loss_scale, int stage, int mode, void* stream);
/* the engine's staging copy of the last gathered input_ids ([B*L] int64, device): the rows of the word-embedding gradient */
const int64_t* mb_bert_staged_input_ids(const mb_bert_engine* e);
/* `batch = tuple(t.to(DEVICE) for t in batch)` (multimodal_driver.py:359, :396, :429) for callers that drive the passes
 * themselves (evaluation, data parallel): ONE gather launch copies the six batch tensors into the engine's staging buffers.
 * The sources may be pinned HOST memory (hipHostMalloc / torch pin_memory: the kernel reads it across PCIe, no copy engine, no
 * extra stream) or device memory.  labels may be NULL.  staged6 receives the device pointers to hand to mb_bert_forward /
 * mb_bert_backward in the order input_ids, visual, acoustic, attention_mask, token_type_ids, labels.  mb_bert_train_step
 * does this gather itself (its sources may be pinned host memory too). */
int mb_bert_load_batch(mb_bert_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                       const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                       const void** staged6, void* stream);
/* number of graphs captured / replays launched so far (tests, bench) */
int mb_bert_graph_stats(const mb_bert_engine* e, size_t* captures, size_t* launches);

/* Update classes: per-group AdamW hyper-parameters in mb_bert_train_step (a larger learning rate for the new parameters, layer-wise
 * learning-rate decay, ...).  An update CLASS is one optimizer parameter group's lr / beta1 / beta2 / eps / weight_decay /
 * correct_bias; a SEGMENT is a run of consecutive tensors of the flat layout that belong to one class.
 * set_update_map: segment s covers elements [boundaries[s], boundaries[s + 1]) and belongs to class classes[s] (n_segments + 1
 *   boundaries, n_segments classes; host memory, copied).  The boundaries must be tensor offsets (mb_bert_tensor_info), ascending, from 0
 *   to mb_bert_param_count (MAG-XLNet: mb_xlnet_trainable_count) -- MB_ERR_SHAPE otherwise; more than MB_UPDATE_CLASSES_MAX classes or
 *   MB_UPDATE_SEGMENTS_MAX segments, or a class outside [0, n_classes): MB_ERR_ARG.  A refused map leaves the previous one in force.
 *   n_classes = 0 (the other arguments are ignored) clears the map: the step of the two parameter groups again, the default.  The map is
 *   part of the identity of a captured step graph (rider slices and the sweep are cut at the segment boundaries); installing the map
 *   that is already in force changes nothing.
 * set_update_decay (after set_update_map, which clears every mark): no_decay[s] != 0 marks segment s as one that does not decay -- it
 *   updates with its class's lr / beta1 / beta2 / eps / correct_bias and weight_decay 0 (n_segments bytes, the map's count; host memory,
 *   copied).  This lets the decayed and the undecayed parameter group of one learning rate share a class: layer-wise groups of a 24-layer
 *   model are 52 groups and 26 classes.  The marks are part of the map's identity like the boundaries: a changed mark re-captures,
 *   marks that are already in force change nothing.  NULL engine or marks, or another segment count than the map's: MB_ERR_ARG; no map
 *   set: MB_ERR_MODE.
 * set_update_values: the hyper-parameters of every class (arrays of n_classes, which must be the map's; host memory, copied) that the
 *   following mb_bert_train_step calls consume, until the next call.  With a map set the scalar lr .. weight_decay and correct_bias arguments of the
 *   step are ignored -- opt_step, grad_scale and loss_scale are used as ever -- and inside a segment the class's own weight_decay decides
 *   whether it decays, not the slab.  A step that ends with the optimizer (m, v given) while a map without values is set returns MB_ERR_ARG.
 *   New values never re-capture a graph: they reach the device with the step prologue, as the two groups' scalars do.
 * update_stats: the last enqueued update -- elements updated by riders inside the backward launches, elements updated by the sweep at the
 *   end of the step, and the number of segments of the map it ran under (0: the two parameter groups).  Any pointer may be NULL.
 *   With frozen segments, ridden + swept + frozen_elems (freeze_stats) = the update range.
 * set_update_frozen (after set_update_map, which clears every mark): frozen[s] != 0 marks segment s as one no parameter group holds
 *   (n_segments bytes, host memory, copied; the segment still names a class, which is not looked at).  MB_ERR_MODE without a map,
 *   MB_ERR_ARG for a wrong count.  A single-call step never changes the parameters, the bf16 shadow or the moments of such a segment, and
 *   leaves its range of the gradient buffer zero after every step that ends with the optimizer.  It also leaves out the launches whose
 *   whole output is frozen: the grouped weight-gradient launch (or, MB_GROUP_WGRAD=0, the four launches) of a layer whose GEMM weights
 *   are all frozen, the scatter into a frozen word table, and the embedding backward when word, position, token-type and LayerNorm
 *   tensors are all frozen.  The input-gradient chain always runs to the bottom (MAG is trainable), and a frozen tensor that a fused
 *   kernel produces next to trainable ones -- a bias, one of a layer's four weights -- is still computed, then cleared by a clear-only
 *   piece of the step's one sweep.  With clipping on, the norm is that of the trainable segments.  The marks are part of the map's
 *   identity: a changed mark re-captures.  When marks are installed or changed the engine clears the frozen ranges of the gradient buffer
 *   once, in front of the next single-call step, and distrusts the word-row stamps.  mb_bert_forward / _backward, the stage-driven calls
 *   and mb_bert_backward_outputs ignore the marks and compute every gradient.
 * freeze_stats: the last enqueued single-call step -- elements in frozen segments, weight-gradient launches (layers) left out, 1 when the
 *   embedding backward (MAG-XLNet: the word scatter) was left out.  All zero without marks.  Any pointer may be NULL.
 * While a map is set mb_bert_train_step_dp returns MB_ERR_MODE. */
#define MB_UPDATE_CLASSES_MAX 32
#define MB_UPDATE_SEGMENTS_MAX 128
int mb_bert_set_update_map(mb_bert_engine* e, int n_classes, int n_segments, const size_t* boundaries, const int* classes);
int mb_bert_set_update_decay(mb_bert_engine* e, int n_segments, const uint8_t* no_decay);
int mb_bert_set_update_values(mb_bert_engine* e, int n_classes, const float* lr, const float* beta1, const float* beta2, const float* eps,
                              const float* weight_decay, const int* correct_bias);
int mb_bert_update_stats(const mb_bert_engine* e, size_t* ridden, size_t* swept, int* segments);
int mb_bert_set_update_frozen(mb_bert_engine* e, int n_segments, const uint8_t* frozen);
int mb_bert_freeze_stats(const mb_bert_engine* e, size_t* frozen_elems, int* wgrad_launches_skipped, int* embed_skipped);

/* Gradient-norm clipping inside mb_bert_train_step.  set_grad_clip: max_norm > 0 turns it on for every later step that ends with the
 * optimizer (m, v given); max_norm <= 0 or non-finite turns it off, the default.  Sticky, like set_update_values.  Such a step updates
 * no parameter before the whole gradient exists -- no riders in the backward launches, so update_stats reports ridden == 0 -- and between its backward and its sweep takes the norm of the flat gradient range [0,
 * mb_bert_param_count) as mb_grad_clip_coef does, with the step's grad_scale, and multiplies the coefficient into the gradient scale the
 * sweep reads from device memory: one extra read of the gradient buffer, no pass that scales it.  After gradient-accumulation
 * micro-steps (no m, v: unaffected) the clipped quantity is the accumulated gradient.  On / off is part of a captured graph's identity;
 * the value reaches the device with the step prologue and never re-captures.  The scratch is device memory the engine allocates on
 * the first such step: mb_bert_workspace_bytes does not change.  mb_bert_train_step_dp returns MB_ERR_MODE while clipping is on.
 * grad_clip_stats: waits for `stream` and returns {norm, coef} of the last update; MB_ERR_MODE when clipping is off or no update has
 * run since it was turned on.  Either pointer may be NULL. */
int mb_bert_set_grad_clip(mb_bert_engine* e, float max_norm);
int mb_bert_grad_clip_stats(mb_bert_engine* e, float* norm, float* coef, void* stream);

/* Measurement hooks (bench.py): with profiling on, every per-layer grouped weight-gradient launch of mb_bert_backward is
 * bracketed by HIP timing events on the engine's internal side stream -- the stream that kernel runs on, which the
 * caller cannot see.  mb_bert_profile_wgrad_us waits for the last backward's events and returns the mean launch
 * duration over the layers, i.e. the in-step duration (concurrent with the dgrad chain), comparable with rocprofv3. */
int mb_bert_set_profiling(mb_bert_engine* e, int on);
int mb_bert_profile_wgrad_us(mb_bert_engine* e, float* avg_us);
/* the same for the two optimizer launches of the last mb_bert_train_step (first launch issued -> second complete, us) */
int mb_bert_profile_adamw_us(mb_bert_engine* e, float* us);

/* ------------------------------------------------------------------------------------------------ MAG-XLNet engine
 * MAG_XLNetForSequenceClassification forward / backward (xlnet.py:432-527 -> :15-429; XLNetLayer / SequenceSummary of
 * transformers 3.0.2) for the driver's configuration (bi-directional, no mems / perm_mask / target_mapping).  max_seq may be
 * anything up to 512 (XLNet has no position table; 512 is the kernels' limit): passes with L <= 128 run the LDS-resident
 * relative-attention kernels, longer ones the tiled kernels (mb_xlnet_attention_tiled_* below), whatever max_seq is.  An engine
 * with max_seq <= 128 carves the workspace it always carved; above it the per-layer saved probabilities stay at 128 rows (for the
 * short passes), the long passes keep per-layer row statistics instead and share two [B * n_head][LP][LP] planes (LP = max_seq
 * rounded up to 64).
 * Same calling conventions as the mb_bert_* family.  Backward stages: 0 = summary + logits_proj, 1..n_layer = layers (last
 * first; the MAG backward runs inside the stage of layer `injection_index`), n_layer+1 = word embedding. */
typedef struct {
    /* d_model: 256 | 512 | 768 (xlnet-base-cased) | 1024 (xlnet-large-cased) with n_head * 64 == d_model; n_layer >= 1;
     * d_inner % 128 == 0; 0 <= injection_index < n_layer (else MB_ERR_ARG).  Any other size: mb_xlnet_create returns MB_ERR_SHAPE. */
    int vocab_size, d_model, n_layer, n_head, d_inner, num_labels;
    int visual_dim, acoustic_dim, injection_index;
    float layer_norm_eps, mag_layer_norm_eps, beta_shift;
    float dropout, summary_last_dropout, mag_dropout;
    int dtype;
    int max_batch, max_seq;
    int ff_activation;           /* MB_ACT_*: the activation of XLNetFeedForward (config.ff_activation), layers and query stream; 0 = erf-GELU.
                                    Any other value: MB_ERR_ARG */
} mb_xlnet_config;

typedef struct mb_xlnet_engine mb_xlnet_engine;

/* XLNet's relative attention core at the operator level (dh = 64; transformers 3.0.2 rel_attn_core):
 *     S[i,j] = ((q_i + r_w_bias) . k_j + (q_i + r_r_bias) . kr[b][L - i + j] + (q_i + r_s_bias) . seg_embed[seg_i != seg_j]) / 8
 *              - 1e30 * [(mask[b][j] == 0 or perm[b][i][j]) and (i != j or gstream)]
 *     vec_i  = head_scale[h] * sum_j dropout(softmax_j S)[i,j] v_j
 * qkv [B*L][3H] token-major (q | k | v), kr [B][2L][H], r_*_bias fp32 [nh][64], seg_embed fp32 [2][nh][64], seg / mask int64 [B][L],
 * perm bytes [B][L][L] or NULL, head_scale fp32 [nh] or NULL, vec / dvec [B*L][H]; the backward writes dqkv [B*L][3H], dkr [B][2L][H]
 * and ADDS the four parameter gradients into d_rwb / d_rrb / d_rsb [nh][64] and d_seg [2][nh][64].  gstream = 1 (the query stream's
 * mask) exists in the forward only.  Dropout: counter hash, element index ((b*nh + h)*L + i)*L + j.
 * mb_xlnet_attention_tiled_*: the kernels the engine runs for 128 < L <= 512, usable at any 1 <= L <= 512.  stats: caller scratch of
 * mb_xlnet_attention_tiled_stats_bytes(B, L, nh), written by the forward (row maxima and 1/normalisers), read by the backward together
 * with the forward's vec.  gsave / pdsave: two caller scratch planes of mb_xlnet_attention_tiled_scratch_bytes(dtype, B, L, nh) each.
 * probs (fp32 [B][nh][L][L] or NULL): the probabilities before dropout; with probs the forward accepts vec = stats = NULL.
 * Every dq / dk / dv / dkr element has one writer: reruns are bit-identical.  MB_ERR_SHAPE (1001) for L outside [1, 512] and when
 * dropout is on and B*nh*L*L >= 2^32; shapes are checked before any pointer is looked at.
 * mb_xlnet_attention_forward / _backward: the engine's dispatch -- L <= 128 the LDS-resident kernels (psave / gsave
 * [B*nh][LP][LP] in the activation dtype, LP = 32 | 64 | 128 >= L: the forward saves the probabilities, the backward reads them;
 * vec / stats / pdsave / perm of the backward unused), above it the tiled ones (psave unused). */
size_t mb_xlnet_attention_tiled_stats_bytes(int B, int L, int nh);
size_t mb_xlnet_attention_tiled_scratch_bytes(int dtype, int B, int L, int nh);
int mb_xlnet_attention_tiled_forward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                                     const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask, void* vec,
                                     float* stats, int B, int L, int nh, const mb_dropkey* drop, const float* head_scale,
                                     const uint8_t* perm, int gstream, float* probs, void* stream);
int mb_xlnet_attention_tiled_backward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                                      const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask,
                                      const void* vec, const void* dvec, const float* stats, void* gsave, void* pdsave, void* dqkv,
                                      void* dkr, float* d_rwb, float* d_rrb, float* d_rsb, float* d_seg, int B, int L, int nh,
                                      const mb_dropkey* drop, const float* head_scale, const uint8_t* perm, void* stream);
int mb_xlnet_attention_forward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                               const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask, void* vec,
                               void* psave, float* stats, int B, int L, int nh, const mb_dropkey* drop, const float* head_scale,
                               const uint8_t* perm, int gstream, void* stream);
int mb_xlnet_attention_backward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                                const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask,
                                const void* psave, const void* vec, const void* dvec, const float* stats, void* gsave, void* pdsave,
                                void* dqkv, void* dkr, float* d_rwb, float* d_rrb, float* d_rsb, float* d_seg, int B, int L, int nh,
                                const mb_dropkey* drop, const float* head_scale, const uint8_t* perm, void* stream);

int mb_xlnet_create(const mb_xlnet_config* cfg, mb_xlnet_engine** out);
void mb_xlnet_destroy(mb_xlnet_engine* e);
int mb_xlnet_num_tensors(const mb_xlnet_engine* e);
/* decay: 1 = weight-decay group, 0 = no-decay group, 2 = frozen (transformer.mask_emb: no gradient in this configuration) */
int mb_xlnet_tensor_info(const mb_xlnet_engine* e, int i, char* name, int name_cap, size_t* offset, size_t* numel,
                         int* ndim, int64_t* shape4, int* decay);
size_t mb_xlnet_param_count(const mb_xlnet_engine* e);
size_t mb_xlnet_decay_count(const mb_xlnet_engine* e);
void mb_xlnet_shadow_range(const mb_xlnet_engine* e, size_t* begin, size_t* end);
size_t mb_xlnet_workspace_bytes(const mb_xlnet_engine* e);
int mb_xlnet_bind(mb_xlnet_engine* e, float* params, float* grads, void* shadow, void* workspace, size_t ws_bytes);
int mb_xlnet_sync_weights(mb_xlnet_engine* e, void* stream);
int mb_xlnet_forward(mb_xlnet_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                     const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                     int training, uint64_t seed, uint64_t step, float* logits, float* loss, float* loss_run,
                     void* stream);
int mb_xlnet_backward(mb_xlnet_engine* e, const float* dlogits, const float* labels, float loss_scale, int stage_begin,
                      int stage_end, void* stream);
const void* mb_xlnet_sequence_output(const mb_xlnet_engine* e);
/* input of layer i as XLNetModel collects it with output_hidden_states (xlnet.py:363-392; before the MAG injection), i = n_layer: the last output */
const void* mb_xlnet_hidden_state(const mb_xlnet_engine* e, int i);
/* output_attentions (xlnet.py:387-427): the softmax probabilities the last forward saved for its backward, layer `layer`:
 * [B * n_head][LP][LP] in the engine's dtype, LP = *padded_len = L rounded up to 32 (entries beyond L are zero), BEFORE the
 * attention dropout (the host multiplies the counter-hash mask of site XS_LAYER0 + 8 * layer in train mode).  Valid until the
 * next forward. */
const void* mb_xlnet_attention_probs(const mb_xlnet_engine* e, int layer, int* padded_len);
/* The same for engines with max_seq > 128, which save no probabilities (mb_xlnet_attention_probs returns NULL there): a post-pass over
 * what the last forward left of layer `layer` (q | k | v, kr) and that pass's attention_mask / token_type_ids / perm_mask, which must
 * still be alive.  out: fp32 [B][n_head][L][L], device -- the probabilities BEFORE the attention dropout and the head mask, as above.
 * Works for every engine and length; valid until the next forward. */
int mb_xlnet_attention_probs_into(mb_xlnet_engine* e, int layer, float* out, void* stream);
/* head_mask (xlnet.py:340-353, 383): fp32 [n_layer][n_head] device memory, sticky until reset with NULL; head h of layer l
 * contributes head_mask[l][h] times its attention output (attn_prob * head_mask after the dropout).  Explicit forwards /
 * backwards only: mb_xlnet_train_step returns MB_ERR_MODE while it is set. */
int mb_xlnet_set_head_mask(mb_xlnet_engine* e, const float* head_mask);
int mb_xlnet_set_head_loss(mb_xlnet_engine* e, int kind, float param, const float* vec);      /* as mb_bert_set_head_loss; the query-stream head has no loss */
int mb_xlnet_get_head_loss(const mb_xlnet_engine* e, int* kind, float* param, float* vec, int* has_vec);
int mb_xlnet_set_head_loss_ex(mb_xlnet_engine* e, const mb_head_loss* hl);                    /* as mb_bert_set_head_loss_ex */
int mb_xlnet_get_head_loss_ex(const mb_xlnet_engine* e, mb_head_loss* hl, float* vec, int* has_vec);
/* perm_mask / input_mask (xlnet.py:258-296): bytes [B][L][L] in device memory, sticky until reset with NULL; perm[b][i][j] != 0 <=>
 * data_mask[i, j, b] = input_mask[j, b] + perm_mask[i, j, b] > 0, i.e. query i may not attend to key j (i == j is always allowed:
 * non_tgt_mask, xlnet.py:288-296).  Combined with the attention_mask argument of the passes by OR.  Explicit forwards /
 * backwards only (mb_xlnet_train_step returns MB_ERR_MODE while it is set).  Masks the content stream (h) and, without the i == j
 * exemption, the query stream of mb_xlnet_query_stream (attn_mask_g, xlnet.py:288-296). */
int mb_xlnet_set_perm_mask(mb_xlnet_engine* e, const uint8_t* perm);
/* target_mapping -> the query stream g (xlnet.py:238-240, 306-313, 374-399; replaces the `g` half of XLNetLayer's two-stream
 * attention, transformers modeling_xlnet XLNetRelativeAttention.forward behind xlnet.py:374-385).  A post-pass over the last
 * mb_xlnet_forward, which must have been an EVAL pass (training == 0) without mems (else MB_ERR_MODE) and whose attention_mask /
 * token_type_ids buffers must still be alive: g starts as mask_emb on M rows per sample, every layer projects it with the
 * layer's q, maps it onto the L positions with target_mapping (fp32 [B][M][L], device; one-hot rows in the usual use, any weights
 * accepted), attends over that layer's content-stream keys / values / positions under the perm_mask / attention_mask WITHOUT the
 * self exemption, maps the result back to the M targets and shares post_attention + feed-forward with h.  head_mask / perm_mask
 * apply as set.  Nothing of the forward is overwritten (a backward after it is still valid; g itself has no backward here).
 * scratch: caller-owned device memory, 256-byte aligned, >= mb_xlnet_query_stream_scratch_bytes(e, B, M, L) for the forward's B, L.
 * On return its first n_layer + 1 blocks of mb_xlnet_query_stream_state_bytes(e, B, M) bytes each hold g in front of layer i
 * ([B][M][d_model], activation dtype; XLNetModel's hidden_states_g) -- block n_layer is output_g, what XLNetModel returns first when
 * target_mapping is given (xlnet.py:396-399; the final dropout is the identity in eval).  logits_g (fp32 [B][num_labels], device)
 * or NULL: SequenceSummary("last") + logits_proj on output_g's last row, as MAG_XLNetForSequenceClassification reads
 * transformer_outputs[0] (xlnet.py:506-509). */
size_t mb_xlnet_query_stream_scratch_bytes(const mb_xlnet_engine* e, int B, int M, int L);
size_t mb_xlnet_query_stream_state_bytes(const mb_xlnet_engine* e, int B, int M);
int mb_xlnet_query_stream(mb_xlnet_engine* e, const float* target_mapping, int M, void* scratch, size_t scratch_bytes,
                          float* logits_g, void* stream);
/* mems (xlnet.py:81-91, 244-245, 374-385: the hidden states cached from the previous segment; keys / values of layer l run over
 * cat([mems[l], h]), klen = mlen + qlen <= max_seq).  Explicit mb_xlnet_forward / mb_xlnet_backward passes only (the single-call
 * steps return MB_ERR_MODE while it is set).  The caller passes the segment as klen rows per sample whose first mlen rows are
 * placeholders (any ids, zero modalities, attention_mask 1, token_type 0): before layer l the engine replaces those rows of the
 * layer's input by mems[l] -- [n_layer][B][mlen][d_model] in the activation dtype, caller-owned device memory, NULL = none; the
 * backward clears the gradient of those rows at every layer seam (the memory is detached, xlnet.py:91) and keeps their share of the
 * k / v weight gradients. */
int mb_xlnet_set_mems(mb_xlnet_engine* e, const void* mems, int mlen);
int mb_xlnet_stage_grad_ranges(const mb_xlnet_engine* e, int stage, size_t* offs, size_t* lens, int cap);
int mb_xlnet_mark_grads_zero(mb_xlnet_engine* e, int known_zero);      /* as mb_bert_mark_grads_zero */
/* inputs_embeds (xlnet.py:306-313) / the base model's autograd edge (xlnet.py:396-405 returns autograd tensors), as for MAG-BERT:
 * mb_xlnet_set_inputs_embeds: fp32 [B*L][d_model] word embeddings for the next passes (NULL = input_ids again), their gradient
 * after a backward in mb_xlnet_inputs_embeds_grad; mb_xlnet_model_output: the last layer's output after the final dropout
 * (whole sequence, activation dtype, scratch valid until the next backward); mb_xlnet_backward_outputs: its gradient back in,
 * then stages 1 .. n_layer + 1 of mb_xlnet_backward. */
int mb_xlnet_set_inputs_embeds(mb_xlnet_engine* e, const float* inputs_embeds);
const float* mb_xlnet_inputs_embeds_grad(const mb_xlnet_engine* e);
const void* mb_xlnet_model_output(mb_xlnet_engine* e, void* stream);
int mb_xlnet_backward_outputs(mb_xlnet_engine* e, const void* d_output, void* stream);
int mb_xlnet_set_profiling(mb_xlnet_engine* e, int on);                 /* as mb_bert_set_profiling (the grouped launch has 7 problems) */
int mb_xlnet_profile_wgrad_us(mb_xlnet_engine* e, float* avg_us);
int mb_xlnet_profile_adamw_us(mb_xlnet_engine* e, float* us);
int mb_xlnet_materialize_grads(mb_xlnet_engine* e, void* stream);       /* as mb_bert_materialize_grads */
int mb_xlnet_grads_stale(const mb_xlnet_engine* e);
/* the MAG-XLNet counterparts of mb_bert_train_step / mb_bert_load_batch / mb_bert_graph_stats (same contracts; one iteration of
 * train_epoch, multimodal_driver.py:359-386, for the xlnet-base-cased model).  The two parameter groups are [0, decay_count) and
 * [decay_count, trainable_count); the frozen transformer.mask_emb slot behind them is never updated (HF AdamW skips grad-less
 * parameters). */
int mb_xlnet_train_step(mb_xlnet_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                        const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                        uint64_t seed, uint64_t step, float* logits, float* loss, float* loss_run, float* m, float* v, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int opt_step, int correct_bias, float grad_scale,
                        float loss_scale, int mode, void* stream);
int mb_xlnet_load_batch(mb_xlnet_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                        const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                        const void** staged6, void* stream);
int mb_xlnet_graph_stats(const mb_xlnet_engine* e, size_t* captures, size_t* launches);
size_t mb_xlnet_trainable_count(const mb_xlnet_engine* e);
/* update classes of mb_xlnet_train_step: as mb_bert_set_update_map / _set_update_decay / _set_update_values / _update_stats above; the map covers
 * [0, mb_xlnet_trainable_count), and the sweep of a classed step is one launch here too */
int mb_xlnet_set_update_map(mb_xlnet_engine* e, int n_classes, int n_segments, const size_t* boundaries, const int* classes);
int mb_xlnet_set_update_decay(mb_xlnet_engine* e, int n_segments, const uint8_t* no_decay);
int mb_xlnet_set_update_values(mb_xlnet_engine* e, int n_classes, const float* lr, const float* beta1, const float* beta2, const float* eps,
                               const float* weight_decay, const int* correct_bias);
int mb_xlnet_update_stats(const mb_xlnet_engine* e, size_t* ridden, size_t* swept, int* segments);
/* frozen segments: as mb_bert_set_update_frozen / _freeze_stats above; a frozen layer is one whose seven GEMM weights are all frozen */
int mb_xlnet_set_update_frozen(mb_xlnet_engine* e, int n_segments, const uint8_t* frozen);
int mb_xlnet_freeze_stats(const mb_xlnet_engine* e, size_t* frozen_elems, int* wgrad_launches_skipped, int* embed_skipped);
/* gradient-norm clipping inside mb_xlnet_train_step: as mb_bert_set_grad_clip / _grad_clip_stats above; the norm covers
 * [0, mb_xlnet_trainable_count) */
int mb_xlnet_set_grad_clip(mb_xlnet_engine* e, float max_norm);
int mb_xlnet_grad_clip_stats(mb_xlnet_engine* e, float* norm, float* coef, void* stream);

/* ------------------------------------------------------------------------------------------------ data parallel (new)
 * The reference is single-device (global_configs.py:4,7; multimodal_driver.py:21 imports a DistributedSampler it never uses).
 * Data-parallel fine-tuning here = one process per GPU, replicated parameters, the minibatch cut per rank, and ONE logical
 * all-reduce(sum) of the flat fp32 gradient buffer per optimizer step, issued from C on a side HIP stream in pieces as the backward
 * finishes them (csrc/comm.hip).  An mb_comm owns that stream, its events and the backend:
 *   mb_comm_create_rccl      -- RCCL (dlopen'ed at run time; a process that already carries an RCCL, e.g. PyTorch's, shares it).
 *                               id128 = the 128-byte ncclUniqueId rank 0 got from mb_comm_unique_id and handed to every rank
 *                               (over torch.distributed, a file, MPI: the caller's plumbing);
 *   mb_comm_create_callbacks -- host callbacks (tests: two gloo ranks on one GPU).  all_reduce(ctx, buf, count, dtype, stream):
 *                               in-place sum over the ranks of `count` elements of MB_DT_*; all_gather(ctx, buf, bytes_per_rank,
 *                               stream): in place, rank r's piece at buf + r * bytes_per_rank; both ordered on `stream`.
 * Scratch (caller-owned device memory, mb_comm_bind_scratch): the bf16 wire staging ([n_params] bf16, only with wire_dtype =
 * MB_DT_BF16) and the buffers of the row-wise word-embedding exchange (vocab x world slot table, world x capacity_rows ids and
 * fp32 rows; vocab = 0 -> the table travels in the dense tail piece).  mb_comm_exposed_ms: with timing on, how long the compute
 * stream of the LAST step was stalled on the exchange (synchronises on the timing events).  Error text: mb_comm_last_error(). */
typedef struct mb_comm mb_comm;
typedef int (*mb_all_reduce_cb)(void* ctx, void* buf, size_t count, int dtype, void* stream);
typedef int (*mb_all_gather_cb)(void* ctx, void* buf, size_t bytes_per_rank, void* stream);
int mb_comm_unique_id(void* id128);
int mb_comm_create_rccl(const void* id128, int rank, int world, mb_comm** out);
int mb_comm_create_callbacks(int rank, int world, mb_all_reduce_cb all_reduce, mb_all_gather_cb all_gather, void* ctx, mb_comm** out);
void mb_comm_destroy(mb_comm* c);
int mb_comm_rank(const mb_comm* c);
int mb_comm_world(const mb_comm* c);
void* mb_comm_stream(const mb_comm* c);                 /* the comm stream (hipStream_t) */
size_t mb_comm_scratch_bytes(int world, int wire_dtype, size_t n_params, int vocab, int hidden, int capacity_rows);
int mb_comm_bind_scratch(mb_comm* c, void* scratch, size_t bytes, int wire_dtype, size_t n_params, int vocab, int hidden, int capacity_rows);
/* stand-alone pieces of the exchange (tests; both in place, ordered on `stream`): sum of buf[0, count) over the ranks in the wire
 * format; row-wise sum of a [vocab][hidden] fp32 table of which this rank touched the rows ids[0, T) (T <= capacity_rows) */
int mb_comm_all_reduce(mb_comm* c, float* buf, size_t count, void* stream);
int mb_comm_exchange_rows(mb_comm* c, float* table, const int64_t* ids, int T, void* stream);
/* Gradient accumulation (/root/reference/multimodal_driver.py:375-376, 383-386): micro-steps are plain mb_*_train_step calls without
 * m / v (they accumulate and exchange nothing); the mb_*_train_step_dp that follows them must move the word-embedding table DENSELY
 * (its gradient holds the rows of every micro-step, not only this step's ids): mb_comm_set_row_exchange(c, 0) before it, 1 after. */
int mb_comm_set_row_exchange(mb_comm* c, int rowwise);
/* Sharded optimizer update (ZeRO-1 over the layers' GEMM weights; NEW: the reference runs one AdamW over everything,
 * multimodal_driver.py:345, 384-386).  With sharding on, mb_*_train_step_dp reduce-scatters every piece of layer GEMM-weight
 * gradients instead of all-reducing it, updates this rank's slice of every piece only, and all-gathers what the next forward reads
 * (the bf16 shadow in bf16 mode, the fp32 parameters in fp32 mode) on the comm stream.  With more than one piece the piece finished
 * last (the lowest layers, needed first) stays replicated and the NEXT mb_*_train_step_dp runs its forward as one graph per piece,
 * each waiting for the gather of its own piece only; any other consumer of the weights calls mb_comm_join(c, its stream) first.  In bf16 mode the fp32 masters -- and in either
 * mode Adam's m / v -- of the other ranks' slices are stale until mb_comm_gather_shards(c, flat buffer, 4, stream) refreshes them
 * (state_dict / checkpoints).  mb_comm_shard_slices: this rank's [begin, end) slices of the last sharded step. */
int mb_comm_set_sharding(mb_comm* c, int on);
int mb_comm_sharding(const mb_comm* c);
int mb_comm_join(mb_comm* c, void* stream);
int mb_comm_gather_shards(mb_comm* c, void* base, int elem_bytes, void* stream);
int mb_comm_shard_slices(const mb_comm* c, size_t* begin_end_pairs, int max_pairs);
int mb_comm_set_timing(mb_comm* c, int on);
int mb_comm_exposed_ms(mb_comm* c, float* ms);
int mb_comm_stats(const mb_comm* c, size_t* pieces, size_t* bytes);      /* collectives issued / bytes handed to them in the last step */
const char* mb_comm_last_error(void);
/* One optimizer step of a data-parallel rank as ONE engine call: mb_bert_train_step with the exchange inside.  The step runs as a
 * chain of LINEAR replayed graphs (a graph with a cross-stream fork replays on ROCm 7.2's slow path): forward + head + the
 * backward of the top 4 layers | 4 more | 2 more | the last 2 layers + MAG + embeddings | AdamW of the GEMM weights of the ten
 * layers reduced early | AdamW of the rest (MB_DP_CHUNKS="4,4,2,2" / MB_DP_CHUNK=n change the cut).  Between two of them the host
 * records an event and issues that segment's all-reduce on the comm stream; what the last backward segment produces -- its two
 * layers and the tail (everything that is not a layer's GEMM weight; the word-embedding table row-wise) -- travels under the first
 * AdamW launch.  Everything the single-call step has stays: the deferred LayerNorm reduction, stored (not accumulated) weight
 * gradients, lazy zeroing.  grad_scale = 1 / world for the mean over the global batch (the pieces are SUMs).  m, v must be given
 * (a gradient-accumulation micro-step has nothing to exchange: use mb_bert_train_step). */
int mb_bert_train_step_dp(mb_bert_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                          const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                          uint64_t seed, uint64_t step, float* logits, float* loss, float* loss_run, float* m, float* v, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int opt_step, int correct_bias, float grad_scale,
                          float loss_scale, int mode, void* stream, mb_comm* comm);
int mb_xlnet_train_step_dp(mb_xlnet_engine* e, const int64_t* input_ids, const float* visual, const float* acoustic,
                           const int64_t* attention_mask, const int64_t* token_type_ids, const float* labels, int B, int L,
                           uint64_t seed, uint64_t step, float* logits, float* loss, float* loss_run, float* m, float* v, float lr,
                           float beta1, float beta2, float eps, float weight_decay, int opt_step, int correct_bias, float grad_scale,
                           float loss_scale, int mode, void* stream, mb_comm* comm);

#ifdef __cplusplus
}
#endif
#endif
