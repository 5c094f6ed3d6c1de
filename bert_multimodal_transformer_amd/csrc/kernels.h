// Internal C++ launch API of the HIP kernels (host side).  The public C ABI is include/magbert_hip.h.
#pragma once
#include <cstdio>
#include <cstdlib>
#include "common.h"

namespace mb {

enum {
    MB_OK = 0,
    MB_ERR_SHAPE = 1001,     // unsupported shape / alignment
    MB_ERR_MODE = 1002,      // unsupported epilogue / layout combination
    MB_ERR_DTYPE = 1003,
    MB_ERR_ARG = 1004,
    MB_ERR_COMM = 1005,      // gradient exchange: RCCL missing / no backend (mb_comm_last_error() has the text); 2000 + n = ncclResult_t n
};

// MB_CK_TRACE=1: every failing call of a CK(...) chain is printed with its source line (a bare HIP error code from the middle of a
// 200-kernel step says nothing about which call produced it)
inline void ck_trace(const char* expr, const char* file, int line, int code) {
    static int on = -1;
    if (on < 0) { const char* v = getenv("MB_CK_TRACE"); on = (v && atoi(v)) ? 1 : 0; }
    if (on) fprintf(stderr, "[magbert] %s:%d: %s -> %d\n", file, line, expr, code);
}

// ------------------------------------------------------------------------------------------ GEMM
enum { GEMM_NT = 0,   // A [M][K] row, B [N][K] row      : Y = X W^T            (forward Linear)
       GEMM_NN = 1,   // A [M][K] row, B [K][N] kmaj     : dX = dY W            (dgrad)
       GEMM_TN = 2 }; // A [K][M] kmaj, B [K][N] kmaj    : dW = dY^T X          (wgrad)

enum { EPI_BIAS = 0,          // C = alpha*acc + bias                                   (T out)
       EPI_BIAS_GELU = 1,     // u = acc + bias ; C = gelu'(u) ; C2 = gelu(u) [* dropout]  (T out x2)
       EPI_BIAS_DROP_RES = 2, // C = dropout(acc + bias) + R                            (T out)
       EPI_ADD_RES = 3,       // C = acc (+ R)                                          (T out)
       EPI_DGELU = 4,         // C = acc * R [* dropout], R = the derivative saved by mode 1 / 7  (T out)
       EPI_ACCUM_F32 = 5,     // Cf += acc   (atomic when split-K)                      (fp32 out)
       EPI_BIAS_F32 = 6,      // Cf = alpha*acc + bias                                  (fp32 out)
       EPI_BIAS_ACT = 7 };    // mode 1 with GemmArgs::act (common.h ACT_RELU ... ACT_MISH) in the place of erf-GELU  (T out x2)

struct AdamArgs {
    float lr, beta1, beta2, eps, weight_decay, step_size;   // step_size = lr*sqrt(1-b2^t)/(1-b1^t)
    float grad_scale;                                        // multiply g before use (1/world_size for DP averaging)
};

struct GemmArgs {
    const void* A; const void* B;
    int M, N, K, lda, ldb;
    void* C; int ldc;          // T output (modes 0-4, 7)
    int act;                   // mode 7: the activation, ACT_RELU | ACT_SWISH | ACT_GELU_NEW | ACT_MISH (wave-uniform switch in the epilogue)
    void* C2;                  // second T output (modes 1, 7), same ldc
    float* Cf;                 // fp32 output (modes 5, 6), ldc
    const float* bias;         // [N] fp32 or null
    float* colsum;             // EPI_DGELU: if non-null, colsum[n] += sum_m C[m][n] (bias grad of the previous Linear)
    const void* R; int ldr;    // residual / aux input (T)
    float alpha;
    DropKey drop;
    int kchunk;                // filled by the launcher
    int dbg;                   // ablation switches (MB_GEMM_DBG): 1 = no DMA issue, 2 = no MFMA, 4 = no LDS fragment reads
    int reg_m, reg_n, tpr_m, tpr_n;   // XCD regions (filled by the launcher): reg_m*reg_n == 8, tiles per region
    int overwrite;                    // EPI_ACCUM_F32 without split-K: Cf = acc instead of Cf += acc (the caller knows Cf holds zeros)
    int cvalid;                       // EPI_ACCUM_F32, > 0: only columns [0, cvalid) of the N (padded) ones are stored, one dword per lane -- Cf / ldc
                                      // need no alignment then (MAG's weight gradients go straight into tensors 815 / 842 / 47 / 74 floats wide)
    unsigned long long* trace;        // MB_GEMM_TRACE=1: [blocks][8] wall-clock stamps (100 MHz) of the phases of every block, else null
    // Segmented B (0 = off): B's contiguous dimension (the columns n of a k-major B, the k of a row-major B) is cut into pieces of
    // `bseg` elements that live in separate tensors `bseg_stride` elements apart: element (r, c) sits at
    // B + (c / bseg) * bseg_stride + r * ldb + c % bseg.  This is how MAG-XLNet's q | k | v projections -- three [768][768] tensors
    // next to each other in the flat parameter buffer -- run as ONE forward GEMM (N = 2304) and ONE dgrad (K = 2304) instead of
    // three each.  bseg must be a multiple of the tile (k-major) / of the k-stage (row-major); no split-K.
    int bseg; size_t bseg_stride;
    GradAcc acc;                      // where colsum goes in deterministic mode (common.h); {} = fp32 atomics
};
// copies the stamps of the last traced launch to the host (measurement tooling: tools/gemm_bench --trace); returns the block count
int gemm_trace_fetch(unsigned long long* host_out, int max_blocks);
// the symbol of the kernel this process's last GEMM launch used (mb_debug_gemm_last_kernel) -> its length, 0 = no launch yet
int gemm_last_kernel(char* out, int cap);

// tile: 0 = auto, 64 or 128.  splits: split-K factor (only EPI_ACCUM_F32).
int gemm_launch(int dtype, int layout, int mode, const GemmArgs& a, int splits, int tile, hipStream_t st);

// Grouped wgrad (GEMM_TN, EPI_ACCUM_F32): `count` <= MB_MAX_GROUP (8) problems Cf_g[M_g][N_g] += A_g^T B_g in one launch.
// Needs whole tiles and whole 128-byte K rows for every problem (gemm_grouped_tn_ok tells); tile = 64 | 128.
#define MB_MAX_GROUP 8
// An HF-AdamW update riding inside a grouped weight-gradient launch (MB_ADAMW_RIDE): `blocks` extra workgroups at the head of the grid
// (a multiple of 8: the tiles' XCD placement is unchanged) update n4 quads of weight-decayed parameters -- the GEMM weights of the
// layer whose gradients the PREVIOUS launch completed -- while the other workgroups multiply.  The update is HBM-bound, the tiles
// are not, and the 256 x 128 launch leaves 40 of the 256 CUs without a tile.  p / g / m / v / shadow point at the range's first element.
struct AdamRide {
    float *p, *g, *m, *v;
    bf16* shadow;             // bf16 operand shadow of the range or null
    size_t n4;
    const AdamArgs* dyn;      // this step's scalars (device memory: the step prologue writes them)
    int blocks;               // 0 = no rider
    int zero_grad;            // 0: the next backward overwrites these gradients (engine_common.h keep_in_step)
};
void gemm_log_ride(const AdamRide& r);      // MB_GEMM_LOG=1: "[magbert ride] params=... blocks=..." for a launch that carries riders (gemm.hip)
struct GroupedGemmArgs {
    GemmArgs g[MB_MAX_GROUP];
    int first[MB_MAX_GROUP + 1];    // first block (region placement) or first tile of the group-wide list (chunk > 0) of every problem
    int count;
    int chunk;                      // > 0: tiles per XCD of the group-wide XCD-compact placement (gemm.hip); 0: per-problem regions
    AdamRide ride;                  // ride.blocks > 0: that many workgroups in front of the tiles run an optimizer update instead
    // Gathered k loop (the 256 x 128 ping-pong kernel only): problem i sums over the k rows rows[i][0 .. n) of BOTH operands, in list order,
    // n = min(K, *nrows[i]) -- read by the kernel, a multiple of 64 and at least 192; the list holds at least that many valid entries
    // (< K).  rows[i] == null: the dense loop over all K rows.
    const uint32_t* rows[MB_MAX_GROUP];
    const uint32_t* nrows[MB_MAX_GROUP];
    const char* note;               // host only: what the launch's MB_GEMM_LOG line says about the lists (may be null)
};
// the row lists of a gathered grouped launch, per problem (null = dense)
struct GroupedRows { const uint32_t* rows[MB_MAX_GROUP]; const uint32_t* nrows[MB_MAX_GROUP]; const char* note; };      // note: for the MB_GEMM_LOG line
// A dgrad launch (GEMM_NN; mode EPI_ADD_RES or EPI_DGELU) with riders: gemm_nn_ride_tiles -> the tile count (padded to 8) of the launch
// gemm_launch would make of `a` when that is one of the two kernels that leave block slots free (64 x 64 three-slot, 128 x 128 two-slot;
// *per_cu = block slots per CU), else 0; gemm_nn_ride_launch: that launch with ride.blocks (a multiple of 8) rider workgroups behind the
// tiles (MB_ERR_MODE when gemm_nn_ride_tiles says 0).
int gemm_nn_ride_tiles(int dtype, int mode, const GemmArgs& a, int* per_cu);
int gemm_nn_ride_launch(int dtype, int mode, const GemmArgs& a, const AdamRide& ride, hipStream_t st);
int gemm_grouped_tn_ok(int dtype, const GemmArgs* probs, int count, int tile);
int gemm_grouped_tn_launch(int dtype, const GemmArgs* probs, int count, int tile, hipStream_t st, int stages = 0,
                           const AdamRide* ride = nullptr,    // stages: 0 = MB_GROUP_STAGES, 4 | 5 = deeper ring (64 x 64 tiles only)
                           const GroupedRows* rows = nullptr);      // gathered k loop; MB_ERR_MODE where gemm_grouped_gather_ok says 0
int gemm_grouped_gather_ok(int dtype, int tile);      // 1: a grouped launch of this dtype and tile runs the kernel that takes row lists

// ------------------------------------------------------------------------------------------ row kernels (rowops.hip)
// LayerNorm over the last dim H (H % 256 == 0, H <= 1024): y = (x-mean)*rstd*gamma + beta ; optional dropout on y.
int ln_forward(int dtype, const void* x, const float* gamma, const float* beta, float eps, void* y,
               float* mean, float* rstd, int rows, int H, DropKey drop, hipStream_t st,
               Prefetch pf = {nullptr, 0, nullptr});
// LayerNorm backward. dy: grad of LN output (after optional dropout `drop_out`), x: saved LN input.
//   dx      = grad wrt LN input                         (T)  [required]
//   dx_drop = dx * mask(drop_in)                        (T)  [optional: grad of the pre-dropout Linear output]
//   dgamma, dbeta += column sums ; dbias += colsum(dx_drop or dx)   (fp32, atomics) [each optional]
int ln_backward(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                void* dx, void* dx_drop, float* dgamma, float* dbeta, float* dbias,
                int rows, int H, DropKey drop_out, DropKey drop_in, hipStream_t st);
// folds a deterministic-mode shadow accumulator into the fp32 gradients g[begin, end) and clears it (common.h GradAcc)
int grad_fold(GradAcc acc, float* g, size_t begin, size_t end, hipStream_t st);
// same, but the three column sums go to per-block partial slabs partials[nblk][3][H] (no atomics); returns nblk through
// *nblk.  ln_reduce_partials adds them into up to 6 destinations in one launch (two LayerNorms of a layer).
size_t ln_partials_floats(int rows, int H);
int ln_backward_partials(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                         void* dx, void* dx_drop, float* partials, int* nblk, int rows, int H, DropKey drop_in, hipStream_t st,
                         Prefetch pf = {nullptr, 0, nullptr});
int ln_reduce_partials(const float* partials_a, const float* partials_b, int nblk, int H, float* const* dst6, hipStream_t st, GradAcc acc = {});
// The same for `layers` layers in ONE launch: layer l's slabs start at partials_x + l * layer_stride floats, its six destinations
// are dst[l][0..5].  (A single-process step has no use for a layer's LayerNorm / bias gradients before AdamW: twelve 5-us
// launches become one.)
#define MB_LN_MAX_LAYERS 32
struct LnReduceDst { float* d[MB_LN_MAX_LAYERS][6]; int nblk[MB_LN_MAX_LAYERS]; };    // nblk[slot] > 0: that slot's own slab count
int ln_reduce_partials_layers(const float* partials_a, const float* partials_b, size_t layer_stride, int layers, int nblk, int H,
                              const LnReduceDst& dst, hipStream_t st, GradAcc acc = {});

// BertEmbeddings: e = dropout(LN(word[ids] + pos[l] + type[seg])).
int embed_ln_forward(int dtype, const int64_t* ids, const int64_t* seg, const float* word, const float* pos,
                     const float* type, const float* gamma, const float* beta, float eps, void* out,
                     float* mean, float* rstd, int B, int L, int H, DropKey drop, hipStream_t st,
                     const int64_t* pos_ids = nullptr);       // [B*L] rows of `pos` (null: arange(L) per sample, bert.py:211-216)
int embed_ln_backward(int dtype, const void* dout, const int64_t* ids, const int64_t* seg, const float* word,
                      const float* pos, const float* type, const float* gamma, const float* mean, const float* rstd,
                      float* dsum_ws, float* dword, float* dpos, float* dtype_, float* dgamma, float* dbeta,
                      int B, int L, int H, int pad_id, DropKey drop, hipStream_t st, const int64_t* pos_ids = nullptr, GradAcc acc = {},
                      // part: dgamma / dbeta go to rows 0 / 1 of a partial set [nblk][3][H] instead (reduced by ln_reduce_partials*)
                      float* part = nullptr, int* nblk = nullptr,
                      // part_b (with part, default positions only): ONE launch that also produces dpos / dtype; dtype[0] -> row 2 of `part`,
                      // dtype[1] -> row 0 of `part_b` (the caller's reduction adds them to dtype_), *nblk = L * ceil(B / 8)
                      float* part_b = nullptr,
                      // id_count: the table the step prologue of THIS batch counted token ids into (vocab_size ints, zero between steps):
                      // rows whose id occurs once add their word-embedding gradient without atomics; the entries are cleared again
                      int* id_count = nullptr);

// column sums: out[n] += sum_m x[m][n]
int colsum(int dtype, const void* x, int ldx, float* out, int rows, int cols, hipStream_t st, GradAcc acc = {});

// fp32 [rows][cols] -> T [rows][cols_pad] zero padded (modality tensors -> MFMA operands)
int pack_pad(int dtype, const float* src, int cols, void* dst, int cols_pad, int rows, hipStream_t st);
// fp32 -> T contiguous conversion (n elements)
int convert(int dtype, const float* src, void* dst, size_t n, hipStream_t st);
int widen(int dtype, const void* src, float* dst, size_t n, hipStream_t st);       // dst fp32 <- src (dtype), n % 4 == 0

// ------------------------------------------------------------------------------------------ MAG (mag.hip)
struct MagDims { int T, H, V, A, Vp, Ap; };
// pack master weights (reference layout) into the MFMA operand layout:
//   We [2H][H]  = [W_hv[:, V:] ; W_ha[:, A:]]     Wv [2H][Vp] = [W_hv[:, :V] ; W_v]     Wa [2H][Ap] = [W_ha[:, :A] ; W_a]
int mag_pack_weights(int dtype, const float* W_hv, const float* W_ha, const float* W_v, const float* W_a,
                     void* We, void* Wv, void* Wa, MagDims d, hipStream_t st);
// scatter-add packed weight grads back into the reference layout
int mag_unpack_wgrads(const float* dWe, const float* dWv, const float* dWa, float* dW_hv, float* dW_ha,
                      float* dW_v, float* dW_a, MagDims d, hipStream_t st);
// gate + norm-ratio clamp + residual + LayerNorm + dropout (modeling.py:27-49) from the three pre-activation panels
int mag_gate_forward(int dtype, const void* e, const void* Ze, const void* Zv, const void* Za,
                     const float* b_hv, const float* b_ha, const float* b_v, const float* b_a,
                     const float* gamma, const float* beta, float ln_eps, float beta_shift,
                     void* out, float* mean, float* rstd, MagDims d, DropKey drop, hipStream_t st);
int mag_gate_backward(int dtype, const void* dout, const void* e, const void* Ze, const void* Zv, const void* Za,
                      const float* b_hv, const float* b_ha, const float* b_v, const float* b_a,
                      const float* gamma, const float* mean, const float* rstd, float beta_shift,
                      void* de, void* dZe, void* dZv, void* dZa,
                      float* db_hv, float* db_ha, float* db_v, float* db_a, float* dgamma, float* dbeta,
                      MagDims d, DropKey drop, hipStream_t st, GradAcc acc = {},
                      // part_a / part_b: instead of adding the six column sums to db_* / dgamma / dbeta, every block writes its slab
                      // of two partial sets [nblk][3][H] ({db_hv, db_ha, db_v}, {db_a, dgamma, dbeta}) for ln_reduce_partials(_layers)
                      float* part_a = nullptr, float* part_b = nullptr, int* nblk = nullptr);

// ------------------------------------------------------------------------------------------ attention (attention.hip)
// qkv: [B*L][3H] token-major (q | k | v, head h at columns h*64..), mask: int64 [B][L] (1 = attend),
// ctx: [B*L][H].  softmax(QK^T/sqrt(dh) + (1-mask)*-10000) -> dropout -> . V   (dh = 64, L <= 128)
// probs (fp32 [B][nh][L][L], may be null): the attention probabilities after dropout and head mask (output_attentions)
// head_scale (fp32 [nh], may be null): head_mask of this layer -- the dropped probabilities of head h are multiplied by it
// stats (fp32, tiled_stats_floats(B, L, nh), may be null for L <= 128): the row statistics the forward leaves for the backward
// L <= 128: the LDS-resident kernels (attention.hip); 128 < L <= 512: the tiled ones (attention_tiled.hip), which need stats and
// ctx (the backward's D_i = dO_i . ctx_i) and take no riders
int attention_forward(int dtype, const void* qkv, const int64_t* mask, void* ctx, int B, int L, int nh,
                      DropKey drop, hipStream_t st, float* probs = nullptr, const float* head_scale = nullptr,
                      float* stats = nullptr);
// dbias (fp32 [3H], may be null): += column sums of dqkv (bias grads of the fused QKV Linear)
int attention_backward(int dtype, const void* qkv, const int64_t* mask, const void* ctx, const void* dctx,
                       void* dqkv, float* dbias, int B, int L, int nh, DropKey drop, hipStream_t st,
                       const float* head_scale = nullptr, GradAcc acc = {},
                       const struct AdamRide* ride = nullptr,      // bf16: AdamW riders behind the (batch, head) workgroups (AdamRide below)
                       float* stats = nullptr);
// the tiled kernels at any 1 <= L <= 512 (attention_tiled.hip): stats = three fp32 planes of B*nh*L rows (m | 1/l | D); the backward
// returns MB_ERR_MODE when handed riders, MB_ERR_SHAPE when dropout is on and B*nh*L*L does not fit the uint32 mask index
size_t tiled_stats_floats(int B, int L, int nh);
int attention_tiled_forward(int dtype, const void* qkv, const int64_t* mask, void* ctx, float* stats, int B, int L, int nh,
                            DropKey drop, hipStream_t st, float* probs = nullptr, const float* head_scale = nullptr);
int attention_tiled_backward(int dtype, const void* qkv, const int64_t* mask, const void* ctx, const void* dctx, float* stats,
                             void* dqkv, float* dbias, int B, int L, int nh, DropKey drop, hipStream_t st,
                             const float* head_scale = nullptr, GradAcc acc = {}, const struct AdamRide* ride = nullptr);
int attention_backward_free_slots(int dtype, int L, int nblk, int cus);      // workgroups that fit the last round of that launch
int attention_trace_fetch(unsigned long long* host_out, int max_blocks);     // MB_ATTN_TRACE=1: stamps of the last attention_backward

// ------------------------------------------------------------------------------------------ XLNet (xlnet_attention.hip, xlnet_rowops.hip)
// relative attention core.  qkv [T][3H] token-major, kr [B][2L][H].  L <= 128: the LDS-resident kernels, psave/gsave [B][nh][LP][LP]
// (LP = 32 | 64 | 128 >= L).  128 < L <= 512: the tiled kernels (xlnet_attention_tiled.hip) -- psave is not touched, the forward leaves
// row statistics in `stats`, the backward needs them, the forward's `vec`, `perm` again (it recomputes the scores) and two scratch planes
// gsave / pdsave of xlnet_tiled_scratch_elems(B, L, nh) elements each; it takes no riders (MB_ERR_MODE).
int xlnet_attention_forward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                            const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask, void* vec,
                            void* psave, int B, int L, int nh, DropKey drop, hipStream_t st, const float* head_scale = nullptr,
                            const uint8_t* perm = nullptr,       // perm [B][L][L] bytes or null: != 0 <=> query i may not attend to key j (xlnet.py:265-296)
                            int gstream = 0,                     // 1: the query stream's mask (attn_mask_g = data_mask, no i == j exemption; xlnet.py:288-296)
                            float* stats = nullptr);             // L > 128: xlnet_tiled_stats_floats(B, L, nh) floats
int xlnet_attention_backward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                             const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask,
                             const void* psave, const void* dvec, void* gsave, void* dqkv, void* dkr, float* d_rwb,
                             float* d_rrb, float* d_rsb, float* d_seg, int B, int L, int nh, DropKey drop, hipStream_t st,
                             const float* head_scale = nullptr,      // head_scale [nh] or null: head_mask of the layer
                             GradAcc acc = {},                       // deterministic mode: the four bias / seg_embed column sums (common.h)
                             const struct AdamRide* ride_q = nullptr, const struct AdamRide* ride_kv = nullptr,      // bf16, L <= 64: riders of the two launches
                             const void* vec = nullptr, const float* stats = nullptr, void* pdsave = nullptr,        // L > 128 (see above)
                             const uint8_t* perm = nullptr);
int xlnet_attention_backward_free_slots(int dtype, int L, int nblk, int cus);
// the tiled kernels at any 1 <= L <= 512: stats = two fp32 planes of B*nh*L rows (m | 1/l); gsave / pdsave = [B*nh][LP][LP] elements of the
// activation dtype, LP = L rounded up to 64 (written by the backward's first launch, read by the other two).  The forward with
// probs (fp32 [B][nh][L][L], the probabilities BEFORE dropout) may be given vec = stats = null: a pure recomputation.
// MB_ERR_SHAPE when dropout is on and B*nh*L*L does not fit the uint32 mask index.
size_t xlnet_tiled_stats_floats(int B, int L, int nh);
size_t xlnet_tiled_scratch_elems(int B, int L, int nh);
int xlnet_attention_tiled_forward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                                  const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask, void* vec,
                                  float* stats, int B, int L, int nh, DropKey drop, hipStream_t st, const float* head_scale = nullptr,
                                  const uint8_t* perm = nullptr, int gstream = 0, float* probs = nullptr);
int xlnet_attention_tiled_backward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                                   const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask,
                                   const void* vec, const void* dvec, const float* stats, void* gsave, void* pdsave, void* dqkv, void* dkr,
                                   float* d_rwb, float* d_rrb, float* d_rsb, float* d_seg, int B, int L, int nh, DropKey drop,
                                   hipStream_t st, const float* head_scale = nullptr, const uint8_t* perm = nullptr, GradAcc acc = {});
// out[t] = dropout(word[ids[t]])  (xlnet.py:304-305) ; backward scatter-adds into dword
int gather_drop_forward(int dtype, const int64_t* ids, const float* word, void* out, int rows, int H, DropKey drop, hipStream_t st);
int gather_drop_backward(int dtype, const void* dout, const int64_t* ids, float* dword, int rows, int H, DropKey drop, hipStream_t st, GradAcc acc = {});
// (both: ids == nullptr = inputs_embeds -- `word` / `dword` are then [rows][H] fp32, read / written row by row)
// dst[i] += src[i], fp32, n % 4 == 0
int add_f32(float* dst, const float* src, size_t n, hipStream_t st);
// y = x * dropout mask over [rows][H] (element index = offset)
int drop_rows(int dtype, const void* x, void* y, int rows, int H, DropKey drop, hipStream_t st);
// pos[b][p][:] = dropout([sin(pos_p * inv_freq) | cos(...)]) with pos_p = L - p, p in [0, 2L)   (xlnet.py:93-146,332-333)
int xlnet_pos_emb(int dtype, void* out, int B, int L, int H, DropKey drop, hipStream_t st);
// xs[b] = x[b, L-1, :] * dropout   (final dropout xlnet.py:396 + SequenceSummary "last") ; backward scatters into a zeroed dx
int last_token_forward(int dtype, const void* x, void* xs, int B, int L, int H, DropKey drop, hipStream_t st);
int last_token_backward(int dtype, const void* dxs, void* dx, int B, int L, int H, DropKey drop, hipStream_t st);
// query stream under target_mapping tm [B][M][L] fp32 (xlnet.py:306-313, 374-399): the mask_emb row broadcast to [rows][H]; the
// attention operand of the g stream (q = tm-mapped qg [B*M][H] onto the L positions, k | v copied from the content stream's
// [T][3H]); the attention output mapped back to the M targets
int xlnet_broadcast_row(int dtype, const float* row, void* out, int rows, int H, hipStream_t st);
int xlnet_map_query(int dtype, const float* tm, const void* qg, const void* qkv_h, void* qkv_g, int B, int M, int L, int H, hipStream_t st);
int xlnet_unmap_vec(int dtype, const float* tm, const void* vec, void* vecg, int B, int M, int L, int H, hipStream_t st);

// ------------------------------------------------------------------------------------------ head (head.hip)
// pooled = tanh(z) ; logits = dropout(pooled) Wc^T + bc ; optional MSE loss (mean over B*nl) accumulated into loss[0]
// and (if non-null) into the running sum loss_run[0].
// The objective (include/magbert_hip.h MB_LOSS_*): a kind, at most one scalar (smooth_l1's beta) and one device vector of nl floats
// (bce's pos_weight, the cross entropy's class weights; null = none).  HL_DEFAULT is MSE at nl == 1 and cross entropy on class
// indices otherwise, labels [B]; mse | l1 | smooth_l1 | bce read labels [B][nl]; HL_CE reads class indices [B] and needs nl >= 2
// (MB_ERR_ARG otherwise, as for an unknown kind).
// Modifiers (mb_head_loss of include/magbert_hip.h; all zero = none, and then the launch is the one it always was): HL_CE takes
// `smoothing` (label smoothing, [0, 1)), `ignore` under `has_ignore` (samples whose label equals it count for nothing) and `gamma`
// (focal, 0 or >= 1, not with smoothing); HL_BCE takes `gamma`.  Anything else: MB_ERR_ARG.  The cross entropy is normalised by the
// class weights -- or the count -- of the kept samples; where that is 0 the loss and every gradient are 0 (torch: NaN).
enum { HL_DEFAULT = 0, HL_MSE = 1, HL_L1 = 2, HL_SMOOTH_L1 = 3, HL_BCE = 4, HL_CE = 5 };
struct HeadLoss { int kind; float param; const float* vec; float smoothing; float gamma; int ignore; int has_ignore; };
inline bool head_loss_modified(const HeadLoss& hl) { return hl.smoothing != 0.f || hl.gamma != 0.f || hl.has_ignore != 0; }
// what the kernels and the engines' setters take (no pointer is followed)
inline bool head_loss_legal(const HeadLoss& hl, int nl) {
    if (hl.kind < HL_DEFAULT || hl.kind > HL_CE || (hl.kind == HL_CE && nl < 2)) return false;
    if (!(hl.smoothing >= 0.f && hl.smoothing < 1.f)) return false;                          // (NaN fails both)
    if (!(hl.gamma == 0.f || (hl.gamma >= 1.f && hl.gamma <= 3.402823466e38f))) return false;       // 0, or finite and >= 1
    if (hl.smoothing > 0.f && hl.gamma > 0.f) return false;
    if ((hl.smoothing > 0.f || hl.has_ignore) && hl.kind != HL_CE) return false;
    if (hl.gamma > 0.f && hl.kind != HL_CE && hl.kind != HL_BCE) return false;
    return true;
}
inline bool head_loss_per_element(int kind) { return kind >= HL_MSE && kind <= HL_BCE; }
int head_forward(const float* z, const float* Wc, const float* bc, const float* labels, float* pooled,
                 float* logits, float* loss, float* loss_run, int B, int H, int nl, DropKey drop, hipStream_t st,
                 HeadLoss hl = HeadLoss{HL_DEFAULT, 0.f, nullptr});
// dlogits (given, or MSE grad if labels != null: 2*(logit-y)/(B*nl)*loss_scale) -> dz (grad wrt pooler pre-activation),
// dWc, dbc accumulated.  dz is written in the activation dtype (operand of the pooler dgrad / wgrad GEMMs).
int head_backward(int dtype, const float* dlogits, const float* logits, const float* labels, float loss_scale,
                  const float* pooled, const float* Wc, void* dz, float* dWc, float* dbc,
                  int B, int H, int nl, DropKey drop, hipStream_t st, GradAcc acc = {}, float* dbp = nullptr,
                  void* zero_p = nullptr, size_t zero_bytes = 0,    // dbp += column sums of dz; zero_p[0, zero_bytes) cleared by extra blocks
                  HeadLoss hl = HeadLoss{HL_DEFAULT, 0.f, nullptr});  // the gradient of that objective where dlogits == null

// ------------------------------------------------------------------------------------------ optimizer (adamw.hip)
// transformers 3.0.2 AdamW over flat fp32 buffers; elements [0, n_decay) use weight_decay, the rest 0.
// shadow (bf16, may be null): shadow[i] = bf16(p[i]) for i in [sh_begin, sh_end). zero_grad: g <- 0 after use.
// dyn (device pointer, may be null): when set, the hyper-parameters are read from *dyn instead of `a` (replayed step graphs)
// keep range [keep_begin, keep_end) (elements, multiples of 4; empty by default): g is NOT zeroed there -- the caller knows the next
// backward overwrites that range (the layers' GEMM weight gradients of a single-call step: 340 MB of zeros per step nobody reads)
int adamw_step(float* p, float* g, float* m, float* v, void* shadow, size_t n, size_t n_decay,
               size_t sh_begin, size_t sh_end, AdamArgs a, int zero_grad, hipStream_t st, const AdamArgs* dyn = nullptr,
               size_t keep_begin = 0, size_t keep_end = 0);
// Word-embedding rows the step did not touch (MB_ADAMW_SKIP_ZERO_ROWS): stamp[row] == state[0] <=> the prologue of a step whose
// backward feeds this update saw `row` in its batch (PrologueArgs::stamp).  When state[1] != 0 the engine vouches that every other row
// of [begin, end) -- rows of `row_len` elements -- holds g == +0.0f: the sweep neither loads that gradient nor stores the zero back,
// and runs the same arithmetic on a +0.0f it makes up.  state[1] == 0: the full read (decided per step, so a replayed graph obeys it).
// Zero moments (MB_ADAMW_SKIP_ZERO_MOMENTS): the top bit of a stamp word is the row's `seen` mark -- set <=> the row may hold non-zero
// moments (the prologue sets it with every stamp, word_moments_scan derives it from m and v); update numbers stay below it.  When
// state[2] != 0 the engine vouches that every row without the mark holds m == v == +0.0f and that this step's scalars leave such a
// row's moments and -- but for the decay -- its parameters bit for bit alone: an untouched row without the mark gets the decay only,
// and neither m, v nor g of it is read or written.  state[2] == 0: the moments of every row are read and written.
#define MB_STAMP_SEEN 0x80000000u
struct WordSkip { const uint32_t* stamp; const uint32_t* state; size_t begin, end; uint32_t row_len; };
// The end-of-step sweep of a single-call step as ONE launch over a table of pieces of the flat buffers (one adamw_step per range
// otherwise).  Everything is ABSOLUTE here: p / g / m / v / shadow are the buffers' first elements, the shadow and keep ranges element
// offsets (multiples of 4) into them.  Piece k covers quads [begin4[k], begin4[k] + start4[k + 1] - start4[k]) of the buffers, start4
// being the running sum of the pieces' lengths, and reads its scalars from cls[slot[k]]; that slot's own weight_decay decides whether
// the piece decays (no n_decay here).  Same per-element arithmetic as adamw_step (adam_update_store): the same bits.
// `cls` is any table of AdamArgs.  An unclassed step hands over its two scalars (engine_common.h adam_state: slot 0 = the decay slab,
// slot 1 = the same scalars with weight_decay 0) and up to three pieces: what the riders left of the layers, the rest of the decay
// slab, the no-decay slab.
// Update classes (include/magbert_hip.h: mb_*_set_update_map): one optimizer parameter group's scalars per slot of a table in device
// memory, and the flat layout cut into segments -- maximal runs of tensors of one class; the pieces are the same ranges cut at the
// segment boundaries.  That table has two halves of MB_CLASSES_MAX slots: slot MB_CLASSES_MAX + c is class c with weight_decay = 0,
// for segments marked no-decay (mb_*_set_update_decay) -- the pieces and riders of such a segment name that slot, and no kernel knows
// about marks.
#define MB_CLASSES_MAX 32
#define MB_SEGMENTS_MAX 128
#define MB_SWEEP_PIECES_MAX (MB_SEGMENTS_MAX + 2)
// Clear-only pieces (frozen segments, mb_*_set_update_frozen): slot == MB_PIECE_CLEAR -- the piece's gradient range gets zeros and no
// parameter, moment or shadow byte of it is read or written; what a backward still wrote into a range no parameter group holds.
// They lie behind every update piece of the table: pieces [0, clear_first) update, pieces [clear_first, count) clear (start4 runs on
// through both), and extra blocks of the same launch take them.
#define MB_PIECE_CLEAR 0xff
struct AdamPieces { uint32_t begin4[MB_SWEEP_PIECES_MAX], start4[MB_SWEEP_PIECES_MAX + 1]; uint8_t slot[MB_SWEEP_PIECES_MAX]; int count, clear_first; };
int adamw_sweep(float* p, float* g, float* m, float* v, void* shadow, const AdamPieces& r, size_t sh_begin, size_t sh_end,
                size_t keep_begin, size_t keep_end, const AdamArgs* cls, const WordSkip& skip, hipStream_t st);

// ------------------------------------------------------------------------------------------ gradient-norm clipping (gradnorm.hip)
// grad_sumsq: partial[b] = the sum over block b's share of g[0, n) of (double)g[i]^2, b < grad_norm_blocks(n) (<= 2048, a function of n
// alone); g needs 4-byte alignment only.  No atomics, fixed order: the same bits on every run.
// grad_clip_finalize (one block): sum = the partials in index order; norm = grad_scale * sqrt(sum); coef = min(1, max_norm / (norm + 1e-6))
// in double (torch.nn.utils.clip_grad_norm_; a non-finite norm gives what the arithmetic gives); out2 = {(float)norm, (float)coef}; then
// tab[k][0 .. count[k]).grad_scale *= (float)coef for both tables (a null table is skipped; 256 entries in all at most: a classed step hands over 2 + both halves of its class table).  dyn (device
// pointer, may be null): {max_norm, grad_scale} are read from there instead (replayed step graphs: PrologueArgs::clip).
unsigned grad_norm_blocks(size_t n);
int grad_sumsq(const float* g, size_t n, double* partial, hipStream_t st);
// grad_sumsq_pieces: the same sum over the pieces of `r` only (begin4 / start4 as the sweep reads them, slots ignored): a step that
// freezes segments takes the norm of the trainable ranges.  The pieces laid end to end are cut into one contiguous share per block on the
// host's layout alone (blocks = grad_norm_blocks(4 * start4[count])), every block adds its share in index order: the same bits on every run.
int grad_sumsq_pieces(const float* g, const AdamPieces& r, double* partial, unsigned* blocks, hipStream_t st);
struct ClipTables { AdamArgs* tab[2]; int count[2]; };
int grad_clip_finalize(const double* partial, unsigned blocks, const float* dyn, float max_norm, float grad_scale, float* out2,
                       const ClipTables& t, hipStream_t st);

// ------------------------------------------------------------------------------------------ step prologue (rowops.hip)
// Everything that changes from one optimizer step to the next, moved into device memory by ONE small launch so that the rest
// of the step can be a replayed hipGraph: the six batch tensors (gathered into the engine's fixed staging buffers), the
// dropout keys of every site for (seed, step) -- same derivation as make_key() on the host -- and the AdamW scalars of the
// two parameter groups (lr, bias-corrected step size, gradient scale), or of every update class of a classed step.
#define MB_PROLOGUE_MAX_COPIES 8
#define MB_LIVE_MAX_SAMPLES 8192
#define MB_LIVE_MAX_ROWS 65536
struct PrologueArgs {
    const uint32_t* src[MB_PROLOGUE_MAX_COPIES]; uint32_t* dst[MB_PROLOGUE_MAX_COPIES]; uint32_t dwords[MB_PROLOGUE_MAX_COPIES];
    int ncopies;
    uint64_t seed, step;
    uint32_t* keys; int nsites;            // keys[2 * site + {0, 1}]
    AdamArgs adam[2]; AdamArgs* adam_dst;  // may be null
    AdamArgs cls[MB_CLASSES_MAX]; AdamArgs* cls_dst; int ncls;      // update classes of a classed step: cls_dst[0 .. ncls) = cls, cls_dst[MB_CLASSES_MAX + c] = cls[c] with weight_decay 0 (2 * MB_CLASSES_MAX slots; may be null)
    float clip[2]; float* clip_dst;        // gradient-norm clipping: clip_dst[0 .. 1] = {max_norm, grad_scale} for grad_clip_finalize (may be null)
    uint32_t* zero_dw;                     // one dword cleared by the launch (the step's loss accumulator), may be null
    // modality tensors packed on the way in: src fp32 [rows][cols] (device or pinned host) -> dst [rows][pitch] of `dtype` (MAG's
    // GEMM operands; columns [cols, pitch) are never written and stay zero) -- what pack_pad does, without its two launches
    struct PackJob { const float* src; void* dst; int rows, cols, pitch, dtype; } pack[2];
    int npack;
    const int64_t* ids; int n_ids; int* id_count;     // id_count[ids[i]] += 1 (see embed_ln_backward), may be null
    // stamp[ids[i]] = stamp_no, the number of the optimizer update that will consume this batch's gradients, and stamp_state[0 .. 1] =
    // {stamp_no, stamp_on} for the sweep of that update (WordSkip above); never cleared, right under graph replay.  May be null
    // stamp_seen (0 or MB_STAMP_SEEN) is or-ed into every stamp stored, stamp_state[2] = stamp_lazy (the moment verdict)
    uint32_t* stamp; uint32_t* stamp_state; uint32_t stamp_no, stamp_on, stamp_seen, stamp_lazy;
    // the live token rows of this batch for the gathered weight gradients (GroupedGemmArgs::rows), built by ONE extra block from the
    // mask the launch gathers: live_rows[0 .. n) = the rows r < live_T (<= MB_LIVE_MAX_ROWS) with live_mask[r] != 0, the first row b * live_L
    // of EVERY sample (the [CLS] row the head reads: it carries a gradient whatever its mask word), and ALL rows of a sample (live_L
    // rows each, at most MB_LIVE_MAX_SAMPLES samples) that has no set mask word, ascending; entries [n, count) name a row
    // whose dY is zero -- the first dead row, else row live_T if live_T < live_Tp (the engine's zero pad rows) --; *live_count = count =
    // max(192, n rounded up to 64).  No such row: every row is live and live_T == live_Tp is a multiple of 64, count = max(192, n) and the
    // entries past n (n < 192 only) are never read by a launch that has K = live_Tp.  live_rows holds max(192, live_Tp) entries.  May be null
    uint32_t* live_rows; uint32_t* live_count; const int64_t* live_mask; int live_T, live_Tp, live_L;
    // cls_rows / cls_count (with live_rows; may be null): the rows b * live_L alone -- what the top layer's out-proj / ffn1 / ffn2 dY is
    // non-zero on --, padded with the same zero row to max(192, B rounded up to 64); a batch without a zero row gets the rows 0 .. T-1.
    // cls_rows holds as many entries as live_rows
    uint32_t* cls_rows; uint32_t* cls_count;
    // MAG's weights packed into the operands of its regrouped GEMMs (mag_pack.h) by EXTRA blocks of this launch, which is waiting for
    // PCIe anyway: the first `copy_blocks` blocks (filled by step_prologue) do everything above, the rest this.  W_hv == null: none
    struct MagPackW { const float* W_hv; const float* W_ha; const float* W_v; const float* W_a; void* We; void* Wv; void* Wa; MagDims d; int dtype; } magw;
    int copy_blocks;
};
static_assert(sizeof(PrologueArgs) <= 2048, "PrologueArgs travels as kernel arguments (4 KB limit)");
int step_prologue(const PrologueArgs& a, hipStream_t st);
// The proof behind WordSkip's state[2]: one wave per row of m / v[begin + row * row_len ...) (rows of row_len floats, multiples of 4,
// 16-byte aligned) sets or clears MB_STAMP_SEEN of stamp[row] -- set <=> any bit of the row's m or v is set -- and keeps the stamp's number.
// A row stamped `keep_no` is left as it is: a micro-step of the update still to come touched it, its moments are about to change.
int word_moments_scan(const float* m, const float* v, uint32_t* stamp, size_t begin, size_t rows, uint32_t row_len, uint32_t keep_no,
                      hipStream_t st);
// p[0, bytes) = 0 as a kernel launch (bytes and p multiples of 4); up to MB_ZERO_MAX ranges in one launch
#define MB_ZERO_MAX 8
struct ZeroRanges {
    uint32_t* p[MB_ZERO_MAX]; size_t ndw[MB_ZERO_MAX]; int n;
    void add(void* ptr, size_t bytes) { if (bytes && n < MB_ZERO_MAX) { p[n] = (uint32_t*)ptr; ndw[n] = bytes / 4; ++n; } }
    bool full() const { return n >= MB_ZERO_MAX; }      // callers that collect an unbounded number of ranges flush (zero_fill_ranges) and reset at this point
};
int zero_fill(void* p, size_t bytes, hipStream_t st);
int zero_fill_ranges(const ZeroRanges& z, hipStream_t st);

}  // namespace mb
