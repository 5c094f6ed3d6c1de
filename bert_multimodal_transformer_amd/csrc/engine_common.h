// Host-side helpers shared by the MAG-BERT and MAG-XLNet step executors (engine.hip, xlnet_engine.hip).
#pragma once
#include <string>
#include <vector>
#include <cstring>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include "kernels.h"
#include "../../include/magbert_hip.h"

using namespace mb;
static_assert(MB_UPDATE_CLASSES_MAX == MB_CLASSES_MAX && MB_UPDATE_SEGMENTS_MAX == MB_SEGMENTS_MAX, "public limits = the kernels' limits");

namespace {

struct TensorInfo {
    std::string name;
    size_t off, numel;
    int ndim;
    int64_t shape[4];
    int decay;
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// an environment switch, or `dflt` when it is not set (env_on: "0" turns it off, any other number on)
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
inline long env_long(const char* name, long dflt) { const char* v = getenv(name); return v ? atol(v) : dflt; }
inline bool env_on(const char* name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; }

inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

inline DropKey make_key(uint64_t seed, uint64_t step, uint32_t site, float p) {
    DropKey k;
    k.dyn = nullptr;
    if (!(p > 0.f)) { k.k0 = k.k1 = k.thresh = 0; k.scale = 1.f; return k; }
    const uint64_t h = splitmix64(splitmix64(seed) ^ splitmix64(step * 0x100000001B3ull + site));
    k.k0 = (uint32_t)h;
    k.k1 = (uint32_t)(h >> 32);
    double t = (double)p * 4294967296.0;
    if (t > 4294967295.0) t = 4294967295.0;
    k.thresh = (uint32_t)(t + 0.5);
    k.scale = 1.0f / (1.0f - p);
    return k;
}
const DropKey kNoDrop = {0u, 0u, 0u, 1.0f, nullptr};
inline DropKey dk(const mb_dropkey* d) {
    if (!d) return kNoDrop;
    DropKey k = {d->k0, d->k1, d->thresh, d->scale, nullptr};
    return k;
}

enum { SITE_EMB = 0, SITE_MAG = 1, SITE_HEAD = 2, SITE_LAYER0 = 16 };   // layer l: 16+4l+{0 attn probs,1 attn out,2 ffn out}

inline size_t esize(int dtype) { return dtype == DT_BF16 ? 2 : 4; }

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; }
};

// workspace of the MAG operator: saved activations + scratch (shared by the op-level API and the engine)
inline int mag_wgrad_tile() {
    static int t = -1;
    if (t < 0) { const char* v = getenv("MB_MAG_WGRAD_TILE"); t = (v && atoi(v) == 128) ? 128 : 64; }
    return t;
}

// ring depth of MAG's grouped weight-gradient launch (64 x 64 tiles only): MB_MAG_WGRAD_STAGES = 2 | 3 | 4 | 5
inline int mag_wgrad_stages() {        // (read per call -- capture time only -- so that a test can compare the variants in one process)
    const char* v = getenv("MB_MAG_WGRAD_STAGES");
    return v ? atoi(v) : 4;
}

struct MagWs {
    int Vp, Ap;
    size_t We, Wv, Wa, vp, ap, Ze, Zv, Za, mean, rstd;                       // forward (saved)
    size_t dZe, dZv, dZa, dep, dWe, dWv, dWa, dvp, dap;                      // backward scratch
    size_t bytes;
    void init(int dtype, int T_, int H, int V, int A) {
        const size_t es = esize(dtype);
        const size_t T = align_up((size_t)T_, 64);   // token rows padded to the GEMM k-tile (pad rows stay zero)
        // modality widths padded to the tile of the grouped weight-gradient launch: 64 -- three problems of 288 + 24 + 48 tiles whose
        // K = T loop of 38 stages is pure latency (35 us for 7 GFLOP).  MB_MAG_WGRAD_TILE=128 (72 + 12 + 12 tiles of 19 stages, one
        // per CU) was measured SLOWER: ~48 us in the kernel trace, +12 .. 28 us per step (profiles/r03_oneoffs_ab.txt)
        const int tile = mag_wgrad_tile();
        Vp = (V + tile - 1) / tile * tile;
        Ap = (A + tile - 1) / tile * tile;
        Carver c;
        We = c.take((size_t)2 * H * H * es); Wv = c.take((size_t)2 * H * Vp * es); Wa = c.take((size_t)2 * H * Ap * es);
        vp = c.take((size_t)T * Vp * es); ap = c.take((size_t)T * Ap * es);
        Ze = c.take((size_t)T * 2 * H * es); Zv = c.take((size_t)T * 2 * H * es); Za = c.take((size_t)T * 2 * H * es);
        mean = c.take((size_t)T * 4); rstd = c.take((size_t)T * 4);
        dZe = c.take((size_t)T * 2 * H * es); dZv = c.take((size_t)T * 2 * H * es); dZa = c.take((size_t)T * 2 * H * es);
        dep = c.take((size_t)T * H * es);
        dWe = c.take((size_t)2 * H * H * 4); dWv = c.take((size_t)2 * H * Vp * 4); dWa = c.take((size_t)2 * H * Ap * 4);
        dvp = c.take((size_t)T * Vp * 4); dap = c.take((size_t)T * Ap * 4);
        bytes = c.off;
    }
};

// the FFN1 forward launch of a configured activation (mb_*_config: 0 = gelu ... 4 = mish): erf-GELU keeps its own epilogue mode
inline int ffn_act_mode(int act) { return act == ACT_GELU ? EPI_BIAS_GELU : EPI_BIAS_ACT; }

#define CK(x) do { int _e = (x); if (_e) { mb::ck_trace(#x, __FILE__, __LINE__, _e); return _e; } } while (0)

inline int gemm(int dtype, int layout, int mode, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
         int ldc, void* C2, float* Cf, const float* bias, const void* R, int ldr, DropKey drop, int splits, int tile,
         hipStream_t st, int bseg = 0, size_t bseg_stride = 0, GradAcc acc = {}, int act = 0) {
    GemmArgs a = {};
    a.acc = acc;
    a.act = act;                                       // EPI_BIAS_ACT only
    a.bseg = bseg; a.bseg_stride = bseg_stride;        // segmented B (kernels.h): pieces of B's contiguous dimension in separate tensors
    a.A = A; a.B = B; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb;
    a.C = C; a.ldc = ldc; a.C2 = C2; a.Cf = Cf; a.bias = bias; a.R = R; a.ldr = ldr; a.alpha = 1.0f; a.drop = drop;
    a.kchunk = K; a.colsum = nullptr;
    if (mode == EPI_DGELU) { a.colsum = Cf; a.Cf = nullptr; }     // EPI_DGELU: the fp32 pointer carries the fused bias grad
    return gemm_launch(dtype, layout, mode, a, splits, tile, st);
}

// dX = dY . W + R (EPI_ADD_RES) or (dY . W) * gelu'(R) with the bias gradient `colsum` (EPI_DGELU), GEMM_NN: the plain launch, or -- when
// riders are active, the launch is one of the two kernels that leave block slots free (kernels.h gemm_nn_ride_tiles) and `take(budget,
// blocks)` hands out a piece of the optimizer update (kernels.h AdamRide) -- the same launch with rider workgroups behind its tiles.
// Budgets: what the free slots stream while the tiles multiply, by the launch's size: 1.25 M parameters next to 11.3 GFLOP for the 64 x 64
// kernel (the riders share SIMDs with the tiles: every instruction of theirs costs the partner wave an MFMA slot, so the gain is small and
// turns at ~1.5 M: same box 3.566 ms without | 3.544 at 1 - 1.5 M | 3.578 at 2.5 M per launch), 14,336 per free slot of the 128 x 128
// kernel (56 CUs that hold one tile instead of two)  (profiles/r06_adamw_ride_dgrad.txt)
inline long ride_pn_params() {       // MB_ADAMW_RIDE_PN_PARAMS: parameters per narrow dgrad launch on the 128 x 64 tile (0 = by the launch's size)
    static long v = -1;
    if (v < 0) { const char* e = getenv("MB_ADAMW_RIDE_PN_PARAMS"); v = e ? atol(e) : 0; }
    return v;
}
// The rider switches both engines have (kernels.h AdamRide).  MB_ADAMW_RIDE=0: no riders at all.  MB_ADAMW_RIDE_DGRAD >= 1: riders in the
// narrow dgrad launches of a layer, 2 (default): and in the ffn2 dgrad (EPI_DGELU); _DGRAD_PARAMS / _DGELU_PARAMS: parameters per such launch
// (0 = by the launch's size, below), _DGRAD_BLOCKS: rider workgroups (0 = every free slot).  MB_ADAMW_RIDE_ATTN: riders in the attention
// backward launches (_ATTN_BLOCKS, _ATTN_PARAMS: as above; the budgets are the engines').
struct RideOpts {
    int dgrad = 2, dgrad_blocks = 0; long dgrad_params = 0, dgelu_params = 0;
    int ride = 1, attn = 1, attn_blocks = 0; long attn_params = 0;
    void read_env() {
        ride = env_int("MB_ADAMW_RIDE", ride);
        dgrad = env_int("MB_ADAMW_RIDE_DGRAD", dgrad);
        dgrad_blocks = env_int("MB_ADAMW_RIDE_DGRAD_BLOCKS", dgrad_blocks);
        dgrad_params = env_long("MB_ADAMW_RIDE_DGRAD_PARAMS", dgrad_params);
        dgelu_params = env_long("MB_ADAMW_RIDE_DGELU_PARAMS", dgelu_params);
        attn = env_int("MB_ADAMW_RIDE_ATTN", attn);
        attn_blocks = env_int("MB_ADAMW_RIDE_ATTN_BLOCKS", attn_blocks);
        attn_params = env_long("MB_ADAMW_RIDE_ATTN_PARAMS", attn_params);
    }
};
template <class Take>
inline int dgrad_with_riders(int dt, int mode, int Mo, int No, int Ko, const void* dY, int ldy, const void* Wt, int ldw, void* dX, int ldx, const void* R,
                             int ldr, float* colsum, DropKey drop, GradAcc acc, hipStream_t st, bool active, const RideOpts& ro, int cus, Take&& take) {
    if (active && ro.dgrad && (mode == EPI_ADD_RES || ro.dgrad >= 2)) {
        GemmArgs a = {};
        a.A = dY; a.B = Wt; a.M = Mo; a.N = No; a.K = Ko; a.lda = ldy; a.ldb = ldw; a.C = dX; a.ldc = ldx; a.R = R; a.ldr = ldr;
        a.alpha = 1.0f; a.drop = drop; a.kchunk = Ko; a.colsum = colsum; a.acc = acc;
        int per_cu = 0;
        const int tiles = gemm_nn_ride_tiles(dt, mode, a, &per_cu);
        const int slots = per_cu * cus, rounds = tiles > 0 ? (tiles + slots - 1) / slots : 0;      // (the riders take what the LAST round leaves free)
        const int blocks = tiles > 0 ? (ro.dgrad_blocks > 0 ? ro.dgrad_blocks : rounds * slots - tiles) / 8 * 8 : 0;
        if (blocks >= 8) {
            size_t budget = ro.dgrad_params > 0 ? (size_t)ro.dgrad_params : (size_t)(1.25e6 * ((double)Mo * No * Ko) / (2400.0 * 768.0 * 3072.0)) / 1024 * 1024;
            if (mode == EPI_DGELU) budget = ro.dgelu_params > 0 ? (size_t)ro.dgelu_params : (size_t)blocks * 14336;
            // the 128 x 64 ping-pong tile (one per CU): the riders are whole idle CUs, ~41 GB/s each for the launch's duration
            else if (per_cu == 1) budget = ride_pn_params() > 0 ? (size_t)ride_pn_params() : (size_t)(blocks * 16384.0 * ((double)Mo * No * Ko) / (2400.0 * 768.0 * 3072.0)) / 1024 * 1024;
            // (16 K parameters per rider CU next to 11.3 GFLOP: more stretches the launch -- 26 K: +1 % per step, 40 K: +6 %; none at all: +0.4 %;
            //  profiles/r06_pn_default_ab.txt)
            const AdamRide r = take(budget, blocks);
            if (r.blocks) return gemm_nn_ride_launch(dt, mode, a, r, st);
        }
    }
    if (mode == EPI_DGELU)
        return gemm(dt, GEMM_NN, EPI_DGELU, Mo, No, Ko, dY, ldy, Wt, ldw, dX, ldx, nullptr, colsum, nullptr, R, ldr, drop, 1, 0, st, 0, 0, acc);
    return gemm(dt, GEMM_NN, EPI_ADD_RES, Mo, No, Ko, dY, ldy, Wt, ldw, dX, ldx, nullptr, nullptr, nullptr, R, ldr, drop, 1, 0, st);
}

// operands of one weight gradient dW[Mo][No] += dY[rows][Mo]^T X[rows][No] (GEMM_TN, EPI_ACCUM_F32)
inline GemmArgs wgrad_args(int Mo, int No, int rows, const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw) {
    GemmArgs a = {};
    a.A = dY; a.B = X; a.M = Mo; a.N = No; a.K = rows; a.lda = ldy; a.ldb = ldx;
    a.C = nullptr; a.ldc = ldw; a.C2 = nullptr; a.Cf = dW; a.bias = nullptr; a.colsum = nullptr; a.R = nullptr; a.ldr = 0;
    a.alpha = 1.0f; a.drop = kNoDrop; a.kchunk = rows; a.dbg = 0; a.reg_m = a.reg_n = a.tpr_m = a.tpr_n = 0;
    return a;
}

// wgrad: dW[N'][K'] += dY^T X, reduction over `rows` tokens; picks tile + split-K to fill the 256 CUs
inline int wgrad(int dtype, int Mo, int No, int rows, const void* dY, int ldy, const void* X, int ldx, float* dW, int ldw,
          hipStream_t st) {
    const long t128 = (long)((Mo + 127) / 128) * ((No + 127) / 128);
    const long t64 = (long)((Mo + 63) / 64) * ((No + 63) / 64);
    // split-K costs one fp32 atomic per output element per split (measured: 4.7 M atomics ~ 50 us), so it is used only
    // when the tile grid alone cannot occupy the chip
    int tile, splits;
    if (t128 >= 256) { tile = 128; splits = 1; }
    else if (t64 >= 100) { tile = 64; splits = 1; }        // measured: [768x3072] K=2432: 64^2 32 us vs 128^2 52 us
    else { tile = 64; splits = (int)((256 + t64 - 1) / t64); }
    if (splits > 8) splits = 8;
    while (splits > 1 && rows / splits < 128) --splits;
    if (splits < 1) splits = 1;
    (void)t128;
    return gemm(dtype, GEMM_TN, EPI_ACCUM_F32, Mo, No, rows, dY, ldy, X, ldx, nullptr, ldw, nullptr, dW, nullptr, nullptr, 0,
                kNoDrop, splits, tile, st);
}

// ------------------------------------------------------------------------------------------------ whole-step machinery
// Shared by both engines (mb_bert_train_step / mb_xlnet_train_step, mb_*_load_batch): everything that changes from one optimizer
// step to the next lives in the workspace -- staging buffers for the six batch tensors, the dropout keys of every site, the AdamW
// scalars of the two parameter groups -- written by ONE prologue launch; the rest of the step is a fixed kernel sequence that can
// be replayed as a hipGraph.
struct StepGraph {
    int B, L, with_opt, overwrite; const void *logits, *loss, *loss_run, *m, *v; float loss_scale; hipStream_t st;
    int nseg;                                       // the step as `nseg` linear graphs launched back to back (1 = the whole step)
    int variant;                                    // which segmentation (0 = the single-process step, else a hash of the data-parallel plan)
    const void* tag;                                // whose events the graphs' nodes record (the mb_comm of a data-parallel step), else null
    std::vector<hipGraph_t> graph; std::vector<hipGraphExec_t> exec;
    size_t ridden = 0, swept = 0; int segments = 0; // what the captured update covers (StepMixin::upd_*: a replay enqueues nothing on the host)
    size_t frozen = 0; int wgrad_skipped = 0, embed_skipped = 0;      // ... and what it left out (StepMixin::frz_*)
    int clip = 0;                                   // the update clips the gradient norm (StepMixin::clip_max > 0; the value is device data)
    void destroy() {
        for (auto x : exec) if (x) hipGraphExecDestroy(x);
        for (auto g : graph) if (g) hipGraphDestroy(g);
        exec.clear(); graph.clear();
    }
};

// one captured pass of a stage-driven (data-parallel) step: stage -1 = forward, 0 .. = backward stage
struct StageGraph { int B, L, stage, overwrite; const void *logits, *loss, *loss_run; float loss_scale; hipStream_t st; hipGraph_t graph; hipGraphExec_t exec; };

struct StepMixin {
    bool dyn = false;              // dropout keys / AdamW scalars are read from device memory (set while a train step is built)
    bool stage_mode = false;       // a stage-driven step is being built: every stage's gradients must be final when the stage returns
    std::vector<StageGraph> stage_graphs;
    // single-call step: the step prologue converts the two modality tensors straight into MAG's packed GEMM operands (set by the
    // engines: workspace offsets of the operands); `packed` tells mag_fwd_impl of the step that the pack_pad launches already happened
    bool pk_enable = false, packed = false;
    // ... and MAG's weight operands too (PrologueArgs::MagPackW, extra blocks of the same launch; the engines fill `pkw` when buffers are
    // bound): the first kernel of every replayed step used to be that pack.  MB_PROLOGUE_PACKW=0: back in the graph
    bool pkw_enable = false, packed_w = false;
    PrologueArgs::MagPackW pkw = {};
    size_t pk_vis = 0, pk_aco = 0; int pk_Vp = 0, pk_Ap = 0, pk_dtype = 0;
    // the switches both engines share through this mixin, read once by mb_*_create before the layout is built (which carves the
    // deterministic shadow).  MB_PROLOGUE_PACK=0: the step prologue stages the fp32 modality tensors and the forward packs them (two
    // more launches); the other four are described at their fields below
    void read_env() {
        ow_enable = env_int("MB_WGRAD_OVERWRITE", ow_enable);
        keep_enable = env_int("MB_ADAMW_KEEP", keep_enable);
        deterministic = env_int("MB_DETERMINISTIC", deterministic);
        pk_enable = env_on("MB_PROLOGUE_PACK", true);
        pkw_enable = env_on("MB_PROLOGUE_PACKW", true);
    }
    // single-call step: the prologue counts the occurrences of every token id (workspace offset of the table, 0 = none); `counted`
    // tells the engine's backward that the table describes the batch of this step
    size_t idcnt_off = 0; bool idcnt_enable = false, counted = false;
    // Live token rows (kernels.h PrologueArgs::live_rows; MB_WGRAD_LIVE_ROWS=0: off): the single-call step's prologue lists the rows of the
    // batch whose mask is set, and the layers' grouped weight gradients sum over those rows only (the dY row of a padding token is
    // exactly zero in every layer).  live_off: workspace offset of the list, live_cap entries, the count word behind them; 0 = the engine
    // carves none.  live_built: this step's prologue wrote the list (cleared with in_step).
    // live_mode (MB_WGRAD_LIVE_ROWS): 0 dense | 1 the live rows in every launch | 2 also the [CLS]-row list (PrologueArgs::cls_rows, a
    // second list of the same size behind the first) for the top layer's out-proj / ffn1 / ffn2 problems.  live_launches: gathered
    // weight-gradient launches the last single-call step enqueued (test hook).
    size_t live_off = 0, live_cap = 0; bool live_enable = false, live_built = false; int live_mode = 0, live_launches = 0;
    uint32_t* live_rows(char* ws) const { return (uint32_t*)(ws + live_off); }
    uint32_t* live_count(char* ws) const { return live_rows(ws) + live_cap; }
    uint32_t* cls_rows(char* ws) const { return live_rows(ws) + live_cap + 8; }
    uint32_t* cls_count(char* ws) const { return cls_rows(ws) + live_cap; }
    // Untouched word rows (kernels.h WordSkip; MB_ADAMW_SKIP_ZERO_ROWS=0: off).  stamp_off: workspace offset of the vocab-sized stamp table
    // followed by the three state words (0 = this engine has none); sweep_no: the number of the next optimizer update, counted on the host
    // (train_step_impl runs for every step, replayed or not), never 0, the table's initial value, and below MB_STAMP_SEEN.
    // stamp_live is the proof the sweep needs: "every word-row gradient was +0.0f at some point, and every backward since then belonged
    // to a single-call step whose prologue stamped its batch with sweep_no".  word_zero is the first half: set only by the engine's own
    // single-call step that ended with the optimizer (its sweep covers the word table and stores the zeros); a caller's claim
    // (mb_*_mark_grads_zero) is about the layers' weight gradients and is not taken for it.  A step that finds word_zero set starts a
    // window, gradient-accumulation micro-steps keep it, and everything else that may write gradients ends both: a backward outside
    // such a step, a stage-driven step, mb_*_mark_grads_zero(0), a newly bound buffer, a step that failed, mb_*_distrust_word_stamps
    // (the Python mirror: torch wrote into the buffer).  Without the proof the sweep reads every gradient, and proves it anew.
    size_t stamp_off = 0, stamp_rows = 0; bool stamp_enable = false, stamp_live = false, word_zero = false;
    uint32_t sweep_no = 1;
    size_t skip_updates = 0;       // updates enqueued with the proof in hand (mb_*_word_skip_updates: what the tests look at)
    // Zero moments (kernels.h WordSkip state[2], MB_STAMP_SEEN; MB_ADAMW_SKIP_ZERO_MOMENTS=0, or the switch above off: off).  mv_clean is
    // the proof the short path needs: "every word row without the seen mark holds +0.0f in m and v of the buffers (mv_m, mv_v)".  Only
    // word_moments_scan proves it -- the moments are the caller's buffers, a fresh optimizer's too -- and it stays true while every
    // update of the word table is a single-call one made with stamp_live: the prologue marks the rows of its batches, every other row
    // gets g = +0.0f, and zero moments stay zero.  Withdrawn by any other update that may write those moments (the first one of a
    // window, a data-parallel or stage-driven step, a failed step), by what withdraws stamp_live for buffer reasons (a newly bound
    // buffer, a change of frozen marks), by other moment buffers, and by mb_*_distrust_word_moments (the Python mirror: torch wrote
    // into m or v, or updated the range itself).  The scan runs in front of the prologue of a step that could use the verdict and
    // lacks only the proof, provided the previous update was a single-call one too (mv_prev_single): a caller that alternates paths
    // never pays a scan per step.  mv_updates / mv_scans: updates enqueued with the verdict set, scans enqueued (what the tests look at).
    bool mv_enable = false, mv_clean = false, mv_prev_single = false;
    const float* mv_m = nullptr; const float* mv_v = nullptr;
    size_t mv_updates = 0, mv_scans = 0;
    void distrust_word_moments() { mv_clean = false; }
    // the short path has the same bits: with g = m = v = +0.0f these scalars give m = v = +0.0f again and p - step_size * (0 / eps) == p
    // bit for bit (no NaN out of 0 * inf, no -0.0f out of a negative factor that would turn a p of -0.0f into +0.0f)
    static bool lazy_scalars_ok(const AdamArgs& a) {
        const float d = a.lr * a.weight_decay;
        return a.eps > 0.f && std::isfinite(a.step_size) && a.step_size >= 0.f && std::isfinite(d) && std::isfinite(a.beta1) && a.beta1 >= 0.f &&
               std::isfinite(a.beta2) && a.beta2 >= 0.f && std::isfinite(a.grad_scale) && a.grad_scale >= 0.f;
    }
    // ... in every slot that covers [b, e) -- the word table -- of this step's update (pa: the prologue's scalars, filled)
    bool lazy_slots_ok(const PrologueArgs& pa, size_t b, size_t e, size_t n_decay) const {
        if (n_classes == 0) return (b >= n_decay || lazy_scalars_ok(pa.adam[0])) && (e <= n_decay || lazy_scalars_ok(pa.adam[1]));
        for (size_t s = 0; s + 1 < seg_bounds.size(); ++s)
            if (seg_bounds[s] < e && seg_bounds[s + 1] > b && !lazy_scalars_ok(pa.cls[seg_class[s]])) return false;
        return true;
    }
    uint32_t* stamp_table(char* ws) const { return (uint32_t*)(ws + stamp_off); }
    uint32_t* stamp_state(char* ws) const { return stamp_table(ws) + stamp_rows; }
    // the unclassed end-of-step sweep as ONE launch over its up-to-three ranges (dp_step.h enqueue_update); false: one launch per range.
    // MAG-BERT: MB_ADAMW_ONE_SWEEP (default on); MAG-XLNet keeps its separate launches
    bool one_sweep = false;
    bool loss_cleared = false;     // single-call step: the step prologue clears the loss accumulator (no zero_fill launch in the forward)
    bool capturing = false;        // the stream is in capture mode: nothing outside the captured sequence may be waited for
    int nsites = 0;
    size_t ws_state = 0, ws_in_ids = 0, ws_in_seg = 0, ws_in_mask = 0, ws_in_vis = 0, ws_in_aco = 0, ws_in_lab = 0;
    std::vector<StepGraph> graphs;
    size_t graph_launches = 0, graph_captures = 0;
    // Captures run on a stream of the engine's own, never on the caller's: hipEventQuery on an event whose last record was on a
    // stream that is capturing NOW fails and invalidates that capture (ROCm 7.2: hipErrorCapturedEvent), and a host framework may
    // poll such events from another thread at any time -- PyTorch's NCCL watchdog does, for collectives it ran on the caller's
    // stream (found by the one-rank RCCL test: a race between its 100 ms poll and the first capture).  A graph is launch-stream
    // agnostic, so the captured sequence is replayed on the caller's stream as before.
    hipStream_t cap = nullptr;
    int capture_stream(hipStream_t* out) {
        if (!cap) CK((int)hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
        *out = cap;
        return MB_OK;
    }
    // Known-zero gradients.  The fused AdamW leaves the flat gradient buffer zeroed (optimizer.zero_grad()); when nothing has
    // written to it since, the layer weight gradients of the next backward are STORED instead of accumulated: the read half of
    // a 340 MB read-modify-write per step (28 MB per layer, straight from HBM: AdamW streamed the zeros out non-temporally).
    // grads_zero: set by a step that ran the optimizer and by mb_*_mark_grads_zero (the host zeroed the buffer itself);
    // consumed -- and cleared -- by the first stage of the next backward.  A false "known zero" is the only way this can go
    // wrong, so everything that is not the engine's own zeroing leaves it false.  MB_WGRAD_OVERWRITE=0 turns it off.
    bool grads_zero = false, ow_pass = false, in_step = false;
    int ow_enable = 1;
    // Lazy zeroing (round 3).  The zeros the fused AdamW writes over the layers' GEMM weight gradients (340 MB per step) are only
    // ever overwritten by the next backward, so a single-call step that ends with the optimizer leaves that range as it is:
    // "logically zero, physically stale" (grads_stale, [stale_begin, stale_end)).  Whoever else is about to look at it gets real
    // zeros first: a backward that accumulates (begin_backward_pass / train_step_impl), mb_*_materialize_grads (called by the
    // Python mirror before optimizer.step(), flat_grads, mark_grads_zero(False)).  MB_ADAMW_KEEP=0 turns it off.
    // deterministic mode (MB_DETERMINISTIC=1, common.h GradAcc): multi-writer gradient sums go to a 64-bit fixed-point shadow of
    // G[det_begin, n) in the workspace and are folded into the fp32 gradients at the end of the backward
    int deterministic = 0;
    size_t ws_det = 0, det_begin = 0, det_end = 0;
    GradAcc acc_of(char* ws, const float* G) const {
        GradAcc a = {nullptr, nullptr};
        if (deterministic && ws && G) { a.shadow = (long long*)(ws + ws_det) - det_begin; a.base = G; }
        return a;
    }
    int cus = 0;                                       // compute units of the current device (AdamRide: slots a grouped launch leaves empty)
    int cu_count() {
        if (cus <= 0) {
            int dev = 0, n = 0;
            if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) cus = n;
            if (cus <= 0) cus = 256;
        }
        return cus;
    }
    bool grads_stale = false, ow_covers = false;       // ow_covers: the overwriting (grouped) launch covers [stale_begin, stale_end)
    size_t stale_begin = 0, stale_end = 0;
    int keep_enable = 1;
    bool keep_in_step() const { return keep_enable && ow_enable && ow_covers && stale_end > stale_begin; }
    int materialize_grads(float* G, hipStream_t st) {
        if (grads_stale && G) CK(zero_fill(G + stale_begin, (stale_end - stale_begin) * sizeof(float), st));
        grads_stale = false;
        return MB_OK;
    }
    int begin_backward_pass(float* G, hipStream_t st) {
        if (in_step) return MB_OK;           // the single-call step decided already (and replays a graph captured for that decision)
        stamp_live = word_zero = false;      // a backward nobody stamped
        frz_dirty = true;                    // ... that computes every gradient, the frozen segments' too
        ow_pass = grads_zero && ow_enable;
        grads_zero = false;
        if (!(ow_pass && ow_covers)) CK(materialize_grads(G, st));      // this pass adds onto the range: it needs the zeros
        grads_stale = false;                 // (else: every layer stage of the pass stores its gradients over the stale values)
        return MB_OK;
    }

    // measurement hooks (bench.py): timing events around every grouped weight-gradient launch and around the optimizer launches
    // of a single-call step; steps run launch by launch while they are on (events cannot live inside a captured graph)
    bool prof = false;
    std::vector<hipEvent_t> pev;   // [2 * layers] grouped weight gradients, then [2] AdamW
    int prof_layers = 0;
    int set_profiling(int on, int layers) {
        if (on && pev.empty()) {
            prof_layers = layers;
            pev.assign((size_t)2 * layers + 2, nullptr);
            for (auto& ev : pev) CK((int)hipEventCreate(&ev));
        }
        prof = on != 0;
        return MB_OK;
    }
    int prof_mark(int idx, hipStream_t st) { return (prof && !capturing && idx < (int)pev.size()) ? (int)hipEventRecord(pev[idx], st) : 0; }
    int prof_span_us(int first, int pairs, float* avg_us) {
        if (!prof || !avg_us || pev.empty()) return MB_ERR_ARG;
        double sum = 0.0;
        for (int i = 0; i < pairs; ++i) {
            float ms = 0.f;
            CK((int)hipEventSynchronize(pev[first + 2 * i + 1]));
            CK((int)hipEventElapsedTime(&ms, pev[first + 2 * i], pev[first + 2 * i + 1]));
            sum += ms;
        }
        *avg_us = (float)(sum * 1e3 / pairs);
        return MB_OK;
    }
    void destroy_prof() { for (auto& ev : pev) if (ev) hipEventDestroy(ev); pev.clear(); }

    void carve_step(Carver& w, size_t Tpad, int V, int A, int max_batch, int num_labels, int nsites_) {
        nsites = nsites_;
        ws_state = w.take(2 * sizeof(AdamArgs) + (size_t)nsites * 8);
        ws_in_ids = w.take(Tpad * 8); ws_in_seg = w.take(Tpad * 8); ws_in_mask = w.take(Tpad * 8);
        ws_in_vis = w.take(Tpad * (size_t)V * 4); ws_in_aco = w.take(Tpad * (size_t)A * 4);
        ws_in_lab = w.take((size_t)max_batch * num_labels * 4);
    }
    void drop_graphs() {
        if (cap) { hipStreamDestroy(cap); cap = nullptr; }
        for (auto& g : graphs) g.destroy();
        graphs.clear();
        for (auto& g : stage_graphs) { hipGraphExecDestroy(g.exec); hipGraphDestroy(g.graph); }
        stage_graphs.clear();
    }
    // replay (capturing on first use) one pass of a stage-driven step; enqueue(st) issues its kernels with dyn keys
    template <class Enq>
    int run_stage_graph(int B, int L, int stage, int overwrite, const void* logits, const void* loss, const void* loss_run, float loss_scale,
                        int mode, hipStream_t st, Enq enqueue) {
        struct Scope { StepMixin* m; ~Scope() { m->dyn = false; m->capturing = false; m->in_step = false; m->stage_mode = false; } } scope{this};
        dyn = true; in_step = true; stage_mode = true;
        stamp_live = word_zero = false;      // (the stage-driven step's prologue stamps nothing)
        mv_clean = mv_prev_single = false;   // (and its update reads no seen mark)
        frz_dirty = true;                    // (and its backward ignores the frozen marks)
        if (mode == 2) return enqueue(st);
        StageGraph* g = nullptr;
        for (auto& x : stage_graphs)
            if (x.B == B && x.L == L && x.stage == stage && x.overwrite == overwrite && x.logits == logits && x.loss == loss && x.loss_run == loss_run &&
                x.loss_scale == loss_scale && x.st == st) { g = &x; break; }
        if (!g) {
            if (stage_graphs.size() >= 256) {
                hipGraphExecDestroy(stage_graphs.front().exec); hipGraphDestroy(stage_graphs.front().graph);
                stage_graphs.erase(stage_graphs.begin());
            }
            StageGraph ng = {B, L, stage, overwrite, logits, loss, loss_run, loss_scale, st, nullptr, nullptr};
            hipStream_t cs = nullptr;
            CK(capture_stream(&cs));
            CK((int)hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed));
            capturing = true;
            const int r = enqueue(cs);
            capturing = false;
            const int r2 = (int)hipStreamEndCapture(cs, &ng.graph);
            if (r) { if (ng.graph) hipGraphDestroy(ng.graph); return r; }
            CK(r2);
            CK((int)hipGraphInstantiate(&ng.exec, ng.graph, nullptr, nullptr, 0));
            stage_graphs.push_back(ng);
            g = &stage_graphs.back();
            ++graph_captures;
        }
        CK((int)hipGraphLaunch(g->exec, st));
        ++graph_launches;
        return MB_OK;
    }
    AdamArgs* adam_state(char* ws) const { return (AdamArgs*)(ws + ws_state); }
    // Update classes (kernels.h AdamPieces, include/magbert_hip.h mb_*_set_update_map).  n_classes == 0 -- the default -- is the step of the
    // two parameter groups: nothing below is looked at.  Otherwise the layout's update range [0, seg_bounds.back()) is cut into segments,
    // segment s = [seg_bounds[s], seg_bounds[s + 1]) belongs to class seg_class[s], and the step prologue writes the scalars of every class
    // (class_vals: what mb_*_set_update_values handed over) into a table of their own: device memory the engine allocates before the
    // first classed update and keeps until it is destroyed -- the workspace, whose size callers have planned with, stays as it was, and
    // so do the two slots of adam_state and the dropout keys behind them.  map_version joins the identity of a captured
    // graph: rider slices and sweep pieces are cut at the segment boundaries at capture time; the values never re-capture.
    // No-decay marks (mb_*_set_update_decay): seg_nodecay[s] != 0 -- segment s updates with its class's lr / betas / eps / bias correction
    // and weight_decay 0, so the decayed and the undecayed parameter group of one learning rate share a class.  The device table has two
    // halves for that: slot c is class c as handed over, slot MB_CLASSES_MAX + c the same scalars with weight_decay = 0 (the prologue
    // writes both from the one cls[c]); riders and sweep pieces of a marked segment read the upper slot, so no kernel looks at a mark.
    // The marks are part of the map's identity (map_version), and set_update_map clears them.
    // Frozen marks (mb_*_set_update_frozen): seg_frozen[s] != 0 -- no parameter group holds segment s.  Its parameters, shadow and moments
    // are never touched: the sweep emits no update piece for it and no rider slice reaches into it.  A single-call step (in_step &&
    // !stage_mode) also leaves out the launches whose whole output is frozen (the engines: a layer's grouped weight gradient, the word
    // scatter, MAG-BERT's embedding backward) and tells the mixin which ranges it therefore did not write (frz_unwritten); every other
    // frozen range was written by a fused kernel and gets a clear-only piece (kernels.h MB_PIECE_CLEAR) in the step's ONE sweep.
    // The explicit and the stage-driven passes ignore the marks and compute every gradient.  Invariant behind the skipped launches:
    // while marks are installed, the frozen ranges of G hold zeros whenever a single-call step begins -- frz_dirty says somebody
    // (an explicit backward, torch, a step from before the marks) may have written there, and train_step_impl clears them once,
    // outside any capture.  Like the no-decay marks they are part of map_version, and set_update_map clears them.
    struct ClassVals { float lr, beta1, beta2, eps, weight_decay; int correct_bias; };
    int n_classes = 0, map_version = 0;
    std::vector<size_t> seg_bounds;
    std::vector<int> seg_class;
    std::vector<uint8_t> seg_nodecay, seg_frozen;
    bool any_frozen = false, frz_dirty = true;
    std::vector<std::pair<size_t, size_t>> frz_unwritten;       // frozen ranges the step being enqueued does not write (ascending, disjoint)
    size_t ride_hopped = 0;                                     // frozen elements the rider cursor of the step being enqueued passed over
    size_t frz_elems = 0; int frz_wgrad_skipped = 0, frz_embed_skipped = 0;       // the last enqueued single-call step (mb_*_freeze_stats)
    std::vector<ClassVals> class_vals;
    AdamArgs* class_table = nullptr;
    size_t upd_ridden = 0, upd_swept = 0; int upd_segments = 0;       // the last enqueued update (mb_*_update_stats)
    int ensure_class_table() {          // (never inside a capture: train_step_impl calls it before the prologue)
        if (!class_table) {
            CK((int)hipMalloc((void**)&class_table, (size_t)2 * MB_CLASSES_MAX * sizeof(AdamArgs)));
            CK((int)hipMemset(class_table, 0, (size_t)2 * MB_CLASSES_MAX * sizeof(AdamArgs)));
        }
        return MB_OK;
    }
    void free_class_table() { if (class_table) { hipFree(class_table); class_table = nullptr; } }
    AdamArgs* class_state(char*) const { return class_table; }
    // Gradient-norm clipping (include/magbert_hip.h: mb_*_set_grad_clip; csrc/gradnorm.hip).  clip_max > 0: a step that ends with the
    // optimizer runs without riders, and between its backward and its sweep the norm of G[0, n_update_end) is taken and the coefficient
    // multiplied into the grad_scale of the tables the sweep reads (enqueue_clip).  clip_buf is device memory of the engine's own, like
    // class_table: {norm, coef} of the last update, {max_norm, grad_scale} as the step prologue deposits them, then the per-block partials.
    // On / off joins the identity of a captured graph (StepGraph::clip); the value never re-captures.
    float clip_max = 0.f;
    bool clip_step = false;        // the step being enqueued clips (set by train_step_impl: clip_max > 0 and m, v given)
    bool clip_ran = false;         // an update with clipping was enqueued since it was turned on
    char* clip_buf = nullptr; size_t clip_cap = 0;
    float* clip_record() const { return (float*)clip_buf; }
    float* clip_params() const { return (float*)clip_buf + 2; }
    double* clip_partials() const { return (double*)(clip_buf + 256); }
    int ensure_clip_buf(size_t n) {          // (never inside a capture: train_step_impl calls it before the prologue)
        const size_t need = 256 + (size_t)grad_norm_blocks(n) * sizeof(double);
        if (clip_buf && need > clip_cap) return MB_ERR_ARG;          // (n is the engine's update range: it never changes)
        if (!clip_buf) { CK((int)hipMalloc((void**)&clip_buf, need)); clip_cap = need; }
        return MB_OK;
    }
    void free_clip_buf() { if (clip_buf) { hipFree(clip_buf); clip_buf = nullptr; clip_cap = 0; } }
    int set_grad_clip(float max_norm) {
        const float v = (std::isfinite(max_norm) && max_norm > 0.f) ? max_norm : 0.f;
        if ((v > 0.f) != (clip_max > 0.f)) clip_ran = false;
        clip_max = v;
        return MB_OK;
    }
    int grad_clip_stats(float* norm, float* coef, hipStream_t st) const {
        if (!(clip_max > 0.f) || !clip_ran || !clip_buf) return MB_ERR_MODE;
        float rec[2] = {0.f, 0.f};
        CK((int)hipStreamSynchronize(st));
        CK((int)hipMemcpy(rec, clip_record(), sizeof rec, hipMemcpyDeviceToHost));
        if (norm) *norm = rec[0];
        if (coef) *coef = rec[1];
        return MB_OK;
    }
    // the two launches between the backward and the sweep of a clipping step: every gradient of G[0, n) is final
    int enqueue_clip(const float* G, size_t n, char* ws, hipStream_t st) {
        unsigned blocks = grad_norm_blocks(n);
        if (any_frozen) {
            // frozen segments: the norm of the trainable ranges only (their frozen neighbours hold what fused kernels wrote this step);
            // never more blocks than the full range has, so the partials fit where ensure_clip_buf put them
            AdamPieces tr;
            CK(sweep_pieces(tr, 0, n, n, n, false));
            CK(grad_sumsq_pieces(G, tr, clip_partials(), &blocks, st));
        } else
        CK(grad_sumsq(G, n, clip_partials(), st));
        // (both halves of the class table: slots [n_classes, MB_CLASSES_MAX) in between hold nothing anybody reads)
        ClipTables t = {{adam_state(ws), n_classes > 0 ? class_state(ws) : nullptr}, {2, n_classes > 0 ? MB_CLASSES_MAX + n_classes : 0}};
        return grad_clip_finalize(clip_partials(), blocks, clip_params(), 0.f, 1.f, clip_record(), t, st);
    }
    int set_update_map(const std::vector<TensorInfo>& tensors, size_t n_update_end, int nc, int ns, const size_t* bounds, const int* classes) {
        if (nc == 0) {          // back to the two parameter groups (graphs captured for them were never dropped)
            n_classes = 0; seg_bounds.clear(); seg_class.clear(); seg_nodecay.clear(); class_vals.clear();
            if (any_frozen) marks_changed();
            seg_frozen.clear(); any_frozen = false;
            return MB_OK;
        }
        if (nc < 0 || nc > MB_CLASSES_MAX || ns < 1 || ns > MB_SEGMENTS_MAX || !bounds || !classes) return MB_ERR_ARG;
        if (bounds[0] != 0 || bounds[ns] != n_update_end) return MB_ERR_SHAPE;
        for (int s = 0; s < ns; ++s) {
            if (bounds[s + 1] <= bounds[s]) return MB_ERR_SHAPE;
            if (classes[s] < 0 || classes[s] >= nc) return MB_ERR_ARG;
            bool at_tensor = false;
            for (const auto& t : tensors) if (t.off == bounds[s]) { at_tensor = true; break; }
            if (!at_tensor) return MB_ERR_SHAPE;
        }
        const bool same = nc == n_classes && (int)seg_class.size() == ns && std::equal(classes, classes + ns, seg_class.begin()) &&
                          std::equal(bounds, bounds + ns + 1, seg_bounds.begin());
        const bool marked = any_frozen || std::any_of(seg_nodecay.begin(), seg_nodecay.end(), [](uint8_t x) { return x != 0; });
        if (same && !marked) return MB_OK;
        if (any_frozen) marks_changed();
        if (!same) class_vals.clear();
        n_classes = nc; seg_bounds.assign(bounds, bounds + ns + 1); seg_class.assign(classes, classes + ns);
        seg_nodecay.assign((size_t)ns, 0);          // a map starts without marks: every segment decays as its class says
        seg_frozen.assign((size_t)ns, 0); any_frozen = false;
        if (++map_version <= 0) map_version = 1;
        return MB_OK;
    }
    int set_update_decay(int ns, const uint8_t* no_decay) {
        if (n_classes == 0) return MB_ERR_MODE;          // marks belong to a map
        if (ns != (int)seg_class.size() || !no_decay) return MB_ERR_ARG;
        bool same = true;
        for (int s = 0; s < ns; ++s) same = same && (no_decay[s] != 0) == (seg_nodecay[s] != 0);
        if (same) return MB_OK;
        for (int s = 0; s < ns; ++s) seg_nodecay[s] = no_decay[s] ? 1 : 0;
        if (++map_version <= 0) map_version = 1;
        return MB_OK;
    }
    // a change of frozen marks: what used to be frozen may hold anything a fused kernel wrote, what becomes frozen may hold a gradient --
    // the next single-call step clears the frozen ranges first; and the word-row stamps prove nothing about a table that was left out
    void marks_changed() { frz_dirty = true; stamp_live = word_zero = false; mv_clean = false; }
    int set_update_frozen(int ns, const uint8_t* frozen) {
        if (n_classes == 0) return MB_ERR_MODE;          // marks belong to a map
        if (ns != (int)seg_class.size() || !frozen) return MB_ERR_ARG;
        bool same = true;
        for (int s = 0; s < ns; ++s) same = same && (frozen[s] != 0) == (seg_frozen[s] != 0);
        if (same) return MB_OK;
        any_frozen = false;
        for (int s = 0; s < ns; ++s) { seg_frozen[s] = frozen[s] ? 1 : 0; any_frozen = any_frozen || frozen[s]; }
        marks_changed();
        if (++map_version <= 0) map_version = 1;
        return MB_OK;
    }
    int freeze_stats(size_t* frozen_elems, int* wgrad_launches_skipped, int* embed_skipped) const {
        if (frozen_elems) *frozen_elems = frz_elems;
        if (wgrad_launches_skipped) *wgrad_launches_skipped = frz_wgrad_skipped;
        if (embed_skipped) *embed_skipped = frz_embed_skipped;
        return MB_OK;
    }
    size_t frozen_total() const {
        size_t n = 0;
        for (size_t s = 0; s + 1 < seg_bounds.size(); ++s) if (seg_frozen[s]) n += seg_bounds[s + 1] - seg_bounds[s];
        return n;
    }
    // every element of [b, e) lies in a frozen segment
    bool range_frozen(size_t b, size_t e) const {
        if (!any_frozen || e <= b || seg_bounds.empty() || e > seg_bounds.back()) return false;
        size_t s = (size_t)(std::upper_bound(seg_bounds.begin(), seg_bounds.end(), b) - seg_bounds.begin()) - 1;
        for (; s + 1 < seg_bounds.size() && seg_bounds[s] < e; ++s) if (!seg_frozen[s]) return false;
        return true;
    }
    // the launches this step may leave out: a single-call step under frozen marks (the explicit and stage-driven passes compute everything)
    bool skipping() const { return any_frozen && in_step && !stage_mode; }
    bool unwritten(size_t b, size_t e) const {
        for (const auto& u : frz_unwritten) if (u.first <= b && e <= u.second) return true;
        return false;
    }
    // a single-call step is about to enqueue its backward: nothing noted, hopped or skipped yet (the engine's note_unwritten calls follow)
    void begin_step_marks() {
        frz_unwritten.clear(); ride_hopped = 0; frz_wgrad_skipped = frz_embed_skipped = 0;
        frz_elems = any_frozen ? frozen_total() : 0;
    }
    void note_unwritten(size_t b, size_t e) {
        if (e <= b) return;
        if (!frz_unwritten.empty() && frz_unwritten.back().second == b) frz_unwritten.back().second = e;
        else frz_unwritten.push_back({b, e});
        std::sort(frz_unwritten.begin(), frz_unwritten.end());
    }
    // zeros over the frozen ranges of G (never inside a capture: train_step_impl, before the prologue)
    int clear_frozen(float* G, hipStream_t st) {
        for (size_t s = 0; s + 1 < seg_bounds.size(); ++s)
            if (seg_frozen[s]) CK(zero_fill(G + seg_bounds[s], (seg_bounds[s + 1] - seg_bounds[s]) * sizeof(float), st));
        frz_dirty = false;
        return MB_OK;
    }
    // the slot of the device class table segment s reads: its class, or the class's weight_decay = 0 twin when the segment is marked
    int seg_slot(size_t s) const { return seg_class[s] + (seg_nodecay[s] ? MB_CLASSES_MAX : 0); }
    int set_update_values(int nc, const float* lr, const float* beta1, const float* beta2, const float* eps, const float* weight_decay,
                          const int* correct_bias) {
        if (nc < 1 || nc != n_classes || !lr || !beta1 || !beta2 || !eps || !weight_decay || !correct_bias) return MB_ERR_ARG;
        class_vals.resize((size_t)nc);
        for (int c = 0; c < nc; ++c) class_vals[c] = ClassVals{lr[c], beta1[c], beta2[c], eps[c], weight_decay[c], correct_bias[c]};
        return MB_OK;
    }
    int update_stats(size_t* ridden, size_t* swept, int* segments) const {
        if (ridden) *ridden = upd_ridden;
        if (swept) *swept = upd_swept;
        if (segments) *segments = upd_segments;
        return MB_OK;
    }
    // riders of a classed step: a slice that ends at element `top` (exclusive) may reach down to the start of the segment that holds
    // top - 1, and reads that segment's slot of the class table
    // A frozen segment under the cursor: when the step does not write it (frz_unwritten) the cursor hops over it, down to `limit` at
    // most (what is final for this host), and the elements count as frozen, not ridden; otherwise the ride ends here -- the sweep owes
    // that range a clear-only piece.  False: nothing to take.
    bool ride_segment(size_t& cursor, size_t limit, size_t* floor, int* cls) {
        while (cursor > limit) {
            const size_t s = (size_t)(std::upper_bound(seg_bounds.begin(), seg_bounds.end(), cursor - 1) - seg_bounds.begin()) - 1;
            if (!seg_frozen[s]) { *floor = seg_bounds[s]; *cls = seg_slot(s); return true; }
            const size_t lo = std::max(seg_bounds[s], limit);
            if (!unwritten(lo, cursor)) return false;
            ride_hopped += cursor - lo; cursor = lo;
        }
        return false;
    }
    // the sweep of a classed step: [b0, e0) and [b1, e1) (ascending, disjoint) cut at the segment boundaries, every piece with its
    // segment's slot of the class table
    int sweep_pieces(AdamPieces& out, size_t b0, size_t e0, size_t b1, size_t e1, bool clear = true, size_t keep_b = 0, size_t keep_e = 0) const {
        std::vector<int> slots(seg_class.size());
        for (size_t s = 0; s < slots.size(); ++s) slots[s] = seg_slot(s);
        return cut_pieces(out, seg_bounds, slots.data(), seg_frozen.empty() ? nullptr : seg_frozen.data(), b0, e0, b1, e1, clear, keep_b, keep_e);
    }
    // The piece table of a sweep (kernels.h AdamPieces): [b0, e0) and [b1, e1) (ascending, disjoint) cut at `bounds`, the part inside
    // [bounds[s], bounds[s + 1]) with slot[s].  An unclassed step cuts at {0, n_decay, n} with slots {0, 1} of adam_state.
    // frozen (null: none): a frozen segment gets no update piece.  clear: what the step's backward wrote of it (everything but
    // frz_unwritten and the keep range [keep_b, keep_e), which stays "logically zero, physically stale" like its trainable neighbours)
    // gets clear-only pieces, which lie behind every update piece of the table (kernels.h AdamPieces::clear_first).
    int cut_pieces(AdamPieces& out, const std::vector<size_t>& bounds, const int* slot, const uint8_t* frozen, size_t b0, size_t e0, size_t b1,
                   size_t e1, bool clear = true, size_t keep_b = 0, size_t keep_e = 0) const {
        out = AdamPieces{};
        const size_t rb[2] = {b0, b1}, re[2] = {e0, e1};
        struct Piece { size_t lo, hi; int slot; };
        std::vector<Piece> upd, clr;
        for (int r = 0; r < 2; ++r)
            for (size_t s = 0; s + 1 < bounds.size(); ++s) {
                const size_t lo = std::max(rb[r], bounds[s]), hi = std::min(re[r], bounds[s + 1]);
                if (lo >= hi) continue;
                if (!frozen || !frozen[s]) { upd.push_back({lo, hi, slot[s]}); continue; }
                if (!clear) continue;
                // [lo, hi) minus the ranges nobody wrote
                std::vector<std::pair<size_t, size_t>> holes = frz_unwritten;
                if (keep_e > keep_b) holes.push_back({keep_b, keep_e});
                std::sort(holes.begin(), holes.end());
                size_t at = lo;
                for (const auto& h : holes) {
                    if (h.second <= at || h.first >= hi) continue;
                    if (h.first > at) clr.push_back({at, h.first, MB_PIECE_CLEAR});
                    at = std::max(at, std::min(h.second, hi));
                }
                if (at < hi) clr.push_back({at, hi, MB_PIECE_CLEAR});
            }
        // (holes that do not fit the table: the two clear pieces -- ascending, disjoint -- with the smallest gap between them become one;
        //  zeros over zeros, or, in the keep range, over values nobody reads)
        while (upd.size() + clr.size() > (size_t)MB_SWEEP_PIECES_MAX && clr.size() > 1) {
            size_t best = 1;
            for (size_t k = 2; k < clr.size(); ++k)
                if (clr[k].lo - clr[k - 1].hi < clr[best].lo - clr[best - 1].hi) best = k;
            clr[best - 1].hi = clr[best].hi;
            clr.erase(clr.begin() + (long)best);
        }
        if (upd.size() + clr.size() > (size_t)MB_SWEEP_PIECES_MAX) return MB_ERR_ARG;
        size_t total4 = 0;
        auto emit = [&](const Piece& pc) {
            if ((pc.lo | pc.hi) % 4 || pc.hi / 4 > 0xffffffffull || total4 + (pc.hi - pc.lo) / 4 > 0xffffffffull) return (int)MB_ERR_SHAPE;
            out.begin4[out.count] = (uint32_t)(pc.lo / 4); out.start4[out.count] = (uint32_t)total4; out.slot[out.count] = (uint8_t)pc.slot;
            total4 += (pc.hi - pc.lo) / 4;
            out.start4[++out.count] = (uint32_t)total4;
            return (int)MB_OK;
        };
        for (const Piece& pc : upd) CK(emit(pc));
        out.clear_first = out.count;
        for (const Piece& pc : clr) CK(emit(pc));
        return MB_OK;
    }
    uint32_t* key_state(char* ws) const { return (uint32_t*)(ws + ws_state + 2 * sizeof(AdamArgs)); }
    DropKey step_key(char* ws, bool training, uint64_t seed, uint64_t step, uint32_t site, float p) const {
        if (!training) return kNoDrop;
        if (!dyn) return make_key(seed, step, site, p);
        DropKey k = make_key(0, 0, site, p);          // thresh / scale of this site; (k0, k1) come from the device table
        if (k.thresh) { k.k0 = k.k1 = 0u; k.dyn = key_state(ws) + 2 * (size_t)site; }
        return k;
    }
    void fill_copies(PrologueArgs& pa, char* ws, const void* ids, const void* vis, const void* aco, const void* mask, const void* seg,
                     const void* lab, int B, int L, int V, int A, int num_labels, bool pack_modalities = false) const {
        const size_t T = (size_t)B * L;
        auto cp = [&](const void* src, size_t off, size_t bytes) {
            pa.src[pa.ncopies] = (const uint32_t*)src; pa.dst[pa.ncopies] = (uint32_t*)(ws + off); pa.dwords[pa.ncopies] = (uint32_t)(bytes / 4);
            ++pa.ncopies;
        };
        cp(ids, ws_in_ids, T * 8); cp(seg, ws_in_seg, T * 8); cp(mask, ws_in_mask, T * 8);
        if (pack_modalities) {
            pa.pack[0] = {(const float*)vis, ws + pk_vis, (int)T, V, pk_Vp, pk_dtype};
            pa.pack[1] = {(const float*)aco, ws + pk_aco, (int)T, A, pk_Ap, pk_dtype};
            pa.npack = 2;
        } else {
            cp(vis, ws_in_vis, T * V * 4); cp(aco, ws_in_aco, T * A * 4);
        }
        // one float per sample -- the regression target (num_labels == 1) or the class index -- or, under a per-element loss, one per logit
        if (lab) cp(lab, ws_in_lab, label_floats(B, num_labels) * 4);
    }
    // The head's objective (kernels.h HeadLoss; include/magbert_hip.h: mb_*_set_head_loss).  Sticky, legal between steps, checked before
    // any device call.  kind and scalar are kernel arguments, baked into every captured graph that holds a head launch: a change drops the
    // engine's graphs (the next step captures again).  The vector lives in device memory of the engine's own, like class_table -- never
    // the workspace -- and is uploaded by the first pass after the setter, outside any capture (sync_head_loss).
    // The options of mb_head_loss (smoothing, focal gamma, ignored label) are kernel arguments like the kind; set_head_loss clears them.
    int loss_kind = HL_DEFAULT; float loss_param = 0.f;
    float loss_smoothing = 0.f, loss_gamma = 0.f; int loss_ignore = 0, loss_has_ignore = 0;
    std::vector<float> loss_vec;             // host copy (empty = none)
    float* loss_vec_dev = nullptr; size_t loss_vec_cap = 0; bool loss_vec_dirty = false;
    size_t label_floats(int B, int num_labels) const { return (size_t)B * (head_loss_per_element(loss_kind) ? num_labels : 1); }
    HeadLoss head_loss() const {
        return HeadLoss{loss_kind, loss_param, loss_vec.empty() ? nullptr : loss_vec_dev, loss_smoothing, loss_gamma, loss_ignore, loss_has_ignore};
    }
    int set_head_loss(int kind, float param, const float* vec, int num_labels) {
        return set_head_loss_ex(mb_head_loss{kind, param, vec, 0.f, 0.f, 0, 0}, num_labels);
    }
    int set_head_loss_ex(const mb_head_loss& in, int num_labels) {
        const int kind = in.kind; float param = in.param; const float* vec = in.vec;
        const int has_ignore = in.has_ignore_index ? 1 : 0, ignore = has_ignore ? in.ignore_index : 0;
        if (!head_loss_legal(HeadLoss{kind, param, nullptr, in.label_smoothing, in.focal_gamma, ignore, has_ignore}, num_labels)) return MB_ERR_ARG;
        if (kind < HL_DEFAULT || kind > HL_CE) return MB_ERR_ARG;
        if (kind == HL_CE && num_labels < 2) return MB_ERR_ARG;
        if (kind == HL_SMOOTH_L1 && !(std::isfinite(param) && param >= 0.f)) return MB_ERR_ARG;
        const bool takes_vec = kind == HL_BCE || kind == HL_CE;
        if (vec && !takes_vec) return MB_ERR_ARG;
        if (vec) {
            bool any = false;
            for (int k = 0; k < num_labels; ++k) {
                if (!(std::isfinite(vec[k]) && vec[k] >= 0.f)) return MB_ERR_ARG;
                any = any || vec[k] > 0.f;
            }
            if (!any) return MB_ERR_ARG;
        }
        if (kind != HL_SMOOTH_L1) param = 0.f;
        std::vector<float> nv;
        if (vec) nv.assign(vec, vec + num_labels);
        if (kind == loss_kind && param == loss_param && nv == loss_vec && in.label_smoothing == loss_smoothing && in.focal_gamma == loss_gamma &&
            has_ignore == loss_has_ignore && ignore == loss_ignore) return MB_OK;
        // graphs in flight read the old arguments (and the old vector): wait for them before they go
        if (!graphs.empty() || !stage_graphs.empty()) { CK((int)hipDeviceSynchronize()); drop_graphs(); }
        loss_kind = kind; loss_param = param;
        loss_smoothing = in.label_smoothing; loss_gamma = in.focal_gamma; loss_has_ignore = has_ignore; loss_ignore = ignore;
        loss_vec_dirty = loss_vec_dirty || nv != loss_vec;
        loss_vec.swap(nv);
        return MB_OK;
    }
    int get_head_loss(int* kind, float* param, float* vec, int* has_vec) const {
        if (kind) *kind = loss_kind;
        if (param) *param = loss_param;
        if (has_vec) *has_vec = loss_vec.empty() ? 0 : 1;
        if (vec) std::copy(loss_vec.begin(), loss_vec.end(), vec);
        return MB_OK;
    }
    int get_head_loss_ex(mb_head_loss* hl, float* vec, int* has_vec) const {
        if (hl) *hl = mb_head_loss{loss_kind, loss_param, nullptr, loss_smoothing, loss_gamma, loss_has_ignore, loss_ignore};
        return get_head_loss(nullptr, nullptr, vec, has_vec);
    }
    // the vector on the device before a head launch reads it (never inside a capture: the passes call it before they enqueue)
    int sync_head_loss() {
        if (!loss_vec_dirty || capturing) return MB_OK;
        if (!loss_vec.empty()) {
            if (loss_vec_cap < loss_vec.size()) {
                if (loss_vec_dev) { CK((int)hipDeviceSynchronize()); hipFree(loss_vec_dev); loss_vec_dev = nullptr; loss_vec_cap = 0; }
                CK((int)hipMalloc((void**)&loss_vec_dev, loss_vec.size() * sizeof(float)));
                loss_vec_cap = loss_vec.size();
            }
            CK((int)hipDeviceSynchronize());            // launches already enqueued, on whichever stream, read the old values
            CK((int)hipMemcpy(loss_vec_dev, loss_vec.data(), loss_vec.size() * sizeof(float), hipMemcpyHostToDevice));
        }
        loss_vec_dirty = false;
        return MB_OK;
    }
    void free_head_loss() { if (loss_vec_dev) { hipFree(loss_vec_dev); loss_vec_dev = nullptr; loss_vec_cap = 0; } }
    void staged(char* ws, bool with_labels, const void** six) const {
        six[0] = ws + ws_in_ids; six[1] = ws + ws_in_vis; six[2] = ws + ws_in_aco; six[3] = ws + ws_in_mask; six[4] = ws + ws_in_seg;
        six[5] = with_labels ? ws + ws_in_lab : nullptr;
    }
};

// enqueue(logits, loss, loss_run, m, v, loss_scale, st): forward (reading the staged batch) + backward + AdamW of one engine
struct NoBetween { int operator()(int, hipStream_t) const { return MB_OK; } };
template <class E, class Enqueue, class Between = NoBetween>
inline int train_step_impl(E* e, char* ws, int V, int A, int num_labels, const void* ids, const void* vis, const void* aco, const void* mask,
                           const void* seg, const void* labels, int B, int L, uint64_t seed, uint64_t step, float* logits, float* loss,
                           float* loss_run, float* m, float* v, float lr, float beta1, float beta2, float eps, float weight_decay,
                           int opt_step, int correct_bias, float grad_scale, float loss_scale, int mode, bool force_launches,
                           hipStream_t st, Enqueue enqueue_inner, int nseg = 1, Between between = Between(), int variant = 0,
                           const void* tag = nullptr, int (*verify)(const void* tag, int nseg, int sg, hipGraph_t gr) = nullptr) {
    if (m && e->n_classes > 0 && (int)e->class_vals.size() != e->n_classes) return MB_ERR_ARG;      // a map without this step's values
    // (a micro-step without the optimizer enqueues the same kernels under any map; data-parallel variants are positive, and refuse a map)
    if (m && e->n_classes > 0 && variant == 0) variant = -e->map_version;
    // (... except under frozen marks: every single-call step then leaves launches out, the micro-steps of an accumulation window too)
    if (e->any_frozen && variant > 0) return MB_ERR_MODE;
    if (e->any_frozen && variant == 0) variant = -e->map_version;
    e->upd_ridden = e->upd_swept = 0; e->upd_segments = 0;
    e->live_launches = 0;
    e->frz_elems = 0; e->frz_wgrad_skipped = e->frz_embed_skipped = 0;
    if (e->any_frozen && e->frz_dirty) CK(e->clear_frozen(e->G, st));
    if (m && e->n_classes > 0) CK(e->ensure_class_table());
    CK(e->sync_head_loss());
    const bool clip = m && e->clip_max > 0.f;
    if (clip && variant > 0) return MB_ERR_MODE;          // (the data-parallel steps refuse before they get here)
    if (clip) CK(e->ensure_clip_buf(e->n_update_end()));
    // The step may be cut into `nseg` segments: enqueue_inner(seg, ...) issues the kernels of one (captured and replayed as its own
    // LINEAR graph), between(seg, st) runs on the host right after segment `seg` was enqueued and is never captured -- the place for
    // cross-stream events (a graph with a fork inside runs on ROCm 7.2's slow path; a chain of linear graphs does not).
    // what this step's backward may assume about the gradient buffer -- part of the graph's identity -- and what it leaves behind
    const int ow = (e->grads_zero && e->ow_enable) ? 1 : 0;
    if (!(ow && e->ow_covers)) CK(e->materialize_grads(e->G, st));      // an accumulating backward needs the zeros that were skipped
    const bool stale_before = e->grads_stale;
    // what the step leaves behind is only known once everything was enqueued: an early error return leaves "nothing known"
    struct Flags {
        E* e; bool ok, with_opt, stale_before, single, lazy;
        ~Flags() {
            e->in_step = false; e->loss_cleared = false; e->packed = false; e->packed_w = false; e->counted = false; e->live_built = false;
            if (ok && e->clip_step) e->clip_ran = true;
            e->clip_step = false;
            e->grads_zero = ok && with_opt;
            e->grads_stale = ok ? (with_opt && e->keep_in_step()) : stale_before;
            // an update was enqueued: its sweep left every word gradient zero, and the next batch is stamped with the next number
            if (ok && with_opt && e->stamp_live) ++e->skip_updates;
            // ... and the zero moments of unmarked word rows zero only if it was a single-call update with that proof (StepMixin::mv_clean)
            if (!ok || (with_opt && !(e->stamp_live && single))) e->mv_clean = false;
            if (ok && with_opt && lazy) ++e->mv_updates;
            if (with_opt) e->mv_prev_single = ok && single;
            if (!ok || with_opt) e->stamp_live = false;
            e->word_zero = ok && with_opt;
            if (ok && with_opt && ++e->sweep_no >= MB_STAMP_SEEN) e->sweep_no = 1u;      // (the top bit of a stamp word is the seen mark)
        }
    } flags{e, false, m != nullptr, stale_before, variant <= 0, false};
    // untouched word rows (StepMixin::stamp_live): this step's prologue stamps its batch, so a window that is live stays live, and
    // word gradients the engine itself left all zero open one
    // (frozen marks: a step without an embedding backward has nobody to consume -- and clear -- the count table, and no sweep piece over
    //  the word table for stamps to guide)
    const bool no_embed = e->any_frozen && e->embed_all_frozen();
    const bool stamping = e->stamp_off != 0 && e->stamp_enable && e->idcnt_enable && ids != nullptr && !no_embed;
    if (!stamping) e->stamp_live = false;
    else if (e->word_zero) e->stamp_live = true;
    e->word_zero = false;                   // (this step's backward writes some of them)
    e->in_step = true; e->ow_pass = ow != 0; e->clip_step = clip;
    auto enqueue = [&](int sg, float* lg, float* ls, float* lr_, float* m_, float* v_, float sc, hipStream_t s) {
        return enqueue_inner(sg, lg, ls, lr_, m_, v_, sc, s);
    };
    PrologueArgs pa = {};
    e->fill_copies(pa, ws, ids, vis, aco, mask, seg, labels, B, L, V, A, num_labels, e->pk_enable);
    e->packed = e->pk_enable;
    if (e->pkw_enable && e->pkw.W_hv) pa.magw = e->pkw;
    e->packed_w = pa.magw.W_hv != nullptr;
    pa.seed = seed; pa.step = step; pa.keys = e->key_state(ws); pa.nsites = e->nsites;
    pa.zero_dw = (uint32_t*)loss; e->loss_cleared = loss != nullptr;
    if (e->idcnt_enable && ids && !no_embed) { pa.ids = (const int64_t*)ids; pa.n_ids = B * L; pa.id_count = (int*)(ws + e->idcnt_off); }
    e->counted = pa.id_count != nullptr;
    if (stamping) { pa.stamp = e->stamp_table(ws); pa.stamp_state = e->stamp_state(ws); pa.stamp_no = e->sweep_no; pa.stamp_on = e->stamp_live ? 1u : 0u; }
    if (stamping && e->mv_enable) pa.stamp_seen = MB_STAMP_SEEN;
    // live token rows for the weight gradients (not the data-parallel variants: they stay dense)
    if (e->live_off != 0 && e->live_enable && variant <= 0 && mask != nullptr && (size_t)align_up((size_t)B * L, 64) <= e->live_cap &&
        B <= MB_LIVE_MAX_SAMPLES && B * L <= MB_LIVE_MAX_ROWS) {
        pa.live_rows = e->live_rows(ws); pa.live_count = e->live_count(ws); pa.live_mask = (const int64_t*)mask;
        pa.live_T = B * L; pa.live_Tp = (int)align_up((size_t)B * L, 64); pa.live_L = L;
        if (e->live_mode >= 2) { pa.cls_rows = e->cls_rows(ws); pa.cls_count = e->cls_count(ws); }
        e->live_built = true;
    }
    if (m) {
        double ss = lr;
        if (correct_bias) ss = (double)lr * sqrt(1.0 - pow((double)beta2, (double)opt_step)) / (1.0 - pow((double)beta1, (double)opt_step));
        AdamArgs a;
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.step_size = (float)ss;
        a.grad_scale = grad_scale;
        pa.adam[0] = a;
        a.weight_decay = 0.f;
        pa.adam[1] = a;
        pa.adam_dst = e->adam_state(ws);
        for (int c = 0; c < e->n_classes; ++c) {          // classed step: every class's scalars, derived the same way
            const auto& cv = e->class_vals[c];
            double cs = cv.lr;
            if (cv.correct_bias) cs = (double)cv.lr * sqrt(1.0 - pow((double)cv.beta2, (double)opt_step)) / (1.0 - pow((double)cv.beta1, (double)opt_step));
            AdamArgs k;
            k.lr = cv.lr; k.beta1 = cv.beta1; k.beta2 = cv.beta2; k.eps = cv.eps; k.weight_decay = cv.weight_decay; k.step_size = (float)cs;
            k.grad_scale = grad_scale;
            pa.cls[c] = k;
        }
        if (e->n_classes > 0) { pa.ncls = e->n_classes; pa.cls_dst = e->class_state(ws); }
        if (clip) { pa.clip[0] = e->clip_max; pa.clip[1] = grad_scale; pa.clip_dst = e->clip_params(); }
    }
    // zero moments (StepMixin::mv_clean): the verdict of this step's sweep, and the scan that proves it where only the proof is missing
    // (on the step's stream in front of the prologue, which marks this batch's rows; never captured).  A clipping step reads every
    // moment -- its grad_scale is a device value -- and keeps the proof; a frozen word table has no update piece to shorten.
    if (m && v && (m != e->mv_m || v != e->mv_v)) { e->mv_clean = false; e->mv_m = m; e->mv_v = v; }
    if (m && v && e->mv_enable && stamping && e->stamp_live && variant <= 0 && !clip) {
        const WordSkip wsk = e->word_skip(ws);
        if (wsk.stamp && wsk.end > wsk.begin && !e->range_frozen(wsk.begin, wsk.end) && e->lazy_slots_ok(pa, wsk.begin, wsk.end, e->n_decay)) {
            if (!e->mv_clean && e->mv_prev_single) {
                CK(word_moments_scan(m, v, e->stamp_table(ws), wsk.begin, (wsk.end - wsk.begin) / wsk.row_len, wsk.row_len, e->sweep_no, st));
                e->mv_clean = true; ++e->mv_scans;
            }
            flags.lazy = e->mv_clean;
        }
    }
    pa.stamp_lazy = flags.lazy ? 1u : 0u;
    CK(step_prologue(pa, st));
    if (mode == 2 || force_launches) {
        e->dyn = true;
        int r = MB_OK;
        for (int sg = 0; sg < nseg && r == MB_OK; ++sg) {
            r = enqueue(sg, logits, loss, loss_run, m, v, loss_scale, st);
            if (r == MB_OK) r = between(sg, st);
        }
        e->dyn = false;
        flags.ok = r == MB_OK;
        return r;
    }
    StepGraph* g = nullptr;
    for (auto& x : e->graphs)
        if (x.B == B && x.L == L && x.with_opt == (m != nullptr) && x.overwrite == ow && x.logits == logits && x.loss == loss && x.loss_run == loss_run &&
            x.m == m && x.v == v && x.loss_scale == loss_scale && x.st == st && x.nseg == nseg && x.variant == variant && x.tag == tag &&
            x.clip == (clip ? 1 : 0)) { g = &x; break; }
    if (!g) {
        if (e->graphs.size() >= 32) {          // callers that keep changing output pointers: do not grow without bound
            e->graphs.front().destroy();
            e->graphs.erase(e->graphs.begin());
        }
        StepGraph ng = {B, L, m != nullptr, ow, logits, loss, loss_run, m, v, loss_scale, st, nseg, variant, tag, {}, {}};
        ng.clip = clip ? 1 : 0;
        hipStream_t cs = nullptr;
        CK(e->capture_stream(&cs));
        for (int sg = 0; sg < nseg; ++sg) {
            hipGraph_t gr = nullptr;
            hipGraphExec_t ex = nullptr;
            CK((int)hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed));
            e->dyn = true; e->capturing = true;
            const int r = enqueue(sg, logits, loss, loss_run, m, v, loss_scale, cs);
            e->dyn = false; e->capturing = false;
            const int r2 = (int)hipStreamEndCapture(cs, &gr);
            if (r || r2) { mb::ck_trace(r ? "enqueue(segment) inside the capture" : "hipStreamEndCapture", __FILE__, __LINE__, r ? r : r2);
                           if (gr) hipGraphDestroy(gr); ng.destroy(); return r ? r : r2; }
            if (verify) { const int rv = verify(tag, nseg, sg, gr); if (rv) { mb::ck_trace("finish(segment graph)", __FILE__, __LINE__, rv); hipGraphDestroy(gr); ng.destroy(); return rv; } }
            const int r3 = (int)hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0);
            if (r3) { mb::ck_trace("hipGraphInstantiate", __FILE__, __LINE__, r3); hipGraphDestroy(gr); ng.destroy(); return r3; }
            ng.graph.push_back(gr); ng.exec.push_back(ex);
        }
        ng.ridden = e->upd_ridden; ng.swept = e->upd_swept; ng.segments = e->upd_segments;
        ng.frozen = e->frz_elems; ng.wgrad_skipped = e->frz_wgrad_skipped; ng.embed_skipped = e->frz_embed_skipped;
        e->graphs.push_back(ng);
        g = &e->graphs.back();
        ++e->graph_captures;
    }
    for (int sg = 0; sg < nseg; ++sg) {
        CK((int)hipGraphLaunch(g->exec[sg], st));
        CK(between(sg, st));
    }
    ++e->graph_launches;
    e->upd_ridden = g->ridden; e->upd_swept = g->swept; e->upd_segments = g->segments;
    e->frz_elems = g->frozen; e->frz_wgrad_skipped = g->wgrad_skipped; e->frz_embed_skipped = g->embed_skipped;
    flags.ok = true;
    return MB_OK;
}

// ------------------------------------------------------------------------------------------------ MAG operator
// rows [T, Tp) of MAG's k-major GEMM operands (packed modalities, the three dZ): cleared by the engines whenever the token count
// changes (never inside a captured step), instead of by a launch in every forward and every backward
inline int mag_clear_pad_rows(int dtype, char* ws, const MagWs& w, int T, int H, hipStream_t st) {
    const size_t Tp = align_up((size_t)T, 64), es = esize(dtype);
    if (Tp == (size_t)T) return MB_OK;
    auto zp = [&](size_t off, size_t cols) { return (int)hipMemsetAsync(ws + off + (size_t)T * cols * es, 0, (Tp - T) * cols * es, st); };
    CK(zp(w.vp, w.Vp)); CK(zp(w.ap, w.Ap));
    CK(zp(w.dZe, 2 * (size_t)H)); CK(zp(w.dZv, 2 * (size_t)H)); CK(zp(w.dZa, 2 * (size_t)H));
    return MB_OK;
}
inline int mag_fwd_impl(int dtype, const void* text, const float* visual, const float* acoustic, const float* W_hv,
                 const float* b_hv, const float* W_ha, const float* b_ha, const float* W_v, const float* b_v,
                 const float* W_a, const float* b_a, const float* ln_w, const float* ln_b, float ln_eps, float beta_shift,
                 DropKey drop, void* out, char* ws, const MagWs& w, int T, int H, int V, int A, bool repack, hipStream_t st,
                 bool pads_clean = false, bool packed = false) {
    // packed: the step prologue already wrote this batch's packed modality operands (ws + w.vp / w.ap)
    // pads_clean: the caller keeps rows [T, Tp) of the k-major operands zero itself (the engines: mag_clear_pad_rows whenever the
    // token count changes -- no kernel ever writes those rows); the stand-alone operator clears them on every call
    MagDims d = {T, H, V, A, w.Vp, w.Ap};
    if (repack) CK(mag_pack_weights(dtype, W_hv, W_ha, W_v, W_a, ws + w.We, ws + w.Wv, ws + w.Wa, d, st));
    if (!packed) {
        CK(pack_pad(dtype, visual, V, ws + w.vp, w.Vp, T, st));
        CK(pack_pad(dtype, acoustic, A, ws + w.ap, w.Ap, T, st));
    }
    if (!pads_clean) {
        const int Tp = (int)align_up((size_t)T, 64);
        const size_t es = esize(dtype);
        if (Tp > T) {
            ZeroRanges z = {};
            z.add(ws + w.vp + (size_t)T * w.Vp * es, (size_t)(Tp - T) * w.Vp * es);
            z.add(ws + w.ap + (size_t)T * w.Ap * es, (size_t)(Tp - T) * w.Ap * es);
            CK(zero_fill_ranges(z, st));
        }
    }
    CK(gemm(dtype, GEMM_NT, EPI_BIAS, T, 2 * H, H, text, H, ws + w.We, H, ws + w.Ze, 2 * H, nullptr, nullptr, nullptr,
            nullptr, 0, kNoDrop, 1, 0, st));
    CK(gemm(dtype, GEMM_NT, EPI_BIAS, T, 2 * H, w.Vp, ws + w.vp, w.Vp, ws + w.Wv, w.Vp, ws + w.Zv, 2 * H, nullptr, nullptr,
            nullptr, nullptr, 0, kNoDrop, 1, 0, st));
    CK(gemm(dtype, GEMM_NT, EPI_BIAS, T, 2 * H, w.Ap, ws + w.ap, w.Ap, ws + w.Wa, w.Ap, ws + w.Za, 2 * H, nullptr, nullptr,
            nullptr, nullptr, 0, kNoDrop, 1, 0, st));
    CK(mag_gate_forward(dtype, text, ws + w.Ze, ws + w.Zv, ws + w.Za, b_hv, b_ha, b_v, b_a, ln_w, ln_b, ln_eps, beta_shift,
                        out, (float*)(ws + w.mean), (float*)(ws + w.rstd), d, drop, st));
    return MB_OK;
}

inline int mag_bwd_impl(int dtype, const void* d_out, const void* text, const float* b_hv, const float* b_ha, const float* b_v,
                 const float* b_a, const float* ln_w, float beta_shift, DropKey drop, char* ws, const MagWs& w, void* d_text,
                 float* d_visual, float* d_acoustic, float* dW_hv, float* db_hv, float* dW_ha, float* db_ha, float* dW_v,
                 float* db_v, float* dW_a, float* db_a, float* dln_w, float* dln_b, int T, int H, int V, int A,
                 bool text_padded, hipStream_t st, GradAcc acc = {}, bool pads_clean = false, float* part_a = nullptr,
                 float* part_b = nullptr, int* part_nblk = nullptr, bool dw_zero = false, int* path = nullptr) {
    // dw_zero: the caller knows the four weight-gradient tensors hold zeros (the engines' store path): plain stores, no read-modify-write
    // path (test hook mb_debug_mag_backward_ex only): three ints out -- grouped launch or not, direct stores or not, tile
    MagDims d = {T, H, V, A, w.Vp, w.Ap};
    const int Tp = (int)align_up((size_t)T, 64);      // zero-padded token rows of the workspace operands
    const size_t es = esize(dtype);
    const int Kt = text_padded ? Tp : T;
    // The weight gradients as ONE grouped launch (like a layer's four): alone, the modality problems are 24 / 48 tiles whose duration
    // is the K = T loop latency (three launches of ~34 us each).
    //  * direct (default): six problems of H output rows each -- (text | visual | acoustic operand) x (gate half | projection half of
    //    the dZ columns) -- that store straight into dW_hv / dW_ha / dW_v / dW_a: column offsets V / A inside rows 815 / 842 floats
    //    wide, only the V / A real columns of the padded modality operands (GemmArgs::cvalid: dword stores, no alignment needed).
    //    No packed accumulators, no unpack launch (round 4: 7.4 us + 12 MB of traffic per step).
    //  * MB_MAG_WGRAD_DIRECT=0: three problems into packed fp32 scratch + mag_unpack_wgrads (rounds 2-3).
    const char* dv = getenv("MB_MAG_WGRAD_DIRECT");
    const int direct_env = dv ? atoi(dv) : 1;
    const char* dZe = ws + w.dZe; const char* dZv = ws + w.dZv; const char* dZa = ws + w.dZa;
    GemmArgs wg[6];
    int nwg = 3;
    wg[0] = wgrad_args(2 * H, H, Kt, dZe, 2 * H, text, H, (float*)(ws + w.dWe), H);
    wg[1] = wgrad_args(2 * H, w.Vp, Tp, dZv, 2 * H, ws + w.vp, w.Vp, (float*)(ws + w.dWv), w.Vp);
    wg[2] = wgrad_args(2 * H, w.Ap, Tp, dZa, 2 * H, ws + w.ap, w.Ap, (float*)(ws + w.dWa), w.Ap);
    const int wtile = (w.Vp % 128 == 0 && w.Ap % 128 == 0 && H % 128 == 0 && mag_wgrad_tile() == 128 && gemm_grouped_tn_ok(dtype, wg, 3, 128)) ? 128 : 64;
    const bool grouped = text_padded && gemm_grouped_tn_ok(dtype, wg, 3, wtile);
    const bool direct = grouped && direct_env != 0;
    if (path) { path[0] = grouped ? 1 : 0; path[1] = direct ? 1 : 0; path[2] = wtile; }
    if (direct) {
        const size_t half = (size_t)H * es;          // the projection half of a dZ row starts H columns in
        wg[0] = wgrad_args(H, H, Kt, dZe, 2 * H, text, H, dW_hv + V, V + H);                 wg[0].cvalid = H;
        wg[1] = wgrad_args(H, H, Kt, dZe + half, 2 * H, text, H, dW_ha + A, A + H);          wg[1].cvalid = H;
        wg[2] = wgrad_args(H, w.Vp, Tp, dZv, 2 * H, ws + w.vp, w.Vp, dW_hv, V + H);          wg[2].cvalid = V;
        wg[3] = wgrad_args(H, w.Vp, Tp, dZv + half, 2 * H, ws + w.vp, w.Vp, dW_v, V);        wg[3].cvalid = V;
        wg[4] = wgrad_args(H, w.Ap, Tp, dZa, 2 * H, ws + w.ap, w.Ap, dW_ha, A + H);          wg[4].cvalid = A;
        wg[5] = wgrad_args(H, w.Ap, Tp, dZa + half, 2 * H, ws + w.ap, w.Ap, dW_a, A);        wg[5].cvalid = A;
        nwg = 6;
        if (!gemm_grouped_tn_ok(dtype, wg, nwg, wtile)) return MB_ERR_SHAPE;
    }
    {
        // one launch clears the pad rows of this call's k-major operands and (ungrouped path) the packed weight-gradient accumulators
        ZeroRanges z = {};
        if (Tp > T && !pads_clean) {
            z.add(ws + w.dZe + (size_t)T * 2 * H * es, (size_t)(Tp - T) * 2 * H * es);
            z.add(ws + w.dZv + (size_t)T * 2 * H * es, (size_t)(Tp - T) * 2 * H * es);
            z.add(ws + w.dZa + (size_t)T * 2 * H * es, (size_t)(Tp - T) * 2 * H * es);
        }
        if (!grouped) {
            z.add(ws + w.dWe, (size_t)2 * H * H * 4);
            z.add(ws + w.dWv, (size_t)2 * H * w.Vp * 4);
            z.add(ws + w.dWa, (size_t)2 * H * w.Ap * 4);
        }
        if (z.n) CK(zero_fill_ranges(z, st));
    }
    CK(mag_gate_backward(dtype, d_out, text, ws + w.Ze, ws + w.Zv, ws + w.Za, b_hv, b_ha, b_v, b_a, ln_w,
                         (const float*)(ws + w.mean), (const float*)(ws + w.rstd), beta_shift, ws + w.dep, ws + w.dZe,
                         ws + w.dZv, ws + w.dZa, db_hv, db_ha, db_v, db_a, dln_w, dln_b, d, drop, st, acc, part_a, part_b, part_nblk));
    if (grouped) {
        for (int i = 0; i < nwg; ++i) wg[i].overwrite = direct ? (dw_zero ? 1 : 0) : 1;      // (the packed accumulators are always stored)
        CK(gemm_grouped_tn_launch(dtype, wg, nwg, wtile, st, wtile == 64 ? mag_wgrad_stages() : 0));
    } else {
        CK(wgrad(dtype, 2 * H, H, text_padded ? Tp : T, ws + w.dZe, 2 * H, text, H, (float*)(ws + w.dWe), H, st));
        CK(wgrad(dtype, 2 * H, w.Vp, Tp, ws + w.dZv, 2 * H, ws + w.vp, w.Vp, (float*)(ws + w.dWv), w.Vp, st));
        CK(wgrad(dtype, 2 * H, w.Ap, Tp, ws + w.dZa, 2 * H, ws + w.ap, w.Ap, (float*)(ws + w.dWa), w.Ap, st));
    }
    if (!direct)
        CK(mag_unpack_wgrads((const float*)(ws + w.dWe), (const float*)(ws + w.dWv), (const float*)(ws + w.dWa), dW_hv, dW_ha,
                             dW_v, dW_a, d, st));
    // d_text = dZe . We + (ds + d||e|| term)
    CK(gemm(dtype, GEMM_NN, EPI_ADD_RES, T, H, 2 * H, ws + w.dZe, 2 * H, ws + w.We, H, d_text, H, nullptr, nullptr, nullptr,
            ws + w.dep, H, kNoDrop, 1, 0, st));
    if (d_visual) {
        CK(gemm(dtype, GEMM_NN, EPI_BIAS_F32, T, w.Vp, 2 * H, ws + w.dZv, 2 * H, ws + w.Wv, w.Vp, nullptr, w.Vp, nullptr,
                (float*)(ws + w.dvp), nullptr, nullptr, 0, kNoDrop, 1, 0, st));
        CK((int)hipMemcpy2DAsync(d_visual, (size_t)V * 4, ws + w.dvp, (size_t)w.Vp * 4, (size_t)V * 4, T,
                                 hipMemcpyDeviceToDevice, st));
    }
    if (d_acoustic) {
        CK(gemm(dtype, GEMM_NN, EPI_BIAS_F32, T, w.Ap, 2 * H, ws + w.dZa, 2 * H, ws + w.Wa, w.Ap, nullptr, w.Ap, nullptr,
                (float*)(ws + w.dap), nullptr, nullptr, 0, kNoDrop, 1, 0, st));
        CK((int)hipMemcpy2DAsync(d_acoustic, (size_t)A * 4, ws + w.dap, (size_t)w.Ap * 4, (size_t)A * 4, T,
                                 hipMemcpyDeviceToDevice, st));
    }
    return MB_OK;
}


}  // namespace
