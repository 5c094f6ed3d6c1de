// step_bench -- torch-free driver of the MAG-BERT step engine through the C ABI (include/magbert_hip.h).
//
// Measurement tooling (not product): runs the same optimizer step bench.py times -- forward + fused MSE + backward +
// HF-AdamW on one synthetic minibatch in prepare_bert_input's layout (/root/reference/multimodal_driver.py:143-180) -- from a
// plain C++ process, so a GPU-box visit costs seconds instead of a Python/torch start-up, and rocprofv3 can wrap it.
//
//   step_bench [--model bert|xlnet] [--steps K] [--warmup W] [--batch B] [--seq L] [--dtype bf16|fp32] [--visual V] [--layers N]
//              [--hidden H] [--heads n] [--inter I]       (both models; bert-large-uncased / xlnet-large-cased = --layers 24 --hidden 1024
//                                                          --heads 16 --inter 4096; --heads defaults to H / 64, --inter to 4 H)
//              [--graph 0|1|2] [--h2d 0|1|2] [--nbatch n] [--dp 0|1] [--wire fp32|bf16] [--sparse 0|1] [--timing 0|1] [--shard 0|1]
//              [--vocab n]   (MAG-BERT: a word table of n rows, ids folded into it -- with a small one every row is touched)
//   --dp 1:  the data-parallel step, mb_bert_train_step_dp, with a ONE-rank RCCL communicator created here through the C ABI
//            (mb_comm_unique_id / mb_comm_create_rccl): the N > 1 code path -- graph chain, comm stream, events, ncclAllReduce /
//            ncclAllGather calls, the row-wise word-embedding exchange -- without a second GPU.  Needs --graph 1|2.
//   --graph: 0 forward/backward/AdamW calls, 1 mb_bert_train_step hipGraph replay, 2 mb_bert_train_step stream launches
//   --layer_decay D, --head_lr_mult K (each off at 1; --graph 1|2, no --dp): per-group learning rates as update classes
//            (mb_*_set_update_map / _set_update_values) -- layer l of N at lr * D^(N - l), the embeddings at lr * D^(N + 1), MAG / pooler /
//            heads at K * lr, every learning rate split by the no-decay rule: two classes per depth while that fits the class table, one
//            class per depth with no-decay marks on the undecayed segments otherwise (mb_*_set_update_decay) -- the same update
//   --max_grad_norm X (--graph 1|2, no --dp; 0 = off): gradient-norm clipping inside the step (mb_*_set_grad_clip); the norm and coefficient
//            of the last update are printed
//   --freeze_layers N, --freeze_emb 0|1 (--graph 1|2, no --dp): the lowest N layers / the embedding tables are in no update class
//            (mb_*_set_update_frozen): no weight-gradient launch for those layers, no embedding backward; composes with --layer_decay and
//            --max_grad_norm.  Without --layer_decay the rest is the two parameter groups as a two-class map.  Prints mb_*_freeze_stats.
//   --act gelu|relu|swish|silu|gelu_new|mish: the feed-forward activation (mb_bert_config.hidden_act / mb_xlnet_config.ff_activation)
//   --loss default|mse|l1|smooth_l1|bce|cross_entropy [--loss_beta X]: the head's objective (mb_*_set_head_loss_ex)
//   --num_labels N: the head's width (default 1).  Labels are drawn to match: regression targets, class indices in [0, N) for the
//            cross entropy (and the default kind at N > 1), {0, 1} targets for bce
//   --loss_smoothing X, --loss_gamma X, --loss_ignore K: label smoothing, the focal exponent, ignore_index of mb_head_loss; with
//            --loss_ignore every fifth sample carries the label K
//   --inject N: MAG in front of encoder layer N (injection_index of either config; default 0 for MAG-BERT, 1 for MAG-XLNet)
//   --h2d:   0 batch resident in HBM, 1 hipMemcpyAsync per step, 2 batch read in place from pinned host memory by the prologue
//
// Prints one line per run: ms/step (HIP events around the K timed steps), host enqueue ms/step, samples/s, final loss.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/magbert_hip.h"

#define HCK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(_e)); exit(2); } } while (0)
#define MCK(x) do { int _e = (x); if (_e) { fprintf(stderr, "%s:%d magbert error %d: %s\n", __FILE__, __LINE__, _e, mb_error_string(_e)); exit(3); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static inline uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static inline float urand() { return (float)((rnd() >> 40) * (1.0 / 16777216.0)); }
static inline float nrand() { float u = urand() + 1e-7f, v = urand(); return sqrtf(-2.f * logf(u)) * cosf(6.2831853f * v); }

struct Batch { int64_t *ids, *seg, *mask; float *vis, *aco, *lab; };

int main(int argc, char** argv) {
    int steps = 30, warmup = 5, B = 48, L = 50, V = 47, A = 74, layers = 12, graph = 0, h2d = 0, nbatch = 4, dtype = MB_DT_BF16;
    int dp = 0, wire = MB_DT_F32, sparse = 1, timing = 0, shard = 0, xl = 0, hidden = 768, heads = 0, inter = 0;
    double layer_decay = 1.0, head_lr_mult = 1.0, max_grad_norm = 0.0;
    int freeze_layers = 0, freeze_emb = 0, act = MB_ACT_GELU, inject = -1;      // --inject N: MAG in front of layer N (default: 0 | MAG-XLNet: 1)
    int vocab_rows = 30522;     // --vocab n: a smaller word table, every id folded into it (every row of a small one is touched within a few batches)
    int all_live = 0;           // --all_live 1: every sample has L - 2 words (no padding token: the worst case of the live-row weight gradients)
    const char* act_name = "gelu";
    int loss_kind = MB_LOSS_DEFAULT; double loss_beta = 1.0; const char* loss_name = "default";
    int num_labels = 1, loss_has_ignore = 0, loss_ignore = 0; double loss_smoothing = 0.0, loss_gamma = 0.0;
    for (int i = 1; i + 1 < argc; i += 2) {
        std::string k = argv[i]; const char* v = argv[i + 1];
        if (k == "--steps") steps = atoi(v); else if (k == "--warmup") warmup = atoi(v); else if (k == "--batch") B = atoi(v);
        else if (k == "--seq") L = atoi(v); else if (k == "--visual") V = atoi(v); else if (k == "--layers") layers = atoi(v);
        else if (k == "--graph") graph = atoi(v); else if (k == "--h2d") h2d = atoi(v); else if (k == "--nbatch") nbatch = atoi(v);
        else if (k == "--dtype") dtype = strcmp(v, "fp32") == 0 ? MB_DT_F32 : MB_DT_BF16;
        else if (k == "--dp") dp = atoi(v); else if (k == "--sparse") sparse = atoi(v); else if (k == "--timing") timing = atoi(v);
        else if (k == "--shard") shard = atoi(v);
        else if (k == "--hidden") hidden = atoi(v); else if (k == "--heads") heads = atoi(v); else if (k == "--inter") inter = atoi(v);
        else if (k == "--model") xl = strcmp(v, "xlnet") == 0;       // MAG-XLNet (BASELINE.json configs[3]): the single-call step only (--graph 1|2)
        else if (k == "--layer_decay") layer_decay = atof(v); else if (k == "--head_lr_mult") head_lr_mult = atof(v);
        else if (k == "--max_grad_norm") max_grad_norm = atof(v);
        else if (k == "--freeze_layers") freeze_layers = atoi(v); else if (k == "--freeze_emb") freeze_emb = atoi(v);
        else if (k == "--inject") inject = atoi(v);
        else if (k == "--all_live") all_live = atoi(v);
        else if (k == "--vocab") vocab_rows = atoi(v);      // MAG-BERT: rows of the word table (ids are folded into them; >= 103)
        else if (k == "--act") {
            const char* names[] = {"gelu", "relu", "swish", "gelu_new", "mish"};
            act = strcmp(v, "silu") == 0 ? MB_ACT_SWISH : -1;
            for (int a = 0; a < 5; ++a) if (strcmp(v, names[a]) == 0) act = a;
            if (act < 0) { fprintf(stderr, "--act: gelu | relu | swish | silu | gelu_new | mish\n"); return 1; }
            act_name = v;
        }
        else if (k == "--loss") {
            const char* names[] = {"default", "mse", "l1", "smooth_l1", "bce", "cross_entropy"};
            loss_kind = -1;
            for (int a = 0; a < 6; ++a) if (strcmp(v, names[a]) == 0) loss_kind = a;
            if (loss_kind < 0) { fprintf(stderr, "--loss: default | mse | l1 | smooth_l1 | bce | cross_entropy\n"); return 1; }
            loss_name = v;
        }
        else if (k == "--loss_beta") loss_beta = atof(v);
        else if (k == "--num_labels") num_labels = atoi(v);
        else if (k == "--loss_smoothing") loss_smoothing = atof(v);
        else if (k == "--loss_gamma") loss_gamma = atof(v);
        else if (k == "--loss_ignore") { loss_has_ignore = 1; loss_ignore = atoi(v); }
        else if (k == "--wire") wire = strcmp(v, "bf16") == 0 ? MB_DT_BF16 : MB_DT_F32;
        else { fprintf(stderr, "unknown option %s (options: --model --steps --warmup --batch --seq --dtype --visual --layers --hidden --heads --inter "
                               "--graph --h2d --nbatch --dp --wire --sparse --timing --shard --layer_decay --head_lr_mult --max_grad_norm --freeze_layers --freeze_emb --act --loss --loss_beta --num_labels --loss_smoothing --loss_gamma --loss_ignore --inject --all_live --vocab)\n", k.c_str()); return 1; }
    }
    if (heads <= 0) heads = hidden / 64;
    if (inter <= 0) inter = 4 * hidden;
    mb_bert_config c = {};
    c.vocab_size = vocab_rows; c.hidden_size = hidden; c.num_layers = layers; c.num_heads = heads; c.intermediate_size = inter;
    if (num_labels < 1) { fprintf(stderr, "--num_labels: at least 1\n"); return 1; }
    c.max_position = 512; c.type_vocab = 2; c.num_labels = num_labels; c.visual_dim = V; c.acoustic_dim = A; c.pad_token_id = 0;
    c.layer_norm_eps = 1e-12f; c.mag_layer_norm_eps = 1e-5f; c.beta_shift = 1.0f;
    c.hidden_dropout = 0.1f; c.attn_dropout = 0.1f; c.mag_dropout = 0.5f; c.dtype = dtype; c.max_batch = B; c.max_seq = L;
    c.hidden_act = act; c.injection_index = inject < 0 ? 0 : inject;
    mb_bert_engine* e = nullptr;
    mb_xlnet_engine* ex = nullptr;
    size_t n, nd, wsb, shb, she;
    if (xl) {
        if (!graph || dp) { fprintf(stderr, "--model xlnet: the single-call step only (--graph 1|2, no --dp)\n"); return 1; }
        mb_xlnet_config xc = {};
        xc.vocab_size = 32000; xc.d_model = hidden; xc.n_layer = layers; xc.n_head = heads; xc.d_inner = inter; xc.num_labels = num_labels;
        xc.visual_dim = V; xc.acoustic_dim = A; xc.injection_index = inject < 0 ? 1 : inject;
        xc.layer_norm_eps = 1e-12f; xc.mag_layer_norm_eps = 1e-5f; xc.beta_shift = 1.0f;
        xc.dropout = 0.1f; xc.summary_last_dropout = 0.1f; xc.mag_dropout = 0.5f; xc.dtype = dtype; xc.max_batch = B; xc.max_seq = L;
        xc.ff_activation = act;
        MCK(mb_xlnet_create(&xc, &ex));
        n = mb_xlnet_param_count(ex); nd = mb_xlnet_decay_count(ex); wsb = mb_xlnet_workspace_bytes(ex);
        mb_xlnet_shadow_range(ex, &shb, &she);
    } else {
        MCK(mb_bert_create(&c, &e));
        n = mb_bert_param_count(e); nd = mb_bert_decay_count(e); wsb = mb_bert_workspace_bytes(e);
        mb_bert_shadow_range(e, &shb, &she);
    }
    if (loss_kind != MB_LOSS_DEFAULT || loss_smoothing != 0.0 || loss_gamma != 0.0 || loss_has_ignore) {
        const mb_head_loss hlx = {loss_kind, loss_kind == MB_LOSS_SMOOTH_L1 ? (float)loss_beta : 0.f, nullptr, (float)loss_smoothing, (float)loss_gamma,
                                  loss_has_ignore, loss_ignore};       // (an option the kind does not take: MB_ERR_ARG from the setter)
        if (xl) MCK(mb_xlnet_set_head_loss_ex(ex, &hlx)); else MCK(mb_bert_set_head_loss_ex(e, &hlx));
    }
    const bool per_element = loss_kind >= MB_LOSS_MSE && loss_kind <= MB_LOSS_BCE;      // labels [B][num_labels], else [B]
    const bool class_labels = loss_kind == MB_LOSS_CROSS_ENTROPY || (loss_kind == MB_LOSS_DEFAULT && num_labels > 1);
    const int lab_per = per_element ? num_labels : 1;
    float *P, *G, *M, *Vv; void *SH, *WS;
    HCK(hipMalloc(&P, n * 4)); HCK(hipMalloc(&G, n * 4)); HCK(hipMalloc(&M, n * 4)); HCK(hipMalloc(&Vv, n * 4));
    HCK(hipMalloc(&SH, n * 2)); HCK(hipMalloc(&WS, wsb));
    HCK(hipMemset(G, 0, n * 4)); HCK(hipMemset(M, 0, n * 4)); HCK(hipMemset(Vv, 0, n * 4));
    {   // init law of the reference (N(0, 0.02), biases 0, LayerNorm 1/0)
        std::vector<float> h(n, 0.f);
        char name[160]; size_t off, numel; int nd_, dec; int64_t shp[4];
        const int ntens = xl ? mb_xlnet_num_tensors(ex) : mb_bert_num_tensors(e);
        for (int i = 0; i < ntens; ++i) {
            if (xl) MCK(mb_xlnet_tensor_info(ex, i, name, 160, &off, &numel, &nd_, shp, &dec));
            else MCK(mb_bert_tensor_info(e, i, name, 160, &off, &numel, &nd_, shp, &dec));
            const std::string s = name;
            const bool ln = s.find("LayerNorm") != std::string::npos || s.find("layer_norm") != std::string::npos;
            const bool bias = s.size() > 5 && s.compare(s.size() - 5, 5, ".bias") == 0;
            for (size_t j = 0; j < numel; ++j) h[off + j] = ln ? (bias ? 0.f : 1.f) : (bias ? 0.f : 0.02f * nrand());
        }
        HCK(hipMemcpy(P, h.data(), n * 4, hipMemcpyHostToDevice));
    }
    hipStream_t st; HCK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (xl) { MCK(mb_xlnet_bind(ex, P, G, dtype == MB_DT_BF16 ? SH : nullptr, WS, wsb)); MCK(mb_xlnet_sync_weights(ex, st)); }
    else { MCK(mb_bert_bind(e, P, G, dtype == MB_DT_BF16 ? SH : nullptr, WS, wsb)); MCK(mb_bert_sync_weights(e, st)); }

    // synthetic batches (host pinned + device resident)
    const size_t T = (size_t)B * L;
    const size_t bytes = T * 8 * 3 + T * V * 4 + T * A * 4 + (size_t)B * lab_per * 4;
    std::vector<char*> hb(nbatch), db(nbatch);
    auto view = [&](char* p) { Batch b; b.ids = (int64_t*)p; b.seg = b.ids + T; b.mask = b.seg + T; b.vis = (float*)(b.mask + T);
                               b.aco = b.vis + T * V; b.lab = b.aco + T * A; return b; };
    for (int k = 0; k < nbatch; ++k) {
        HCK(hipHostMalloc((void**)&hb[k], bytes)); HCK(hipMalloc((void**)&db[k], bytes));
        Batch b = view(hb[k]);
        memset(hb[k], 0, bytes);
        for (int s = 0; s < B; ++s) {
            const int nw_drawn = 5 + (int)(rnd() % (uint64_t)(L - 2 - 5 + 1));      // (drawn either way: the same ids and modalities follow)
            const int nw = all_live ? L - 2 : nw_drawn;
            b.ids[s * L] = 101; b.mask[s * L] = 1;
            for (int t = 1; t <= nw; ++t) {
                b.ids[s * L + t] = (1000 + (int64_t)(rnd() % 29522)) % (xl ? 32000 : vocab_rows); b.mask[s * L + t] = 1;
                for (int j = 0; j < V; ++j) b.vis[((size_t)s * L + t) * V + j] = nrand();
                for (int j = 0; j < A; ++j) b.aco[((size_t)s * L + t) * A + j] = nrand();
            }
            b.ids[s * L + nw + 1] = 102; b.mask[s * L + nw + 1] = 1;
            for (int j = 0; j < lab_per; ++j) {
                const float u = urand();
                b.lab[(size_t)s * lab_per + j] = class_labels ? (float)std::min(num_labels - 1, (int)(u * num_labels))
                                                 : loss_kind == MB_LOSS_BCE ? (u < 0.5f ? 0.f : 1.f) : 6.f * u - 3.f;
            }
            if (loss_has_ignore && s % 5 == 4) b.lab[s] = (float)loss_ignore;
        }
        HCK(hipMemcpy(db[k], hb[k], bytes, hipMemcpyHostToDevice));
    }
    float *logits, *loss;
    HCK(hipMalloc(&logits, (size_t)B * num_labels * 4)); HCK(hipMalloc(&loss, 8)); HCK(hipMemset(loss, 0, 8));

    mb_comm* comm = nullptr;
    if (dp) {
        if (!graph) { fprintf(stderr, "--dp 1 needs --graph 1|2\n"); return 1; }
        char id[128];
        MCK(mb_comm_unique_id(id));
        int rc = mb_comm_create_rccl(id, 0, 1, &comm);
        if (rc) { fprintf(stderr, "mb_comm_create_rccl: %d %s\n", rc, mb_comm_last_error()); return 3; }
        const int vocab = sparse ? c.vocab_size : 0;
        const size_t sb = mb_comm_scratch_bytes(1, wire, n, vocab, c.hidden_size, B * L);
        void* scratch; HCK(hipMalloc(&scratch, sb));
        MCK(mb_comm_bind_scratch(comm, scratch, sb, wire, n, vocab, c.hidden_size, B * L));
        MCK(mb_comm_set_timing(comm, timing));
        if (shard) { MCK(mb_comm_set_sharding(comm, 1)); if (!mb_comm_sharding(comm)) fprintf(stderr, "--shard 1: a one-rank group shards nothing without MB_DP_SHARD_FORCE=1\n"); }
        HCK(hipDeviceSynchronize());
    }
    const float lr = 1e-5f, b1 = 0.9f, b2 = 0.999f, eps = 1e-6f, wd = 0.01f;
    int t_opt = 0;
    const bool classed = layer_decay != 1.0 || head_lr_mult != 1.0;
    const bool freezing = freeze_layers > 0 || freeze_emb != 0;
    int n_classes = 0, n_segments = 0;
    if (classed || freezing) {
        if (!graph || dp) { fprintf(stderr, "--layer_decay / --head_lr_mult / --freeze_*: the single-call step only (--graph 1|2, no --dp)\n"); return 1; }
        if (freeze_layers > layers) { fprintf(stderr, "--freeze_layers: at most %d\n", layers); return 1; }
        // depth 0 = embeddings (and any other encoder tensor), l + 1 = layer l, layers + 1 = MAG / pooler / heads
        // Two classes per depth (decayed / not) while they fit the table; deeper models share one class per depth and mark the
        // no-decay segments (mb_*_set_update_decay) -- the same update either way
        const bool split = !classed || 2 * (layers + 2) <= MB_UPDATE_CLASSES_MAX;
        if (layers + 2 > MB_UPDATE_CLASSES_MAX) { fprintf(stderr, "--layer_decay / --head_lr_mult: at most %d layers\n", MB_UPDATE_CLASSES_MAX - 2); return 1; }
        std::vector<uint8_t> marks, frozen;
        std::vector<int> slot_of(2 * (layers + 2), -1);
        std::vector<size_t> bounds; std::vector<int> cls;
        std::vector<float> c_lr, c_b1, c_b2, c_eps, c_wd; std::vector<int> c_cb;
        char name[160]; size_t off, numel; int nd_, dec; int64_t shp[4];
        const int ntens = xl ? mb_xlnet_num_tensors(ex) : mb_bert_num_tensors(e);
        size_t end = 0;
        for (int i = 0; i < ntens; ++i) {           // (the table is in layout order)
            if (xl) MCK(mb_xlnet_tensor_info(ex, i, name, 160, &off, &numel, &nd_, shp, &dec));
            else MCK(mb_bert_tensor_info(e, i, name, 160, &off, &numel, &nd_, shp, &dec));
            if (dec == 2) continue;                 // frozen
            const std::string s = name;
            int depth = 0;
            const size_t at = s.find(".layer.");
            if (at != std::string::npos) depth = atoi(s.c_str() + at + 7) + 1;
            else if (s.find("MAG.") != std::string::npos || s.find("pooler.") != std::string::npos || s.find("classifier.") != std::string::npos ||
                     s.find("sequence_summary.") != std::string::npos || s.find("logits_proj.") != std::string::npos) depth = layers + 1;
            const bool no_decay = s.find("bias") != std::string::npos || s.find("LayerNorm.weight") != std::string::npos;
            // frozen: the lowest layers, the embedding tables (MAG-BERT: with their LayerNorm) -- in no class, a segment of their own
            const bool fz = (depth >= 1 && depth <= freeze_layers) ||
                            (freeze_emb && (s.find("embeddings.") != std::string::npos || s.find("word_embedding") != std::string::npos));
            if (fz) {
                if (cls.empty() || !frozen.back()) { bounds.push_back(off); cls.push_back(0); marks.push_back(0); frozen.push_back(1); }
                end = (off + numel + 63) / 64 * 64;
                continue;
            }
            const int key = classed ? 2 * depth + ((split && no_decay) ? 1 : 0) : (no_decay ? 1 : 0);
            if (slot_of[key] < 0) {
                slot_of[key] = n_classes++;
                c_lr.push_back(depth == layers + 1 ? (float)(lr * head_lr_mult) : (float)(lr * pow(layer_decay, layers + 1 - depth)));
                c_b1.push_back(b1); c_b2.push_back(b2); c_eps.push_back(eps); c_wd.push_back((split && no_decay) ? 0.f : wd); c_cb.push_back(1);
            }
            const uint8_t mark = (!split && no_decay) ? 1 : 0;
            if (cls.empty() || frozen.back() || cls.back() != slot_of[key] || marks.back() != mark) {
                bounds.push_back(off); cls.push_back(slot_of[key]); marks.push_back(mark); frozen.push_back(0);
            }
            end = (off + numel + 63) / 64 * 64;
        }
        bounds.push_back(end);
        n_segments = (int)cls.size();
        if (xl) { MCK(mb_xlnet_set_update_map(ex, n_classes, n_segments, bounds.data(), cls.data()));
                  if (!split) MCK(mb_xlnet_set_update_decay(ex, n_segments, marks.data()));
                  if (freezing) MCK(mb_xlnet_set_update_frozen(ex, n_segments, frozen.data()));
                  MCK(mb_xlnet_set_update_values(ex, n_classes, c_lr.data(), c_b1.data(), c_b2.data(), c_eps.data(), c_wd.data(), c_cb.data())); }
        else { MCK(mb_bert_set_update_map(e, n_classes, n_segments, bounds.data(), cls.data()));
               if (!split) MCK(mb_bert_set_update_decay(e, n_segments, marks.data()));
               if (freezing) MCK(mb_bert_set_update_frozen(e, n_segments, frozen.data()));
               MCK(mb_bert_set_update_values(e, n_classes, c_lr.data(), c_b1.data(), c_b2.data(), c_eps.data(), c_wd.data(), c_cb.data())); }
    }
    if (max_grad_norm > 0.0) {
        if (!graph || dp) { fprintf(stderr, "--max_grad_norm: the single-call step only (--graph 1|2, no --dp)\n"); return 1; }
        if (xl) MCK(mb_xlnet_set_grad_clip(ex, (float)max_grad_norm)); else MCK(mb_bert_set_grad_clip(e, (float)max_grad_norm));
    }
    auto step = [&](int i) {
        char* src = db[i % nbatch];
        if (h2d == 1) HCK(hipMemcpyAsync(src, hb[i % nbatch], bytes, hipMemcpyHostToDevice, st));     // copy engine, same stream
        if (h2d == 2) src = hb[i % nbatch];       // zero-copy: the step prologue gathers the batch out of pinned host memory (--graph 1|2)
        Batch b = view(src);
        ++t_opt;
        if (graph && dp) {
            MCK(mb_bert_train_step_dp(e, b.ids, b.vis, b.aco, b.mask, b.seg, b.lab, B, L, 1234, (uint64_t)t_opt, logits, loss, loss + 1,
                                      M, Vv, lr, b1, b2, eps, wd, t_opt, 1, 1.0f, 1.0f, graph, st, comm));
            return;
        }
        if (xl) {
            MCK(mb_xlnet_train_step(ex, b.ids, b.vis, b.aco, b.mask, b.seg, b.lab, B, L, 1234, (uint64_t)t_opt, logits, loss, loss + 1,
                                    M, Vv, lr, b1, b2, eps, wd, t_opt, 1, 1.0f, 1.0f, graph, st));
            return;
        }
        if (graph) {
            MCK(mb_bert_train_step(e, b.ids, b.vis, b.aco, b.mask, b.seg, b.lab, B, L, 1234, (uint64_t)t_opt, logits, loss, loss + 1,
                                   M, Vv, lr, b1, b2, eps, wd, t_opt, 1, 1.0f, 1.0f, graph, st));
            return;
        }
        MCK(mb_bert_forward(e, b.ids, b.vis, b.aco, b.mask, b.seg, b.lab, B, L, 1, 1234, (uint64_t)t_opt, logits, loss, loss + 1, st));
        MCK(mb_bert_backward(e, nullptr, b.lab, 1.0f, 0, layers + 2, st));
        MCK(mb_adamw_step(P, G, M, Vv, dtype == MB_DT_BF16 ? SH : nullptr, nd, nd, shb, she, lr, b1, b2, eps, wd, t_opt, 1, 1.0f, 1, st));
        MCK(mb_adamw_step(P + nd, G + nd, M + nd, Vv + nd, nullptr, n - nd, 0, 0, 0, lr, b1, b2, eps, 0.f, t_opt, 1, 1.0f, 1, st));
    };
    for (int i = 0; i < warmup; ++i) step(i);
    HCK(hipStreamSynchronize(st));
    hipEvent_t e0, e1; HCK(hipEventCreate(&e0)); HCK(hipEventCreate(&e1));
    HCK(hipEventRecord(e0, st));
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < steps; ++i) step(warmup + i);
    auto t1 = std::chrono::steady_clock::now();
    HCK(hipEventRecord(e1, st));
    HCK(hipEventSynchronize(e1));
    auto t2 = std::chrono::steady_clock::now();
    float ms = 0.f; HCK(hipEventElapsedTime(&ms, e0, e1));
    float hl[2]; HCK(hipMemcpy(hl, loss, 8, hipMemcpyDeviceToHost));
    const double host_ms = std::chrono::duration<double, std::milli>(t1 - t0).count() / steps;
    const double wall_ms = std::chrono::duration<double, std::milli>(t2 - t0).count() / steps;
    char shape[192] = "";
    if ((hidden != 768 || heads != 12 || inter != 3072)) snprintf(shape, sizeof shape, " hidden=%d heads=%d inter=%d", hidden, heads, inter);
    if (act != MB_ACT_GELU) snprintf(shape + strlen(shape), sizeof shape - strlen(shape), " act=%s", act_name);
    if (loss_kind != MB_LOSS_DEFAULT) snprintf(shape + strlen(shape), sizeof shape - strlen(shape), " loss=%s", loss_name);
    if (num_labels != 1) snprintf(shape + strlen(shape), sizeof shape - strlen(shape), " num_labels=%d", num_labels);
    if (loss_smoothing != 0.0) snprintf(shape + strlen(shape), sizeof shape - strlen(shape), " smoothing=%g", loss_smoothing);
    if (loss_gamma != 0.0) snprintf(shape + strlen(shape), sizeof shape - strlen(shape), " gamma=%g", loss_gamma);
    if (loss_has_ignore) snprintf(shape + strlen(shape), sizeof shape - strlen(shape), " ignore=%d", loss_ignore);
    printf("step_bench %sdtype=%s B=%d L=%d V=%d layers=%d%s graph=%d h2d=%d : %.3f ms/step (events) %.3f ms/step (wall) host-enqueue %.3f ms/step "
           "%.1f samples/s last-loss %.4f mean-loss %.4f\n",
           xl ? "model=xlnet " : "", dtype == MB_DT_BF16 ? "bf16" : "fp32", B, L, V, layers, shape, graph, h2d, ms / steps, wall_ms, host_ms, B * 1e3 / (ms / steps), hl[0],
           hl[1] / (steps + warmup));
    if (graph && !dp) {
        size_t ridden = 0, swept = 0; int segs = 0;
        if (xl) MCK(mb_xlnet_update_stats(ex, &ridden, &swept, &segs)); else MCK(mb_bert_update_stats(e, &ridden, &swept, &segs));
        printf("step_bench update: classes=%d segments=%d ridden=%zu swept=%zu (layer_decay=%g head_lr_mult=%g)\n", n_classes, segs, ridden, swept,
               layer_decay, head_lr_mult);
        if (freezing) {
            size_t fe = 0; int wg = 0, emb = 0;
            if (xl) MCK(mb_xlnet_freeze_stats(ex, &fe, &wg, &emb)); else MCK(mb_bert_freeze_stats(e, &fe, &wg, &emb));
            printf("step_bench freeze: freeze_layers=%d freeze_emb=%d frozen_elems=%zu wgrad_launches_skipped=%d embed_skipped=%d\n", freeze_layers,
                   freeze_emb, fe, wg, emb);
        }
        if (max_grad_norm > 0.0) {
            float norm = 0.f, coef = 0.f;
            if (xl) MCK(mb_xlnet_grad_clip_stats(ex, &norm, &coef, st)); else MCK(mb_bert_grad_clip_stats(e, &norm, &coef, st));
            printf("step_bench clip: max_grad_norm=%g last norm=%.6g coef=%.6g\n", max_grad_norm, norm, coef);
        }
    }
    if (comm) {
        float ex = 0.f; size_t pieces = 0, cbytes = 0;
        MCK(mb_comm_exposed_ms(comm, &ex)); MCK(mb_comm_stats(comm, &pieces, &cbytes));
        printf("step_bench dp: 1-rank RCCL, wire=%s sparse=%d shard=%d : %zu collectives / %.1f MB per step, comm_exposed %.4f ms (last step)\n",
               wire == MB_DT_BF16 ? "bf16" : "fp32", sparse, mb_comm_sharding(comm), pieces, cbytes * 1e-6, ex);
        mb_comm_destroy(comm);
    }
    if (xl) mb_xlnet_destroy(ex); else mb_bert_destroy(e);
    return 0;
}
