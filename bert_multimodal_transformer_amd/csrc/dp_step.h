// The data-parallel single-call step both engines share (mb_bert_train_step_dp, mb_xlnet_train_step_dp: include/magbert_hip.h,
// csrc/comm.hip): the step with the gradient exchange inside.  `plan` = layers per backward segment (dp_chunk_plan: 4, 4, 2, 2).
// Segments, each a LINEAR graph:
//   s < nb      : (s = 0: forward + head) + the backward of plan[s] layers (+ s = nb-1: the embedding stage -- MAG-BERT: MAG + embeddings
//                 + the ONE LayerNorm / bias reduction)  -> between: all-reduce of those layers' GEMM weights (the last one: + the tail's exchange)
//   nb          : AdamW over the GEMM weights of every layer but the last segment's   (waits for the early pieces only)
//   nb + 1      : AdamW over the last segment's layers, the rest of the decay slab and the no-decay slab   (waits for everything)
// An engine E gives the templates what differs by name through four accessors next to n_update_end() -- n_layers(), layer_begin(l) (flat
// offset of layer l's first GEMM weight), layers_end() (end of the layers' GEMM weights) and width() -- and its prepare-pass,
// forward-range and backward functions as callables (they are file-static in each engine's translation unit).
// The optimizer end of the single-process step (enqueue_update) lives here too: it reads the engines through the same accessors.
#pragma once
#include "engine_common.h"
#include "comm.h"

namespace {

// AdamW of flat range [b, en) of the decay slab (GEMM weights), inside a step (scalars from device memory)
template <class E>
int adamw_decay_range(E* e, float* m, float* v, size_t b, size_t en, hipStream_t st) {
    if (en <= b) return MB_OK;
    const AdamArgs none = {};
    const bool keep = e->keep_in_step();          // the layers' GEMM weight gradients: overwritten by the next backward, not zeroed
    auto clampr = [&](size_t x) { return x < b ? (size_t)0 : (x > en ? en - b : x - b); };
    const size_t shb = clampr(e->sh_begin), she = clampr(e->sh_end);
    const size_t kb = keep ? clampr(e->stale_begin) : 0, ke = keep ? clampr(e->stale_end) : 0;
    void* sh = e->c.dtype == DT_BF16 ? (void*)(e->SH + b * 2) : nullptr;
    return adamw_step(e->P + b, e->G + b, m + b, v + b, sh, en - b, en - b, shb, she, none, 1, st, e->adam_state(e->ws), kb, ke);
}

// The optimizer end of a single-process single-call step, behind the engine's backward: the clip (StepMixin::clip_step: the whole
// gradient is final, its norm and the coefficient go into the scalars the sweep reads), the update statistics and the sweep of what
// the riders (MB_ADAMW_RIDE) left -- they took [ride_cursor, layers_end()) of the decay slab when `ride`.  On top of dp_step's
// accessors an engine gives word_skip(ws): the WordSkip of its word table when it can vouch for untouched rows, {} otherwise.
//   classed step (kernels.h AdamPieces): the ranges cut at the segment boundaries, every piece with its class's slot, ONE launch;
//   unclassed: what the riders left of the layers, the rest of the decay slab, the no-decay slab -- ONE launch over that table
//   (one_sweep; MB_ADAMW_ONE_SWEEP=0 with a word skip: one launch per range, each a one-piece table), which leaves the gradients of
//   the word rows this update's batches did not touch alone (WordSkip, StepMixin::stamp_live: the prologue put the verdict of THIS step
//   into device memory, so the captured launch is the same either way);
//   neither: adamw_step per range.
template <class E>
int enqueue_update(E* e, float* m, float* v, bool ride, bool clip, hipStream_t st) {
    char* ws = e->ws;
    const int NL = e->n_layers();
    const size_t nd = e->n_decay, n = e->n_update_end(), wend = e->layers_end();
    if (clip) CK(e->enqueue_clip(e->G, n, ws, st));
    CK(e->prof_mark(2 * NL, st));
    e->upd_ridden = ride ? wend - e->ride_cursor - e->ride_hopped : 0; e->upd_swept = n - e->upd_ridden - e->frz_elems;
    e->upd_segments = e->n_classes > 0 ? (int)e->seg_class.size() : 0;
    const bool classed = e->n_classes > 0;
    const WordSkip skip = e->word_skip(ws);
    if (classed || e->one_sweep || skip.stamp) {
        const bool keep = e->keep_in_step(), one = classed || e->one_sweep;
        const size_t kb = keep ? e->stale_begin : 0, ke = keep ? e->stale_end : 0;
        const int slots[2] = {0, 1};
        AdamPieces all;
        if (classed) CK(e->sweep_pieces(all, 0, ride ? e->ride_cursor : wend, wend, n, true, kb, ke));
        else CK(e->cut_pieces(all, {0, nd, n}, slots, nullptr, 0, ride ? e->ride_cursor : 0, ride ? wend : 0, n));
        for (int k = 0; k < (one ? 1 : all.count); ++k) {
            AdamPieces p = all;
            if (!one) { p = AdamPieces{}; p.begin4[0] = all.begin4[k]; p.start4[1] = all.start4[k + 1] - all.start4[k]; p.slot[0] = all.slot[k]; p.count = p.clear_first = 1; }
            CK(adamw_sweep(e->P, e->G, m, v, e->c.dtype == DT_BF16 ? (void*)e->SH : nullptr, p, e->sh_begin, e->sh_end, kb, ke,
                           classed ? e->class_state(ws) : e->adam_state(ws), skip, st));
        }
        return e->prof_mark(2 * NL + 1, st);
    }
    const AdamArgs none = {};
    if (ride) CK(adamw_decay_range(e, m, v, 0, e->ride_cursor, st));       // what no launch carried (layer 0 always)
    CK(adamw_decay_range(e, m, v, ride ? wend : 0, nd, st));
    CK(adamw_step(e->P + nd, e->G + nd, m + nd, v + nd, nullptr, n - nd, 0, 0, 0, none, 1, st, e->adam_state(ws) + 1));
    return e->prof_mark(2 * NL + 1, st);
}

// AdamW over [b, en) of the decay slab inside a data-parallel step.  Sharded update (comm->shard): of every chunk of layer GEMM weights
// inside the range only this rank's slice and the replicated remainder are updated (csrc/comm.h: dp_shard_slice); the other slices'
// gradient copies were not reduced here -- they are dead, and cleared unless the next backward overwrites them anyway.
template <class E>
int adamw_decay_range_dp(E* e, const mb_comm* comm, const DpSpec& sp, float* m, float* v, size_t b, size_t en, hipStream_t st) {
    if (!comm->shard) return adamw_decay_range(e, m, v, b, en, st);
    std::vector<std::pair<size_t, size_t>> ch(sp.chunk.begin(), sp.chunk.begin() + sp.n_sharded);      // (the rest is replicated)
    std::sort(ch.begin(), ch.end());
    size_t cur = b;
    ZeroRanges dead = {};
    for (const auto& c : ch) {
        if (c.second <= cur || c.first >= en) continue;
        if (c.first < cur || c.second > en) return MB_ERR_MODE;          // (ranges are unions of whole chunks)
        CK(adamw_decay_range(e, m, v, cur, c.first, st));
        const ShardSlice sl = dp_shard_slice(comm, c.first, c.second);
        CK(adamw_decay_range(e, m, v, sl.mine_b, sl.mine_e, st));
        CK(adamw_decay_range(e, m, v, sl.rem_b, sl.rem_e, st));
        if (!e->keep_in_step()) {
            if (dead.n + 2 > MB_ZERO_MAX) { CK(zero_fill_ranges(dead, st)); dead = ZeroRanges{}; }       // (add() drops what does not fit)
            dead.add(e->G + c.first, (sl.mine_b - c.first) * 4);
            dead.add(e->G + sl.mine_e, (sl.rem_b - sl.mine_e) * 4);
        }
        cur = c.second;
    }
    if (dead.n) CK(zero_fill_ranges(dead, st));
    return adamw_decay_range(e, m, v, cur, en, st);
}

// The kernels of segment `seg`.  forward(l0, l1, first, last, logits, loss, loss_run, st) = the engine's forward of layers [l0, l1) on
// the staged batch; backward(stage_begin, stage_end, loss_scale, st) = its backward stages on the staged labels.
template <class E, class Forward, class Backward>
int enqueue_step_dp(E* e, int seg, const std::vector<int>& plan, const mb_comm* comm, const DpSpec& sp, float* logits, float* loss,
                    float* loss_run, float* m, float* v, float loss_scale, hipStream_t st, Forward& forward, Backward& backward) {
    const int NL = e->n_layers(), nb = (int)plan.size();
    // sharded update with several pieces: nf forward-only segments in front (piece k = the layers of chunk nb-1-k, lowest first); the
    // last piece -- the top layers + head -- stays in front of the first backward segment
    const int nf = comm->nf;
    auto layers_of = [&](int chunk, int& l0, int& l1) { l1 = NL; for (int s = 0; s < chunk; ++s) l1 -= plan[s]; l0 = l1 - plan[chunk]; };
    if (seg <= nf) {
        int l0 = 0, l1 = NL;
        if (nf > 0) layers_of(nb - 1 - seg, l0, l1);
        CK(forward(l0, l1, seg == 0, seg == nf, logits, loss, loss_run, st));
        if (seg < nf) return MB_OK;
    }
    seg -= nf;
    if (seg < nb) {
        int done = 0;
        for (int s = 0; s < seg; ++s) done += plan[s];
        // backward stages: 0 = head, 1 .. NL = layers NL-1 .. 0, NL+1 = the embedding stage
        return backward(seg == 0 ? 0 : 1 + done, seg == nb - 1 ? NL + 2 : 1 + done + plan[seg], loss_scale, st);
    }
    const AdamArgs none = {};
    const size_t nd = e->n_decay, n = e->n_update_end(), wend = e->layers_end();
    const size_t split = e->layer_begin(plan[nb - 1] < NL ? plan[nb - 1] : 0);      // first GEMM weight of the layers reduced early
    if (seg == nb) {
        CK(e->prof_mark(2 * NL, st));
        if (nb > 1) return adamw_decay_range_dp(e, comm, sp, m, v, split, wend, st);
        // (one backward segment: no early range -- dp_between waited for everything -- so this segment takes the no-decay slab)
        return adamw_step(e->P + nd, e->G + nd, m + nd, v + nd, nullptr, n - nd, 0, 0, 0, none, 1, st, e->adam_state(e->ws) + 1);
    }
    CK(adamw_decay_range_dp(e, comm, sp, m, v, 0, nb > 1 ? split : wend, st));
    CK(adamw_decay_range(e, m, v, wend, nd, st));
    if (nb > 1) CK(adamw_step(e->P + nd, e->G + nd, m + nd, v + nd, nullptr, n - nd, 0, 0, 0, none, 1, st, e->adam_state(e->ws) + 1));
    return e->prof_mark(2 * NL + 1, st);
}

// The step behind an engine's argument checks: the plan and what it exchanges, the shard checks, then dp_step_begin -> training = 1 ->
// prepare(T, st) (the engine's prepare-pass) -> the graphs' variant -> train_step_impl over nf + nb + 2 segments.
template <class E, class Prepare, class Forward, class Backward>
int train_step_dp(E* e, const int64_t* input_ids, const float* visual, const float* acoustic, const int64_t* attention_mask,
                  const int64_t* token_type_ids, const float* labels, int B, int L, uint64_t seed, uint64_t step, float* logits, float* loss,
                  float* loss_run, float* m, float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int opt_step,
                  int correct_bias, float grad_scale, float loss_scale, int mode, hipStream_t st, mb_comm* comm, Prepare prepare,
                  Forward forward, Backward backward) {
    const auto& c = e->c;
    const int NL = e->n_layers();
    const std::vector<int> plan = dp_chunk_plan(NL);
    const int nb = (int)plan.size();
    DpSpec sp;
    for (int s = 0, hi = NL; s < nb; ++s) {            // segment s finishes layers [hi - plan[s], hi)
        const int lo_l = hi - plan[s];
        sp.chunk.push_back({e->layer_begin(lo_l), hi < NL ? e->layer_begin(hi) : e->layers_end()});
        hi = lo_l;
    }
    sp.tail_begin = e->layers_end(); sp.tail_end = e->n_update_end();
    sp.word_off = e->word; sp.word_rows = c.vocab_size; sp.H = e->width();
    sp.ids = (const int64_t*)(e->ws + e->ws_in_ids); sp.T = B * L;
    sp.n_sharded = dp_sharded_chunks(comm, nb);
    const int nf = dp_forward_segments(comm, nb);
    comm->nf = nf;
    if (comm->shard) {
        // what the next forward reads of a layer's GEMM weights: their bf16 shadow (bf16 mode) or the fp32 parameters themselves
        const bool bf = c.dtype == DT_BF16;
        for (const auto& ch : sp.chunk)
            if (bf && (!e->SH || ch.first < e->sh_begin || ch.second > e->sh_end)) return MB_ERR_MODE;
        sp.gather_base = bf ? (char*)e->SH : (char*)e->P; sp.gather_es = bf ? 2 : 4;
    }
    CK(dp_step_begin(comm, st, nf > 0));          // (sharded update: the previous step's all-gathers -- cut mode: awaited piece by piece)
    e->training = 1;
    CK(prepare(B * L, st));
    // (the plan is part of the graphs' identity: nseg alone would not tell 4,4,2,2 from 2,2,4,4)
    unsigned vh = 1;                                   // (unsigned: deep models have many pieces, the hash may wrap)
    for (int x : plan) vh = vh * 13u + (unsigned)x;
    vh = (vh * 4u + (unsigned)comm->event_mode) * 2u + (comm->shard ? 1u : 0u);
    const int variant = (int)(vh & 0x7fffffffu) | 1;   // never 0, the single-process step's
    return train_step_impl(e, e->ws, c.visual_dim, c.acoustic_dim, c.num_labels, input_ids, visual, acoustic, attention_mask, token_type_ids,
                           labels, B, L, seed, step, logits, loss, loss_run, m, v, lr, beta1, beta2, eps, weight_decay, opt_step,
                           correct_bias, grad_scale, loss_scale, mode, e->prof, st,
                           [&](int sg, float* lg, float* ls, float* lr_, float* m_, float* v_, float sc, hipStream_t s) {
                               CK(dp_segment_begin(comm, nb, sg, s));
                               CK(enqueue_step_dp(e, sg, plan, comm, sp, lg, ls, lr_, m_, v_, sc, s, forward, backward));
                               CK(dp_segment_end(comm, nb, sg, s));
                               return (int)MB_OK;
                           },
                           nf + nb + 2, [&](int sg, hipStream_t s) { return dp_between(comm, sp, e->G, sg, s); }, variant, comm, dp_finish_segment_graph);
}

}  // namespace
