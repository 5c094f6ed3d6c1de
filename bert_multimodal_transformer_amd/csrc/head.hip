// Classification head of MAG_BertForSequenceClassification (/root/reference/bert.py:304-322) fused with the
// driver's MSE loss (/root/reference/multimodal_driver.py:372-373):
//   pooled = tanh(z)  [z = h[:,0] Wp^T + bp comes from the GEMM]  ->  dropout(0.1)  ->  logits = . Wc^T + bc
//   loss = mean((logits - labels)^2)                                  num_labels == 1 (the driver's regression)
//   loss = mean_b(logsumexp(logits_b) - logits_b[label_b])            num_labels  > 1 (bert.py:318-320 / xlnet.py:519-522:
//          CrossEntropyLoss; labels[b] then holds the class index of sample b as a float)
// Other objectives (kernels.h HeadLoss, include/magbert_hip.h mb_*_set_head_loss): the kind is a kernel argument, uniform for the
// launch -- a scalar branch, as EPI_BIAS_ACT switches its activation.  The per-element kinds read labels[b * nl + k]:
//   mse        mean (x - y)^2                                         l1   mean |x - y|   (gradient 0 at x == y)
//   smooth_l1  mean of 0.5 d^2 / beta where |d| < beta, else |d| - 0.5 beta   (beta == 0: the expressions of l1)
//   bce        mean of (1 - y) x + (1 + (p_k - 1) y) (max(-x, 0) + log1p(exp(-|x|)))   p = pos_weight [nl] or null
//   weighted cross entropy   sum_b w[y_b] nll_b / sum_b w[y_b]: every wave sums w[y_b] over the batch itself, in a fixed order
//              (lane-strided, then wave_sum), so every block holds the same bits without a launch or an atomic of its own
// Modifiers (kernels.h HeadLoss: smoothing, gamma, ignore; mb_head_loss of include/magbert_hip.h), kernel arguments like the kind:
//   cross entropy, q = softmax(x_b), kept = (y_b != ignore), W = sum over kept b of w[y_b] (w = 1 without weights: the kept count):
//     smoothing e   [ (1 - e) sum_kept w[y_b] (-log q_by) + (e / C) sum_kept sum_k w_k (-log q_bk) ] / W
//     focal gamma   sum_kept w[y_b] (1 - p)^gamma (-log p) / W,  p = q_by;  1 - p is summed from the non-target exponentials and
//                   log p taken by log1p of it where p > 0.5, so neither tail cancels; gamma == 0 runs the weighted expressions
//     a label equal to `ignore` is left out even where it names a class (the test comes before the weight lookup); its sample
//     gives 0 to the loss, to W and to every gradient, and its dz row is written as zeros
//     W == 0 (every sample ignored, or every kept one at weight 0): loss 0 and all gradients 0 -- torch returns NaN there; a NaN
//     must not reach the AdamW moments
//   bce, focal gamma   mean of (1 - p_t)^gamma l,  l = the bce term above,  1 - p_t = y sigmoid(-x) + (1 - y) sigmoid(x)
//   W is the generalised head_weight_sum: every wave sums it itself in the same lane-strided order -- no launch, no atomic.
//   A launch with any modifier set runs a third instantiation (OPT), so the two below keep the code they had.
// The default kind -- MSE at num_labels == 1, the cross entropy without weights otherwise -- is an instantiation of its own (DEF), with
// the expressions the kernels always had; `mse` at one label and the unweighted `cross_entropy` go through the same expressions.
// One wave per sample; H = 256 * CH (CH chunks of 4 columns per lane: CH = 3 is bert-base, 4 bert-large).  Tiny, launch-latency bound.
#include <algorithm>
#include "kernels.h"

namespace mb {

__device__ __forceinline__ float head_sign(float d) { return (float)(d > 0.f) - (float)(d < 0.f); }      // sign(0) = 0
// loss of one logit x against its target y under a per-element kind (class k: bce's pos_weight entry)
__device__ __forceinline__ float head_loss_term(const HeadLoss hl, float x, float y, int k) {
    const float d = x - y;
    switch (hl.kind) {
        case HL_MSE: return d * d;
        case HL_L1: return fabsf(d);
        case HL_SMOOTH_L1: {
            const float ad = fabsf(d);
            return ad < hl.param ? 0.5f * d * d / hl.param : ad - 0.5f * hl.param;
        }
        default: {      // HL_BCE
            const float lw = hl.vec ? 1.0f + (hl.vec[k] - 1.0f) * y : 1.0f;
            return (1.0f - y) * x + lw * (fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))));
        }
    }
}
// ... and its derivative in x (before the division by B * nl)
__device__ __forceinline__ float head_loss_grad(const HeadLoss hl, float x, float y, int k) {
    const float d = x - y;
    switch (hl.kind) {
        case HL_MSE: return 2.0f * d;
        case HL_L1: return head_sign(d);
        case HL_SMOOTH_L1: return fabsf(d) < hl.param ? d / hl.param : head_sign(d);
        default: {      // HL_BCE: sigmoid(-x) from exp(-|x|), so neither tail overflows
            const float lw = hl.vec ? 1.0f + (hl.vec[k] - 1.0f) * y : 1.0f;
            const float e = expf(-fabsf(x));
            const float sg = (x >= 0.f ? e : 1.0f) / (1.0f + e);
            return (1.0f - y) - lw * sg;
        }
    }
}
// u^g for u >= 0: 1 at g == 0 whatever u is (gamma = 1 at 1 - p == 0 must give 1, not 0 * inf)
__device__ __forceinline__ float head_pow(float u, float g) { return g == 0.f ? 1.0f : (u > 0.f ? powf(u, g) : 0.f); }
// sigmoid focal loss on top of bce's term l: m^gamma l with m = 1 - p_t = y sigmoid(-x) + (1 - y) sigmoid(x); both sigmoids from
// exp(-|x|), so neither tail overflows
__device__ __forceinline__ float head_bce_focal_term(const HeadLoss hl, float x, float y, int k) {
    const float e = expf(-fabsf(x));
    const float sn = (x >= 0.f ? e : 1.0f) / (1.0f + e), sp = (x >= 0.f ? 1.0f : e) / (1.0f + e);      // sigmoid(-x), sigmoid(x)
    const float m = y * sn + (1.0f - y) * sp;
    return head_pow(m, hl.gamma) * head_loss_term(hl, x, y, k);
}
// ... and its derivative: gamma m^(gamma-1) m' l + m^gamma l',  m' = sigmoid(x) sigmoid(-x) (1 - 2 y)
__device__ __forceinline__ float head_bce_focal_grad(const HeadLoss hl, float x, float y, int k) {
    const float e = expf(-fabsf(x));
    const float sn = (x >= 0.f ? e : 1.0f) / (1.0f + e), sp = (x >= 0.f ? 1.0f : e) / (1.0f + e);
    const float m = y * sn + (1.0f - y) * sp;
    const float dm = sp * sn * (1.0f - 2.0f * y);
    return hl.gamma * head_pow(m, hl.gamma - 1.0f) * dm * head_loss_term(hl, x, y, k) + head_pow(m, hl.gamma) * head_loss_grad(hl, x, y, k);
}
// weighted cross entropy: w[class], 0 for an index outside the table (the hosts refuse such labels; nothing is read out of bounds)
__device__ __forceinline__ float head_class_weight(const float* __restrict__ w, int y, int nl) {
    return (unsigned)y < (unsigned)nl ? w[y] : 0.f;
}
// ... and the summed weights of the batch's targets: the same bits in every wave of every block (whole waves call this)
__device__ __forceinline__ float head_weight_sum(const float* __restrict__ labels, const float* __restrict__ w, int B, int nl, int lane) {
    float t = 0.f;
    for (int i = lane; i < B; i += 64) t += head_class_weight(w, (int)labels[i], nl);
    return wave_sum(t);
}
// ... generalised (OPT): the weights -- without a table, the count -- of the samples whose label is not `ignore`, in the same order
__device__ __forceinline__ float head_kept_sum(const float* __restrict__ labels, const HeadLoss hl, int B, int nl, int lane) {
    float t = 0.f;
    for (int i = lane; i < B; i += 64) {
        const int y = (int)labels[i];
        if (hl.has_ignore && y == hl.ignore) continue;
        t += hl.vec ? head_class_weight(hl.vec, y, nl) : 1.0f;
    }
    return wave_sum(t);
}
// focal factors of one kept sample from its logits x[0, nl), their maximum mx and the class y: omp = 1 - p summed from the non-target
// exponentials, nlp = -log p (log1p where p > 0.5).  -> (1 - p)^gamma; *grad = (1 - p)^gamma + gamma p (1 - p)^(gamma-1) (-log p), the
// factor in front of (q_k - [k == y]) in the logit gradient; *se_ = sum_k exp(x_k - mx), so that q_k = expf(x_k - mx) / *se_.
// (1 - p)^gamma multiplies the relative error of 1 - p by gamma: the exponentials are expf of x_k - mx, not __expf of x_k - lse
__device__ __forceinline__ float head_focal(const float* __restrict__ x, int nl, int y, float mx, float gamma, float* omp_, float* nlp_,
                                            float* grad, float* se_) {
    float se = 0.f, so = 0.f, et = 0.f, xt = mx;
    for (int k = 0; k < nl; ++k) {
        const float e = expf(x[k] - mx);
        se += e;
        if (k == y) { et = e; xt = x[k]; }
        else so += e;
    }
    const float omp = so / se;
    const float nlp = omp < 0.5f ? -log1pf(-omp) : logf(se) - (xt - mx);
    const float pw = head_pow(omp, gamma);
    *omp_ = omp;
    *nlp_ = nlp;
    *se_ = se;
    *grad = pw + gamma * (et / se) * head_pow(omp, gamma - 1.0f) * nlp;
    return pw;
}

// Atomics on ONE address serialise at the L2 (measured: 48 samples x 2 atomics = most of a 15 us launch), so the four waves of
// a block meet in LDS first: one loss atomic per block, one classifier-gradient atomic per column per block.
// DEF: the default kind as an instantiation of its own -- MSE at nl == 1, cross entropy otherwise, written with the expressions and
// the label indexing the kernels had before there was a choice, so that the step every untouched model runs compiles to what it was
// (the general form costs the forward 11 to 22 VGPRs and measured +0.2 % on the MAG-BERT step: profiles/head_loss.txt).
// V: which instantiation -- GEN (a kind, no modifier), DEF (below), OPT (a kind with modifiers; kernels.h head_loss_modified)
enum { HV_GEN = 0, HV_DEF = 1, HV_OPT = 2 };
template <int CH, int V>
__global__ void __launch_bounds__(256) head_fwd_kernel(const float* __restrict__ z, const float* __restrict__ Wc,
                                                       const float* __restrict__ bc, const float* __restrict__ labels,
                                                       float* __restrict__ pooled, float* __restrict__ logits, float* loss,
                                                       float* loss_run, int B, int nl, DropKey drop, HeadLoss hl_) {
    constexpr bool DEF = V == HV_DEF, OPT = V == HV_OPT;
    // (DEF: what the per-element branch runs; `ce` picks the branch.  GEN: the modifiers are compile-time zeros)
    const HeadLoss hl = DEF ? HeadLoss{HL_MSE, 0.f, nullptr} : OPT ? hl_ : HeadLoss{hl_.kind, hl_.param, hl_.vec};
    drop.resolve();
    constexpr int H = CH * 256;
    __shared__ float lsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    const bool valid = b < B;
    float mine = 0.f;
    if (valid) {
        f32x4 pd[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int col = (c * 64 + lane) * 4;
            f32x4 t = *(const f32x4*)(z + (size_t)b * H + col);
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = tanhf(t[r]);
            *(f32x4*)(pooled + (size_t)b * H + col) = t;
            const uint32_t idx = (uint32_t)b * H + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) pd[c][r] = t[r] * drop_mult(drop, idx + r);
        }
        // cross entropy (nl > 1): online log-sum-exp over the classes, kept by lane 0
        float mx = -3.0e38f, se = 0.f, tgt = 0.f;
        const bool ce = DEF ? nl > 1 : hl.kind == HL_CE;               // uniform
        const int y = (labels && ce) ? (int)labels[b] : -1;
        const float fN = DEF ? (float)B : (float)(B * nl);             // per-element kinds: the mean runs over B * nl
        const float wtot = OPT ? ((labels && ce) ? head_kept_sum(labels, hl, B, nl, lane) : 0.f)
                               : (labels && ce && hl.vec) ? head_weight_sum(labels, hl.vec, B, nl, lane) : 0.f;
        for (int k = 0; k < nl; ++k) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const f32x4 w = *(const f32x4*)(Wc + (size_t)k * H + (c * 64 + lane) * 4);
                const f32x4 t = pd[c] * w;
                s += (t[0] + t[1]) + (t[2] + t[3]);
            }
            s = wave_sum(s) + bc[k];
            if (lane == 0) {
                logits[(size_t)b * nl + k] = s;
                if (OPT && labels && !ce && hl.gamma != 0.f) {
                    mine += head_bce_focal_term(hl, s, labels[(size_t)b * nl + k], k) / fN;
                } else if (labels && !ce) {
                    mine += head_loss_term(hl, s, DEF ? labels[b] : labels[(size_t)b * nl + k], k) / fN;
                } else if (labels) {
                    const float nm = fmaxf(mx, s);
                    se = se * __expf(mx - nm) + __expf(s - nm);
                    mx = nm;
                    if (k == y) tgt = s;
                }
            }
        }
        if (OPT && lane == 0 && labels && ce) {
            // lane 0 reads back the logits it has just written: the smoothing and focal sums need the finished log-sum-exp
            const float* xb = logits + (size_t)b * nl;
            const float wy = hl.vec ? head_class_weight(hl.vec, y, nl) : 1.0f;
            if ((hl.has_ignore && y == hl.ignore) || !(wtot > 0.f)) {
                mine = 0.f;
            } else if (hl.gamma != 0.f) {
                float omp, nlp, ga, fse;
                const float pw = head_focal(xb, nl, y, mx, hl.gamma, &omp, &nlp, &ga, &fse);
                mine = wy * pw * nlp / wtot;
            } else {
                float v = wy * (mx + __logf(se) - tgt);
                if (hl.smoothing != 0.f) {
                    const float lse = mx + __logf(se);
                    float sm = 0.f;
                    for (int k = 0; k < nl; ++k) sm += (hl.vec ? hl.vec[k] : 1.0f) * (lse - xb[k]);
                    v = (1.0f - hl.smoothing) * v + hl.smoothing / (float)nl * sm;
                }
                mine = v / wtot;
            }
        } else if (lane == 0 && labels && ce) {
            if (hl.vec) mine = head_class_weight(hl.vec, y, nl) * (mx + __logf(se) - tgt) / wtot;
            else mine = (mx + __logf(se) - tgt) / (float)B;
        }
    }
    if (labels == nullptr || (loss == nullptr && loss_run == nullptr)) return;      // uniform
    if (lane == 0) lsum[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float t = (lsum[0] + lsum[1]) + (lsum[2] + lsum[3]);
        if (loss) atomicAdd(loss, t);
        if (loss_run) atomicAdd(loss_run, t);
    }
}

template <class T, int CH, int V>
__global__ void __launch_bounds__(256) head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ logits,
                                                       const float* __restrict__ labels, float loss_scale,
                                                       const float* __restrict__ pooled, const float* __restrict__ Wc,
                                                       T* __restrict__ dz, float* dWc, float* dbc, int B, int nl,
                                                       DropKey drop, GradAcc acc, float* dbp, u32x4* __restrict__ zero_p,
                                                       size_t zero_n16, int nb, HeadLoss hl_) {
    constexpr bool DEF = V == HV_DEF, OPT = V == HV_OPT;
    const HeadLoss hl = DEF ? HeadLoss{HL_MSE, 0.f, nullptr} : OPT ? hl_ : HeadLoss{hl_.kind, hl_.param, hl_.vec};
    // blocks [nb, gridDim.x): clear zero_p[0, zero_n16) -- the token-gradient buffer whose [CLS] / last-token rows the next launch
    // fills (one launch less per backward than a separate zero_fill)
    if ((int)blockIdx.x >= nb) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (size_t i = (size_t)(blockIdx.x - nb) * 256 + threadIdx.x; i < zero_n16; i += (size_t)(gridDim.x - nb) * 256) zero_p[i] = z;
        return;
    }
    drop.resolve();
    constexpr int H = CH * 256;
    __shared__ float wsum[4][H];
    __shared__ float bsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    const bool valid = b < B;
    const int bb = valid ? b : 0;
    f32x4 dpd[CH], pl[CH], dm[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
        dpd[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        pl[c] = *(const f32x4*)(pooled + (size_t)bb * H + col);
        const uint32_t idx = (uint32_t)bb * H + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) dm[c][r] = drop_mult(drop, idx + r);
    }
    float lse = 0.f;
    int y = -1;
    const bool ce = DEF ? nl > 1 : hl.kind == HL_CE;           // uniform
    const float fN = DEF ? (float)B : (float)(B * nl);
    float wy = 1.0f, wtot = 0.f;                // weighted cross entropy: this sample's class weight, the batch's summed weights
    if (OPT) { if (!dlogits && ce) wtot = head_kept_sum(labels, hl, B, nl, lane); }
    else if (!dlogits && ce && hl.vec) wtot = head_weight_sum(labels, hl.vec, B, nl, lane);
    // OPT: `live` = this sample has a gradient (kept, and W > 0); wall = sum_j w_j (smoothing); omp, fg, fmx, fse = head_focal's 1 - p,
    // factor, maximum and sum of exponentials
    bool live = true;
    float wall = 0.f, omp = 0.f, fg = 1.0f, fmx = 0.f, fse = 1.0f;
    if (valid && !dlogits && ce) {              // cross entropy: d logit_k = (softmax_k - [k == label]) / B
        float mx = -3.0e38f;
        for (int k = 0; k < nl; ++k) mx = fmaxf(mx, logits[(size_t)b * nl + k]);
        float se = 0.f;
        for (int k = 0; k < nl; ++k) se += __expf(logits[(size_t)b * nl + k] - mx);
        lse = mx + __logf(se);
        y = (int)labels[b];
        if (hl.vec) wy = head_class_weight(hl.vec, y, nl);
        if (OPT) {
            live = !(hl.has_ignore && y == hl.ignore) && wtot > 0.f;
            if (hl.smoothing != 0.f)
                for (int k = 0; k < nl; ++k) wall += hl.vec ? hl.vec[k] : 1.0f;
            if (live && hl.gamma != 0.f) {
                float nlp;
                fmx = mx;
                head_focal(logits + (size_t)b * nl, nl, y, mx, hl.gamma, &omp, &nlp, &fg, &fse);
            }
        }
    }
    for (int k = 0; k < nl; ++k) {
        float dl = 0.f;
        if (valid) {
            if (dlogits) dl = dlogits[(size_t)b * nl + k];
            else if (OPT && !ce && hl.gamma != 0.f) dl = head_bce_focal_grad(hl, logits[(size_t)b * nl + k], labels[(size_t)b * nl + k], k) / fN * loss_scale;
            else if (OPT && ce) {
                const float q = __expf(logits[(size_t)b * nl + k] - lse);
                if (!live) dl = 0.f;                // an ignored sample, or W == 0: exactly 0 (the dz row below is still written)
                else if (hl.gamma != 0.f) dl = wy * fg * (k == y ? -omp : expf(logits[(size_t)b * nl + k] - fmx) / fse) / wtot * loss_scale;
                else if (hl.smoothing != 0.f) {
                    const float wk = hl.vec ? hl.vec[k] : 1.0f;
                    dl = ((1.0f - hl.smoothing) * (wy * (q - (k == y ? 1.0f : 0.0f))) + hl.smoothing / (float)nl * (q * wall - wk)) / wtot * loss_scale;
                } else dl = wy * (q - (k == y ? 1.0f : 0.0f)) / wtot * loss_scale;
            }
            else if (!ce) dl = (DEF ? head_loss_grad(hl, logits[b], labels[b], k) : head_loss_grad(hl, logits[(size_t)b * nl + k], labels[(size_t)b * nl + k], k)) / fN * loss_scale;
            else if (hl.vec) dl = wy * (__expf(logits[(size_t)b * nl + k] - lse) - (k == y ? 1.0f : 0.0f)) / wtot * loss_scale;
            else dl = (__expf(logits[(size_t)b * nl + k] - lse) - (k == y ? 1.0f : 0.0f)) / (float)B * loss_scale;
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int col = (c * 64 + lane) * 4;
            dpd[c] += dl * *(const f32x4*)(Wc + (size_t)k * H + col);
            if (dWc) *(f32x4*)(&wsum[wave][col]) = dl * pl[c] * dm[c];
        }
        if (lane == 0) bsum[wave] = dl;
        if (dWc || dbc) {                 // uniform
            __syncthreads();
            if (dWc)
                for (int col = threadIdx.x; col < H; col += 256)
                    grad_add(acc, dWc + (size_t)k * H + col, (wsum[0][col] + wsum[1][col]) + (wsum[2][col] + wsum[3][col]));
            if (dbc && threadIdx.x == 0) grad_add(acc, dbc + k, (bsum[0] + bsum[1]) + (bsum[2] + bsum[3]));
            __syncthreads();
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * 64 + lane) * 4;
        const f32x4 d = dpd[c] * dm[c] * (1.0f - pl[c] * pl[c]);       // (dpd == 0 for a wave without a sample)
        if (valid) store4(dz + (size_t)b * H + col, d);
        if (dbp) *(f32x4*)(&wsum[wave][col]) = d;
    }
    if (dbp) {                            // uniform: the pooler / summary bias gradient = column sums of dz (was a colsum launch)
        __syncthreads();
        for (int col = threadIdx.x; col < H; col += 256)
            grad_add(acc, dbp + col, (wsum[0][col] + wsum[1][col]) + (wsum[2][col] + wsum[3][col]));
    }
}

// what the kernels take: a known kind, and no vector where the kind reads none (the default kind runs the DEF instantiation)
static int head_loss_resolve(HeadLoss& hl, int nl) {
    if (!head_loss_legal(hl, nl)) return MB_ERR_ARG;
    if (!hl.has_ignore) hl.ignore = 0;
    if (hl.kind != HL_BCE && hl.kind != HL_CE) hl.vec = nullptr;
    return MB_OK;
}

int head_forward(const float* z, const float* Wc, const float* bc, const float* labels, float* pooled, float* logits,
                 float* loss, float* loss_run, int B, int H, int nl, DropKey drop, hipStream_t st, HeadLoss hl) {
    if (H != 256 && H != 512 && H != 768 && H != 1024) return MB_ERR_SHAPE;
    if (B <= 0) return MB_OK;
    if (int r = head_loss_resolve(hl, nl)) return r;
#define MB_HEAD_FWD_(CH, DEF) hipLaunchKernelGGL((head_fwd_kernel<CH, DEF>), dim3((B + 3) / 4), dim3(256), 0, st, z, Wc, bc, labels, pooled, logits, loss, \
                                                 loss_run, B, nl, drop, hl)
#define MB_HEAD_FWD(CH) do { if (hl.kind == HL_DEFAULT) MB_HEAD_FWD_(CH, HV_DEF); else if (head_loss_modified(hl)) MB_HEAD_FWD_(CH, HV_OPT); \
                             else MB_HEAD_FWD_(CH, HV_GEN); } while (0)
    switch (H / 256) { case 1: MB_HEAD_FWD(1); break; case 2: MB_HEAD_FWD(2); break; case 3: MB_HEAD_FWD(3); break; default: MB_HEAD_FWD(4); break; }
#undef MB_HEAD_FWD
#undef MB_HEAD_FWD_
    return (int)hipGetLastError();
}

int head_backward(int dtype, const float* dlogits, const float* logits, const float* labels, float loss_scale,
                  const float* pooled, const float* Wc, void* dz, float* dWc, float* dbc, int B, int H, int nl,
                  DropKey drop, hipStream_t st, GradAcc acc, float* dbp, void* zero_p, size_t zero_bytes, HeadLoss hl) {
    if (H != 256 && H != 512 && H != 768 && H != 1024) return MB_ERR_SHAPE;
    if (B <= 0) return MB_OK;
    if (int r = head_loss_resolve(hl, nl)) return r;
    if (!dlogits && !(logits && labels)) return MB_ERR_ARG;
    if (zero_bytes % 16 || ((uintptr_t)zero_p & 15)) return MB_ERR_SHAPE;
    const int nb = (B + 3) / 4;
    const size_t n16 = zero_p ? zero_bytes / 16 : 0;
    const int zb = n16 ? (int)std::min<size_t>((n16 + 1023) / 1024, 512) : 0;
    if (dtype != DT_BF16 && dtype != DT_F32) return MB_ERR_DTYPE;
#define MB_HEAD_BWD_(T, CH, DEF) hipLaunchKernelGGL((head_bwd_kernel<T, CH, DEF>), dim3(nb + zb), dim3(256), 0, st, dlogits, logits, labels, loss_scale, \
                                                    pooled, Wc, (T*)dz, dWc, dbc, B, nl, drop, acc, dbp, (u32x4*)zero_p, n16, nb, hl)
#define MB_HEAD_BWD(T, CH) do { if (hl.kind == HL_DEFAULT) MB_HEAD_BWD_(T, CH, HV_DEF); else if (head_loss_modified(hl)) MB_HEAD_BWD_(T, CH, HV_OPT); \
                                else MB_HEAD_BWD_(T, CH, HV_GEN); } while (0)
#define MB_HEAD_BWD_CH(CH) do { if (dtype == DT_BF16) MB_HEAD_BWD(bf16, CH); else MB_HEAD_BWD(float, CH); } while (0)
    switch (H / 256) { case 1: MB_HEAD_BWD_CH(1); break; case 2: MB_HEAD_BWD_CH(2); break; case 3: MB_HEAD_BWD_CH(3); break; default: MB_HEAD_BWD_CH(4); break; }
#undef MB_HEAD_BWD_CH
#undef MB_HEAD_BWD
#undef MB_HEAD_BWD_
    return (int)hipGetLastError();
}

}  // namespace mb
