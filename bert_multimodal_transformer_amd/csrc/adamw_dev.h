// Device side of HF-AdamW (adamw.hip) shared with the kernels that carry an update inside their own launch (gemm.hip / gemm_pp.hip:
// AdamRide -- the optimizer update of the PREVIOUS layer's GEMM weights as extra workgroups of a layer's weight-gradient launch).
#pragma once
#include "kernels.h"

namespace mb {

// one quad of four consecutive parameters
struct AdamQuad { f32x4 p, g, m, v; };
template <bool NT> __device__ __forceinline__ AdamQuad adam_load(const float* p, const float* g, const float* m, const float* v, size_t i) {
    AdamQuad q;
    if constexpr (NT) {          // streamed once per step, never re-read before it is rewritten: keep it out of the caches
        q.p = __builtin_nontemporal_load((const f32x4*)(p + i)); q.g = __builtin_nontemporal_load((const f32x4*)(g + i));
        q.m = __builtin_nontemporal_load((const f32x4*)(m + i)); q.v = __builtin_nontemporal_load((const f32x4*)(v + i));
    } else {
        q.p = *(const f32x4*)(p + i); q.g = *(const f32x4*)(g + i); q.m = *(const f32x4*)(m + i); q.v = *(const f32x4*)(v + i);
    }
    return q;
}
// ... whose gradient is only loaded when `live`: the caller knows it to be +0.0f otherwise (kernels.h WordSkip) and pairs this with
// zero_grad = 0 in adam_update_store, so the quad's gradient is neither read nor written -- and the arithmetic sees the same +0.0f
template <bool NT> __device__ __forceinline__ AdamQuad adam_load(const float* p, const float* g, const float* m, const float* v, size_t i, bool live) {
    AdamQuad q;
    q.g = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (NT) {
        q.p = __builtin_nontemporal_load((const f32x4*)(p + i));
        if (live) q.g = __builtin_nontemporal_load((const f32x4*)(g + i));
        q.m = __builtin_nontemporal_load((const f32x4*)(m + i)); q.v = __builtin_nontemporal_load((const f32x4*)(v + i));
    } else {
        q.p = *(const f32x4*)(p + i);
        if (live) q.g = *(const f32x4*)(g + i);
        q.m = *(const f32x4*)(m + i); q.v = *(const f32x4*)(v + i);
    }
    return q;
}
// ... and the parameters alone of a quad whose moments are known to be +0.0f and whose gradient is +0.0f too (kernels.h WordSkip:
// MB_STAMP_SEEN clear, state[2] set): adam_decay_store is the other half
template <bool NT> __device__ __forceinline__ f32x4 adam_load_p(const float* p, size_t i) {
    if constexpr (NT) return __builtin_nontemporal_load((const f32x4*)(p + i));
    else return *(const f32x4*)(p + i);
}
// What adam_update_store does to such a quad: with g = m = v = +0.0f the moments come out +0.0f again and p - step_size * (0 / (0 + eps))
// is p bit for bit (the host vouches for the scalars: engine_common.h StepMixin::lazy_scalars_ok), so only the decoupled decay is
// left -- the same statement, contraction off -- and m, v and g are neither read nor written.
template <bool NT> __device__ __forceinline__ void adam_decay_store(f32x4 qp, float* p, bf16* shadow, size_t i, float decay, size_t n_decay,
                                                                    size_t sh_begin, size_t sh_end) {
#pragma clang fp contract(off)
    if (i < n_decay && decay > 0.f) qp -= decay * qp;
    if constexpr (NT) __builtin_nontemporal_store(qp, (f32x4*)(p + i));
    else *(f32x4*)(p + i) = qp;
    if (shadow && i >= sh_begin && i < sh_end) store4(shadow + i, qp);
}
template <bool NT> __device__ __forceinline__ void adam_update_store(AdamQuad q, float* p, float* g, float* m, float* v, bf16* shadow, size_t i,
                                                                     const AdamArgs& a, float omb1, float omb2, float decay, size_t n_decay,
                                                                     size_t sh_begin, size_t sh_end, size_t keep_begin, size_t keep_end, int zero_grad) {
    // No FMA contraction: the update is inlined into several kernels (the sweep, the riders of a weight-gradient launch), and left to the
    // compiler each context fuses different multiply-add pairs -- 1-ulp differences in m / v from the second step on (measured:
    // scripts/exp/ride_diag.py).  Unfused is also the reference's arithmetic: exp_avg.mul_(b1).add_(g, alpha=1-b1) rounds twice.
#pragma clang fp contract(off)
    q.g *= a.grad_scale;
    q.m = a.beta1 * q.m + omb1 * q.g;
    q.v = a.beta2 * q.v + omb2 * q.g * q.g;
#pragma unroll
    for (int r = 0; r < 4; ++r) q.p[r] -= a.step_size * (q.m[r] / (sqrtf(q.v[r]) + a.eps));
    if (i < n_decay && decay > 0.f) q.p -= decay * q.p;
    const bool zg = zero_grad && !(i >= keep_begin && i < keep_end);
    if constexpr (NT) {
        __builtin_nontemporal_store(q.p, (f32x4*)(p + i));
        __builtin_nontemporal_store(q.m, (f32x4*)(m + i));
        __builtin_nontemporal_store(q.v, (f32x4*)(v + i));
        if (zg) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, (f32x4*)(g + i));
    } else {
        *(f32x4*)(p + i) = q.p;
        *(f32x4*)(m + i) = q.m;
        *(f32x4*)(v + i) = q.v;
        if (zg) *(f32x4*)(g + i) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (shadow && i >= sh_begin && i < sh_end) store4(shadow + i, q.p);
}

// The update loop of adamw.hip's kernels: a 256-thread block walks quads [begin, end) of the buffers (`begin` is this thread's first
// quad) with two quads of every stream in flight.  skip_on (kernels.h WordSkip): a quad of [ws.begin, ws.end) whose row carries no
// stamp `stamp_no` gets g = +0.0f without the load and keeps the zero it has without the store; a wave may straddle two rows (768
// floats = three waves of quads), which costs a divergent load.  lazy_on (with skip_on only): such a quad whose row does not carry
// MB_STAMP_SEEN either -- the one table word tells both -- has zero moments: adam_load_p / adam_decay_store, 8 instead of 24 bytes per
// parameter.  A literal `false` folds all of that away.
// (The element index is formed inside the bounds check: hoisted above it, the single-range kernel takes 68 VGPRs instead of 62 and
//  loses its eighth wave per SIMD -- tests/test_host_cpu.py::test_adamw_kernels_keep_their_residency.)
template <bool NT>
__device__ __forceinline__ void adam_span(float* p, float* g, float* m, float* v, bf16* shadow, size_t begin, size_t end, const AdamArgs& a,
                                          size_t n_decay, size_t sh_begin, size_t sh_end, size_t keep_begin, size_t keep_end, int zero_grad,
                                          bool skip_on, bool lazy_on, const WordSkip& ws, uint32_t stamp_no) {
    constexpr int UNR = 2; const size_t stride = 256;
    const float omb1 = 1.0f - a.beta1, omb2 = 1.0f - a.beta2;
    const float decay = a.lr * a.weight_decay;
    for (size_t i4 = begin; i4 < end; i4 += stride * UNR) {
        AdamQuad q[UNR];
        bool live[UNR], lazy[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            live[u] = true; lazy[u] = false;
            if (i4 + u * stride < end) {
                const size_t i = (i4 + u * stride) * 4;
                if (skip_on && i >= ws.begin && i < ws.end) {
                    const uint32_t w = ws.stamp[(uint32_t)(i - ws.begin) / ws.row_len];
                    live[u] = (w & ~MB_STAMP_SEEN) == stamp_no;
                    lazy[u] = lazy_on && !live[u] && !(w & MB_STAMP_SEEN);
                }
                if (lazy[u]) q[u].p = adam_load_p<NT>(p, i);
                else q[u] = adam_load<NT>(p, g, m, v, i, live[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (i4 + u * stride < end) {
                if (lazy[u]) adam_decay_store<NT>(q[u].p, p, shadow, (i4 + u * stride) * 4, decay, n_decay, sh_begin, sh_end);
                else adam_update_store<NT>(q[u], p, g, m, v, shadow, (i4 + u * stride) * 4, a, omb1, omb2, decay, n_decay, sh_begin, sh_end,
                                           keep_begin, keep_end, live[u] ? zero_grad : 0);
            }
    }
}

// One rider workgroup (kernels.h AdamRide): workgroup `rb` of `r.blocks` owns one contiguous range of every stream.  A rider has a
// CU's memory pipeline to itself but only its own 4-8 waves to cover the HBM latency with, so the loop is a two-stage software
// pipeline: the loads of one half-iteration (UNR quads per stream and thread) are in flight while the other half is updated and
// stored.  Same arithmetic, same order as adam_span (adam_update_store, contraction off): the same bits.
template <int NTHREADS, int UNR>
__device__ __forceinline__ void adam_ride_block(const AdamRide& r, int rb) {
    if (r.n4 == 0) return;
    const AdamArgs a = *r.dyn;
    const float omb1 = 1.0f - a.beta1, omb2 = 1.0f - a.beta2;
    const float decay = a.lr * a.weight_decay;
    const size_t per = ((r.n4 + r.blocks - 1) / r.blocks + NTHREADS - 1) / NTHREADS * NTHREADS;
    const size_t begin = (size_t)rb * per + threadIdx.x;
    const size_t end = r.n4 < (size_t)(rb + 1) * per ? r.n4 : (size_t)(rb + 1) * per;
    const size_t all = ~(size_t)0;
    constexpr size_t half = (size_t)NTHREADS * UNR;          // quads per half-iteration
    AdamQuad qa[UNR], qb[UNR];
    auto load = [&](AdamQuad (&q)[UNR], size_t i4) {
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (i4 + (size_t)u * NTHREADS < end) q[u] = adam_load<true>(r.p, r.g, r.m, r.v, (i4 + (size_t)u * NTHREADS) * 4);
    };
    auto update = [&](AdamQuad (&q)[UNR], size_t i4) {
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (i4 + (size_t)u * NTHREADS < end)
                adam_update_store<true>(q[u], r.p, r.g, r.m, r.v, r.shadow, (i4 + (size_t)u * NTHREADS) * 4, a, omb1, omb2, decay, all, 0, r.shadow ? all : 0,
                                        0, 0, r.zero_grad);
    };
    load(qa, begin);
    for (size_t i4 = begin; i4 < end; i4 += 2 * half) {
        load(qb, i4 + half);
        update(qa, i4);
        load(qa, i4 + 2 * half);
        update(qb, i4 + half);
    }
}

}  // namespace mb
