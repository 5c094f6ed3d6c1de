// transformers==3.0.2 AdamW (/root/reference/multimodal_driver.py:28,345,384) as ONE launch over flat buffers.
//   m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2 ; p <- p - step_size * m / (sqrt(v) + eps) ; p <- p - lr*wd*p
// (eps OUTSIDE the sqrt and before bias correction, decoupled decay AFTER the update on the updated p --
//  not torch.optim.AdamW).  HBM-bound: reads p,g,m,v and writes p,m,v = 28 B/param, + 4 B/param to zero the
//  gradient in place (replaces optimizer.zero_grad()) + 2 B/param for the bf16 operand shadow of GEMM weights.
// The flat layout puts every weight-decayed tensor first: elements [0, n_decay) decay, the rest do not.
#include <cstdlib>
#include "kernels.h"
#include "adamw_dev.h"

namespace mb {

// One range: every block owns ONE contiguous piece of each of the seven streams and keeps two quads in flight (adam_span; round 3,
// tools/adamw_bench: 5.38 vs 5.10 TB/s for a grid-strided loop, profiles/r03_adamw_variants.txt)
template <bool NT>
__global__ void __launch_bounds__(256) adamw_range_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, bf16* __restrict__ shadow, size_t n4, size_t n_decay,
                                                          size_t sh_begin, size_t sh_end, size_t keep_begin, size_t keep_end, AdamArgs a,
                                                          const AdamArgs* __restrict__ dyn, int zero_grad) {
    if (dyn) a = *dyn;                  // replayed step graph: this step's lr / step size / gradient scale live in device memory
    const size_t per = ((n4 + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
    const size_t begin = (size_t)blockIdx.x * per + threadIdx.x, end = min(n4, (size_t)(blockIdx.x + 1) * per);
    adam_span<NT>(p, g, m, v, shadow, begin, end, a, n_decay, sh_begin, sh_end, keep_begin, keep_end, zero_grad, false, false, WordSkip{}, 0u);
}

// scalar tail (n % 4 elements) -- only hit by stand-alone tensors, the engine's flat buffers are 64-aligned
__global__ void adamw_tail_kernel(float* p, float* g, float* m, float* v, size_t begin, size_t n, size_t n_decay, AdamArgs a,
                                  const AdamArgs* dyn, int zero_grad) {
    if (dyn) a = *dyn;
    const size_t i = begin + threadIdx.x;
    if (i >= n) return;
    {
#pragma clang fp contract(off)
    const float gv = g[i] * a.grad_scale;
    const float mv = a.beta1 * m[i] + (1.0f - a.beta1) * gv;
    const float vv = a.beta2 * v[i] + (1.0f - a.beta2) * gv * gv;
    float pv = p[i] - a.step_size * (mv / (sqrtf(vv) + a.eps));
    if (i < n_decay && a.lr * a.weight_decay > 0.f) pv -= a.lr * a.weight_decay * pv;
    p[i] = pv; m[i] = mv; v[i] = vv;
    if (zero_grad) g[i] = 0.f;
    }
}

// What both launchers share.  MB_GEMM_LOG=1 (bench.py's in-run trace): how many parameters this launch covers -- with riders (kernels.h
// AdamRide) the sweep at the end of a step is no longer "all of them"; bench.py prices the step's sweep from this line, one launch, one
// line.  MB_ADAMW_NT=0: plain loads / stores (non-temporal measured 1.1 % faster per step: 4.86 vs 4.91 ms).  MB_ADAMW_GRID caps the
// grid of update blocks, which is one block per 256 quads and 16 per CU at most otherwise.
struct AdamLaunch { bool nt; unsigned grid; };
static int adam_launch(const float* p, const float* g, const float* m, const float* v, size_t n, size_t n4, AdamLaunch* out) {
    static int log = -1, nt = -1, vgrid = 0;
    if (log < 0) {
        const char* e = getenv("MB_GEMM_LOG"); log = e ? atoi(e) : 0;
        e = getenv("MB_ADAMW_NT"); nt = e ? atoi(e) : 1;
        e = getenv("MB_ADAMW_GRID"); vgrid = e ? atoi(e) : 0;
    }
    if (log) fprintf(stderr, "[magbert adamw] n=%zu\n", n);
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return MB_ERR_SHAPE;
    unsigned grid = (unsigned)((n4 + 255) / 256);
    if (grid > 256 * 16) grid = 256 * 16;
    if (vgrid > 0 && (unsigned)vgrid < grid) grid = (unsigned)vgrid;
    *out = AdamLaunch{nt != 0, grid};
    return MB_OK;
}

int adamw_step(float* p, float* g, float* m, float* v, void* shadow, size_t n, size_t n_decay, size_t sh_begin,
               size_t sh_end, AdamArgs a, int zero_grad, hipStream_t st, const AdamArgs* dyn, size_t keep_begin, size_t keep_end) {
    if (n == 0) return MB_OK;
    const size_t n4 = n / 4;
    AdamLaunch l;
    if (const int rc = adam_launch(p, g, m, v, n, n4, &l)) return rc;
    if ((n_decay % 4 && n_decay < n) || (sh_begin % 4) || (sh_end % 4) || (keep_begin % 4) || (keep_end % 4)) return MB_ERR_SHAPE;
    if (n4) {
        auto k = l.nt ? adamw_range_kernel<true> : adamw_range_kernel<false>;
        hipLaunchKernelGGL(k, dim3(l.grid), dim3(256), 0, st, p, g, m, v, (bf16*)shadow, n4, n_decay, sh_begin, sh_end, keep_begin, keep_end, a,
                           dyn, zero_grad);
    }
    if (n % 4) hipLaunchKernelGGL(adamw_tail_kernel, dim3(1), dim3(64), 0, st, p, g, m, v, n4 * 4, n, n_decay, a, dyn, zero_grad);
    return (int)hipGetLastError();
}

// The end-of-step sweep of a single-call step (kernels.h AdamPieces / WordSkip): the update pieces laid end to end -- the host laid out
// their running sums -- are cut into one contiguous share per block, as adamw_range_kernel cuts one range; a block whose share crosses
// a piece boundary walks both parts, and finds the pieces in front of its own with scalar loads of the kernel arguments only.  Piece k
// reads its scalars from cls[slot[k]], and that slot's weight_decay decides whether it decays.  `cls` is any table of AdamArgs: the two
// scalars of an unclassed step (slot 0 = the decay slab, slot 1 = the same with weight_decay 0) or the class table.
// Pieces [clear_first, count) are clear-only (slot MB_PIECE_CLEAR, frozen segments): zeros over their gradient ranges, by blocks of their own.
template <bool NT>
__global__ void __launch_bounds__(256) adamw_sweep_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, bf16* __restrict__ shadow, const AdamPieces R,
                                                          size_t sh_begin, size_t sh_end, size_t keep_begin, size_t keep_end,
                                                          const AdamArgs* __restrict__ cls, WordSkip ws, unsigned upd_blocks) {
    if (blockIdx.x >= upd_blocks) {
        // Clear-only pieces (MB_PIECE_CLEAR, pieces [clear_first, count)): blocks of their own behind the update's, which walk the clear
        // pieces laid end to end the same way and store zeros over the gradient -- no parameter, moment or shadow byte is touched.
        // (As a branch inside the update loop below the same stores cost that loop 22 registers: 90 against 68 VGPRs, 5 resident
        //  blocks per CU instead of 7.)
        const size_t c0 = R.start4[R.clear_first], ctotal4 = R.start4[R.count] - c0;
        const unsigned nclr = gridDim.x - upd_blocks;
        const size_t cper = ((ctotal4 + nclr - 1) / nclr + 255) / 256 * 256;
        const size_t cb = c0 + (size_t)(blockIdx.x - upd_blocks) * cper, ce = min(c0 + ctotal4, cb + cper);
#pragma unroll 1
        for (int k = R.clear_first; k < R.count; ++k) {
            const size_t off = R.start4[k], nxt = R.start4[k + 1];
            if (nxt <= cb) continue;
            if (off >= ce) break;
            const size_t lo = max(cb, off), hi = min(ce, nxt);
            const size_t base4 = (size_t)R.begin4[k] - off;
            for (size_t i4 = base4 + lo + threadIdx.x; i4 < base4 + hi; i4 += 256) {
                if constexpr (NT) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, (f32x4*)(g + i4 * 4));
                else *(f32x4*)(g + i4 * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        return;
    }
    const size_t total4 = R.start4[R.clear_first];
    const size_t per = ((total4 + upd_blocks - 1) / upd_blocks + 255) / 256 * 256;
    const size_t vb = (size_t)blockIdx.x * per, ve = min(total4, vb + per);
    const bool skip_on = ws.stamp != nullptr && ws.state[1] != 0u;
    const uint32_t stamp_no = skip_on ? ws.state[0] : 0u;
    const bool lazy_on = skip_on && ws.state[2] != 0u;          // (this step's moment verdict: kernels.h WordSkip)
#pragma unroll 1
    for (int k = 0; k < R.clear_first; ++k) {
        const size_t off = R.start4[k], nxt = R.start4[k + 1];
        if (nxt <= vb) continue;
        if (off >= ve) break;
        const size_t lo = max(vb, off), hi = min(ve, nxt);
        if (lo >= hi) continue;
        const AdamArgs a = cls[R.slot[k]];
        const size_t base4 = (size_t)R.begin4[k] - off;          // quad index in the buffers = base4 + index in the laid-out pieces
        adam_span<NT>(p, g, m, v, shadow, base4 + lo + threadIdx.x, base4 + hi, a, ~(size_t)0, sh_begin, sh_end, keep_begin, keep_end, 1,
                      skip_on, lazy_on, ws, stamp_no);
    }
}

int adamw_sweep(float* p, float* g, float* m, float* v, void* shadow, const AdamPieces& r, size_t sh_begin, size_t sh_end,
                size_t keep_begin, size_t keep_end, const AdamArgs* cls, const WordSkip& skip, hipStream_t st) {
    if (r.count < 0 || r.count > MB_SWEEP_PIECES_MAX || r.clear_first < 0 || r.clear_first > r.count || !cls) return MB_ERR_ARG;
    if (r.count && r.start4[0] != 0u) return MB_ERR_ARG;
    for (int k = 0; k < r.count; ++k)          // update pieces first, every clear-only piece behind them
        if (r.start4[k + 1] < r.start4[k] || (k < r.clear_first ? r.slot[k] >= 2 * MB_CLASSES_MAX : r.slot[k] != MB_PIECE_CLEAR)) return MB_ERR_SHAPE;
    const size_t n4 = r.count ? r.start4[r.clear_first] : 0, c4 = r.count ? r.start4[r.count] - n4 : 0;
    if (n4 + c4 == 0) return MB_OK;
    if ((sh_begin % 4) || (sh_end % 4) || (keep_begin % 4) || (keep_end % 4)) return MB_ERR_SHAPE;
    if (skip.stamp && (!skip.state || skip.row_len == 0 || (skip.begin | skip.end | skip.row_len) % 4 || skip.end < skip.begin ||
                       skip.end - skip.begin > 0xffffffffull)) return MB_ERR_SHAPE;
    AdamLaunch l;
    if (const int rc = adam_launch(p, g, m, v, n4 * 4, n4, &l)) return rc;
    // clear-only pieces: 2,048 quads per block (32 KB of zeros), one block per CU at most -- a few tensors of biases and LayerNorm weights
    unsigned cgrid = (unsigned)((c4 + 2047) / 2048);
    if (cgrid > 256) cgrid = 256;
    auto k = l.nt ? adamw_sweep_kernel<true> : adamw_sweep_kernel<false>;
    hipLaunchKernelGGL(k, dim3(l.grid + cgrid), dim3(256), 0, st, p, g, m, v, (bf16*)shadow, r, sh_begin, sh_end, keep_begin, keep_end, cls, skip,
                       l.grid);
    return (int)hipGetLastError();
}

}  // namespace mb
