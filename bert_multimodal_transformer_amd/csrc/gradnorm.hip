// Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, error_if_nonfinite=False) as two launches over a flat fp32 range:
//   grad_sumsq:          one double per block, the sum of the squares of the block's share of g[0, n)
//   grad_clip_finalize:  norm = grad_scale * sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)), and coef multiplied into the
//                        grad_scale field of AdamArgs tables in device memory -- the tables every AdamW kernel of a single-call step reads
//                        its scalars from (kernels.h AdamArgs, engine_common.h adam_state / class_state).  The gradient buffer itself is
//                        never scaled: no pass over it beyond the one read.
// HBM-bound (4 B/element).  Every element is widened to double BEFORE it is squared (1e20f squared is finite, 1e-30f squared is not 0) and
// every sum is a double in a fixed order -- no atomics -- so the result is the same bits run to run, and within ~1e-13 relative of any
// other summation order.
#include "kernels.h"

namespace mb {

#define MB_GRADNORM_MAX_BLOCKS 2048

// the grid: a function of n alone (the partials' count is the scratch size callers plan with)
unsigned grad_norm_blocks(size_t n) {
    const size_t b = (n / 4 + 1023) / 1024;          // four quads per thread per pass
    return b < 1 ? 1u : (b > MB_GRADNORM_MAX_BLOCKS ? (unsigned)MB_GRADNORM_MAX_BLOCKS : (unsigned)b);
}

__device__ __forceinline__ double sq4(f32x4 x, double acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { const double d = (double)x[r]; acc = fma(d, d, acc); }
    return acc;
}

// g needs 4-byte alignment only: the elements in front of the first 16-byte boundary and behind the last whole quad go to thread 0 of block 0
__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partial) {
    constexpr int UNR = 4;
    size_t head = (size_t)((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) / 4;
    if (head > n) head = n;
    const f32x4* __restrict__ q = (const f32x4*)(g + head);
    const size_t n4 = (n - head) / 4;
    const size_t stride = (size_t)gridDim.x * 256;
    double acc[UNR] = {0.0, 0.0, 0.0, 0.0};
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + (UNR - 1) * stride < n4; i += UNR * stride) {
        f32x4 x[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) x[u] = q[i + u * stride];
#pragma unroll
        for (int u = 0; u < UNR; ++u) acc[u] = sq4(x[u], acc[u]);
    }
    for (; i < n4; i += stride) acc[0] = sq4(q[i], acc[0]);
    double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (size_t k = 0; k < head; ++k) { const double d = (double)g[k]; s = fma(d, d, s); }
        for (size_t k = head + n4 * 4; k < n; ++k) { const double d = (double)g[k]; s = fma(d, d, s); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ double wave_sum[4];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// The sum over a table of pieces (kernels.h AdamPieces: quads [begin4[k], begin4[k] + start4[k + 1] - start4[k]) of g): the pieces laid end
// to end are cut into one contiguous share per block, a block walks the pieces its share overlaps in table order.  Every address is a
// whole quad (the pieces are tensor-aligned offsets into a 16-byte aligned buffer).
__global__ void __launch_bounds__(256) grad_sumsq_pieces_kernel(const float* __restrict__ g, const AdamPieces R, double* __restrict__ partial) {
    const size_t total4 = R.start4[R.count];
    const size_t per = ((total4 + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
    const size_t vb = (size_t)blockIdx.x * per, ve = min(total4, vb + per);
    const f32x4* __restrict__ q = (const f32x4*)g;
    double acc[2] = {0.0, 0.0};
#pragma unroll 1
    for (int k = 0; k < R.count; ++k) {
        const size_t off = R.start4[k], nxt = R.start4[k + 1];
        if (nxt <= vb) continue;
        if (off >= ve) break;
        const size_t lo = max(vb, off), hi = min(ve, nxt);
        if (lo >= hi) continue;
        const size_t base4 = (size_t)R.begin4[k] - off;
        size_t i = base4 + lo + threadIdx.x;
        const size_t end = base4 + hi;
        for (; i + 256 < end; i += 512) {
            const f32x4 x0 = q[i], x1 = q[i + 256];
            acc[0] = sq4(x0, acc[0]); acc[1] = sq4(x1, acc[1]);
        }
        if (i < end) acc[0] = sq4(q[i], acc[0]);
    }
    double s = acc[0] + acc[1];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ double wave_sum[4];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// One block.  The partials are summed in index order in two levels: thread t adds partials [8t, 8t + 8) one after the other, thread 0 then
// adds the 256 sums one after the other.  dyn (device, may be null): {max_norm, grad_scale} of this step, where the step prologue put them.
__global__ void __launch_bounds__(256) grad_clip_finalize_kernel(const double* __restrict__ partial, unsigned blocks, const float* __restrict__ dyn,
                                                                 float max_norm, float grad_scale, float* __restrict__ out2, ClipTables t) {
    static_assert(MB_GRADNORM_MAX_BLOCKS == 256 * 8, "eight partials per thread");
    __shared__ double part[256];
    __shared__ float coef_f;
    double s = 0.0;
    for (unsigned k = threadIdx.x * 8u; k < threadIdx.x * 8u + 8u && k < blocks; ++k) s += partial[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (dyn) { max_norm = dyn[0]; grad_scale = dyn[1]; }
        double sum = 0.0;
        for (int k = 0; k < 256; ++k) sum += part[k];
        const double norm = (double)grad_scale * sqrt(sum);
        const double c = (double)max_norm / (norm + 1e-6);
        const double coef = c > 1.0 ? 1.0 : c;          // (a NaN stays a NaN, as torch.clamp(max=1.0) leaves it)
        out2[0] = (float)norm;
        out2[1] = coef_f = (float)coef;
    }
    __syncthreads();
    const float cf = coef_f;
    int at = (int)threadIdx.x;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (t.tab[k] && at >= 0 && at < t.count[k]) t.tab[k][at].grad_scale *= cf;
        at -= t.tab[k] ? t.count[k] : 0;
    }
}

int grad_sumsq(const float* g, size_t n, double* partial, hipStream_t st) {
    if ((n && !g) || !partial || ((uintptr_t)g & 3) || ((uintptr_t)partial & 7)) return MB_ERR_ARG;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grad_norm_blocks(n)), dim3(256), 0, st, g, n, partial);
    return (int)hipGetLastError();
}

int grad_sumsq_pieces(const float* g, const AdamPieces& r, double* partial, unsigned* blocks, hipStream_t st) {
    if (!g || !partial || !blocks || ((uintptr_t)g & 15) || ((uintptr_t)partial & 7)) return MB_ERR_ARG;
    if (r.count < 0 || r.count > MB_SWEEP_PIECES_MAX || (r.count && r.start4[0] != 0u)) return MB_ERR_ARG;
    for (int k = 0; k < r.count; ++k) if (r.start4[k + 1] < r.start4[k]) return MB_ERR_SHAPE;
    const size_t n4 = r.count ? r.start4[r.count] : 0;
    *blocks = grad_norm_blocks(n4 * 4);          // (no piece at all: one block that writes a zero)
    hipLaunchKernelGGL(grad_sumsq_pieces_kernel, dim3(*blocks), dim3(256), 0, st, g, r, partial);
    return (int)hipGetLastError();
}

int grad_clip_finalize(const double* partial, unsigned blocks, const float* dyn, float max_norm, float grad_scale, float* out2,
                       const ClipTables& t, hipStream_t st) {
    if (!partial || !out2 || blocks < 1 || blocks > MB_GRADNORM_MAX_BLOCKS) return MB_ERR_ARG;
    int total = 0;
    for (int k = 0; k < 2; ++k) {
        if (t.count[k] < 0 || (t.count[k] > 0 && !t.tab[k])) return MB_ERR_ARG;
        total += t.tab[k] ? t.count[k] : 0;
    }
    if (total > 256) return MB_ERR_ARG;
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, st, partial, blocks, dyn, max_norm, grad_scale, out2, t);
    return (int)hipGetLastError();
}

}  // namespace mb
