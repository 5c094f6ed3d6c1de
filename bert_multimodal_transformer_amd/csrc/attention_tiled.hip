// Tiled fused self-attention for the BERT encoder, forward and backward (dh = 64, 1 <= L <= 512).
//
// Same arithmetic and tensor contract as the LDS-resident kernels of attention.hip, which hold a whole sequence of one head in LDS
// and so stop at L = 128:
//     S = Q K^T / 8 + (1 - mask) * -10000 ;  P = softmax(S) ;  ctx = head_scale[h] * dropout(P) V
// Here the sequence is cut into 64-row blocks.  One workgroup = one (batch, head, 64-row block), four waves of 16 rows each; the
// other operand streams through a two-slot LDS ring of 64-row tiles, register-staged (the global loads of tile t+1 are issued before
// the products of tile t and written to the other slot after them: one barrier per tile).
//   forward : query blocks; online softmax over the key tiles (running max m, the normaliser sums the UNDROPPED exponentials,
//             dropout multiplies only the P.V operand); stores m and 1/l of every row.  probs (output_attentions): a second sweep
//             over the keys with the final row statistics.
//   backward: FlashAttention-2's deterministic form, two launches, every dQ / dK / dV element written by exactly one workgroup.
//             dq    : query blocks -> D_i = dO_i . ctx_i (ctx already carries dropout and head_scale), stored for the next launch;
//                     sweep over the key tiles: recompute P from (m, 1/l), dS = P (head_scale dropout(dO V^T) - D) / 8 -> dQ += dS K
//             dkdv  : key blocks   -> sweep over the query tiles: P^T, dS^T -> dV += head_scale dropout(P)^T dO, dK += dS^T Q
// The fused-QKV bias gradient (column sums of dQ / dK / dV) goes through grad_add once per column per workgroup.
// Row statistics ("stats", caller scratch, tiled_stats_floats): three fp32 planes of B*nh*L rows -- m | 1/l (forward) | D (backward).
// Dropout masks: counter hash (common.h), index ((b*nh + h)*L + i)*L + j over the full L, as in attention.hip.
#include "attn_common.h"

namespace mb {

namespace {

constexpr int kTNW = 4, kTThreads = kTNW * 64;     // waves (16 rows each) and threads of every tiled workgroup

// register-staged copy of one 64-row tile of N head images (rows >= valid read as zero): issue() ahead of the products that hide the
// loads, commit() into the LDS images behind them (T14 of the HIP guide)
template <class T, int N>
struct TileStage {
    static constexpr int CPR = AttnCfg<T>::ROWB / 16;          // 16-byte chunks per 64-element row: 8 (bf16) | 16 (fp32)
    static constexpr int IT = 64 * CPR / kTThreads;            // chunks per thread and image: 2 | 4
    u32x4 v[N][IT];
    __device__ __forceinline__ void issue(const T* const (&src)[N], const size_t (&ld)[N], int valid) {
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int id = threadIdx.x + it * kTThreads, row = id / CPR, c = id % CPR;
                v[n][it] = u32x4{0u, 0u, 0u, 0u};
                if (row < valid) v[n][it] = *(const u32x4*)((const char*)(src[n] + (size_t)row * ld[n]) + c * 16);
            }
    }
    __device__ __forceinline__ void commit(char* const (&img)[N], int pitch) const {
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int id = threadIdx.x + it * kTThreads, row = id / CPR, c = id % CPR;
                *(u32x4*)(img[n] + row * pitch + c * 16) = v[n][it];
            }
    }
};

// shift: common_key_bias of the sample (attn_common.h): kMaskNeg when it has no real key at all, else 0 (x - 0 is x: the same bits).
// All four sweeps that form scores take it off, so the m the forward stores is the m the backward recomputes against.
__device__ __forceinline__ float key_bias(const int64_t* __restrict__ mrow, int j, int L, float shift) {
    return j < L ? (1.0f - (float)mrow[j]) * kMaskNeg - shift : kPadNeg;
}

// this lane's MFMA fragment of row `row` of a token-major head (frag_nat's layout, straight from global memory; rows >= L are zero)
template <class T>
__device__ __forceinline__ typename Frag<T>::type frag_row(const T* __restrict__ head, size_t ld, int row, int L, int sl, int lane) {
    typedef AttnCfg<T> C;
    typename Frag<T>::type f = {};
    if (row < L) f = *(const typename Frag<T>::type*)(head + (size_t)row * ld + sl * C::SLAB + (lane >> 4) * C::EPV);
    return f;
}

// column sums of the [64 rows][64] output tiles of the four waves (o[dt][r] = X[row of lane & 15][dt*16 + (lane>>4)*4 + r], rows
// outside the sequence passed as zero) -> one grad_add per column.  Called by every thread, after a barrier that freed `csw`.
template <int NS>
__device__ __forceinline__ void flush_colsums(const f32x4 (&o)[NS][4], float* csw, float* const (&dst)[NS], const GradAcc& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sred = row16_sum_to_lane15(o[s][dt][r]);
                if ((lane & 15) == 15) csw[(s * kTNW + wave) * 64 + dt * 16 + (lane >> 4) * 4 + r] = sred;
            }
    __syncthreads();
    for (int x = threadIdx.x; x < NS * 64; x += kTThreads) {
        const int s = x >> 6, col = x & 63;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < kTNW; ++w) t += csw[(s * kTNW + w) * 64 + col];
        grad_add(acc, dst[s] + col, t);
    }
}

}  // namespace

// Waves per SIMD = workgroups per CU.  Forward, bf16: four (37 KB of LDS, <= 128 registers: as many as the LDS allows).  Backward
// and fp32: two (<= 256 registers) -- capped at 128 the bf16 backward kernels spill (dq 44, dkdv ~150 registers), mostly the
// dropout hashes of a 16-element score tile.
#define MB_TILED_BOUNDS(T, FWD) __launch_bounds__(kTThreads, (FWD && sizeof(T) == 2) ? 4 : 2)

// =============================================================================================== forward
template <class T>
__global__ void MB_TILED_BOUNDS(T, true) attn_tiled_fwd_kernel(const T* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                         T* __restrict__ ctx, float* __restrict__ stats, float* __restrict__ probs,
                                                         const float* __restrict__ head_scale, int L, int nh, int nqb,
                                                         size_t plane, DropKey drop) {
    drop.resolve();
    typedef AttnCfg<T> C;
    typedef AccOp<T> AO;
    typedef typename Frag<T>::type F;
    constexpr int PIT = C::ROWB + 16, IMG = 64 * PIT, DSL = 64 / C::SLAB, LSL = 64 / C::SLAB;
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG + 64 * 4];      // ring slot: K | V | key bias
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bh = blockIdx.x / nqb, b = bh / nh, h = bh % nh;
    const int H = nh * 64;
    const size_t ld = (size_t)3 * H;
    const T* base = qkv + (size_t)b * L * ld + h * 64;
    const int64_t* mrow = mask + (size_t)b * L;
    const int i = (blockIdx.x % nqb) * 64 + wave * 16 + (lane & 15);      // this lane's query row
    const int nkt = (L + 63) / 64;

    const float shift = common_key_bias(mrow, L, lane);      // (before the fragments are loaded: a scalar from here on)
    TileStage<T, 2> st;
    float mb = 0.f;
    auto issue = [&](int t) {
        const T* const src[2] = {base + (size_t)t * 64 * ld + H, base + (size_t)t * 64 * ld + 2 * H};
        const size_t lds[2] = {ld, ld};
        st.issue(src, lds, L - t * 64);
        if (threadIdx.x < 64) mb = key_bias(mrow, t * 64 + threadIdx.x, L, shift);
    };
    auto commit = [&](int slot) {
        char* const img[2] = {smem[slot], smem[slot] + IMG};
        st.commit(img, PIT);
        if (threadIdx.x < 64) ((float*)(smem[slot] + 2 * IMG))[threadIdx.x] = mb;
    };
    issue(0);
    F qf[DSL];
#pragma unroll
    for (int sl = 0; sl < DSL; ++sl) qf[sl] = frag_row<T>(base, ld, i, L, sl, lane);
    commit(0);
    __syncthreads();

    const float scale = 0.125f;
    const float hs = head_scale ? head_scale[h] : 1.0f;
    const uint32_t rowidx = ((uint32_t)bh * L + (uint32_t)i) * L;
    // s[jt][r] = S[i][j], j = t*64 + jt*16 + (lane>>4)*4 + r  (mma16 with K as X, Q as Y: the lane owns one query row)
    auto scores = [&](const char* Ki, const float* mbias, f32x4 (&s)[4]) {
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            s[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sl = 0; sl < DSL; ++sl) mma16(s[jt], frag_nat<T>(Ki, PIT, jt * 16 + (lane & 15), sl, lane), qf[sl]);
            s[jt] = s[jt] * scale + *(const f32x4*)(mbias + jt * 16 + (lane >> 4) * 4);
        }
    };
    float m = -3.0e38f, lpart = 0.f;        // running row max (uniform over the row's four lanes), this lane's share of the normaliser
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < nkt; ++t) {
        const int slot = t & 1;
        if (t + 1 < nkt) issue(t + 1);
        const char* Ki = smem[slot];
        const char* Vi = smem[slot] + IMG;
        f32x4 s[4];
        scores(Ki, (const float*)(smem[slot] + 2 * IMG), s);
        float mx = m;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) mx = fmaxf(mx, fmaxf(fmaxf(s[jt][0], s[jt][1]), fmaxf(s[jt][2], s[jt][3])));
        mx = quad_max(mx);
        const float alpha = __expf(m - mx);          // (first tile: exp(-3e38) = 0; tile 0 always holds key 0 < L)
        m = mx;
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[jt][r] = __expf(s[jt][r] - mx);
                sum += s[jt][r];
                s[jt][r] *= drop_mult(drop, rowidx + t * 64 + jt * 16 + (lane >> 4) * 4 + r);     // the P.V operand only
            }
        lpart = lpart * alpha + sum;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            o[dt] = o[dt] * alpha;
#pragma unroll
            for (int sl = 0; sl < LSL; ++sl)
                mma16(o[dt], AO::kmaj(Vi, PIT, sl, dt * 16 + (lane & 15), lane), AO::make(&s[sl * AO::TILES]));
        }
        if (t + 1 < nkt) commit(slot ^ 1);
        __syncthreads();
    }
    const float inv = 1.0f / quad_sum(lpart);
    if (i < L) {
        // o[dt][r] = ctx[i][dt*16 + (lane>>4)*4 + r]
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4(ctx + ((size_t)b * L + i) * H + h * 64 + dt * 16 + (lane >> 4) * 4, o[dt] * (inv * hs));
        if ((lane >> 4) == 0) { stats[(size_t)bh * L + i] = m; stats[plane + (size_t)bh * L + i] = inv; }
    }
    if (probs == nullptr) return;
    // output_attentions: the probabilities after dropout, times head_scale -- a second sweep once the normaliser is known
    issue(0);
    commit(0);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < nkt; ++t) {
        const int slot = t & 1;
        if (t + 1 < nkt) issue(t + 1);
        f32x4 s[4];
        scores(smem[slot], (const float*)(smem[slot] + 2 * IMG), s);
        if (i < L) {
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t * 64 + jt * 16 + (lane >> 4) * 4 + r;
                    if (j < L) probs[((size_t)bh * L + i) * L + j] = __expf(s[jt][r] - m) * inv * drop_mult(drop, rowidx + j) * hs;
                }
        }
        if (t + 1 < nkt) commit(slot ^ 1);
        __syncthreads();
    }
}

// =============================================================================================== backward: dQ (query blocks)
template <class T>
__global__ void MB_TILED_BOUNDS(T, false) attn_tiled_dq_kernel(const T* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                        const T* __restrict__ ctx, const T* __restrict__ dctx, float* __restrict__ stats,
                                                        T* __restrict__ dqkv, float* __restrict__ dbias,
                                                        const float* __restrict__ head_scale, int L, int nh, int nqb, size_t plane,
                                                        DropKey drop, GradAcc acc) {
    drop.resolve();
    typedef AttnCfg<T> C;
    typedef AccOp<T> AO;
    typedef typename Frag<T>::type F;
    constexpr int PIT = C::ROWB + 16, IMG = 64 * PIT, DSL = 64 / C::SLAB, LSL = 64 / C::SLAB;
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG + 64 * 4];      // ring slot: K | V | key bias
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bh = blockIdx.x / nqb, b = bh / nh, h = bh % nh;
    const int H = nh * 64;
    const size_t ld = (size_t)3 * H;
    const T* base = qkv + (size_t)b * L * ld + h * 64;
    const T* obase = dctx + (size_t)b * L * H + h * 64;
    const int64_t* mrow = mask + (size_t)b * L;
    const int i = (blockIdx.x % nqb) * 64 + wave * 16 + (lane & 15);
    const int nkt = (L + 63) / 64;

    const float shift = common_key_bias(mrow, L, lane);      // (before the fragments are loaded: a scalar from here on)
    TileStage<T, 2> st;
    float mb = 0.f;
    auto issue = [&](int t) {
        const T* const src[2] = {base + (size_t)t * 64 * ld + H, base + (size_t)t * 64 * ld + 2 * H};
        const size_t lds[2] = {ld, ld};
        st.issue(src, lds, L - t * 64);
        if (threadIdx.x < 64) mb = key_bias(mrow, t * 64 + threadIdx.x, L, shift);
    };
    auto commit = [&](int slot) {
        char* const img[2] = {smem[slot], smem[slot] + IMG};
        st.commit(img, PIT);
        if (threadIdx.x < 64) ((float*)(smem[slot] + 2 * IMG))[threadIdx.x] = mb;
    };
    issue(0);
    F qf[DSL], of[DSL];
    float dpart = 0.f;
#pragma unroll
    for (int sl = 0; sl < DSL; ++sl) {
        qf[sl] = frag_row<T>(base, ld, i, L, sl, lane);
        of[sl] = frag_row<T>(obase, H, i, L, sl, lane);
        const F cf = frag_row<T>(ctx + (size_t)b * L * H + h * 64, H, i, L, sl, lane);
#pragma unroll
        for (int e = 0; e < C::EPV; ++e) dpart += (float)of[sl][e] * (float)cf[e];
    }
    const float D = quad_sum(dpart);                  // D_i = dO_i . ctx_i
    float mi = 0.f, invi = 0.f;                       // (rows >= L: P = 0)
    if (i < L) {
        mi = stats[(size_t)bh * L + i];
        invi = stats[plane + (size_t)bh * L + i];
        if ((lane >> 4) == 0) stats[2 * plane + (size_t)bh * L + i] = D;
    }
    commit(0);
    __syncthreads();

    const float scale = 0.125f;
    const float hs = head_scale ? head_scale[h] : 1.0f;
    const uint32_t rowidx = ((uint32_t)bh * L + (uint32_t)i) * L;
    f32x4 oq[1][4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oq[0][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < nkt; ++t) {
        const int slot = t & 1;
        if (t + 1 < nkt) issue(t + 1);
        const char* Ki = smem[slot];
        const char* Vi = smem[slot] + IMG;
        const float* mbias = (const float*)(smem[slot] + 2 * IMG);
        f32x4 sp[4], dp[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            sp[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sl = 0; sl < DSL; ++sl) {
                mma16(sp[jt], frag_nat<T>(Ki, PIT, jt * 16 + (lane & 15), sl, lane), qf[sl]);
                mma16(dp[jt], frag_nat<T>(Vi, PIT, jt * 16 + (lane & 15), sl, lane), of[sl]);
            }
        }
        // sp[jt][r] = S[i][j] (pre-scale), dp[jt][r] = (dO V^T)[i][j],  j = t*64 + jt*16 + (lane>>4)*4 + r
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const f32x4 mb4 = *(const f32x4*)(mbias + jt * 16 + (lane >> 4) * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __expf(sp[jt][r] * scale + mb4[r] - mi) * invi;
                const float dm = drop_mult(drop, rowidx + t * 64 + jt * 16 + (lane >> 4) * 4 + r) * hs;
                sp[jt][r] = p * (dp[jt][r] * dm - D) * scale;        // dS_ij
            }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int sl = 0; sl < LSL; ++sl)
                mma16(oq[0][dt], AO::kmaj(Ki, PIT, sl, dt * 16 + (lane & 15), lane), AO::make(&sp[sl * AO::TILES]));
        if (t + 1 < nkt) commit(slot ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        if (i < L) store4(dqkv + ((size_t)b * L + i) * ld + h * 64 + dt * 16 + (lane >> 4) * 4, oq[0][dt]);
        else oq[0][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (dbias != nullptr) {
        float* const dst[1] = {dbias + h * 64};
        flush_colsums<1>(oq, (float*)smem, dst, acc);
    }
}

// =============================================================================================== backward: dK, dV (key blocks)
template <class T>
__global__ void MB_TILED_BOUNDS(T, false) attn_tiled_dkdv_kernel(const T* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                          const T* __restrict__ dctx, const float* __restrict__ stats,
                                                          T* __restrict__ dqkv, float* __restrict__ dbias,
                                                          const float* __restrict__ head_scale, int L, int nh, int nkb, size_t plane,
                                                          DropKey drop, GradAcc acc) {
    drop.resolve();
    typedef AttnCfg<T> C;
    typedef AccOp<T> AO;
    typedef typename Frag<T>::type F;
    constexpr int PIT = C::ROWB + 16, IMG = 64 * PIT, DSL = 64 / C::SLAB, LSL = 64 / C::SLAB;
    __shared__ __attribute__((aligned(16))) char smem[2][2 * IMG + 3 * 64 * 4];      // ring slot: Q | dO | m, 1/l, D of the rows
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bh = blockIdx.x / nkb, b = bh / nh, h = bh % nh;
    const int H = nh * 64;
    const size_t ld = (size_t)3 * H;
    const T* base = qkv + (size_t)b * L * ld + h * 64;
    const T* obase = dctx + (size_t)b * L * H + h * 64;
    const int j = (blockIdx.x % nkb) * 64 + wave * 16 + (lane & 15);      // this lane's key
    const int nqt = (L + 63) / 64;

    TileStage<T, 2> st;
    float rs[3] = {0.f, 0.f, 0.f};
    auto issue = [&](int t) {
        const T* const src[2] = {base + (size_t)t * 64 * ld, obase + (size_t)t * 64 * H};
        const size_t lds[2] = {ld, (size_t)H};
        st.issue(src, lds, L - t * 64);
        const int row = t * 64 + (int)threadIdx.x;
        if (threadIdx.x < 64) {
#pragma unroll
            for (int k = 0; k < 3; ++k) rs[k] = row < L ? stats[k * plane + (size_t)bh * L + row] : 0.f;    // (rows >= L: P = 0)
        }
    };
    auto commit = [&](int slot) {
        char* const img[2] = {smem[slot], smem[slot] + IMG};
        st.commit(img, PIT);
        if (threadIdx.x < 64) {
#pragma unroll
            for (int k = 0; k < 3; ++k) ((float*)(smem[slot] + 2 * IMG))[k * 64 + threadIdx.x] = rs[k];
        }
    };
    issue(0);
    F kf[DSL], vf[DSL];
#pragma unroll
    for (int sl = 0; sl < DSL; ++sl) {
        kf[sl] = frag_row<T>(base + H, ld, j, L, sl, lane);
        vf[sl] = frag_row<T>(base + 2 * H, ld, j, L, sl, lane);
    }
    const float mbj = key_bias(mask + (size_t)b * L, j, L, common_key_bias(mask + (size_t)b * L, L, lane));
    commit(0);
    __syncthreads();

    const float scale = 0.125f;
    const float hs = head_scale ? head_scale[h] : 1.0f;
    f32x4 oc[2][4];                    // [0] dK, [1] dV: oc[.][dt][r] = X[j][dt*16 + (lane>>4)*4 + r]
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oc[0][dt] = oc[1][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < nqt; ++t) {
        const int slot = t & 1;
        if (t + 1 < nqt) issue(t + 1);
        const char* Qi = smem[slot];
        const char* Oi = smem[slot] + IMG;
        const float* rm = (const float*)(smem[slot] + 2 * IMG);
        f32x4 sp[4], dp[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            sp[it] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[it] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sl = 0; sl < DSL; ++sl) {
                mma16(sp[it], frag_nat<T>(Qi, PIT, it * 16 + (lane & 15), sl, lane), kf[sl]);
                mma16(dp[it], frag_nat<T>(Oi, PIT, it * 16 + (lane & 15), sl, lane), vf[sl]);
            }
        }
        // sp[it][r] = S[i][j] (pre-scale), dp[it][r] = (dO V^T)[i][j],  i = t*64 + it*16 + (lane>>4)*4 + r
        // dropout index of (i, j) = ib + (it*16 + r) * L: one vector base, the rest uniform
        const uint32_t ib = ((uint32_t)bh * L + (uint32_t)(t * 64 + (lane >> 4) * 4)) * L + (uint32_t)j;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int i0 = it * 16 + (lane >> 4) * 4;
            const f32x4 rm4 = *(const f32x4*)(rm + i0), ri4 = *(const f32x4*)(rm + 64 + i0), rd4 = *(const f32x4*)(rm + 128 + i0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __expf(sp[it][r] * scale + mbj - rm4[r]) * ri4[r];
                const float dm = drop_mult(drop, ib + (uint32_t)((it * 16 + r) * L)) * hs;
                sp[it][r] = p * (dp[it][r] * dm - rd4[r]) * scale;     // dS^T        -> dK
                dp[it][r] = p * dm;                                    // dropped P^T -> dV
            }
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int sl = 0; sl < LSL; ++sl)
                mma16(oc[1][dt], AO::kmaj(Oi, PIT, sl, dt * 16 + (lane & 15), lane), AO::make(&dp[sl * AO::TILES]));
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int sl = 0; sl < LSL; ++sl)
                mma16(oc[0][dt], AO::kmaj(Qi, PIT, sl, dt * 16 + (lane & 15), lane), AO::make(&sp[sl * AO::TILES]));
        if (t + 1 < nqt) commit(slot ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            if (j < L) store4(dqkv + ((size_t)b * L + j) * ld + (s + 1) * H + h * 64 + dt * 16 + (lane >> 4) * 4, oc[s][dt]);
            else oc[s][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    if (dbias != nullptr) {
        float* const dst[2] = {dbias + H + h * 64, dbias + 2 * H + h * 64};
        flush_colsums<2>(oc, (float*)smem, dst, acc);
    }
}

// =============================================================================================== host
size_t tiled_stats_floats(int B, int L, int nh) { return (size_t)3 * B * nh * L; }

// shapes (and the uint32 dropout index) are checked before any pointer is looked at
static int tiled_check(int dtype, int B, int L, int nh, const DropKey& drop) {
    if (B < 1 || L < 1 || L > 512 || nh < 1 || (int64_t)B * nh * ((L + 63) / 64) > 0x7fffffff) return MB_ERR_SHAPE;
    if (drop.thresh != 0u && (uint64_t)B * nh * L * L >= ((uint64_t)1 << 32)) return MB_ERR_SHAPE;
    if (dtype != DT_BF16 && dtype != DT_F32) return MB_ERR_DTYPE;
    return MB_OK;
}

int attention_tiled_forward(int dtype, const void* qkv, const int64_t* mask, void* ctx, float* stats, int B, int L, int nh,
                            DropKey drop, hipStream_t st, float* probs, const float* head_scale) {
    if (int e = tiled_check(dtype, B, L, nh, drop)) return e;
    if (!qkv || !mask || !ctx || !stats) return MB_ERR_ARG;
    const int nqb = (L + 63) / 64;
    const size_t plane = (size_t)B * nh * L;
    const dim3 grid(B * nh * nqb), block(kTThreads);
    if (dtype == DT_BF16)
        hipLaunchKernelGGL(attn_tiled_fwd_kernel<bf16>, grid, block, 0, st, (const bf16*)qkv, mask, (bf16*)ctx, stats, probs, head_scale,
                           L, nh, nqb, plane, drop);
    else
        hipLaunchKernelGGL(attn_tiled_fwd_kernel<float>, grid, block, 0, st, (const float*)qkv, mask, (float*)ctx, stats, probs,
                           head_scale, L, nh, nqb, plane, drop);
    return (int)hipGetLastError();
}

int attention_tiled_backward(int dtype, const void* qkv, const int64_t* mask, const void* ctx, const void* dctx, float* stats,
                             void* dqkv, float* dbias, int B, int L, int nh, DropKey drop, hipStream_t st, const float* head_scale,
                             GradAcc acc, const AdamRide* ride) {
    if (int e = tiled_check(dtype, B, L, nh, drop)) return e;
    if (ride != nullptr && ride->blocks > 0) return MB_ERR_MODE;          // no optimizer riders in the tiled launches
    if (!qkv || !mask || !ctx || !dctx || !stats || !dqkv) return MB_ERR_ARG;
    const int nb = (L + 63) / 64;
    const size_t plane = (size_t)B * nh * L;
    const dim3 grid(B * nh * nb), block(kTThreads);
    if (dtype == DT_BF16) {
        hipLaunchKernelGGL(attn_tiled_dq_kernel<bf16>, grid, block, 0, st, (const bf16*)qkv, mask, (const bf16*)ctx, (const bf16*)dctx,
                           stats, (bf16*)dqkv, dbias, head_scale, L, nh, nb, plane, drop, acc);
        if (hipError_t e = hipGetLastError()) return (int)e;
        hipLaunchKernelGGL(attn_tiled_dkdv_kernel<bf16>, grid, block, 0, st, (const bf16*)qkv, mask, (const bf16*)dctx,
                           (const float*)stats, (bf16*)dqkv, dbias, head_scale, L, nh, nb, plane, drop, acc);
    } else {
        hipLaunchKernelGGL(attn_tiled_dq_kernel<float>, grid, block, 0, st, (const float*)qkv, mask, (const float*)ctx,
                           (const float*)dctx, stats, (float*)dqkv, dbias, head_scale, L, nh, nb, plane, drop, acc);
        if (hipError_t e = hipGetLastError()) return (int)e;
        hipLaunchKernelGGL(attn_tiled_dkdv_kernel<float>, grid, block, 0, st, (const float*)qkv, mask, (const float*)dctx,
                           (const float*)stats, (float*)dqkv, dbias, head_scale, L, nh, nb, plane, drop, acc);
    }
    return (int)hipGetLastError();
}

}  // namespace mb
