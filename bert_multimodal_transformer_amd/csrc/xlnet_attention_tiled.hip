// Tiled XLNet relative attention, forward and backward (head dim 64, 1 <= L <= 512).
//
// Same arithmetic and tensor contract as the LDS-resident kernels of xlnet_attention.hip, which keep all keys, values and the
// relative-position window of one head in LDS and so stop at L = 128:
//     ac[i,j] = (q_i + r_w_bias) . k_j
//     bd[i,j] = (q_i + r_r_bias) . kr[b][L - i + j]
//     ef[i,j] = (q_i + r_s_bias) . seg_embed[seg_i != seg_j]
//     S = (ac + bd + ef) / 8 - 1e30 * masked(i,j) ;  P = softmax_j(S) ;  vec_i = head_scale[h] * sum_j dropout(P)[i,j] v_j
// Here the sequence is cut into 64-row blocks.  One workgroup = one (batch, head, 64-row block), four waves of 16 rows each.
//   forward (query blocks): the query fragments live in registers; K and V stream through a two-slot LDS ring of 64-row tiles,
//       register-staged (the loads of tile t+1 are issued before the products of tile t and committed behind them: one barrier per
//       tile).  The position term of query block i0 and key tile j0 touches the 127 rows of kr from L - i0 - 63 + j0 on; the next
//       key tile moves that window by exactly 64, so kr streams as 64-row chunks through a THREE-slot ring (tile t reads chunks t and
//       t + 1 while chunk t + 2 arrives).  rel_shift is an index map on a raw per-wave product strip [16][96] (a wave's 16 rows
//       reach 79 of the block's 127 positions), never a copy of scores.  The bias columns r_w_bias . k_j and r_r_bias . kr_p are
//       formed from the staging registers at commit time (no extra pass over the images, no extra barrier).  Online softmax over
//       the key tiles; stores the running maximum m and 1/l of every row ("stats").  Keys j >= L of the last tile do not exist:
//       their score is -inf (XLNet's own mask value is -1e30, which must keep its weight in a fully masked row).
//   backward, three launches, every dq / dk / dv / dkr element written by exactly one workgroup (no atomics on them):
//       bwd_q   (query blocks)   : recomputes P from (m, 1/l) -- padding and perm applied again --, G = dL/d(ac+bd+ef) and the
//                                  dropped probabilities Pd go out ONCE to two shared [B*nh][LP][LP] scratch planes (LP = L rounded up
//                                  to 64: aligned 16-byte tile rows); dq = G.K + Gshift.KR + sum_j G.seg and the four small parameter
//                                  gradients (one grad_add per column per workgroup)
//       bwd_kv  (key blocks)     : dk = G^T (q + r_w_bias), dv = Pd^T dO over the query tiles, both operands read k-major
//       bwd_pos (position blocks): dkr[p] = sum_i G[i, p - L + i] (q_i + r_r_bias): 64 rows of dkr, sweeping the query tiles that hold
//                                  a piece of the block's shifted diagonal band
// Row statistics: two fp32 planes of B*nh*L rows -- m | 1/l.  The backward's D_i = dvec_i . vec_i needs the forward's vec in fp32; in
// bf16, where vec is rounded, bwd_q forms D_i = sum_j Pd_ij (dvec V^T)_ij in a sweep of its own instead.
// Dropout masks: counter hash (common.h), index ((b*nh + h)*L + i)*L + j over the true L, as in xlnet_attention.hip.
#include "attn_common.h"

namespace mb {

namespace {

constexpr int kXNW = 4, kXThreads = kXNW * 64;      // waves (16 rows each) and threads of every tiled workgroup
constexpr float kXlMaskT = 1.0e30f;                 // modeling_xlnet: attn_score - 1e30 * attn_mask (fp32)
constexpr int kMetaPad = 1 << 16, kMetaNone = 1 << 17;      // key meta word: segment id | padding key | key beyond L

struct XlTParams {
    const float* r_w_bias; const float* r_r_bias; const float* r_s_bias;   // [nh][64]
    const float* seg_embed;                                                // [2][nh][64]
    const int64_t* seg; const int64_t* mask;                               // [B][L]
    const float* head_scale;                                               // [nh] or null
    const uint8_t* perm;                                                   // [B][L][L] bytes or null
    int gstream;                                                           // 1 = no i == j exemption (query stream, forward only)
    GradAcc acc;
};

// LDS map of the two query-block kernels: K | V ring (2 slots), kr ring (3 slots), per-wave strips, bias columns, key meta words and
// the head's r_w_bias | r_r_bias
template <class T> struct XlCfg {
    typedef AttnCfg<T> C;
    static constexpr int PIT = C::ROWB + 16, IMG = 64 * PIT, RPIT = 96 * (int)sizeof(T) + 16;
    static constexpr int DSL = 64 / C::SLAB;
    static constexpr int O_KR = 4 * IMG, O_ST = O_KR + 3 * IMG, O_CK = O_ST + kXNW * 16 * RPIT, O_META = O_CK + 2 * 64 * 4,
                         O_CR = O_META + 2 * 64 * 4, O_BIAS = O_CR + 3 * 64 * 4, BYTES = O_BIAS + 2 * 64 * 4;
};

__device__ __forceinline__ void wave_lds_fence() {      // a strip written and read by ONE wave: LDS operations of a wave execute in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// register-staged copy of 64-row tiles of N head images (rows outside [lo, hi) read as zero): issue() ahead of the products that hide
// the loads, commit() into the LDS images behind them
template <class T, int N>
struct XTileStage {
    static constexpr int CPR = AttnCfg<T>::ROWB / 16;          // 16-byte chunks per 64-element row: 8 (bf16) | 16 (fp32)
    static constexpr int IT = 64 * CPR / kXThreads;            // chunks per thread and image: 2 | 4
    u32x4 v[N][IT];
    __device__ __forceinline__ void issue1(int n, const T* src, size_t ld, int lo, int hi) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int id = threadIdx.x + it * kXThreads, row = id / CPR, c = id % CPR;
            v[n][it] = u32x4{0u, 0u, 0u, 0u};
            if (row >= lo && row < hi) v[n][it] = *(const u32x4*)((const char*)(src + (ptrdiff_t)row * (ptrdiff_t)ld) + c * 16);
        }
    }
    __device__ __forceinline__ void commit1(int n, char* img, int pitch) const {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int id = threadIdx.x + it * kXThreads, row = id / CPR, c = id % CPR;
            *(u32x4*)(img + row * pitch + c * 16) = v[n][it];
        }
    }
    // cdst[row] = bias . row of image n, from the staging registers: the CPR consecutive lanes of a row each hold EPV elements
    __device__ __forceinline__ void bias_dot(int n, float* cdst, const float* bias64) const {
        constexpr int EPV = AttnCfg<T>::EPV;
        float bias[EPV];
#pragma unroll
        for (int q = 0; q < EPV; q += 4) *(f32x4*)(bias + q) = *(const f32x4*)(bias64 + (threadIdx.x % CPR) * EPV + q);
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int id = threadIdx.x + it * kXThreads, row = id / CPR, c = id % CPR;
            union { u32x4 u; T e[EPV]; } x;
            x.u = v[n][it];
            float part = 0.f;
#pragma unroll
            for (int q = 0; q < EPV; ++q) part += bias[q] * to_f(x.e[q]);
#pragma unroll
            for (int o = 1; o < CPR; o <<= 1) part += __shfl_xor(part, o, 64);
            if (c == 0) cdst[row] = part;
        }
    }
};

// this lane's MFMA fragment of row `row` of a token-major head (frag_nat's layout, straight from global memory; rows >= L are zero)
template <class T>
__device__ __forceinline__ typename Frag<T>::type xfrag_row(const T* __restrict__ head, size_t ld, int row, int L, int sl, int lane) {
    typedef AttnCfg<T> C;
    typename Frag<T>::type f = {};
    if (row < L) f = *(const typename Frag<T>::type*)(head + (size_t)row * ld + sl * C::SLAB + (lane >> 4) * C::EPV);
    return f;
}

// column sums of the [64 rows][64] output tiles of the four waves -> one grad_add per column (as attention_tiled.hip)
template <int NS>
__device__ __forceinline__ void xflush_colsums(const f32x4 (&o)[NS][4], float* csw, float* const (&dst)[NS], const GradAcc& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sred = row16_sum_to_lane15(o[s][dt][r]);
                if ((lane & 15) == 15) csw[(s * kXNW + wave) * 64 + dt * 16 + (lane >> 4) * 4 + r] = sred;
            }
    __syncthreads();
    for (int x = threadIdx.x; x < NS * 64; x += kXThreads) {
        const int s = x >> 6, col = x & 63;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < kXNW; ++w) t += csw[(s * kXNW + w) * 64 + col];
        grad_add(acc, dst[s] + col, t);
    }
}

// The stream of one query block: K | V tiles and kr chunks into their rings, bias columns and key meta words next to them.
// Chunk k holds the kr rows [c0 + 64 k, c0 + 64 k + 64) of this sample, c0 = L - i0 - 63 (rows outside [0, 2L) are zero).
template <class T>
struct XlStream {
    typedef AttnCfg<T> C;
    typedef XlCfg<T> X;
    XTileStage<T, 3> st;
    int meta;
    const T* kv; const T* krb; size_t ld; int H, L, c0;
    const int64_t* segrow; const int64_t* maskrow;
    char* smem;
    __device__ __forceinline__ void init(const T* base, const T* krsample, int H_, int L_, int i0, const XlTParams& xp, int b, int h, char* sm) {
        H = H_; L = L_; ld = (size_t)3 * H_; kv = base + H_; krb = krsample + h * 64; c0 = L_ - i0 - 63;
        segrow = xp.seg + (size_t)b * L_; maskrow = xp.mask + (size_t)b * L_; smem = sm;
        if (threadIdx.x < 128) ((float*)(sm + X::O_BIAS))[threadIdx.x] = threadIdx.x < 64 ? xp.r_w_bias[h * 64 + threadIdx.x] : xp.r_r_bias[h * 64 + threadIdx.x - 64];
        meta = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void issue_kv(int t) {
        st.issue1(0, kv + (size_t)t * 64 * ld, ld, 0, L - t * 64);
        st.issue1(1, kv + (size_t)t * 64 * ld + H, ld, 0, L - t * 64);
        if (threadIdx.x < 64) {
            const int j = t * 64 + threadIdx.x;
            meta = j < L ? (((int)segrow[j] & 0xffff) | (maskrow[j] == 0 ? kMetaPad : 0)) : kMetaNone;
        }
    }
    __device__ __forceinline__ void commit_kv(int t) {
        const int slot = t & 1;
        st.commit1(0, smem + slot * 2 * X::IMG, X::PIT);
        st.commit1(1, smem + slot * 2 * X::IMG + X::IMG, X::PIT);
        st.bias_dot(0, (float*)(smem + X::O_CK) + slot * 64, (const float*)(smem + X::O_BIAS));
        if (threadIdx.x < 64) ((int*)(smem + X::O_META))[slot * 64 + threadIdx.x] = meta;
    }
    __device__ __forceinline__ void issue_kr(int k) {
        const int p0 = c0 + 64 * k;                           // sample row of the chunk's row 0 (may be negative)
        st.issue1(2, krb + (ptrdiff_t)p0 * H, (size_t)H, -p0, 2 * L - p0);
    }
    __device__ __forceinline__ void commit_kr(int k) {
        const int slot = k % 3;
        st.commit1(2, smem + X::O_KR + slot * X::IMG, X::PIT);
        st.bias_dot(2, (float*)(smem + X::O_CR) + slot * 64, (const float*)(smem + X::O_BIAS) + 64);
    }
    // K | V tile 0 and chunks 0, 1 (call with the rings free; ends in a barrier)
    __device__ __forceinline__ void prime() {
        issue_kv(0); issue_kr(0);
        commit_kv(0); commit_kr(0);
        issue_kr(1);
        commit_kr(1);
        __syncthreads();
    }
    // in front of the products of tile t / behind them (the caller's barrier follows)
    __device__ __forceinline__ void ahead(int t, int nkt) {
        if (t + 1 < nkt) { issue_kv(t + 1); issue_kr(t + 2); }
    }
    __device__ __forceinline__ void behind(int t, int nkt) {
        if (t + 1 < nkt) { commit_kv(t + 1); commit_kr(t + 2); }
    }
};

// masked, scaled scores of key tile t for this lane's query row i: s[jt][r] = S[i][j], j = t*64 + jt*16 + (lane>>4)*4 + r.
// NPT position tiles of 16 from window row `wstart` on go through the wave's raw strip; `coff` = strip column of window row 48 - 16 wave;
// prow = this row's perm bytes or null.
template <class T, int NPT>
__device__ __forceinline__ void xl_tile_scores(const char* smem, int t, const typename Frag<T>::type (&qf)[XlCfg<T>::DSL], char* raw,
                                               int wstart, int coff, int i, int si, float e0, float e1, const uint8_t* __restrict__ prow, int gstream,
                                               int lane, f32x4 (&s)[4]) {
    typedef XlCfg<T> X;
    const int slot = t & 1, g = lane >> 4, ii = lane & 15;
    const char* Ki = smem + slot * 2 * X::IMG;
    const float* cK = (const float*)(smem + X::O_CK) + slot * 64;
    const int* meta = (const int*)(smem + X::O_META) + slot * 64;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        s[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < X::DSL; ++sl) mma16(s[jt], frag_nat<T>(Ki, X::PIT, jt * 16 + ii, sl, lane), qf[sl]);
    }
#pragma unroll
    for (int q = 0; q < NPT; ++q) {
        const int wr = wstart + q * 16, cslot = (t + (wr >> 6)) % 3, row0 = wr & 63;
        const char* Ri = smem + X::O_KR + cslot * X::IMG;
        f32x4 rw = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < X::DSL; ++sl) mma16(rw, frag_nat<T>(Ri, X::PIT, row0 + ii, sl, lane), qf[sl]);
        rw += *(const f32x4*)((const float*)(smem + X::O_CR) + cslot * 64 + row0 + g * 4);
        store4((T*)(raw + ii * X::RPIT) + q * 16 + g * 4, rw);          // raw[i][p] = (q_i + r_r_bias) . kr_p
    }
    wave_lds_fence();
    const float scale = 0.125f;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        const f32x4 ck4 = *(const f32x4*)(cK + jt * 16 + g * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jj = jt * 16 + g * 4 + r, j = t * 64 + jj;
            const int mj = meta[jj];
            const float bd = to_f(*(const T*)(raw + ii * X::RPIT + (coff + 15 - ii + jj) * (int)sizeof(T)));
            float sc = (s[jt][r] + ck4[r] + bd + (si == (mj & 0xffff) ? e0 : e1)) * scale;
            if (mj & kMetaNone) sc = -INFINITY;
            else if ((i != j || gstream) && ((mj & kMetaPad) || (prow != nullptr && prow[j] != 0))) sc -= kXlMaskT;
            s[jt][r] = sc;
        }
    }
    wave_lds_fence();
}

// e_s = (q_i + r_s_bias) . seg_embed[s] (seg_embed rounded to the activation dtype, as the resident kernels' MFMA operand)
template <class T>
__device__ __forceinline__ void xl_seg_terms(const typename Frag<T>::type (&qf)[XlCfg<T>::DSL], const XlTParams& xp, int h, int nh, int lane,
                                             float& e0, float& e1) {
    typedef AttnCfg<T> C;
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int sl = 0; sl < XlCfg<T>::DSL; ++sl)
#pragma unroll
        for (int e = 0; e < C::EPV; ++e) {
            const int d = sl * C::SLAB + (lane >> 4) * C::EPV + e;
            const float qv = (float)qf[sl][e] + xp.r_s_bias[h * 64 + d];
            a0 += qv * to_f(from_f<T>(xp.seg_embed[(size_t)h * 64 + d]));
            a1 += qv * to_f(from_f<T>(xp.seg_embed[((size_t)nh + h) * 64 + d]));
        }
    e0 = quad_sum(a0);
    e1 = quad_sum(a1);
}

}  // namespace

// bf16: two workgroups per CU by LDS (80.1 KB) and by registers (<= 256); fp32 (the parity mode) holds up to 150 KB of LDS: one.
#define MB_XLT_BOUNDS __launch_bounds__(kXThreads, sizeof(T) == 2 ? 2 : 1)

// =============================================================================================== forward
template <class T>
__global__ void MB_XLT_BOUNDS xl_tiled_fwd_kernel(const T* __restrict__ qkv, const T* __restrict__ kr, XlTParams xp, T* __restrict__ vec,
                                                  float* __restrict__ stats, float* __restrict__ probs, int L, int nh, int nqb, size_t plane,
                                                  DropKey drop) {
    drop.resolve();
    typedef AttnCfg<T> C;
    typedef XlCfg<T> X;
    typedef AccOp<T> AO;
    typedef typename Frag<T>::type F;
    constexpr int LSL = 64 / C::SLAB;
    __shared__ __attribute__((aligned(16))) char smem[X::BYTES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bh = blockIdx.x / nqb, b = bh / nh, h = bh % nh;
    const int H = nh * 64;
    const size_t ld = (size_t)3 * H;
    const T* base = qkv + (size_t)b * L * ld + h * 64;
    const int i0 = (blockIdx.x % nqb) * 64;
    const int i = i0 + wave * 16 + (lane & 15);      // this lane's query row
    const int nkt = (L + 63) / 64;

    XlStream<T> sm;
    sm.init(base, kr + (size_t)b * 2 * L * H, H, L, i0, xp, b, h, smem);
    sm.issue_kv(0); sm.issue_kr(0);
    F qf[X::DSL];
#pragma unroll
    for (int sl = 0; sl < X::DSL; ++sl) qf[sl] = xfrag_row<T>(base, ld, i, L, sl, lane);
    sm.commit_kv(0); sm.commit_kr(0);
    sm.issue_kr(1);
    float e0, e1;
    xl_seg_terms<T>(qf, xp, h, nh, lane, e0, e1);
    const int si = i < L ? ((int)xp.seg[(size_t)b * L + i] & 0xffff) : -1;
    sm.commit_kr(1);
    __syncthreads();

    char* raw = smem + X::O_ST + wave * 16 * X::RPIT;
    const int wstart = 48 - 16 * wave;
    const float hs = xp.head_scale ? xp.head_scale[h] : 1.0f;
    const uint32_t rowidx = ((uint32_t)bh * L + (uint32_t)i) * L;
    const uint8_t* prow = (xp.perm != nullptr && i < L) ? xp.perm + ((size_t)b * L + i) * L : nullptr;
    float m = -3.0e38f, lpart = 0.f;        // running row max (uniform over the row's four lanes), this lane's share of the normaliser
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < nkt; ++t) {
        int lane = threadIdx.x & 63;          // opaque per tile: see xl_tiled_bwd_q_kernel
        asm volatile("" : "+v"(lane));
        sm.ahead(t, nkt);
        const char* Vi = smem + (t & 1) * 2 * X::IMG + X::IMG;
        f32x4 s[4];
        xl_tile_scores<T, 5>(smem, t, qf, raw, wstart, 0, i, si, e0, e1, prow, xp.gstream, lane, s);
        float mx = m;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) mx = fmaxf(mx, fmaxf(fmaxf(s[jt][0], s[jt][1]), fmaxf(s[jt][2], s[jt][3])));
        mx = quad_max(mx);                  // finite: tile 0 holds key 0 < L, and a masked score is -1e30, not -inf
        const float alpha = __expf(m - mx);
        m = mx;
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[jt][r] = __expf(s[jt][r] - mx);          // keys beyond L: exp(-inf) = 0
                sum += s[jt][r];
                s[jt][r] *= drop_mult(drop, rowidx + t * 64 + jt * 16 + (lane >> 4) * 4 + r);     // the P.V operand only
            }
        lpart = lpart * alpha + sum;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            o[dt] = o[dt] * alpha;
#pragma unroll
            for (int sl = 0; sl < LSL; ++sl)
                mma16(o[dt], AO::kmaj(Vi, X::PIT, sl, dt * 16 + (lane & 15), lane), AO::make(&s[sl * AO::TILES]));
        }
        sm.behind(t, nkt);
        __syncthreads();
    }
    const float inv = 1.0f / quad_sum(lpart);
    if (i < L && vec != nullptr) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4(vec + ((size_t)b * L + i) * H + h * 64 + dt * 16 + (lane >> 4) * 4, o[dt] * (inv * hs));
        if ((lane >> 4) == 0 && stats != nullptr) { stats[(size_t)bh * L + i] = m; stats[plane + (size_t)bh * L + i] = inv; }
    }
    if (probs == nullptr) return;
    // the probabilities before dropout: a second sweep once the normaliser is known
    sm.prime();
#pragma unroll 1
    for (int t = 0; t < nkt; ++t) {
        sm.ahead(t, nkt);
        f32x4 s[4];
        xl_tile_scores<T, 5>(smem, t, qf, raw, wstart, 0, i, si, e0, e1, prow, xp.gstream, lane, s);
        if (i < L) {
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t * 64 + jt * 16 + (lane >> 4) * 4 + r;
                    if (j < L) probs[((size_t)bh * L + i) * L + j] = __expf(s[jt][r] - m) * inv;
                }
        }
        sm.behind(t, nkt);
        __syncthreads();
    }
}

// =============================================================================================== backward: query blocks
template <class T>
__global__ void MB_XLT_BOUNDS xl_tiled_bwd_q_kernel(const T* __restrict__ qkv, const T* __restrict__ kr, XlTParams xp,
                                                    const T* __restrict__ vec, const T* __restrict__ dvec, const float* __restrict__ stats,
                                                    T* __restrict__ gsave, T* __restrict__ pdsave, T* __restrict__ dqkv, float* d_rwb,
                                                    float* d_rrb, float* d_rsb, float* d_seg, int L, int nh, int nqb, size_t plane,
                                                    DropKey drop) {
    drop.resolve();
    typedef AttnCfg<T> C;
    typedef XlCfg<T> X;
    typedef AccOp<T> AO;
    typedef typename Frag<T>::type F;
    constexpr int LSL = 64 / C::SLAB, RSL = 96 / C::SLAB;
    __shared__ __attribute__((aligned(16))) char smem[X::BYTES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, ii = lane & 15;
    const int bh = blockIdx.x / nqb, b = bh / nh, h = bh % nh;
    const int H = nh * 64;
    const size_t ld = (size_t)3 * H;
    const T* base = qkv + (size_t)b * L * ld + h * 64;
    const int i0 = (blockIdx.x % nqb) * 64;
    const int i = i0 + wave * 16 + ii;
    const int nkt = (L + 63) / 64, LP = nkt * 64;
    (void)g;

    XlStream<T> sm;
    sm.init(base, kr + (size_t)b * 2 * L * H, H, L, i0, xp, b, h, smem);
    sm.issue_kv(0); sm.issue_kr(0);
    F qf[X::DSL], of[X::DSL];
    float dpart = 0.f;
#pragma unroll
    for (int sl = 0; sl < X::DSL; ++sl) {
        qf[sl] = xfrag_row<T>(base, ld, i, L, sl, lane);
        of[sl] = xfrag_row<T>(dvec + (size_t)b * L * H + h * 64, H, i, L, sl, lane);
        if constexpr (sizeof(T) == 4) {
            const F cf = xfrag_row<T>(vec + (size_t)b * L * H + h * 64, H, i, L, sl, lane);
#pragma unroll
            for (int e = 0; e < C::EPV; ++e) dpart += (float)of[sl][e] * (float)cf[e];
        }
    }
    float D = quad_sum(dpart);                        // fp32: D_i = dvec_i . vec_i (vec carries dropout and head_scale); bf16: below
    float mi = 0.f, invi = 0.f;
    if (i < L) { mi = stats[(size_t)bh * L + i]; invi = stats[plane + (size_t)bh * L + i]; }
    sm.commit_kv(0); sm.commit_kr(0);
    sm.issue_kr(1);
    float e0, e1;
    xl_seg_terms<T>(qf, xp, h, nh, lane, e0, e1);
    const int si = i < L ? ((int)xp.seg[(size_t)b * L + i] & 0xffff) : -1;
    char* Ss = smem + X::O_ST + wave * 16 * X::RPIT;      // the wave's strip: raw position products, then G shifted to position space
    sm.commit_kr(1);
    __syncthreads();

    // window rows [wstart, wstart + 96) of every tile hold all 79 positions the wave's rows reach (wave 0: moved down to end at 128)
    const int wstart = 48 - 16 * wave < 32 ? 48 - 16 * wave : 32, coff = 48 - 16 * wave - wstart;
    const float scale = 0.125f;
    const float hs = xp.head_scale ? xp.head_scale[h] : 1.0f;
    const uint32_t rowidx = ((uint32_t)bh * L + (uint32_t)i) * L;
    const uint8_t* prow = (xp.perm != nullptr && i < L) ? xp.perm + ((size_t)b * L + i) * L : nullptr;
    const size_t srow = ((size_t)bh * LP + (i < LP ? i : 0)) * LP;      // scratch row of this lane
    if constexpr (sizeof(T) == 2) {
        // bf16: D_i = sum_j Pd_ij (dvec V^T)_ij from a sweep of its own, in fp32 and with the very products the main sweep forms.  The
        // forward's vec is rounded to bf16, and dvec_i . vec_i carries that rounding (2^-9 of |vec|, 64 terms) into every G_ij = P_ij
        // (.. - D_i): where a row's probability sits on ONE key G is exactly zero, and what came out instead was 4e-3 per row --
        // summed over the rows of a fully padded sample into dkr[L] (their diagonals all map there): 7.3e-2 at L = 200, 1.5e-1 at
        // L = 449 against max|dkr| 1.0, and 7.8e-3 at L = 1 where dkr is zero.  Costs the forward's products once more.
        float dacc = 0.f;
#pragma unroll 1
        for (int t = 0; t < nkt; ++t) {
            int lane = threadIdx.x & 63;          // opaque per tile: see the main sweep
            asm volatile("" : "+v"(lane));
            const int g = lane >> 4, ii = lane & 15;
            sm.ahead(t, nkt);
            const char* Vi = smem + (t & 1) * 2 * X::IMG + X::IMG;
            f32x4 s[4];
            xl_tile_scores<T, 6>(smem, t, qf, Ss, wstart, coff, i, si, e0, e1, prow, 0, lane, s);
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                f32x4 dpj = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int sl = 0; sl < X::DSL; ++sl) mma16(dpj, frag_nat<T>(Vi, X::PIT, jt * 16 + ii, sl, lane), of[sl]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = i < L ? __expf(s[jt][r] - mi) * invi : 0.f;
                    const float dm = drop_mult(drop, rowidx + t * 64 + jt * 16 + g * 4 + r) * hs;
                    dacc += (p * dm) * dpj[r];
                }
            }
            sm.behind(t, nkt);
            __syncthreads();
        }
        D = quad_sum(dacc);
        if (nkt > 1) sm.prime();              // (one tile: the rings still hold tile 0 and chunks 0, 1)
    }
    float g0 = 0.f, g1 = 0.f;
    f32x4 oa[4], ob[4];                // dq pieces: G.K and Gshift.KR
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oa[dt] = ob[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < nkt; ++t) {
        // (the lane index is made opaque per tile: hoisted out of the loop, the LDS addresses of every fragment read below -- loop
        //  invariants all -- take more registers than the kernel has, and recomputing them is a few VALU operations per read.
        //  With it: 252 registers here, 209 in the forward, no spills; without it 256 and 6 spilled.  The margin under the 256 of
        //  two workgroups per CU is FOUR registers and rests on this compiler's allocation: tests/test_xlnet_long_cpu.py reads the
        //  code object and fails on any spill, scratch or a third of the register file -- a compiler change shows there first)
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));
        const int g = lane >> 4, ii = lane & 15;
        sm.ahead(t, nkt);
        const char* Ki = smem + (t & 1) * 2 * X::IMG;
        const char* Vi = Ki + X::IMG;
        const int* meta = (const int*)(smem + X::O_META) + (t & 1) * 64;
        f32x4 s[4];
        xl_tile_scores<T, 6>(smem, t, qf, Ss, wstart, coff, i, si, e0, e1, prow, 0, lane, s);
        // s -> G, dp -> Pd ; the strip's columns [coff + 15 - ii, coff + 78 - ii] of row ii are rewritten every tile, the others stay
        // what the raw products left there: they are cleared first
        for (int x = lane; x < 16 * X::RPIT / 16; x += 64) *(u32x4*)(Ss + x * 16) = u32x4{0u, 0u, 0u, 0u};
        wave_lds_fence();
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            f32x4 dpj = {0.f, 0.f, 0.f, 0.f};          // (dvec V^T)[i][j], then Pd
#pragma unroll
            for (int sl = 0; sl < X::DSL; ++sl) mma16(dpj, frag_nat<T>(Vi, X::PIT, jt * 16 + ii, sl, lane), of[sl]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jj = jt * 16 + g * 4 + r;
                const float p = i < L ? __expf(s[jt][r] - mi) * invi : 0.f;        // keys beyond L: exp(-inf) = 0
                const float dm = drop_mult(drop, rowidx + t * 64 + jj) * hs;
                const float gv = p * (dpj[r] * dm - D) * scale;
                s[jt][r] = gv;
                dpj[r] = p * dm;
                if (si == (meta[jj] & 0xffff)) g0 += gv; else g1 += gv;
                *(T*)(Ss + ii * X::RPIT + (coff + 15 - ii + jj) * (int)sizeof(T)) = from_f<T>(gv);
            }
            if (i < L) {
                store4(gsave + srow + t * 64 + jt * 16 + g * 4, s[jt]);
                store4(pdsave + srow + t * 64 + jt * 16 + g * 4, dpj);
            }
        }
        wave_lds_fence();
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
            for (int sl = 0; sl < LSL; ++sl)
                mma16(oa[dt], AO::kmaj(Ki, X::PIT, sl, dt * 16 + ii, lane), AO::make(&s[sl * AO::TILES]));
#pragma unroll
            for (int sl = 0; sl < RSL; ++sl) {
                const int wr = wstart + sl * C::SLAB + g * C::EPV, cslot = (t + (wr >> 6)) % 3;
                mma16(ob[dt], frag_kmaj(smem + X::O_KR + cslot * X::IMG, X::PIT, wr & 63, dt * 16 + ii, T()),
                      frag_nat<T>(Ss, X::RPIT, ii, sl, lane));
            }
        }
        wave_lds_fence();
        sm.behind(t, nkt);
        __syncthreads();
    }
    g0 = quad_sum(g0);
    g1 = quad_sum(g1);
    f32x4 oc[5][4];                    // column-sum tiles: [0] G.K  [1] Gshift.KR  [2] sum_j G.seg ; [3], [4] seg_embed gradient rows
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const int d = dt * 16 + g * 4;
        oc[0][dt] = oa[dt]; oc[1][dt] = ob[dt];
        if (i < L) {
            const f32x4 s0v = *(const f32x4*)(xp.seg_embed + (size_t)h * 64 + d), s1v = *(const f32x4*)(xp.seg_embed + ((size_t)nh + h) * 64 + d);
            const f32x4 rs = *(const f32x4*)(xp.r_s_bias + h * 64 + d);
            oc[2][dt] = g0 * s0v + g1 * s1v;
            store4(dqkv + ((size_t)b * L + i) * ld + h * 64 + d, oc[0][dt] + oc[1][dt] + oc[2][dt]);
            const f32x4 qv = load4(base + (size_t)i * ld + d) + rs;          // q_i + r_s_bias
            oc[3][dt] = g0 * qv;
            oc[4][dt] = g1 * qv;
        } else {
#pragma unroll
            for (int n = 0; n < 5; ++n) oc[n][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    float* const dst[5] = {d_rwb + h * 64, d_rrb + h * 64, d_rsb + h * 64, d_seg + (size_t)h * 64, d_seg + ((size_t)nh + h) * 64};
    xflush_colsums<5>(oc, (float*)smem, dst, xp.acc);      // (the last tile's barrier freed the rings)
}

// =============================================================================================== backward: key blocks (dk, dv)
template <class T>
__global__ void MB_XLT_BOUNDS xl_tiled_bwd_kv_kernel(const T* __restrict__ qkv, XlTParams xp, const T* __restrict__ dvec,
                                                     const T* __restrict__ gsave, const T* __restrict__ pdsave, T* __restrict__ dqkv,
                                                     int L, int nh, int nkb) {
    typedef AttnCfg<T> C;
    constexpr int PIT = C::ROWB + 16, IMG = 64 * PIT, LSL = 64 / C::SLAB;
    __shared__ __attribute__((aligned(16))) char smem[2][4 * IMG];      // ring slot: Q | dO | G | Pd tiles, rows = queries
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int bh = blockIdx.x / nkb, b = bh / nh, h = bh % nh, kb = blockIdx.x % nkb;
    const int H = nh * 64;
    const size_t ld = (size_t)3 * H;
    const T* base = qkv + (size_t)b * L * ld + h * 64;
    const T* obase = dvec + (size_t)b * L * H + h * 64;
    const int jl = wave * 16 + (lane & 15), j = kb * 64 + jl;      // this lane's key
    const int nqt = (L + 63) / 64, LP = nqt * 64;
    const T* gb = gsave + (size_t)bh * LP * LP + kb * 64;
    const T* pb = pdsave + (size_t)bh * LP * LP + kb * 64;

    XTileStage<T, 4> st;
    auto issue = [&](int t) {
        const int valid = L - t * 64;
        st.issue1(0, base + (size_t)t * 64 * ld, ld, 0, valid);
        st.issue1(1, obase + (size_t)t * 64 * H, (size_t)H, 0, valid);
        st.issue1(2, gb + (size_t)t * 64 * LP, (size_t)LP, 0, valid);
        st.issue1(3, pb + (size_t)t * 64 * LP, (size_t)LP, 0, valid);
    };
    auto commit = [&](int slot) {
#pragma unroll
        for (int n = 0; n < 4; ++n) st.commit1(n, smem[slot] + n * IMG, PIT);
    };
    issue(0);
    commit(0);
    __syncthreads();
    float csum = 0.f;
    f32x4 ov[4], ok[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ov[dt] = ok[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < nqt; ++t) {
        const int slot = t & 1;
        if (t + 1 < nqt) issue(t + 1);
        const char* Qi = smem[slot];
        const char* Oi = Qi + IMG;
        const char* Gi = Oi + IMG;
        const char* Pi = Gi + IMG;
#pragma unroll
        for (int m = 0; m < 16; ++m) csum += to_f(*(const T*)(Gi + (g + 4 * m) * PIT + jl * (int)sizeof(T)));
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int sl = 0; sl < LSL; ++sl) {
                const int k0 = sl * C::SLAB + g * C::EPV;
                mma16(ov[dt], frag_kmaj(Oi, PIT, k0, dt * 16 + (lane & 15), T()), frag_kmaj(Pi, PIT, k0, jl, T()));
                mma16(ok[dt], frag_kmaj(Qi, PIT, k0, dt * 16 + (lane & 15), T()), frag_kmaj(Gi, PIT, k0, jl, T()));
            }
        if (t + 1 < nqt) commit(slot ^ 1);
        __syncthreads();
    }
    csum = quad_sum(csum);
    if (j < L) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const int d = dt * 16 + g * 4;
            store4(dqkv + ((size_t)b * L + j) * ld + 2 * H + h * 64 + d, ov[dt]);
            store4(dqkv + ((size_t)b * L + j) * ld + H + h * 64 + d, ok[dt] + csum * *(const f32x4*)(xp.r_w_bias + h * 64 + d));      // + (sum_i G[i,j]) r_w_bias
        }
    }
}

// =============================================================================================== backward: position blocks (dkr)
template <class T>
__global__ void MB_XLT_BOUNDS xl_tiled_bwd_pos_kernel(const T* __restrict__ qkv, XlTParams xp, const T* __restrict__ gsave,
                                                      T* __restrict__ dkr, int L, int nh, int npb) {
    typedef AttnCfg<T> C;
    constexpr int PIT = C::ROWB + 16, IMG = 64 * PIT, LSL = 64 / C::SLAB;
    __shared__ __attribute__((aligned(16))) char smem[2 * IMG + kXNW * 16 * PIT];      // Q tile ring | per-wave diagonal strips [16 p][64 i]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
    const int bh = blockIdx.x / npb, b = bh / nh, h = bh % nh, p0 = (blockIdx.x % npb) * 64;
    const int H = nh * 64;
    const size_t ld = (size_t)3 * H;
    const T* base = qkv + (size_t)b * L * ld + h * 64;
    const int p = p0 + wave * 16 + (lane & 15);          // this lane's position row
    const int nqt = (L + 63) / 64, LP = nqt * 64;
    const T* gb = gsave + (size_t)bh * LP * LP;
    char* St = smem + 2 * IMG + wave * 16 * PIT;
    // query tiles that hold a piece of the band j = p - L + i, p in [p0, p0 + 64): j in [p0 - L + 64 t, p0 - L + 64 t + 126] meets [0, L)
    int t_lo = L - p0 - 126 <= 0 ? 0 : (L - p0 - 126 + 63) / 64;
    int t_hi = 2 * L - 1 - p0 < 0 ? -1 : (2 * L - 1 - p0) / 64;
    if (t_hi > nqt - 1) t_hi = nqt - 1;

    XTileStage<T, 1> st;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float csum = 0.f;
    if (t_lo <= t_hi) {
        st.issue1(0, base + (size_t)t_lo * 64 * ld, ld, 0, L - t_lo * 64);
        st.commit1(0, smem + (t_lo & 1) * IMG, PIT);
    }
    __syncthreads();
#pragma unroll 1
    for (int t = t_lo; t <= t_hi; ++t) {
        if (t + 1 <= t_hi) st.issue1(0, base + (size_t)(t + 1) * 64 * ld, ld, 0, L - (t + 1) * 64);
        const char* Qi = smem + (t & 1) * IMG;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int il = it * 16 + g * 4;
            f32x4 gv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = t * 64 + il + r, j = p - L + i;
                gv[r] = (i < L && j >= 0 && j < L) ? to_f(gb[(size_t)i * LP + j]) : 0.f;
                csum += gv[r];
            }
            store4((T*)(St + (lane & 15) * PIT) + il, gv);
        }
        wave_lds_fence();
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int sl = 0; sl < LSL; ++sl)
                mma16(o[dt], frag_kmaj(Qi, PIT, sl * C::SLAB + g * C::EPV, dt * 16 + (lane & 15), T()), frag_nat<T>(St, PIT, lane & 15, sl, lane));
        wave_lds_fence();
        if (t + 1 <= t_hi) st.commit1(0, smem + ((t + 1) & 1) * IMG, PIT);
        __syncthreads();
    }
    csum = quad_sum(csum);
    if (p < 2 * L) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const int d = dt * 16 + g * 4;
            store4(dkr + ((size_t)b * 2 * L + p) * H + h * 64 + d, o[dt] + csum * *(const f32x4*)(xp.r_r_bias + h * 64 + d));
        }
    }
}

// =============================================================================================== host
size_t xlnet_tiled_stats_floats(int B, int L, int nh) { return (size_t)2 * B * nh * L; }
size_t xlnet_tiled_scratch_elems(int B, int L, int nh) {
    const size_t LP = (size_t)(L + 63) / 64 * 64;
    return (size_t)B * nh * LP * LP;
}

// shapes (and the uint32 dropout index) are checked before any pointer is looked at
static int xl_tiled_check(int dtype, int B, int L, int nh, const DropKey& drop) {
    if (B < 1 || L < 1 || L > 512 || nh < 1 || (int64_t)B * nh * ((2 * L + 63) / 64) > 0x7fffffff) return MB_ERR_SHAPE;
    if (drop.thresh != 0u && (uint64_t)B * nh * L * L >= ((uint64_t)1 << 32)) return MB_ERR_SHAPE;
    if (dtype != DT_BF16 && dtype != DT_F32) return MB_ERR_DTYPE;
    return MB_OK;
}

int xlnet_attention_tiled_forward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                                  const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask, void* vec,
                                  float* stats, int B, int L, int nh, DropKey drop, hipStream_t st, const float* head_scale,
                                  const uint8_t* perm, int gstream, float* probs) {
    if (int e = xl_tiled_check(dtype, B, L, nh, drop)) return e;
    if (!qkv || !kr || !r_w_bias || !r_r_bias || !r_s_bias || !seg_embed || !seg || !mask || (!vec && !probs)) return MB_ERR_ARG;
    const XlTParams xp = {r_w_bias, r_r_bias, r_s_bias, seg_embed, seg, mask, head_scale, perm, gstream, GradAcc{nullptr, nullptr}};
    const int nqb = (L + 63) / 64;
    const size_t plane = (size_t)B * nh * L;
    const dim3 grid(B * nh * nqb), block(kXThreads);
    if (dtype == DT_BF16)
        hipLaunchKernelGGL(xl_tiled_fwd_kernel<bf16>, grid, block, 0, st, (const bf16*)qkv, (const bf16*)kr, xp, (bf16*)vec, stats, probs, L, nh,
                           nqb, plane, drop);
    else
        hipLaunchKernelGGL(xl_tiled_fwd_kernel<float>, grid, block, 0, st, (const float*)qkv, (const float*)kr, xp, (float*)vec, stats, probs, L,
                           nh, nqb, plane, drop);
    return (int)hipGetLastError();
}

template <class T>
static int xl_tiled_backward_launch(const void* qkv, const void* kr, const XlTParams& xp, const void* vec, const void* dvec, const float* stats,
                                    void* gsave, void* pdsave, void* dqkv, void* dkr, float* d_rwb, float* d_rrb, float* d_rsb, float* d_seg,
                                    int B, int L, int nh, DropKey drop, hipStream_t st) {
    const int nb = (L + 63) / 64, npb = (2 * L + 63) / 64;
    const size_t plane = (size_t)B * nh * L;
    hipLaunchKernelGGL(xl_tiled_bwd_q_kernel<T>, dim3(B * nh * nb), dim3(kXThreads), 0, st, (const T*)qkv, (const T*)kr, xp, (const T*)vec,
                       (const T*)dvec, stats, (T*)gsave, (T*)pdsave, (T*)dqkv, d_rwb, d_rrb, d_rsb, d_seg, L, nh, nb, plane, drop);
    if (hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(xl_tiled_bwd_kv_kernel<T>, dim3(B * nh * nb), dim3(kXThreads), 0, st, (const T*)qkv, xp, (const T*)dvec, (const T*)gsave,
                       (const T*)pdsave, (T*)dqkv, L, nh, nb);
    if (hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(xl_tiled_bwd_pos_kernel<T>, dim3(B * nh * npb), dim3(kXThreads), 0, st, (const T*)qkv, xp, (const T*)gsave, (T*)dkr, L, nh,
                       npb);
    return (int)hipGetLastError();
}

int xlnet_attention_tiled_backward(int dtype, const void* qkv, const void* kr, const float* r_w_bias, const float* r_r_bias,
                                   const float* r_s_bias, const float* seg_embed, const int64_t* seg, const int64_t* mask,
                                   const void* vec, const void* dvec, const float* stats, void* gsave, void* pdsave, void* dqkv, void* dkr,
                                   float* d_rwb, float* d_rrb, float* d_rsb, float* d_seg, int B, int L, int nh, DropKey drop,
                                   hipStream_t st, const float* head_scale, const uint8_t* perm, GradAcc acc) {
    if (int e = xl_tiled_check(dtype, B, L, nh, drop)) return e;
    if (!qkv || !kr || !r_w_bias || !r_r_bias || !r_s_bias || !seg_embed || !seg || !mask || !vec || !dvec || !stats || !gsave || !pdsave ||
        !dqkv || !dkr || !d_rwb || !d_rrb || !d_rsb || !d_seg)
        return MB_ERR_ARG;
    const XlTParams xp = {r_w_bias, r_r_bias, r_s_bias, seg_embed, seg, mask, head_scale, perm, 0, acc};
    if (dtype == DT_BF16)
        return xl_tiled_backward_launch<bf16>(qkv, kr, xp, vec, dvec, stats, gsave, pdsave, dqkv, dkr, d_rwb, d_rrb, d_rsb, d_seg, B, L, nh, drop, st);
    return xl_tiled_backward_launch<float>(qkv, kr, xp, vec, dvec, stats, gsave, pdsave, dqkv, dkr, d_rwb, d_rrb, d_rsb, d_seg, B, L, nh, drop, st);
}

}  // namespace mb
