// attn_bench -- torch-free timing of the BERT attention core through the C ABI (mb_attention_forward / _backward), with the
// per-block phase stamps of the backward when MB_ATTN_TRACE=1.  Measurement tooling (not product).
//   attn_bench [--batch B] [--seq L] [--heads nh] [--reps n] [--p dropout] [--tiled 0|1] [--xlnet 0|1]
// --tiled 1: the tiled pair (mb_attention_tiled_*, L <= 512; the engines' kernels for L > 128), with its row-statistics scratch
// --xlnet 1: MAG-XLNet's relative attention instead (mb_xlnet_attention_forward / _backward: the LDS-resident kernels, L <= 128; with
//            --tiled 1 mb_xlnet_attention_tiled_*, L <= 512: one forward launch, three backward launches -- a kernel trace splits them)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/magbert_hip.h"
#define HCK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(_e)); exit(2); } } while (0)
#define MCK(x) do { int _e = (x); if (_e) { fprintf(stderr, "%s:%d magbert error %d: %s\n", __FILE__, __LINE__, _e, mb_error_string(_e)); exit(3); } } while (0)

static void* dev_rand(size_t n_bf16, uint32_t seed) {
    std::vector<uint16_t> h(n_bf16);
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n_bf16; ++i) {
        s = s * 1664525u + 1013904223u;
        const float v = ((int)((s >> 9) & 0x7FFF) - 16384) * (1.0f / 16384.f);
        uint32_t b; memcpy(&b, &v, 4);
        h[i] = (uint16_t)(b >> 16);
    }
    void* d; HCK(hipMalloc(&d, n_bf16 * 2)); HCK(hipMemcpy(d, h.data(), n_bf16 * 2, hipMemcpyHostToDevice));
    return d;
}

int main(int argc, char** argv) {
    int B = 48, L = 50, nh = 12, reps = 96, tiled = 0, xlnet = 0; float pdrop = 0.1f;
    for (int i = 1; i + 1 < argc; i += 2) {
        std::string k = argv[i];
        if (k == "--batch") B = atoi(argv[i + 1]); else if (k == "--seq") L = atoi(argv[i + 1]); else if (k == "--heads") nh = atoi(argv[i + 1]);
        else if (k == "--reps") reps = atoi(argv[i + 1]); else if (k == "--p") pdrop = (float)atof(argv[i + 1]);
        else if (k == "--tiled") tiled = atoi(argv[i + 1]); else if (k == "--xlnet") xlnet = atoi(argv[i + 1]);
    }
    const int H = nh * 64, T = B * L, nset = 6;
    hipStream_t st; HCK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    std::vector<void*> qkv(nset), dctx(nset), ctx(nset), dqkv(nset);
    for (int s = 0; s < nset; ++s) {
        qkv[s] = dev_rand((size_t)T * 3 * H, 1 + s); dctx[s] = dev_rand((size_t)T * H, 20 + s);
        HCK(hipMalloc(&ctx[s], (size_t)T * H * 2)); HCK(hipMalloc(&dqkv[s], (size_t)T * 3 * H * 2));
    }
    std::vector<int64_t> hm((size_t)T, 1);
    for (int b = 0; b < B; ++b) for (int l = L - (b % 7); l < L; ++l) hm[(size_t)b * L + l] = 0;       // ragged tails like the padded batches
    int64_t* mask; HCK(hipMalloc(&mask, (size_t)T * 8)); HCK(hipMemcpy(mask, hm.data(), (size_t)T * 8, hipMemcpyHostToDevice));
    mb_dropkey key; mb_make_dropkey(1, 1, 17, pdrop, &key);
    hipEvent_t e0, e1; HCK(hipEventCreate(&e0)); HCK(hipEventCreate(&e1));
    auto timeit = [&](const char* name, auto launch) {
        for (int i = 0; i < 6; ++i) launch(i);
        HCK(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) launch(i);
        HCK(hipEventRecord(e1, st)); HCK(hipEventSynchronize(e1));
        float ms; HCK(hipEventElapsedTime(&ms, e0, e1));
        printf("%-28s B=%d L=%d heads=%d p=%.2f : %7.2f us/launch\n", name, B, L, nh, pdrop, ms * 1e3 / reps);
    };
    if (xlnet) {
        // left-padded batches (XLNet's layout), two segment ids, small random biases
        for (int b = 0; b < B; ++b) for (int l = 0; l < L; ++l) hm[(size_t)b * L + l] = l >= (b % 7) ? 1 : 0;
        HCK(hipMemcpy(mask, hm.data(), (size_t)T * 8, hipMemcpyHostToDevice));
        std::vector<int64_t> hs((size_t)T, 0);
        for (int b = 0; b < B; ++b) hs[(size_t)b * L + L - 1] = 2;
        int64_t* seg; HCK(hipMalloc(&seg, (size_t)T * 8)); HCK(hipMemcpy(seg, hs.data(), (size_t)T * 8, hipMemcpyHostToDevice));
        std::vector<float> hb((size_t)5 * H);
        for (size_t i = 0; i < hb.size(); ++i) hb[i] = (float)((int)((i * 2654435761u) >> 20 & 1023) - 512) * (1.0f / 2048.f);
        float* bias; HCK(hipMalloc(&bias, hb.size() * 4)); HCK(hipMemcpy(bias, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
        float* dpar; HCK(hipMalloc(&dpar, hb.size() * 4)); HCK(hipMemset(dpar, 0, hb.size() * 4));
        const float *rwb = bias, *rrb = bias + H, *rsb = bias + 2 * H, *sege = bias + 3 * H;
        const int LP = L <= 32 ? 32 : (L <= 64 ? 64 : 128);
        const size_t plane = std::max(mb_xlnet_attention_tiled_scratch_bytes(MB_DT_BF16, B, L, nh), (size_t)B * nh * LP * LP * 2);
        std::vector<void*> kr(nset), dkr(nset), psave(nset), gsave(nset), pdsave(nset);
        std::vector<float*> stats(nset);
        for (int s = 0; s < nset; ++s) {
            kr[s] = dev_rand((size_t)2 * T * H, 40 + s);
            HCK(hipMalloc(&dkr[s], (size_t)2 * T * H * 2)); HCK(hipMalloc(&psave[s], plane)); HCK(hipMalloc(&gsave[s], plane));
            HCK(hipMalloc(&pdsave[s], plane)); HCK(hipMalloc(&stats[s], mb_xlnet_attention_tiled_stats_bytes(B, L, nh)));
        }
        if (tiled) {
            timeit("xlnet tiled attention forward", [&](int i) {
                const int s = i % nset;
                MCK(mb_xlnet_attention_tiled_forward(MB_DT_BF16, qkv[s], kr[s], rwb, rrb, rsb, sege, seg, mask, ctx[s], stats[s], B, L, nh, &key,
                                                     nullptr, nullptr, 0, nullptr, st)); });
            timeit("xlnet tiled attention backward", [&](int i) {
                const int s = i % nset;
                MCK(mb_xlnet_attention_tiled_backward(MB_DT_BF16, qkv[s], kr[s], rwb, rrb, rsb, sege, seg, mask, ctx[s], dctx[s], stats[s], gsave[s],
                                                      pdsave[s], dqkv[s], dkr[s], dpar, dpar + H, dpar + 2 * H, dpar + 3 * H, B, L, nh, &key, nullptr,
                                                      nullptr, st)); });
            return 0;
        }
        timeit("xlnet attention forward", [&](int i) {
            const int s = i % nset;
            MCK(mb_xlnet_attention_forward(MB_DT_BF16, qkv[s], kr[s], rwb, rrb, rsb, sege, seg, mask, ctx[s], psave[s], stats[s], B, L, nh, &key,
                                           nullptr, nullptr, 0, st)); });
        timeit("xlnet attention backward", [&](int i) {
            const int s = i % nset;
            MCK(mb_xlnet_attention_backward(MB_DT_BF16, qkv[s], kr[s], rwb, rrb, rsb, sege, seg, mask, psave[s], ctx[s], dctx[s], stats[s], gsave[s],
                                            pdsave[s], dqkv[s], dkr[s], dpar, dpar + H, dpar + 2 * H, dpar + 3 * H, B, L, nh, &key, nullptr, nullptr,
                                            st)); });
        return 0;
    }
    if (tiled) {
        std::vector<float*> stats(nset);
        for (int s = 0; s < nset; ++s) HCK(hipMalloc(&stats[s], mb_attention_tiled_stats_bytes(B, L, nh)));
        timeit("tiled attention forward", [&](int i) {
            MCK(mb_attention_tiled_forward(MB_DT_BF16, qkv[i % nset], mask, ctx[i % nset], stats[i % nset], B, L, nh, &key, nullptr, nullptr, st)); });
        timeit("tiled attention backward", [&](int i) {
            MCK(mb_attention_tiled_backward(MB_DT_BF16, qkv[i % nset], mask, ctx[i % nset], dctx[i % nset], stats[i % nset], dqkv[i % nset],
                                            nullptr, B, L, nh, &key, nullptr, st)); });
        return 0;
    }
    timeit("attention forward", [&](int i) { MCK(mb_attention_forward(MB_DT_BF16, qkv[i % nset], mask, ctx[i % nset], B, L, nh, &key, st)); });
    timeit("attention backward", [&](int i) { MCK(mb_attention_backward(MB_DT_BF16, qkv[i % nset], mask, dctx[i % nset], dqkv[i % nset], B, L, nh, &key, st)); });
    std::vector<unsigned long long> tr((size_t)8192 * 8);
    const int nb = mb_debug_attention_trace(tr.data(), 8192);
    if (nb > 0) {
        static const char* nm[6] = {"entry", "operands staged", "query sweep done", "key sweep done", "bias sums in LDS", "exit"};
        static const int slot[6] = {0, 1, 2, 4, 6, 5};
        unsigned long long t00 = ~0ull;
        for (int b = 0; b < nb; ++b) t00 = std::min(t00, tr[(size_t)b * 8]);
        printf("    %d blocks; us after the first block's entry (min / median / max), then per-block phase length (median)\n", nb);
        for (int k = 0; k < 6; ++k) {
            std::vector<double> a, d;
            for (int b = 0; b < nb; ++b) {
                if (!tr[(size_t)b * 8 + slot[k]]) continue;          // phase not reached (no bias gradient requested)
                a.push_back((double)(tr[(size_t)b * 8 + slot[k]] - t00) * 0.01);
                if (k) d.push_back((double)(tr[(size_t)b * 8 + slot[k]] - tr[(size_t)b * 8 + slot[k - 1]]) * 0.01);
            }
            if (a.empty()) continue;
            std::sort(a.begin(), a.end()); std::sort(d.begin(), d.end());
            printf("    %-18s %7.2f %7.2f %7.2f   %7.2f\n", nm[k], a.front(), a[a.size() / 2], a.back(), k ? d[d.size() / 2] : 0.0);
        }
    }
    return 0;
}
