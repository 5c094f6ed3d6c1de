// 256 x 128 bf16 GEMM tile run by EIGHT waves as two staggered four-wave groups ("ping-pong").
//
// Same math and the same callers as gemm.hip (the Linear layers of the encoder and the weight gradients of loss.backward()); what
// differs is who is on the matrix pipe when.
//
// Why: two co-resident 128 x 128 blocks per CU need the CU's whole 64 B/clk L2 -> LDS fill path at full MFMA rate and sit at ~50 %
// of it.  One 256 x 128 tile moves 25 % fewer operand bytes per FLOP -- but eight waves that issue DMA, read LDS and
// run MFMA in lockstep leave every SIMD's matrix pipe idle while both of its waves read fragments (the round-2 kernel that lost).
// Here a k-stage is two phases per wave, and the workgroup's two halves run them in opposite order:
//
//   LOAD(t): all fragment reads of k-stage t (64 registers: the wave's 64 x 64 quarter of its group's 128 x 128 half, two 32-deep
//            slabs) and NOTHING else; nothing for the matrix pipe
//   COMP(t): 32 MFMAs out of registers, with this wave's 6 DMA pieces of a later stage and the next LOAD's addresses between them
//
// A SIMD hosts wave w (group 0) and wave w+4 (group 1): while one of them feeds the matrix pipe the other feeds the LDS / DMA
// queues -- the complementary pairing MI355X_MICROARCH.md "Two waves per SIMD" item 5 asks for.  The two groups share the B image
// (128 columns) and the barrier; group 0 owns tile rows 0-127, group 1 rows 128-255.  gemm_pn_kernel / gemm_pt_kernel are the same
// loop on a 128 x 64 tile with 128 k per stage and on a 256 x 64 tile with 64 k per stage.
//
// The schedule.  B(0) is the barrier behind the prologue, B(t+1) the ONE barrier of k-stage t; "interval t" is what runs between
// B(t) and B(t+1).  Group 0 meets B(t+1) behind its COMP(t), group 1 behind its LOAD(t), so group 1 runs one phase behind:
//
//     interval   t                              t+1
//     group 0    LOAD(t)    COMP(t)   | B(t+1)  LOAD(t+1)  COMP(t+1) | B(t+2)
//     group 1    COMP(t-1)  LOAD(t)   | B(t+1)  COMP(t)    LOAD(t+1) | B(t+2)
//
// Ring: three slots of one stage each (48 KB; 40 KB in the tall form); stage t lives in slot t % 3.  A wave requests its six pieces
// of a whole stage inside one COMP, never anywhere else in the loop:
//   group 0 in COMP(t) = interval t     : stage t+2 -> slot (t+2) % 3, where stage t-1 lived
//   group 1 in COMP(t) = interval t+1   : stage t+3 -> slot  t    % 3, where stage t   lived
// (the prologue requests stages 0 and 1 for both groups and stage 2 for group 1; the tail, where no stage is left to request, is
//  described at the loop).
//   WAR  Every read of stage s is issued in LOAD(s) -- interval s for both groups -- and has returned (lds_wait_all at the end of
//        LOAD) before its wave arrives at B(s+1).  Group 0 overwrites stage t-1 in interval t, behind B(t); group 1 overwrites stage t
//        in interval t+1, behind B(t+1).
//   RAW  Stage t+1 is first read in interval t+1, behind B(t+1).  Its pieces were requested in interval t-1 (group 0: COMP(t-1),
//        group 1: COMP(t-2)), and each wave counts its own out -- s_waitcnt vmcnt(pieces per stage): only the stage it requested
//        last, t+2, may still be in flight -- before it arrives at B(t+1): group 0 at the end of COMP(t), group 1 at the end of LOAD(t).
//        A piece has had at least two phases to land by then.
// Both groups run BOTH waits, so the loop has no branch on the group around them: group 0's wait behind LOAD(t) is free (nothing
// younger than stage t+1 is in flight), group 1's behind COMP(t) asks for stage t+2 an interval before it is needed.
//
// The gathered form (GATHER, gemm_pp_grouped_tn_gather_kernel: a weight gradient summed over listed k rows only).  Stage t holds the k
// rows list[t * 64 .. + 64); a wave's six pieces of a stage hold eight consecutive entries, fetched by ONE scalar load (lgkmcnt) -- never
// by a vector load, which the vmcnt counting above would miscount.  Per wave: COMP that requests stage r also forms, behind its last piece,
// the lane offsets of stage r + 1 out of entries the COMP before fetched, and fetches, at its top, the entries of stage r + 2.
//   RAW  (entries) fetched at the top of one COMP, first read in the next one: the wave's own LOAD lies between them and ends on
//        lds_wait_all = lgkmcnt(0); the compiler, which sees the load, puts its own lgkmcnt wait in front of the take-over behind the last
//        MFMA, where no LDS read is in flight.  (offsets) written behind the last piece of COMP, read by the pieces of the next COMP: in
//        order in one wave.
//   WAR  (offsets) a piece reads its offset register when it issues, and the wave issues in order: the forming behind it cannot overtake.
//        (entries) the registers a fetch writes are free: their last reader, the forming of the COMP before, has issued.
// LOAD holds what it held; the ring, the barriers and both vmcnt waits are those of the dense loop, whose instantiations do not change.
// The stage count comes from device memory, so the loop forms offsets up to two stages past its end: the fetch clamps to the last stage.
//
// MB_PP_ONE_BARRIER=0 builds the form the kernel was first written in (scripts/build_variant.py; the A/B oracle of the hazard argument
// above): a second barrier per stage, met by group 0 behind LOAD and by group 1 behind COMP, so that all eight waves change phase
// together -- the same per-wave instruction order, DMA schedule and waits.  That pair only forces the alternation, which B(t+1)
// restores every stage anyway (group 0 leaves it into a LOAD, group 1 into a COMP), and an eight-wave barrier costs ~200 clocks of
// a ~750-clock phase (profiles/r06_pn_looptrace.txt).
#include "gemm_tile.h"
#include "adamw_dev.h"

#ifndef MB_RIDE_UNR
#define MB_RIDE_UNR 3          // quads in flight per thread and pipeline stage of a rider workgroup (A/B builds: -DMB_RIDE_UNR=4|5|6)
#endif

namespace mb {

constexpr int kPpBM = 256, kPpBN = 128, kPpKB = 128, kPpSlots = 3, kPpWaves = 8;
constexpr int kPpStage = (kPpBM + kPpBN) * kPpKB;       // 48 KB
// The narrow form for the N = 768 launches (T = 2400: 228 tiles, one per CU, where 256 x 128 would make 60): 128 x 64 outputs, 128 k
// per stage (256-byte k rows) -- the SAME 48-KB stage, the same six DMA pieces per wave; a wave owns 32 x 32 outputs and four
// 32-deep slabs: 16 MFMAs and 16 (row image) / 24-32 (k-major) fragment reads per stage.  25 % fewer operand bytes per FLOP than
// the 64 x 64 tiles those launches run otherwise (they are bound by the L2 -> LDS fill).
constexpr int kPnBM = 128, kPnBN = 64, kPnKB = 256;
// The tall form for the same launches at T = 4096 (MOSEI shape: 128 x 64 would make 384 tiles = one and a half rounds): 256 x 64 outputs,
// 64 k per stage -- 40-KB stages, five DMA pieces per wave; a wave owns 64 x 32 outputs and two slabs (16 MFMAs, 12 / 16 reads per
// stage).  16 x 12 = 192 tiles at T = 4096: one round, and 64 CUs left to the riders.
constexpr int kPtBM = 256, kPtBN = 64, kPtKB = 128;
static_assert((kPnBM + kPnBN) * kPnKB == kPpStage, "both forms share the ring geometry");

#ifdef MB_GEMM_LOOPTRACE
// wave 0 (group 0) and wave 4 (group 1) stamp kPpIters k-stages from stage kPpFirst on, kPpPoints shader-clock stamps each:
// 0 top of LOAD | 1 reads issued | 2 reads returned (+ group 1: stage t+1 landed) | 3 barrier passed | 4 MFMAs + DMA issued |
// 5 group 0: stage t+1 landed  (the next stage's point 0 closes the second barrier)
constexpr int kPpFirst = 4, kPpIters = 10, kPpPoints = 6;
#endif

// dst = s + v as a pinned statement (stays between the MFMAs it is written between)
__device__ __forceinline__ void pinned_add(uint32_t& dst, uint32_t s, uint32_t v) { asm volatile("v_add_u32 %0, %1, %2" : "=v"(dst) : "s"(s), "v"(v)); }

typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

// GATHER (both operands k-major, the 256 x 128 tile): stage t holds the k rows rows[t * 64 .. + 64) instead of t * 64 .. + 64, `gstages`
// stages in all (the caller read the count: wave-uniform).
template <int BM, int BN, int KB, bool AK, bool BK, int MODE, bool GATHER = false>
__device__ __forceinline__ void gemm_pp_body(const GemmArgs& p, const int m0, const int n0, char* smem,
                                             const uint32_t* __restrict__ rows = nullptr, const int gstages = 0) {
    typedef bf16 T;
    constexpr int NW = kPpWaves, STAGE = (BM + BN) * KB;
    constexpr int BKE = KB / 2;                    // 64 (128) k per stage
    // a wave: 64 x 64 (32 x 32) outputs, two (four) 32-deep slabs per stage
    constexpr int MT = BM / 64, NT = BN / 32, NSLAB = BKE / 32;
    typedef Dma<T, BM, AK, KB, NW> DA;
    typedef Dma<T, BN, BK, KB, NW> DB;
    constexpr int G = DA::NI + DB::NI;             // DMA pieces per wave per stage (4 + 2)
    typedef typename DA::template Reader<MT, NSLAB> RA;
    typedef typename DB::template Reader<NT, NSLAB> RB_;
    constexpr int NRA = MT * RA::READS_PER_FRAG, NRB = NT * RB_::READS_PER_FRAG;
    constexpr int NM = MT * NT * NSLAB;            // MFMAs per stage (32 | 16)
    constexpr bool SPREAD = NM < 32;               // DMA pieces at even distances over the MFMAs of COMP (else: behind the first MFMAs)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                     // waves w and w + 4 share a SIMD (MI355X_MICROARCH.md, LDS: dispatch order 0 -> 2 -> 1 -> 3)
    const int wr = wave >> 1, wc = wave & 1;       // 4 x 2 waves; wr 0-1 = group 0
    int nt_;
    if constexpr (GATHER) nt_ = gstages; else nt_ = p.K / BKE;
    const int nt = nt_;                            // >= 3 (launcher)
    const T* __restrict__ A = (const T*)p.A;
    const T* __restrict__ B = (const T*)p.B;
    // segmented B (GemmArgs::bseg), as in gemm2_body
    int n0b = n0, seg_stages = 0;
    uint32_t seg_extra = 0;
    if (p.bseg > 0) {
        if constexpr (BK) { B += (size_t)(n0 / p.bseg) * p.bseg_stride; n0b = n0 % p.bseg; }
        else { seg_stages = p.bseg / BKE; seg_extra = (uint32_t)((p.bseg_stride - (size_t)p.bseg) * sizeof(T)); }
    }
    int seg_left = seg_stages;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (the narrow tile has four accumulator tiles per wave: slab after slab into the same four, an MFMA meets its predecessor on that
    //  tile four issues later -- which is not what its COMP waits for: profiles/r06_pn_nacc.txt)

    auto stamp = [&](int k) {
        if (p.trace && tid == 0) p.trace[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kTraceStride + k] = wall_clock64();
    };
#ifdef MB_GEMM_LOOPTRACE
    __shared__ uint32_t lt[2][kPpIters * kPpPoints];
#define PP_LT(t, j) do { if (p.trace && (t) >= kPpFirst && (t) < kPpFirst + kPpIters && (tid & 255) == 0) \
                             lt[grp][((t) - kPpFirst) * kPpPoints + (j)] = (uint32_t)__builtin_readcyclecounter(); } while (0)
#else
#define PP_LT(t, j) do { } while (0)
#endif
    stamp(0);
    EpiPre<T, BM, BN, MODE, NW> pre;
    pre.fetch(p, m0, n0, tid);                     // the oldest loads in flight: counted out by the first vmcnt wait

    RA ra;
    RB_ rb;
    const uint32_t lds0 = (uint32_t)(size_t)LDS_PTR(smem);
    ra.init(lds0, wr * (BM / 4), 0, lane);
    rb.init(lds0 + BM * KB, wc * (BN / 2), 0, lane);
    // A wave's pieces of a stage are CONSECUTIVE 1-KB pieces of the image (wave * NI + i): one m0 per operand and stage, piece i is
    // the instruction's immediate offset i * 1024 -- which the hardware adds to the LDS address AND to the memory address, so the
    // lane offsets are taken back by i * 1024 and the descriptors' bases by kBias to keep them non-negative.
    constexpr uint32_t kBias = 4096;
    uint32_t va[DA::NI], vb[DB::NI];
#pragma unroll
    for (int i = 0; i < DA::NI; ++i) va[i] = DA::dma_voff_blk(wave * DA::NI + i, p.lda, m0, p.M, lane) + kBias - (uint32_t)i * 1024u;
#pragma unroll
    for (int i = 0; i < DB::NI; ++i) vb[i] = DB::dma_voff_blk(wave * DB::NI + i, p.ldb, n0b, p.N, lane) + kBias - (uint32_t)i * 1024u;
    const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)A - kBias), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)B - kBias), 0, -1, 0x00020000);
    const uint32_t ksa = DA::k_stride_bytes(p.lda) * BKE, ksb = DB::k_stride_bytes(p.ldb) * BKE;      // operand bytes per stage
    // GATHER: a wave's pieces of a stage hold the EIGHT k rows wave * 8 .. + 8 of both images (A: 4 pieces x 2 rows, B: 2 pieces x 4
    // rows), i.e. eight consecutive list entries: ONE scalar load per stage (lgkmcnt, not the vmcnt the DMA pieces are counted out with).
    // A lane's offset of a piece is (its row's list entry) * ld * 2 + ca | cb (the column part: dma_voff_blk at ld = 0, which also holds
    // the swizzle -- a function of the stage-local k only); the entry is selected per lane out of the 2 | 4 scalars of the piece with
    // lane masks (bitwise select), and the scalar stage offsets soa / sob stay 0.
    [[maybe_unused]] uint32_t ca[DA::NI], cb[DB::NI], fa32 = 0, fb16 = 0, fb32 = 0, fb48 = 0;
    [[maybe_unused]] u32x8 gidx = {}, gnext = {};  // the list entries of the stage whose offsets are formed next; of the one behind it (in flight)
    [[maybe_unused]] int grq = 0;                  // ... and that stage
    [[maybe_unused]] const uint32_t lda2 = (uint32_t)p.lda * 2u, ldb2 = (uint32_t)p.ldb * 2u;
    if constexpr (GATHER) {
        static_assert(AK && BK && DA::NI == 4 && DB::NI == 2 && DA::RB == 512 && DB::RB == 256 && BKE == 64 && NW == 8,
                      "the gathered loop is written for the 256 x 128 k-major tile");
#pragma unroll
        for (int i = 0; i < DA::NI; ++i) ca[i] = DA::dma_voff_blk(wave * DA::NI + i, 0, m0, p.M, lane) + kBias - (uint32_t)i * 1024u;
#pragma unroll
        for (int i = 0; i < DB::NI; ++i) cb[i] = DB::dma_voff_blk(wave * DB::NI + i, 0, n0b, p.N, lane) + kBias - (uint32_t)i * 1024u;
        fa32 = (lane & 32) ? 0xffffffffu : 0u;                       // A piece: lanes 32-63 hold its second row
        fb16 = (lane & 16) ? 0xffffffffu : 0u;                       // B piece: row (lane >> 4) & 3
        fb32 = (lane & 32) ? 0xffffffffu : 0u;
        fb48 = fb16 & fb32;
    }
    // the eight entries of stage s (clamped: the loop forms offsets up to two stages past the last one, which nobody uses)
    auto gather_fetch = [&](int s) {
        if constexpr (GATHER) {
            const int sc = s < nt ? s : nt - 1;
            uintptr_t a = (uintptr_t)(rows + ((size_t)sc * BKE + (size_t)wave * 8));
            asm volatile("" : "+s"(a));             // (the load stays behind the pinned statements in front of it)
            gnext = *(const __attribute__((address_space(4))) u32x8*)a;
        }
    };
    // piece I's lane offsets (A pieces first) out of gidx, as pinned statements
    auto gather_form = [&](auto ic) {
        if constexpr (GATHER) {
            constexpr int I = decltype(ic)::value;
            // (named here: operands that appear in asm statements only are not captured by a generic lambda)
            const uint32_t ma = fa32, m16 = fb16, m32 = fb32, m48 = fb48, la = lda2, lb = ldb2;
            uint32_t t;
            if constexpr (I < DA::NI) {
                const uint32_t s0 = gidx[2 * I], x = s0 ^ gidx[2 * I + 1];
                asm volatile("v_and_b32 %0, %1, %2" : "=v"(t) : "s"(x), "v"(ma));
                asm volatile("v_xor_b32 %0, %1, %0" : "+v"(t) : "s"(s0));
                asm volatile("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(va[I]) : "v"(t), "s"(la), "v"(ca[I]));
            } else {
                constexpr int J = I - DA::NI;
                const uint32_t s0 = gidx[4 * J], x1 = s0 ^ gidx[4 * J + 1], x2 = s0 ^ gidx[4 * J + 2], x3 = x1 ^ gidx[4 * J + 2] ^ gidx[4 * J + 3];
                uint32_t u;
                asm volatile("v_and_b32 %0, %1, %2" : "=v"(t) : "s"(x1), "v"(m16));
                asm volatile("v_and_b32 %0, %1, %2" : "=v"(u) : "s"(x2), "v"(m32));
                asm volatile("v_xor_b32 %0, %0, %1" : "+v"(t) : "v"(u));
                asm volatile("v_and_b32 %0, %1, %2" : "=v"(u) : "s"(x3), "v"(m48));
                asm volatile("v_xor_b32 %0, %0, %1" : "+v"(t) : "v"(u));
                asm volatile("v_xor_b32 %0, %1, %0" : "+v"(t) : "s"(s0));
                const uint32_t c = cb[J];
                uint32_t& dst = vb[J];
                asm volatile("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(dst) : "v"(t), "s"(lb), "v"(c));
            }
        }
    };
    // the offsets of stage grq out of gidx, then the entries of the stage behind it (prologue form: no MFMAs to sit between)
    auto gather_next = [&]() {
        if constexpr (GATHER) {
            static_for<G>([&](auto ic) { gather_form(ic); });
            gather_fetch(++grq);
            gidx = gnext;
        }
    };
    // (The narrow tile's COMP takes ~440 clocks for 272 of MFMA whatever sits next to them -- six pieces or three, spread or not, one
    //  accumulator chain or four, 16 partner reads or 8: profiles/r06_pn_looptrace.txt, r06_pn_nacc.txt, r06_pn_ksw.txt,
    //  r06_pp_split_dma.txt)
#ifndef MB_PP_ONE_BARRIER
#define MB_PP_ONE_BARRIER 1
#endif
    constexpr bool ONEB = MB_PP_ONE_BARRIER != 0;   // one barrier per k-stage (the file header)
    uint32_t soa = 0, sob = 0;                      // scalar byte offsets of the next stage to request, in k order
#ifdef MB_GEMM_ABLATE
    const bool no_dma = (p.dbg & 1) != 0, no_reads = (p.dbg & 4) != 0, no_mfma = (p.dbg & 2) != 0;
#else
    constexpr bool no_dma = false, no_reads = false, no_mfma = false;
#endif
    // piece I (A pieces first) of this wave's share of the next stage in k order -> ring slot at byte offset `slot`
    auto dma_piece = [&](auto ic, uint32_t slot) {
        constexpr int I = decltype(ic)::value;
        if (no_dma) return;
        // (the immediate must be a literal: a template-dependent argument of the builtin fails the host pass)
#define MB_PP_PIECE(RS, PTR, VOFF, SOFF, J) do { \
            if constexpr ((J) == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, PTR, 16, VOFF, SOFF, 0, 0); \
            else if constexpr ((J) == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, PTR, 16, VOFF, SOFF, 1024, 0); \
            else if constexpr ((J) == 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, PTR, 16, VOFF, SOFF, 2048, 0); \
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, PTR, 16, VOFF, SOFF, 3072, 0); } while (0)
        static_assert(DA::NI <= 4 && DB::NI <= 4, "immediate offsets reach 4095");
        if constexpr (I < DA::NI)
            MB_PP_PIECE(rsa, (__attribute__((address_space(3))) void*)LDS_PTR(smem + slot + wave * (DA::NI * 1024)), (int)va[I], (int)soa, I);
        else
            MB_PP_PIECE(rsb, (__attribute__((address_space(3))) void*)LDS_PTR(smem + slot + BM * KB + wave * (DB::NI * 1024)), (int)vb[I - DA::NI], (int)sob, I - DA::NI);
#undef MB_PP_PIECE
    };
    auto dma_advance = [&]() {
        if constexpr (GATHER) return;               // (the offsets of the next stage are formed in COMP, or by gather_next)
        soa += ksa; sob += ksb;
        if (seg_stages > 0 && --seg_left == 0) { sob += seg_extra; seg_left = seg_stages; }
    };
    auto issue_stage = [&](uint32_t slot) {          // this wave's G pieces of the next stage, back to back (prologue and tail)
        static_for<G>([&](auto ic) { dma_piece(ic, slot); });
        dma_advance();
    };
    // An instruction of the wave that is NOT on the matrix pipe costs a whole MFMA time (~16 clocks) while its SIMD partner issues
    // MFMAs back to back, and ~4 clocks inside the MFMA stream itself (tools/mfma_lds_probe, profiles/r06_mfma_lds_probe.txt): so LOAD
    // holds the fragment reads and nothing else -- their addresses are computed in the COMP phase before (addr_*), the DMA pieces
    // ride between the MFMAs.
    uint32_t addr_a[RA::NB], addr_b[RB_::NB];
#pragma unroll
    for (int j = 0; j < RA::NB; ++j) addr_a[j] = ra.base[j];
#pragma unroll
    for (int j = 0; j < RB_::NB; ++j) addr_b[j] = rb.base[j];
    FragU fa[NSLAB][MT], fb[NSLAB][NT];
    auto read_stage = [&]() {                      // every fragment of the stage addr_* points at, slab by slab
        if (no_reads) return;
        static_for<NSLAB>([&](auto sc) {
            constexpr int S = decltype(sc)::value;
            static_for<NRB>([&](auto rc) { rb.template emit_at<decltype(rc)::value, S>(fb[S], addr_b); });
            static_for<NRA>([&](auto rc) { ra.template emit_at<decltype(rc)::value, S>(fa[S], addr_a); });
        });
    };
    // COMP: the stage's MFMAs with (DMA ? this wave's pieces of its next stage : nothing) and the next stage's read addresses between them
    constexpr int NADDR = RA::NB + RB_::NB;
    auto comp_stage_ = [&](auto dmac, auto mfc, uint32_t slot, uint32_t nxt) {
        constexpr bool DMA = decltype(dmac)::value, MF = decltype(mfc)::value;
        constexpr int NF = (DMA ? G : 0) + NADDR;
        auto addr_add = [&](auto jc) {
            constexpr int J = decltype(jc)::value;
            if constexpr (J < RA::NB) pinned_add(addr_a[J], nxt, ra.base[J]);
            else pinned_add(addr_b[J - RA::NB], nxt, rb.base[J - RA::NB]);
        };
        static_for<NM>([&](auto mc) {
            constexpr int M = decltype(mc)::value, S = M / (MT * NT), Q = M % (MT * NT);
            if constexpr (MF) mma16_pinned(acc[Q / NT][Q % NT], fb[S][Q % NT].v, fa[S][Q / NT].v);
            if constexpr (SPREAD) {
                // the narrow tile has 16 MFMAs for the same six pieces: one behind (almost) every MFMA, each piece held the wave's issue for
                // ~30 clocks (COMP 464 clocks for 272 of MFMA, profiles/r06_pn_looptrace.txt) -- a piece every ~2.7 MFMAs is what the
                // 256 x 128 form has and pays nothing for
                constexpr int d0 = DMA ? (M * G + NM - 1) / NM : 0, d1 = DMA ? ((M + 1) * G + NM - 1) / NM : 0;
                static_for<d1 - d0>([&](auto fc) { dma_piece(std::integral_constant<int, d0 + decltype(fc)::value>{}, slot); });
                constexpr int a0 = M * NADDR / NM, a1 = (M + 1) * NADDR / NM;
                static_for<a1 - a0>([&](auto fc) { addr_add(std::integral_constant<int, a0 + decltype(fc)::value>{}); });
            } else {
                constexpr int f0 = M * NF / NM, f1 = (M + 1) * NF / NM;
                static_for<f1 - f0>([&](auto fc) {
                    constexpr int F = f0 + decltype(fc)::value;
                    if constexpr (DMA && F < G) dma_piece(std::integral_constant<int, F>{}, slot);
                    else addr_add(std::integral_constant<int, F - (DMA ? G : 0)>{});
                });
                if constexpr (GATHER && DMA) {
                    // the entries for the COMP after are fetched at the top (a scalar load: a whole COMP to land, counted out by the compiler's
                    // lgkmcnt wait where they are taken over, behind the last MFMA -- no LDS read is in flight in COMP); behind the last piece
                    // of this COMP (MFMA 13 of 32) the offsets of the stage the NEXT COMP requests, one piece every third MFMA, out of the
                    // entries the COMP before fetched
                    static_assert(NM == 32 && G == 6 && (13 * NF) / NM >= G - 1 && (14 * NF) / NM >= G, "the last piece rides behind MFMA 13");
                    if constexpr (M >= 14 && M < 14 + 3 * G && (M - 14) % 3 == 0) gather_form(std::integral_constant<int, (M - 14) / 3>{});
                    if constexpr (M == 0) gather_fetch(++grq);
                    if constexpr (M == NM - 1) gidx = gnext;
                }
            }
        });
        if constexpr (DMA) dma_advance();
    };
    auto comp_stage = [&](auto dmac, uint32_t slot, uint32_t nxt) {
#ifdef MB_GEMM_ABLATE
        if (no_mfma) { comp_stage_(dmac, std::false_type{}, slot, nxt); return; }
#endif
        comp_stage_(dmac, std::true_type{}, slot, nxt);
    };
    typedef std::integral_constant<int, 1> W1;       // wait until only the newest stage is in flight
    typedef std::integral_constant<int, 0> W0;       // drain
    typedef std::integral_constant<int, -1> WN;      // nothing to wait for
    auto land = [&](auto wc_) {
        constexpr int W = decltype(wc_)::value;
        if constexpr (W == 1) wait_vmcnt<G>();
        else if constexpr (W == 0) wait_vmcnt<0>();
    };

    // Prologue: stages 0 and 1 for everybody; group 1, whose first COMP comes an interval late, also requests stage 2 here (group 0
    // requests it in COMP(0)).  Then stage 0 is counted out: everything but the one (group 1: two) stages requested behind it.
    if constexpr (GATHER) { gather_fetch(0); gidx = gnext; gather_next(); }      // offsets of stage 0, entries of stage 1
    issue_stage(0u);
    if constexpr (GATHER) gather_next();
    issue_stage((uint32_t)STAGE);
    if constexpr (GATHER) gather_next();             // the loop is entered with the offsets of the stage the first COMP requests (group 0:
    if (grp) {                                       // 2, group 1: 3) and the entries of the one behind it
        issue_stage(2u * STAGE);
        if constexpr (GATHER) gather_next();
        wait_vmcnt<2 * G>();
    } else wait_vmcnt<G>();
    __builtin_amdgcn_s_barrier();                    // B(0): stage 0 has landed for everybody
    stamp(1);
    if (!ONEB && grp) __builtin_amdgcn_s_barrier();  // (two-barrier form) group 1 runs one phase behind
    // cur: the slot LOAD(t) reads, t % 3.  dslot: the slot this wave's next request goes to -- group 0: (t+2) % 3, group 1: (t+3) % 3.
    uint32_t cur = 0u, dslot = grp ? 0u : 2u * STAGE;
    // One k-stage of one wave: LOAD(t), COMP(t), and the barrier between them (group 1) or behind them (group 0).
    // DM: who requests a stage in this COMP -- 1 = every wave, between the MFMAs (the loop) | 2 = group 0 only, in front of the MFMAs (stage
    //     nt-3: group 0 requests the last stage, nt-1; group 1 did in its COMP(nt-4), or in the prologue) | 0 = nobody (nothing is left)
    // wc_: what `land` waits for -- W1 = all but the stage requested last | W0 = everything (stage nt-2: the last stage lands) | WN = nothing
    auto stage = [&](int t, auto dm, auto wc_) {
        constexpr int DM = decltype(dm)::value;
        (void)t;
        // ---- LOAD(t): the reads of slot `cur`, returned before the wave goes on (WAR: its next barrier frees the slot)
        PP_LT(t, 0);
        read_stage();
        PP_LT(t, 1);
        lds_wait_all();
        land(wc_);                                   // RAW, group 1: its share of stage t+1 has landed (group 0: nothing younger than stage t+1 yet)
        PP_LT(t, 2);
        __builtin_amdgcn_sched_barrier(0);           // the scalar bookkeeping of COMP stays behind the barrier (in LOAD it would cost ~16 clocks each)
        if (!ONEB || grp) __builtin_amdgcn_s_barrier();      // group 1: B(t+1)
        __builtin_amdgcn_sched_barrier(0);
        PP_LT(t, 3);
        // ---- COMP(t): the MFMAs, with the request of stage t+2 (group 0) / t+3 (group 1) into `dslot` between them
        const uint32_t nxt = cur == 2u * STAGE ? 0u : cur + STAGE;
        if constexpr (DM == 2) { if (!grp) issue_stage(dslot); }
        // the multiplying wave outranks its SIMD partner's reads: by age alone the older wave (group 0) wins BOTH ways and group 1's
        // 32 MFMAs take ~930 clocks instead of ~510 (profiles/r06_pp_looptrace.txt)
        if (!(p.dbg & 16)) __builtin_amdgcn_s_setprio(1);
        comp_stage(std::integral_constant<bool, DM == 1>{}, dslot, nxt);
        if (!(p.dbg & 16)) __builtin_amdgcn_s_setprio(0);
        PP_LT(t, 4);
        land(wc_);                                   // RAW, group 0: its share of stage t+1 has landed (group 1: of stage t+2, an interval early)
        PP_LT(t, 5);
        if (!ONEB || !grp) __builtin_amdgcn_s_barrier();     // group 0: B(t+1)
        cur = nxt;
        dslot = dslot == 2u * STAGE ? 0u : dslot + STAGE;
    };
    typedef std::integral_constant<int, 0> D0;
    typedef std::integral_constant<int, 1> D1;
    typedef std::integral_constant<int, 2> D2;
    int t = 0;
    for (; t + 3 < nt; ++t) stage(t, D1{}, W1{});
    stage(t, D2{}, W1{});
    stage(t + 1, D0{}, W0{});
    stage(t + 2, D0{}, WN{});
    if (!ONEB && !grp) __builtin_amdgcn_s_barrier(); // (two-barrier form) pairs with group 1's last COMP
    stamp(2);
    gemm_epilogue<T, BM, BN, MODE, false, NW>(p, acc, m0, n0, wave, lane, smem, pre);
    if (p.trace) {
        stamp(3);
        wait_vmcnt<0>();
        stamp(4);
#ifdef MB_GEMM_LOOPTRACE
        if ((tid & 255) == 0) {
            unsigned long long* dst = p.trace + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kTraceStride + 8 + grp * kPpIters * kPpPoints;
            for (int i = 0; i < kPpIters * kPpPoints; ++i) dst[i] = lt[grp][i];
        }
#endif
    }
#undef PP_LT
}

template <bool AK, bool BK, int MODE>
__global__ void __launch_bounds__(512) gemm_pp_kernel(const GemmArgs p) {
    __shared__ __attribute__((aligned(1024))) char smem[kPpSlots * kPpStage];
    int m0, n0;
    if (!tile_origin<kPpBM, kPpBN>(p, m0, n0, blockIdx.x)) return;
    gemm_pp_body<kPpBM, kPpBN, kPpKB, AK, BK, MODE>(p, m0, n0, smem);
}

template <bool AK, bool BK, int MODE>
__global__ void __launch_bounds__(512) gemm_pn_kernel(const GemmArgs p) {
    __shared__ __attribute__((aligned(1024))) char smem[kPpSlots * kPpStage];
    int m0, n0;
    if (!tile_origin<kPnBM, kPnBN>(p, m0, n0, blockIdx.x)) return;
    gemm_pp_body<kPnBM, kPnBN, kPnKB, AK, BK, MODE>(p, m0, n0, smem);
}

// a narrow dgrad launch (dX = dY W + R) with riders: 228 tiles at T = 2400 leave whole CUs idle (16 once the grid's padding is counted
// per XCD); the riders come FIRST in the grid (multiples of 8: the tiles keep their XCDs) and each takes a CU to itself
__global__ void __launch_bounds__(512) gemm_pn_ride_kernel(const GemmArgs p, const AdamRide ride) {
    __shared__ __attribute__((aligned(1024))) char smem[kPpSlots * kPpStage];
    if ((int)blockIdx.x < ride.blocks) {
        adam_ride_block<512, MB_RIDE_UNR>(ride, (int)blockIdx.x);
        return;
    }
    int m0, n0;
    if (!tile_origin<kPnBM, kPnBN>(p, m0, n0, (int)blockIdx.x - ride.blocks)) return;
    gemm_pp_body<kPnBM, kPnBN, kPnKB, false, true, EPI_ADD_RES>(p, m0, n0, smem);
}

template <bool AK, bool BK, int MODE>
__global__ void __launch_bounds__(512) gemm_pt_kernel(const GemmArgs p) {
    __shared__ __attribute__((aligned(1024))) char smem[kPpSlots * (kPtBM + kPtBN) * kPtKB];
    int m0, n0;
    if (!tile_origin<kPtBM, kPtBN>(p, m0, n0, blockIdx.x)) return;
    gemm_pp_body<kPtBM, kPtBN, kPtKB, AK, BK, MODE>(p, m0, n0, smem);
}
__global__ void __launch_bounds__(512) gemm_pt_ride_kernel(const GemmArgs p, const AdamRide ride) {
    __shared__ __attribute__((aligned(1024))) char smem[kPpSlots * (kPtBM + kPtBN) * kPtKB];
    if ((int)blockIdx.x < ride.blocks) {
        adam_ride_block<512, MB_RIDE_UNR>(ride, (int)blockIdx.x);
        return;
    }
    int m0, n0;
    if (!tile_origin<kPtBM, kPtBN>(p, m0, n0, (int)blockIdx.x - ride.blocks)) return;
    gemm_pp_body<kPtBM, kPtBN, kPtKB, false, true, EPI_ADD_RES>(p, m0, n0, smem);
}

// the weight gradients of a layer (dW = dY^T X: both operands k-major), one launch (gemm.hip: launch_grouped places the tiles)
__global__ void __launch_bounds__(512) gemm_pp_grouped_tn_kernel(const GroupedGemmArgs ga) {
    __shared__ __attribute__((aligned(1024))) char smem[kPpSlots * kPpStage];
    if ((int)blockIdx.x < ga.ride.blocks) {          // rider: an optimizer update on a CU that has no tile (kernels.h AdamRide)
        adam_ride_block<512, MB_RIDE_UNR>(ga.ride, (int)blockIdx.x);
        return;
    }
    int g, m0, n0;
    if (!grouped_tile_origin<kPpBM, kPpBN>(ga, g, m0, n0)) return;
    gemm_pp_body<kPpBM, kPpBN, kPpKB, true, true, EPI_ACCUM_F32>(ga.g[g], m0, n0, smem);
}

// ... summed over listed k rows only (GroupedGemmArgs::rows: the live token rows of the batch).  A problem without a list runs the dense
// loop; the stage count of a listed one is read here, once, from device memory -- grid and arguments do not depend on it.
__global__ void __launch_bounds__(512) gemm_pp_grouped_tn_gather_kernel(const GroupedGemmArgs ga) {
    __shared__ __attribute__((aligned(1024))) char smem[kPpSlots * kPpStage];
    if ((int)blockIdx.x < ga.ride.blocks) {
        adam_ride_block<512, MB_RIDE_UNR>(ga.ride, (int)blockIdx.x);
        return;
    }
    int g, m0, n0;
    if (!grouped_tile_origin<kPpBM, kPpBN>(ga, g, m0, n0)) return;
    const uint32_t* rows = ga.rows[g];
    if (rows == nullptr) {
        gemm_pp_body<kPpBM, kPpBN, kPpKB, true, true, EPI_ACCUM_F32>(ga.g[g], m0, n0, smem);
        return;
    }
    const uint32_t n = *(const __attribute__((address_space(4))) uint32_t*)(uintptr_t)ga.nrows[g];
    const int K = ga.g[g].K;
    int stages = (int)(n < (uint32_t)K ? n : (uint32_t)K) / 64;
    if (stages < 3) stages = 3;                      // (the ring's minimum; the launcher saw K >= 192, a list holds at least 192 entries)
    gemm_pp_body<kPpBM, kPpBN, kPpKB, true, true, EPI_ACCUM_F32, true>(ga.g[g], m0, n0, smem, rows, stages);
}

int gemm_pp_launch(bool ak, bool bk, int mode, const GemmArgs& p, dim3 grid, hipStream_t st) {
#define MB_PP(AKV, BKV, MODEV) \
    if (ak == AKV && bk == BKV && mode == MODEV) { \
        MB_GEMM_LAUNCH((gemm_pp_kernel<AKV, BKV, MODEV>), grid, dim3(512), st, p, &p, 1); \
        return (int)hipGetLastError(); \
    }
    MB_PP(false, false, EPI_BIAS)
    MB_PP(false, false, EPI_BIAS_GELU)
    MB_PP(false, false, EPI_BIAS_ACT)
    MB_PP(false, true, EPI_DGELU)
    MB_PP(true, true, EPI_ACCUM_F32)
#undef MB_PP
    return MB_ERR_MODE;
}

// the 128 x 64 form (bf16; K a multiple of 128, at least three stages): the N = 768 forward and dgrad launches
int gemm_pn_launch(bool ak, bool bk, int mode, const GemmArgs& p, dim3 grid, hipStream_t st, bool tall) {
#define MB_PN(AKV, BKV, MODEV) \
    if (ak == AKV && bk == BKV && mode == MODEV) { \
        if (tall) MB_GEMM_LAUNCH((gemm_pt_kernel<AKV, BKV, MODEV>), grid, dim3(512), st, p, &p, 1); \
        else MB_GEMM_LAUNCH((gemm_pn_kernel<AKV, BKV, MODEV>), grid, dim3(512), st, p, &p, 1); \
        return (int)hipGetLastError(); \
    }
    MB_PN(false, false, EPI_BIAS)
    MB_PN(false, false, EPI_BIAS_DROP_RES)
    MB_PN(false, false, EPI_ADD_RES)
    MB_PN(false, true, EPI_ADD_RES)
#undef MB_PN
    return MB_ERR_MODE;
}

int gemm_pn_ride_launch(const GemmArgs& p, const AdamRide& ride, dim3 grid, hipStream_t st, bool tall) {
    gemm_log_ride(ride);
    if (tall) {
        gemm_log((const void*)gemm_pt_ride_kernel, st, &p, 1);
        hipLaunchKernelGGL(gemm_pt_ride_kernel, dim3(grid.x + ride.blocks), dim3(512), 0, st, p, ride);
    } else {
        gemm_log((const void*)gemm_pn_ride_kernel, st, &p, 1);
        hipLaunchKernelGGL(gemm_pn_ride_kernel, dim3(grid.x + ride.blocks), dim3(512), 0, st, p, ride);
    }
    return (int)hipGetLastError();
}

int gemm_pp_grouped_launch(const GroupedGemmArgs& ga, int grid, hipStream_t st) {
    bool gather = false;
    for (int i = 0; i < ga.count; ++i) gather = gather || ga.rows[i] != nullptr;
    if (gather) {
        for (int i = 0; i < ga.count; ++i)
            if (ga.rows[i] && (!ga.nrows[i] || ((uintptr_t)ga.rows[i] % 32) || ((uintptr_t)ga.nrows[i] % 4))) return MB_ERR_ARG;
        gemm_log((const void*)gemm_pp_grouped_tn_gather_kernel, st, ga.g, ga.count, ga.note ? ga.note : "rows=listed");
        hipLaunchKernelGGL(gemm_pp_grouped_tn_gather_kernel, dim3(grid + ga.ride.blocks), dim3(512), 0, st, ga);
        gemm_log_ride(ga.ride);
        return (int)hipGetLastError();
    }
    MB_GEMM_LAUNCH(gemm_pp_grouped_tn_kernel, dim3(grid + ga.ride.blocks), dim3(512), st, ga, ga.g, ga.count);
    gemm_log_ride(ga.ride);
    return (int)hipGetLastError();
}

}  // namespace mb
