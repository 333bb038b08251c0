// fp32 MFMA GEMM for gfx950 with an optional fused LSTM-cell epilogue.
//
//   PLAIN:  C[M][N]  = A[M][K] . Bt[N][K]^T (+ bias)
//   LSTM:   z = [x | ctx | h][M][K] . Wt[4U][K]^T + b ; (h', c') = cell(z, c)     (U = units)
//
// The A operand is the concatenation of up to three row-gathered K-segments (layer input, attention
// context, recurrent state), so "x.K + h.R" of a Keras LSTMCell (seq2seq.py:272,337,344) is ONE
// contraction and the gate pre-activations never leave the accumulators.  Weight rows are stored
// gate-interleaved in blocks of 32 units ([unit/32][gate i,f,c,o][unit%32]) so that a 128-column block
// tile holds all four gates of 32 units and a wave's four 32x32 accumulator tiles hold, register for
// register, the i/f/c/o pre-activations of the same (row, unit).
//
// Tiling: 128x128 block tile, BK = 16, 256 threads = 4 waves, each wave 32 rows x 128 columns
// (4 x v_mfma_f32_32x32x2_f32 accumulators, exact fp32 = a k-ordered fmaf chain).  Operands are staged
// K-contiguous in LDS with a +4-float row pad (80-B rows: ds_read_b128 is conflict-free for its 16-lane
// groups) and double-buffered; each lane reads four consecutive k per ds_read_b128 and feeds them to
// four MFMAs (the k order inside a tile is permuted identically for A and B, which a sum allows).
// Small launches take the 32x128-tile variant of gemm_skinny.hip instead (gemm_plan.h; same values bit for bit).
#include "common.h"
#include <cstdlib>
#include <cstdio>

namespace casv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// Diagnostic build (-DCASV_GEMM_PROF): thread 0 of every workgroup of the 128x128 LSTM kernel adds its shader-clock cycles
// in prologue / steady-state loop / epilogue, the loop's tile count and its wall-clock ticks (10 ns) to g_gemm_prof;
// gemm_prof_dump() prints and clears them (engine.hip calls it after a beamed decode).
#ifdef CASV_GEMM_PROF
__device__ unsigned long long g_gemm_prof[16 + 64];
#define CASV_STAMP(x) { asm volatile("" ::: "memory"); x = __builtin_amdgcn_s_memtime(); asm volatile("" ::: "memory"); }
void gemm_prof_dump() {
    unsigned long long h[16 + 64];
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_gemm_prof), sizeof(h));
    if (h[5]) {
        fprintf(stderr, "gemm_prof workgroup cycles, histogram in bins of 16384:");
        for (int i = 0; i < 64; ++i) if (h[16 + i]) fprintf(stderr, " %d:%llu", i, h[16 + i]);
        fprintf(stderr, "\n");
    }
    if (h[5]) fprintf(stderr, "gemm_prof prologue parts: setup %.0f, cell-state addresses %.0f, tiles 0/1 requested %.0f, landed+stored+tiles 2/3 requested+frags %.0f | tail tiles %.0f, epilogue %.0f cyc\n",
                      (double)h[8] / h[5], (double)h[9] / h[5], (double)h[10] / h[5], (double)h[11] / h[5], (double)h[12] / h[5], (double)h[13] / h[5]);
    if (h[5])
        fprintf(stderr, "gemm_prof: %llu workgroups: prologue %.0f cyc, loop %.1f cyc/tile over %.1f tiles, tail+epilogue %.0f cyc, "
                "whole workgroup %.0f cyc, loop clock %.3f GHz\n", h[5], (double)h[0] / h[5], (double)h[1] / (double)h[2], (double)h[2] / h[5],
                (double)h[3] / h[5], (double)h[6] / h[5], (double)h[1] / (double)h[4] * 0.1);
    unsigned long long z[16 + 64] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_prof), z, sizeof(z));
}
#endif

#ifndef CASV_PLAIN_WIDE
#define CASV_PLAIN_WIDE 1           // the PLAIN kernel's full-tile epilogue stores 16 bytes per lane through an in-quad transpose (0: A/B builds)
#endif

constexpr int BM = 128, BN = 128, BK = 16, LDW = BK + 4;   // 80-B LDS rows: ds_read_b128 conflict-free
constexpr int TILE_FLOATS = 128 * LDW;               // one operand tile
constexpr int GEMM_LDS_BYTES = 2 * 2 * TILE_FLOATS * 4;
constexpr int CELL_LDS_BYTES = 128 * 128;            // LSTM epilogue: the tile's previous cell state, [half][row][16 floats]
constexpr int STASH_LDS_BYTES = 256 * 6 * 8;         // per thread: row pointers that wait for their turn outside the register file
// SPLIT variant (option split_bf16, an experiment -- see the comment in front of gemm_tile): an operand tile lies in LDS as three
// bf16 planes of 128 rows x 16 k (32-byte rows, the two 16-byte halves of a row swapped where bit 4 of the row is set: conflict-free
// for ds_read_b128's 16-lane groups without padding)
constexpr int SPLIT_PLANE_BYTES = 128 * 32;
constexpr int SPLIT_BUF_FLOATS = 6 * SPLIT_PLANE_BYTES / 4;     // A planes 0..2, B planes 0..2

// Software pipeline (per wave, so that ONE wave keeps its SIMD's matrix pipe busy and the two waves
// of a SIMD do not have to be out of phase to cover each other):
//   while the 32 MFMAs of tile kt run from fragment registers F[kt&1],
//     F[(kt+1)&1] <- LDS[(kt+1)&1]   (10 ds_read_b128; that buffer was filled during kt-1)
//     LDS[kt&1]   <- G               (tile kt+2, global loads issued during kt-1; the buffer's old
//                                     content, tile kt, already sits in F[kt&1])
//     G           <- global tile kt+3
//   one barrier per tile.
// KS = 2 (train step only): two 4-wave groups per workgroup take alternate K-tiles of the SAME output tile and add
// their accumulators through LDS before the epilogue -- a deterministic split-K that halves the critical path of the
// small-M recurrent GEMMs (M = 512 gives only 64 workgroups).  Inference keeps KS = 1 so that a row's sum order never
// depends on the batch it sits in.
// Tile (bm, bn) of job g by the calling workgroup; split-K part zidx of nsplit.
//
// SPLIT (KS = 1 only; option split_bf16, a measured experiment and NOT the default arithmetic): every fp32 operand value is taken
// apart into three bf16 values x = x0 + x1 + x2 (round to nearest, each remainder exact in fp32, so the sum is exact) while its tile
// is staged into LDS, and a K tile is contracted as six v_mfma_f32_32x32x16_bf16 products per 32x32 block with fp32 accumulation --
// a1.b1, a0.b2, a0.b1, a2.b0, a1.b0, a0.b0 (the order of gemm_split.hip's 256x256 tiles: an element's sum is the same instruction
// sequence in both, so the two tile shapes give the same bits); the three dropped products are below 2^-25 |a||b| -- at 6/16 of the matrix-pipe time of
// the fp32-input instruction.  The sums are fp32-accurate but NOT the k-ordered fmaf chain of the other kernels: results agree with
// them to rounding, not bit for bit.  Fragment registers roll instead of being double-buffered: a plane's fragments of tile kt + 1
// are read into the registers of tile kt as soon as their last product has issued (B planes 2 and 1 and A plane 0 behind the
// tile's barrier, B plane 0 at the head of the next tile), so one barrier per tile still separates every LDS buffer's reads from
// the stores that refill it.
// ACC (SPLIT only): the variant that honours GemmArgs.acc_in -- an instantiation of its own, so that the launches without the field
// keep their register allocation (the accumulators are live through the whole prologue here).
template <int EPI, int KS, bool SPLIT = false, bool ACC = false>
__device__ __forceinline__ void gemm_tile(const GemmArgs& g, const int bm, const int bn, const int zidx, const int nsplit, float* smem_all) {
#ifdef CASV_GEMM_PROF
    const unsigned long long pt0 = __builtin_amdgcn_s_memtime();
    unsigned long long pt1 = pt0, pt2 = pt0, pr1 = 0, pr2 = 0, pa = pt0, pb = pt0, pc = pt0, pe = pt0; int ptiles = 0;
#endif
    const int grp = KS > 1 ? (threadIdx.x >> 8) : 0;
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    static_assert(!SPLIT || KS == 1, "the bf16-split variant has no wave-group split-K");
    constexpr int BUF_FLOATS = SPLIT ? SPLIT_BUF_FLOATS : 2 * TILE_FLOATS;      // one LDS buffer: an A tile and a B tile
    float* smem = smem_all + grp * (2 * BUF_FLOATS);
    const int l31 = lane & 31, lh = lane >> 5;
    // wave-uniform by construction; say so (the value arrives through a vector load)
    const int step = __builtin_amdgcn_readfirstlane(g.step_ptr ? *g.step_ptr : g.step_imm);
    const int nbn = (g.N + BN - 1) / BN;
    const int m0 = bm * BM, n0 = bn * BN;
    if (m0 >= g.M || bm * nbn + bn >= ((g.M + BM - 1) / BM) * nbn) return;
    if (g.nact) {           // every wave looks at the same counts: a uniform exit ahead of the first barrier
        const int mlast = (m0 + BM < g.M ? m0 + BM : g.M) - 1;
        const int l0 = m0 / g.nact_group, l1 = mlast / g.nact_group;
        int alive = 0;
        for (int l = l0 + lane; l <= l1; l += 64) alive |= g.nact[l] > (l == l0 ? m0 - l0 * g.nact_group : 0);
        if (!__any(alive)) return;
    }

    const int r0 = tid >> 2, kc = tid & 3;     // staging: rows r0, r0+64; floats [4kc, 4kc+4)

    // Operand rows of the (up to three) K segments.  The row indices of every gathered segment -- and of the cell state, below --
    // are requested TOGETHER and without branches (a segment without an index array reads a dummy word): one memory round trip
    // for all of them instead of one per segment, each behind its own branch and full wait (round 4, in-kernel stamps: 7 800
    // cycles of set-up in front of the first tile request).
    const float* ap0[2]; const float* ap1[2]; const float* ap2[2];
    int tiles0 = 0, tiles1 = 0, tiles2 = 0;
    int mrow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { const int m = m0 + r0 + 64 * i; mrow[i] = m < g.M ? m : g.M - 1; }
    const int* const no_rows = reinterpret_cast<const int*>(g.Bt);          // any readable word
    // (the segment descriptors as local copies, fetched from the kernel-argument segment in ONE batch of scalar loads: read
    // field by field behind the short-circuit conditions below they were two dozen dependent scalar round trips)
    const Seg sg0 = g.a[0], sg1 = g.a[1], sg2 = g.a[2], sgc = g.c_in;
    const int nseg = g.nseg;
    asm volatile("" :: "s"(sg0.base), "s"(sg0.rows), "s"(sg0.first_base), "s"(sg1.base), "s"(sg1.rows), "s"(sg1.first_base),
                 "s"(sg2.base), "s"(sg2.rows), "s"(sg2.first_base), "s"(sgc.base), "s"(sgc.rows), "s"(sgc.first_base));
    const Seg* const sgs[3] = {&sg0, &sg1, &sg2};
    int ridx[3][2];
    bool act[3], gat[3];
#pragma unroll
    for (int S = 0; S < 3; ++S) {
        const Seg& sg = *sgs[S];
        act[S] = nseg > S && !(sg.skip_first && step == 0 && !sg.first_base);
        gat[S] = act[S] && sg.rows && !(sg.first_base && step == 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) ridx[S][i] = *(gat[S] ? sg.rows + mrow[i] : no_rows);
    }
    const bool cell_lane = EPI == EPI_LSTM && grp == 0 && !g.epi_plain;
    const bool cfirst = cell_lane && sgc.first_base && step == 0;
    const bool czero = cell_lane && sgc.skip_first && step == 0 && !cfirst;
    const bool cstage = cell_lane && !czero;
    int crow[2] = {0, 0};
    const float* cin = !cstage ? nullptr : cfirst ? sgc.first_base
        : sgc.base + (long long)(step * sgc.step_mul + sgc.step_add) * sgc.slot_stride;
    {
        const bool cgat = cstage && sgc.rows && !cfirst;
#pragma unroll
        for (int i = 0; i < 2; ++i) { const int ci = *(cgat ? sgc.rows + mrow[i] : no_rows); crow[i] = cgat ? ci : mrow[i]; }
    }
    auto cptr = [&](int i) { return cin + (long long)crow[i] * sgc.ld + bn * 32 + 4 * kc; };
#define CASV_SETUP_SEG(S, AP, TILES)                                                             \
    if (act[S]) {                                                                                \
        const Seg& sg = *sgs[S];                                                                 \
        const bool first = sg.first_base && step == 0;                                           \
        const float* base = first ? sg.first_base                                                \
            : sg.base + (long long)(step * sg.step_mul + sg.step_add) * sg.slot_stride;          \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                          \
            const int rid = gat[S] ? ridx[S][i] : mrow[i];                                       \
            AP[i] = base + (long long)rid * sg.ld + 4 * kc;                                      \
        }                                                                                        \
        TILES = sg.width / BK;                                                                   \
    } else {                                                                                     \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) AP[i] = nullptr;                           \
    }
    CASV_SETUP_SEG(0, ap0, tiles0)
    CASV_SETUP_SEG(1, ap1, tiles1)
    CASV_SETUP_SEG(2, ap2, tiles2)
#undef CASV_SETUP_SEG
    const int c0 = __builtin_amdgcn_readfirstlane(tiles0), c1 = __builtin_amdgcn_readfirstlane(tiles0 + tiles1);
    const int ntiles_all = __builtin_amdgcn_readfirstlane(tiles0 + tiles1 + tiles2);
    // split-K: this block contracts k-tiles [kt_begin, kt_begin + ntiles)
    const int per = (ntiles_all + nsplit - 1) / nsplit;
    const int kt_begin = zidx * per;
    const int nt_blk = ntiles_all - kt_begin < per ? (ntiles_all - kt_begin > 0 ? ntiles_all - kt_begin : 0) : per;
    // this wave group's share: tiles kt_begin + KS*i + grp
    const int ntiles = (nt_blk - grp + KS - 1) / KS, nt_min = nt_blk / KS, nt_max = (nt_blk + KS - 1) / KS;
    const int koff0 = sg0.koff, koff1 = sg1.koff, koff2 = sg2.koff;

    const float* bp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int n = n0 + r0 + 64 * i; n = n < g.N ? n : g.N - 1;
        bp[i] = g.Bt + (long long)n * g.Ktot + 4 * kc;
    }

    // Segment selection without control flow: pointer = ap0 + mask1*(ap1-ap0) + mask2*(ap2-ap0) with wave-uniform
    // 0/-1 masks, so that the steady-state loop body stays ONE basic block (the scheduler interleaves only inside one).
    const long long d1_0 = (long long)((const char*)ap1[0] - (const char*)ap0[0]), d1_1 = (long long)((const char*)ap1[1] - (const char*)ap0[1]);
    const long long d2_0 = (long long)((const char*)ap2[0] - (const char*)ap0[0]), d2_1 = (long long)((const char*)ap2[1] - (const char*)ap0[1]);
    struct GTile { f32x4 a[2], b[2]; };
    auto load_tile = [&](GTile& gt, int kt_rel) {
        const int kt = kt_rel * KS + grp + kt_begin;
        const long long m1 = (kt >= c0 && kt < c1) ? -1LL : 0LL, m2 = (kt >= c1) ? -1LL : 0LL;
        const int ko = kt - ((int)m1 & c0) - ((int)m2 & c1);                       // tile index inside its segment
        const int kb = koff0 + ((int)m1 & (koff1 - koff0)) + ((int)m2 & (koff2 - koff0)) + ko * BK;
        const char* pa0 = (const char*)ap0[0] + (d1_0 & m1) + (d2_0 & m2) + (long long)ko * (BK * 4);
        const char* pa1 = (const char*)ap0[1] + (d1_1 & m1) + (d2_1 & m2) + (long long)ko * (BK * 4);
        gt.a[0] = *reinterpret_cast<const f32x4*>(pa0); gt.a[1] = *reinterpret_cast<const f32x4*>(pa1);
        gt.b[0] = *reinterpret_cast<const f32x4*>(bp[0] + kb); gt.b[1] = *reinterpret_cast<const f32x4*>(bp[1] + kb);
    };
    // The first tiles of the prologue when they all lie in segment 0 (every launch of the decoder and encoder: the layer input
    // comes first and is at least four tiles wide): addressed without the segment masks, i.e. without waiting for the row
    // indices of the gathered segments behind it (the parents' h rows) -- one dependent memory round trip less in front of
    // the first MFMA of every workgroup.
    auto load_tile_seg0 = [&](GTile& gt, int kt) {
        gt.a[0] = *reinterpret_cast<const f32x4*>(ap0[0] + kt * BK); gt.a[1] = *reinterpret_cast<const f32x4*>(ap0[1] + kt * BK);
        gt.b[0] = *reinterpret_cast<const f32x4*>(bp[0] + koff0 + kt * BK); gt.b[1] = *reinterpret_cast<const f32x4*>(bp[1] + koff0 + kt * BK);
    };
    // The same four loads hidden from the compiler's wait bookkeeping (steady state only).  hipcc's s_waitcnt in front of
    // the LDS store of tile kt + 2 counts in order and drains the loads of tile kt + 3 with it (issued one tile earlier):
    // the prefetch was one tile deep for every second tile.  Issued from asm statements the loads are invisible to that
    // bookkeeping; CASV_TILE_FULL waits with a counted vmcnt(4) instead -- the four loads of the tile about to be stored
    // have landed, the four of the next tile stay in flight -- so every tile's operands have two tile times to arrive.
    auto issue_tile_asm = [&](GTile& gt, const char* pa0, const char* pa1, const float* pb0, const float* pb1) {
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(gt.a[0]) : "v"(pa0));
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(gt.a[1]) : "v"(pa1));
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(gt.b[0]) : "v"(pb0));
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(gt.b[1]) : "v"(pb1));
    };
    auto load_tile_asm = [&](GTile& gt, int kt_rel) {
        const int kt = kt_rel * KS + grp + kt_begin;
        const long long m1 = (kt >= c0 && kt < c1) ? -1LL : 0LL, m2 = (kt >= c1) ? -1LL : 0LL;
        const int ko = kt - ((int)m1 & c0) - ((int)m2 & c1);
        const int kb = koff0 + ((int)m1 & (koff1 - koff0)) + ((int)m2 & (koff2 - koff0)) + ko * BK;
        const char* pa0 = (const char*)ap0[0] + (d1_0 & m1) + (d2_0 & m2) + (long long)ko * (BK * 4);
        const char* pa1 = (const char*)ap0[1] + (d1_1 & m1) + (d2_1 & m2) + (long long)ko * (BK * 4);
        issue_tile_asm(gt, pa0, pa1, bp[0] + kb, bp[1] + kb);
    };
    // Steady state of the KS = 1 kernels: RUNNING operand pointers, advanced by one K tile per request (four 64-bit adds), and
    // re-based where the request stream crosses into the next K segment -- a wave-uniform branch taken twice per K loop at most.
    // The mask arithmetic above costs ~24 vector and ~20 scalar instructions per tile; a wave that has the matrix pipe to itself
    // (its partner workgroup in prologue / epilogue: almost half of a decoder launch) issues them between its own MFMAs:
    // 2317 instead of 2189 cycles per tile in profiles/kloop_probe.hip (ABL = 16 against 0, one workgroup per CU).
    const char* ra0 = nullptr; const char* ra1 = nullptr; const float* rb0 = nullptr; const float* rb1 = nullptr;
    int rleft = 0, rseg = 0;
    // (the gathered segments' row pointers -- and the cell state's -- wait in LDS for their turn instead of in a dozen registers
    // through the whole loop; the B rows are K-contiguous: a scalar step re-bases them)
    const float** const rstash = reinterpret_cast<const float**>(smem_all + KS * (2 * BUF_FLOATS) + CELL_LDS_BYTES / 4) + 6 * tid;
    auto run_set = [&](int kt_rel) {                       // position the running pointers at tile kt_rel
        const int kt = kt_rel * KS + grp + kt_begin;
        const long long m1 = (kt >= c0 && kt < c1) ? -1LL : 0LL, m2 = (kt >= c1) ? -1LL : 0LL;
        const int ko = kt - ((int)m1 & c0) - ((int)m2 & c1);
        const int kb = koff0 + ((int)m1 & (koff1 - koff0)) + ((int)m2 & (koff2 - koff0)) + ko * BK;
        ra0 = (const char*)ap0[0] + (d1_0 & m1) + (d2_0 & m2) + (long long)ko * (BK * 4);
        ra1 = (const char*)ap0[1] + (d1_1 & m1) + (d2_1 & m2) + (long long)ko * (BK * 4);
        rb0 = bp[0] + kb; rb1 = bp[1] + kb;
        rseg = kt >= c1 ? 2 : kt >= c0 ? 1 : 0;
        rleft = (rseg == 0 ? c0 : rseg == 1 ? c1 : ntiles_all) - kt;
        rstash[0] = ap1[0]; rstash[1] = ap1[1]; rstash[2] = ap2[0]; rstash[3] = ap2[1];
        if (EPI == EPI_LSTM) { rstash[4] = cstage ? cptr(0) : bp[0]; rstash[5] = cstage ? cptr(1) : bp[0]; }   // (no cell state: any valid address)
    };
    auto run_advance = [&]() {
        ra0 += BK * 4; ra1 += BK * 4; rb0 += BK; rb1 += BK;
        if (--rleft == 0) {
            asm volatile("" ::: "memory");                  // (stays a branch: as selects it would be the mask arithmetic again)
            if (rseg == 0 && c1 > c0) {
                rseg = 1; rleft = c1 - c0;
                ra0 = (const char*)rstash[0]; ra1 = (const char*)rstash[1];
                rb0 += koff1 - koff0 - c0 * BK; rb1 += koff1 - koff0 - c0 * BK;
            } else if (rseg <= 1 && ntiles_all > c1) {
                const int kprev = rseg == 0 ? koff0 + c0 * BK : koff1 + (c1 - c0) * BK;
                rseg = 2; rleft = ntiles_all - c1;
                ra0 = (const char*)rstash[2]; ra1 = (const char*)rstash[3];
                rb0 += koff2 - kprev; rb1 += koff2 - kprev;
            } else {
                rleft = 1 << 30;                             // behind the last tile: nothing is requested from here any more
            }
        }
    };
    auto load_tile_run = [&](GTile& gt) { issue_tile_asm(gt, ra0, ra1, rb0, rb1); };    // (run_advance() follows behind the tile's MFMAs)
    auto load_tile_run_plain = [&](GTile& gt) {             // the same request, visible to the compiler (tail tiles)
        gt.a[0] = *reinterpret_cast<const f32x4*>(ra0); gt.a[1] = *reinterpret_cast<const f32x4*>(ra1);
        gt.b[0] = *reinterpret_cast<const f32x4*>(rb0); gt.b[1] = *reinterpret_cast<const f32x4*>(rb1);
        run_advance();
    };
    auto store_tile = [&](const GTile& gt, int buf) {
        float* sa = smem + buf * 2 * TILE_FLOATS + r0 * LDW + 4 * kc;
        float* sb = sa + TILE_FLOATS;
        *reinterpret_cast<f32x4*>(sa) = gt.a[0]; *reinterpret_cast<f32x4*>(sa + 64 * LDW) = gt.a[1];
        *reinterpret_cast<f32x4*>(sb) = gt.b[0]; *reinterpret_cast<f32x4*>(sb + 64 * LDW) = gt.b[1];
    };
    // SPLIT: x = x0 + x1 + x2 in bf16 (round to nearest; the remainders are exact), four k of a row at a time -> 8 bytes per plane
#ifndef CASV_ABLM
#define CASV_ABLM 0         // timing-only builds of the SPLIT variant (wrong results), a bit mask: 1 no split arithmetic, 2 no LDS stores, 4 no global loads, 8 no barrier, 16 no fragment reads
#endif
    auto split4 = [&](const f32x4 x, u32x2& p0, u32x2& p1, u32x2& p2, const bool isb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (CASV_ABLM & 1) {
                p0[h] = __float_as_uint(x[2 * h]); p1[h] = __float_as_uint(x[2 * h + 1]); p2[h] = p0[h] ^ p1[h];
                continue;
            }
            const f32x2 v = {x[2 * h], x[2 * h + 1]};
            const unsigned q0 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
            const f32x2 r1 = v - f32x2{__uint_as_float(q0 << 16), __uint_as_float(q0 & 0xffff0000u)};
            const unsigned q1 = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
            const f32x2 r2 = r1 - f32x2{__uint_as_float(q1 << 16), __uint_as_float(q1 & 0xffff0000u)};
            p0[h] = q0; p1[h] = q1; p2[h] = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
        }
    };
    // (staging rows r0 and r0 + 64 share bit 4: one offset serves both)
    const int st_off = r0 * 32 + ((((kc >> 1) ^ (r0 >> 4)) & 1) * 16) + (kc & 1) * 8;
    auto store_tile_split = [&](const GTile& gt, int buf, const bool opa = true, const bool opb = true) {
        if (CASV_ABLM & 2) { asm volatile("" :: "v"(gt.a[0]), "v"(gt.a[1]), "v"(gt.b[0]), "v"(gt.b[1])); return; }
        char* base = reinterpret_cast<char*>(smem + buf * BUF_FLOATS) + st_off;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x2 p0, p1, p2;
            if (opa) {
                split4(gt.a[i], p0, p1, p2, false);
                *reinterpret_cast<u32x2*>(base + i * 64 * 32) = p0;
                *reinterpret_cast<u32x2*>(base + SPLIT_PLANE_BYTES + i * 64 * 32) = p1;
                *reinterpret_cast<u32x2*>(base + 2 * SPLIT_PLANE_BYTES + i * 64 * 32) = p2;
            }
            if (opb) {
                split4(gt.b[i], p0, p1, p2, true);
                *reinterpret_cast<u32x2*>(base + 3 * SPLIT_PLANE_BYTES + i * 64 * 32) = p0;
                *reinterpret_cast<u32x2*>(base + 4 * SPLIT_PLANE_BYTES + i * 64 * 32) = p1;
                *reinterpret_cast<u32x2*>(base + 5 * SPLIT_PLANE_BYTES + i * 64 * 32) = p2;
            }
        }
    };
    // a lane's 8 k of its row: the 16-byte half lh (k = 8 lh .. 8 lh + 7, the same for both operands)
    const int fr_off = l31 * 32 + (((lh ^ (l31 >> 4)) & 1) * 16);
    auto frag_a = [&](int buf, int plane) {
        return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(smem + buf * BUF_FLOATS) + plane * SPLIT_PLANE_BYTES + wave * 32 * 32 + fr_off);
    };
    auto frag_b = [&](int buf, int plane, int c) {
        return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(smem + buf * BUF_FLOATS) + (3 + plane) * SPLIT_PLANE_BYTES + c * 32 * 32 + fr_off);
    };
    const int a_off = (wave * 32 + l31) * LDW + 4 * lh;
    const int b_off = TILE_FLOATS + l31 * LDW + 4 * lh;
    struct Frag { f32x4 a[2]; f32x4 b[4][2]; };
    auto read_frags = [&](Frag& f, int buf) {
        const float* base = smem + buf * 2 * TILE_FLOATS;
#pragma unroll
        for (int j = 0; j < 2; ++j) f.a[j] = *reinterpret_cast<const f32x4*>(base + a_off + 8 * j);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 2; ++j) f.b[c][j] = *reinterpret_cast<const f32x4*>(base + b_off + c * 32 * LDW + 8 * j);
    };

    f32x16 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.0f;
    static_assert(!ACC || SPLIT, "acc_in belongs to the bf16-split variant");
    if constexpr (ACC) {
        // acc_in (gemm_args.h): the accumulators start from what another launch left behind the K segments in front of this job's --
        // plain fp32 register values between two products, so the element's instruction sequence is the one of the undivided
        // contraction.  (A raw plain output is acc + 0.0f, which differs from acc only for acc = -0.  An accumulator starts at +0,
        // and a round-to-nearest sum is -0 only if every term is: +0 plus products never is, whatever their signs -- short of a
        // whole product sum below 2^-150 that underflows to -0, which bf16x3 parts of weights and activations do not reach.)
        // Ordinary loads, requested ahead of tiles 0 and 1 (whose registers are not live yet) and waited for behind those tiles' LDS
        // stores: ahead of every hidden load, nothing pending on any path into the loop.
        const Seg sga = g.acc_in;
        if (sga.base) {
            const float* abase = sga.base + (long long)(step * sga.step_mul + sga.step_add) * sga.slot_stride;
            const float* arow[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                m = m < g.M ? m : g.M - 1;
                arow[r] = abase + (long long)(sga.rows ? sga.rows[m] : m) * sga.ld;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                int n = n0 + c * 32 + l31;
                n = n < g.N ? n : g.N - 1;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][r] = arow[r][n];
            }
        }
    }
    auto mma = [&](const Frag& f) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[j][i], f.b[c][j][i], acc[c], 0, 0, 0);
    };

#ifdef CASV_GEMM_PROF
    CASV_STAMP(pa)
#endif
    // LSTM: the previous cell state of the tile -- 128 rows x 32 units, 128 bytes per (gathered) row -- is fetched like an operand
    // tile: every thread 16-byte pieces of its two staging rows (chunks kc and kc + 4), parked in registers under the K loop and
    // turned into the accumulator layout through LDS behind it.  Round 4, in-kernel stamps of the c3 decode
    // (profiles/r04_gemm_stamps.txt): as 16 dependent 4-byte gathers per lane in the prologue the cell state took 26 000 cycles
    // (11 us) to land -- in front of the first MFMA, because no compiler-tracked load may be pending on a path into the loop --
    // and 23 000 when requested behind the loop instead; 4-byte-per-lane accesses are what the memory pipeline is slowest at.
    // cell-state area behind the tile buffers: [half j of the 128-byte row][row][16 floats], the image a wave's LDS-DMA writes
    // (lane L -> 16 bytes at base + 16 L: rows wave * 16 + L / 4, chunk L % 4)
    float* const cs = smem_all + KS * (2 * BUF_FLOATS);
    auto cell_dma = [&](int i, int j) {
        const float* src = rstash[4 + i] + 16 * j;
        const unsigned dst = __builtin_amdgcn_readfirstlane(
            (unsigned)(size_t)(__attribute__((address_space(3))) float*)cs + (unsigned)((j * 128 + 64 * i + (tid >> 6) * 16) * 64));
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    };
#ifdef CASV_GEMM_PROF
    CASV_STAMP(pb)
#endif
    Frag f0, f1;
    GTile g0, g1;
    // prologue: LDS[0] <- tile 0, LDS[1] <- tile 1, F0 <- LDS[0]; G0 <- tile 2, G1 <- tile 3
    if (KS == 1 && kt_begin == 0 && c0 >= 2 && ntiles > 1) { load_tile_seg0(g0, 0); load_tile_seg0(g1, 1); }
    else {
        if (ntiles > 0) load_tile(g0, 0);
        if (ntiles > 1) load_tile(g1, 1);
    }
#ifdef CASV_GEMM_PROF
    CASV_STAMP(pc)
#endif
    if constexpr (SPLIT) {
        if (ntiles > 0) store_tile_split(g0, 0);
        if (ntiles > 1) store_tile_split(g1, 1);
        if constexpr (ACC) { if (g.acc_in.base) asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])); }
    } else {
        if (ntiles > 0) store_tile(g0, 0);
        if (ntiles > 1) store_tile(g1, 1);
    }
    // SPLIT: rolling fragment registers -- B planes [block][plane], A plane 0 double-buffered (it serves a tile's first and last product)
    bf16x8 sb[4][3], sa0x, sa0y, sa1, sa2;
    auto split_first_frags = [&]() {            // what a tile expects to find in registers: B planes 2 and 1, all of A (tile 0, buffer 0)
#pragma unroll
        for (int c = 0; c < 4; ++c) { sb[c][2] = frag_b(0, 2, c); sb[c][1] = frag_b(0, 1, c); }
        sa0x = frag_a(0, 0); sa1 = frag_a(0, 1); sa2 = frag_a(0, 2);
    };
#define CASV_SPLIT_MMA(A, P)                                                              \
    _Pragma("unroll") for (int c_ = 0; c_ < 4; ++c_)                                      \
        acc[c_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, sb[c_][P], acc[c_], 0, 0, 0);
    // (scheduling fence that vector arithmetic may cross -- the split's arithmetic finds its own place between the
    // products -- while matrix, LDS and memory instructions stay on their side: left to itself the compiler issues a plane's
    // fragment reads two products ahead of their first use and every tile waits for the LDS twice)
#define CASV_SPLIT_PIN __builtin_amdgcn_sched_barrier(0x2);
    // One K tile of the SPLIT variant.  FULL: steady state (tiles KT+1..KT+4 exist, hidden loads, no conditionals).
#define CASV_SPLIT_TILE(AC, AN, G, KT, FULL)                                              \
    {                                                                                     \
        const bool have_ = FULL || (KT) < ntiles, next_ = FULL || (KT) + 1 < ntiles;      \
        const bool reads_ = !(FULL && (CASV_ABLM & 16)), loads_ = !(CASV_ABLM & 4);       \
        if (FULL && loads_) asm volatile("s_waitcnt vmcnt(4)" : "+v"(G.a[0]), "+v"(G.a[1]), "+v"(G.b[0]), "+v"(G.b[1]));  \
        if (have_) {                                                                      \
            if (reads_) _Pragma("unroll") for (int c_ = 0; c_ < 4; ++c_) sb[c_][0] = frag_b((KT) & 1, 0, c_);   \
            if (FULL) CASV_SPLIT_PIN                                                      \
            CASV_SPLIT_MMA(sa1, 1) CASV_SPLIT_MMA(AC, 2) CASV_SPLIT_MMA(AC, 1)    /* (the product order of gemm_split.hip: same bits) */ \
        }                                                                                 \
        if (FULL) CASV_SPLIT_PIN        /* the 12 products stay in front of the barrier: plane 0's reads land under them */ \
        if (!(FULL && (CASV_ABLM & 8))) __syncthreads();                                  \
        if (next_ && reads_) {                                                            \
            _Pragma("unroll") for (int c_ = 0; c_ < 4; ++c_) { sb[c_][2] = frag_b(((KT) + 1) & 1, 2, c_); sb[c_][1] = frag_b(((KT) + 1) & 1, 1, c_); }  \
            AN = frag_a(((KT) + 1) & 1, 0);                                               \
        }                                                                                 \
        if (FULL) CASV_SPLIT_PIN                                                          \
        if (have_) CASV_SPLIT_MMA(sa2, 0)                                                 \
        if (FULL) CASV_SPLIT_PIN                                                          \
        if (next_ && reads_) sa2 = frag_a(((KT) + 1) & 1, 2);                             \
        if (FULL || (KT) + 2 < ntiles) store_tile_split(G, (KT) & 1, true, false);        \
        if (FULL) CASV_SPLIT_PIN                                                          \
        if (have_) CASV_SPLIT_MMA(sa1, 0)                                                 \
        if (FULL) CASV_SPLIT_PIN                                                          \
        if (next_ && reads_) sa1 = frag_a(((KT) + 1) & 1, 1);                             \
        if (FULL || (KT) + 2 < ntiles) store_tile_split(G, (KT) & 1, false, true);        \
        if (FULL) { if (loads_) load_tile_run(G); } else if ((KT) + 4 < ntiles) load_tile_run_plain(G);   \
        if (FULL) CASV_SPLIT_PIN                                                          \
        if (have_) CASV_SPLIT_MMA(AC, 0)                                                  \
        if (FULL) run_advance();                                                          \
    }

    // Steady state (tiles kt+1..kt+4 exist, no conditionals): while the 32 MFMAs of tile kt issue from FC,
    //   LDS[kt&1] <- G (tile kt+2, requested two steps ago; the buffer's old content, tile kt, sits in FC)
    //   G <- global tile kt+4 ;  FN <- LDS[(kt+1)&1]
    // with the issue order pinned: one memory instruction + a few address ops behind each of the first MFMAs,
    // so a wave has no memory-only phase in which its SIMD partner's MFMA stream starves its instruction issue.
#define CASV_TILE_FULL_X(FC, FN, G, KT, NMEM, EXTRA_LOADS)                                \
    {                                                                                     \
        asm volatile("s_waitcnt vmcnt(4)" : "+v"(G.a[0]), "+v"(G.a[1]), "+v"(G.b[0]), "+v"(G.b[1]));  \
        store_tile(G, (KT) & 1);                                                          \
        if (KS == 1) load_tile_run(G); else load_tile_asm(G, (KT) + 4);                  \
        EXTRA_LOADS                                                                       \
        read_frags(FN, ((KT) + 1) & 1);                                                   \
        mma(FC);                                                                          \
        _Pragma("unroll") for (int q_ = 0; q_ < NMEM; ++q_) {                             \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                            \
            __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);                            \
            __builtin_amdgcn_sched_group_barrier(0x320, 1, 0);                            \
        }                                                                                 \
        __builtin_amdgcn_sched_group_barrier(0x008, 32 - NMEM, 0);                        \
        __builtin_amdgcn_sched_barrier(0);   /* keep all 32 MFMAs in front of the barrier: by then the LDS ops have landed */ \
        if (KS == 1) run_advance();          /* (its rare branch ends the tile's basic block: behind everything that interleaves) */ \
        __syncthreads();                                                                  \
    }
#define CASV_TILE_FULL(FC, FN, G, KT) CASV_TILE_FULL_X(FC, FN, G, KT, 18, )
#define CASV_TILE_STEP(FC, FN, G, KT)                                                     \
    {                                                                                     \
        if ((KT) + 2 < ntiles) store_tile(G, (KT) & 1);                                   \
        if ((KT) + 4 < ntiles) { if (KS == 1) load_tile_run_plain(G); else load_tile(G, (KT) + 4); }  \
        if ((KT) + 1 < ntiles) read_frags(FN, ((KT) + 1) & 1);                            \
        if ((KT) < ntiles) mma(FC);                                                       \
        __syncthreads();                                                                  \
    }
    int kt = 0;
    // (hidden transfers in flight across the tail below are older than anything the tail requests itself -- an odd tile count
    // requests one more tile there --, so the compiler's counted waits for its own loads stay correct: they only wait longer)
    const bool c_late = EPI == EPI_LSTM && KS == 1 && nt_min > 5;
    if (nt_min > 5) {
        // Tiles 2 and 3 are requested the hidden way already: a compiler-tracked load pending on ANY path into the loop would
        // put a full vmcnt(0) at the loop head, executed in every iteration.  (The cell-state loads above are older than
        // every tile load, so the counted waits cover them too.)
        // (c0 >= 4: tiles 2 and 3 lie in the layer input too -- their addresses do not wait for the gathered segments' row indices)
        {
            const char *qa0, *qa1, *ra0, *ra1; const float *qb0, *qb1, *rb0, *rb1;
            if (KS == 1 && kt_begin == 0 && c0 >= 4) {      // (KS = 2: a wave group's tiles 2 and 3 are tiles 4 + grp and 6 + grp)
                qa0 = (const char*)(ap0[0] + 2 * BK); qa1 = (const char*)(ap0[1] + 2 * BK); qb0 = bp[0] + koff0 + 2 * BK; qb1 = bp[1] + koff0 + 2 * BK;
                ra0 = (const char*)(ap0[0] + 3 * BK); ra1 = (const char*)(ap0[1] + 3 * BK); rb0 = bp[0] + koff0 + 3 * BK; rb1 = bp[1] + koff0 + 3 * BK;
                asm volatile("" : "+v"(qa0), "+v"(ra0));           // (keeps the two paths apart: a select would wait for the indices)
            } else {
                auto addr = [&](int kt_rel, const char*& pa0, const char*& pa1, const float*& pb0, const float*& pb1) {
                    const int ktt = kt_rel * KS + grp + kt_begin;
                    const long long m1 = (ktt >= c0 && ktt < c1) ? -1LL : 0LL, m2 = (ktt >= c1) ? -1LL : 0LL;
                    const int ko = ktt - ((int)m1 & c0) - ((int)m2 & c1);
                    const int kb = koff0 + ((int)m1 & (koff1 - koff0)) + ((int)m2 & (koff2 - koff0)) + ko * BK;
                    pa0 = (const char*)ap0[0] + (d1_0 & m1) + (d2_0 & m2) + (long long)ko * (BK * 4);
                    pa1 = (const char*)ap0[1] + (d1_1 & m1) + (d2_1 & m2) + (long long)ko * (BK * 4);
                    pb0 = bp[0] + kb; pb1 = bp[1] + kb;
                };
                addr(2, qa0, qa1, qb0, qb1); addr(3, ra0, ra1, rb0, rb1);
            }
            issue_tile_asm(g0, qa0, qa1, qb0, qb1); issue_tile_asm(g1, ra0, ra1, rb0, rb1);
        }
        __syncthreads();
        if constexpr (SPLIT) split_first_frags(); else read_frags(f0, 0);
        // The first steady-state step stores tile 2 into LDS buffer 0: every wave must have taken its fragments of tile 0
        // out of it first.  (Without this barrier only the latency of the tile-2 global loads kept a fast wave's store
        // behind a slow wave's read -- not enough once other kernels share the CU.)
        __syncthreads();
#ifdef CASV_GEMM_PROF
        pt1 = __builtin_amdgcn_s_memtime(); pr1 = __builtin_amdgcn_s_memrealtime();
#endif
        if (KS == 1) run_set(4);                    // the first steady-state tile requests tile 4
        if constexpr (SPLIT) {
            for (; kt + 5 < nt_min; kt += 2) {
                CASV_SPLIT_TILE(sa0x, sa0y, g0, kt, true)
                CASV_SPLIT_TILE(sa0y, sa0x, g1, kt + 1, true)
            }
        } else
        for (; kt + 5 < nt_min; kt += 2) {          // both wave groups have all the tiles of the steady state
            CASV_TILE_FULL(f0, f1, g0, kt)
            CASV_TILE_FULL(f1, f0, g1, kt + 1)
        }
#ifdef CASV_GEMM_PROF
        pt2 = __builtin_amdgcn_s_memtime(); pr2 = __builtin_amdgcn_s_memrealtime(); ptiles = kt;
#endif
        // The cell state is requested behind the LAST tile loads, as LDS-DMA (no registers are held for it; hidden from the
        // compiler's wait bookkeeping like the tile loads): nothing is queued behind it that a counted wait looks at, so however
        // long the gathered rows take (rows of parents from many steps ago: HBM and page-table walks), no operand tile waits for
        // them; they land under the tail tiles.  The tile loads themselves land before the compiler-scheduled rest touches them.
        // (Every steady-state path of the LSTM kernel issues the four transfers -- jobs without a cell state from a valid dummy
        // address -- so that ONE wait statement with ONE count follows the loop: two statements on two paths would meet in copies of
        // registers whose loads are still in flight, csrc/check_asm_loads.py.)
        if (EPI == EPI_LSTM && KS == 1) {
            cell_dma(0, 0); cell_dma(0, 1); cell_dma(1, 0); cell_dma(1, 1);
            asm volatile("s_waitcnt vmcnt(4)" : "+v"(g0.a[0]), "+v"(g0.a[1]), "+v"(g0.b[0]), "+v"(g0.b[1]), "+v"(g1.a[0]), "+v"(g1.a[1]), "+v"(g1.b[0]), "+v"(g1.b[1]));
        } else {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(g0.a[0]), "+v"(g0.a[1]), "+v"(g0.b[0]), "+v"(g0.b[1]), "+v"(g1.a[0]), "+v"(g1.a[1]), "+v"(g1.b[0]), "+v"(g1.b[1]));
        }
    } else {
        if (ntiles > 2) load_tile(g0, 2);
        if (ntiles > 3) load_tile(g1, 3);
        if (KS == 1 && ntiles > 4) run_set(4);
        __syncthreads();
        if constexpr (SPLIT) { if (ntiles > 0) split_first_frags(); } else { if (ntiles > 0) read_frags(f0, 0); }
        __syncthreads();
    }
    if (cstage && !c_late) {        // (short K, odd tile counts, wave-group split-K: through registers, stored into the same image)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                *reinterpret_cast<f32x4*>(cs + (j * 128 + r0 + 64 * i) * 16 + 4 * kc) = *reinterpret_cast<const f32x4*>(cptr(i) + 16 * j);
    }
    if constexpr (SPLIT) {
        for (; kt + 1 < nt_max; kt += 2) {
            CASV_SPLIT_TILE(sa0x, sa0y, g0, kt, false)
            CASV_SPLIT_TILE(sa0y, sa0x, g1, kt + 1, false)
        }
        if (kt < nt_max) CASV_SPLIT_TILE(sa0x, sa0y, g0, kt, false)
    } else {
    for (; kt + 1 < nt_max; kt += 2) {          // same barrier count for both groups
        CASV_TILE_STEP(f0, f1, g0, kt)
        CASV_TILE_STEP(f1, f0, g1, kt + 1)
    }
    if (kt < nt_max) CASV_TILE_STEP(f0, f1, g0, kt)
    }
#undef CASV_SPLIT_TILE
#undef CASV_SPLIT_PIN
#undef CASV_SPLIT_MMA
#undef CASV_TILE_STEP
#undef CASV_TILE_FULL

#ifdef CASV_GEMM_PROF
    pe = __builtin_amdgcn_s_memtime();
#endif
    if (KS > 1) {       // acc(group 0) += acc(group 1), through LDS (all staging reads are behind the last barrier)
        float* red = smem_all + tid;
        if (grp == 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(c * 16 + r) * 256] = acc[c][r];
        }
        __syncthreads();
        if (grp == 1) return;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] += red[(c * 16 + r) * 256];
    }

    // the cell state in the accumulator layout, out of its LDS image (every wave waits for its own transfers first -- also where
    // the image is not read: an LDS-DMA must not outlive the workgroup whose LDS it writes)
    if (c_late) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float cpv[16];
    float bi = 0.f, bf_ = 0.f, bg = 0.f, bo = 0.f;       // LSTM: gate biases of this lane's unit (ONE branch; they arrive under the barrier)
    if (EPI == EPI_LSTM) {          // (uniform over the workgroup's remaining waves: group 1 of a KS = 2 launch has returned)
        if (!g.epi_plain) {
            if (g.bias) { bi = g.bias[n0 + l31]; bf_ = g.bias[n0 + 32 + l31]; bg = g.bias[n0 + 64 + l31]; bo = g.bias[n0 + 96 + l31]; }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r)
                cpv[r] = czero ? 0.0f : cs[((l31 >> 4) * 128 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 16 + (l31 & 15)];
        }
    }

    // ---- epilogue ----
    if (EPI == EPI_PLAIN || g.epi_plain) {
        float* cbase = g.out.base + (long long)(step * g.out.step_mul + g.out.step_add) * g.out.slot_stride;
        if (nsplit == 1 && m0 + BM <= g.M && n0 + BN <= g.N) {
            // full tile, plain stores: no control flow between the 64 stores (a branch per element makes the compiler wait for the
            // element before -- see the LSTM epilogue below); C += : all 64 old values are requested first, then added and stored
            float* cb = cbase + (long long)(m0 + wave * 32 + 4 * lh) * g.out.ld + n0 + l31;
            float bcol[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) bcol[c] = g.bias ? g.bias[n0 + c * 32 + l31] : 0.0f;
            if (g.accumulate) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[c][r] += cb[(long long)((r & 3) + 8 * (r >> 2)) * g.out.ld + c * 32];
            }
#if CASV_PLAIN_WIDE
            if (EPI == EPI_PLAIN && (g.out.ld & 3) == 0) {
                // 16-byte stores through an in-quad transpose: 16 store instructions per wave instead of 64, same bytes and addresses.
                // Pays where tiles are short (the train step's K = 512 contractions: c4 66.4-66.5 -> 66.0-66.3 ms per step); in the
                // LSTM kernel -- its cell epilogue, and the query job that rides in layer 1's launch -- it measured 0.3 % slower (c3).
                const int q = lane & 3;
                float* cq = cb + (long long)q * g.out.ld - q;
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        *reinterpret_cast<QuadF4*>(cq + (long long)(8 * gq) * g.out.ld + c * 32) =
                            quad_transpose(acc[c][4 * gq] + bcol[c], acc[c][4 * gq + 1] + bcol[c], acc[c][4 * gq + 2] + bcol[c], acc[c][4 * gq + 3] + bcol[c], q);
            } else
#endif
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) cb[(long long)((r & 3) + 8 * (r >> 2)) * g.out.ld + c * 32] = acc[c][r] + bcol[c];
        } else
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = n0 + c * 32 + l31;
            if (n < g.N) {
                const float b = g.bias ? g.bias[n] : 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (m < g.M) {
                        float* dst = cbase + (long long)m * g.out.ld + n;
                        if (nsplit > 1) atomicAdd(dst, acc[c][r] + (zidx == 0 ? b : 0.0f));
                        else *dst = g.accumulate ? (*dst + acc[c][r] + b) : (acc[c][r] + b);
                    }
                }
            }
        }
    } else {
        const int u = bn * 32 + l31;     // hidden unit of this lane
        const float* zin = g.zinit.base
            ? g.zinit.base + (long long)(step * g.zinit.step_mul + g.zinit.step_add) * g.zinit.slot_stride : nullptr;
        float* cout = g.c_out.base + (long long)(step * g.c_out.step_mul + g.c_out.step_add) * g.c_out.slot_stride;
        float* hout = g.out.base + (long long)(step * g.out.step_mul + g.out.step_add) * g.out.slot_stride;
        float* gout = g.gates_out.base
            ? g.gates_out.base + (long long)(step * g.gates_out.step_mul + g.gates_out.step_add) * g.gates_out.slot_stride
            : nullptr;
        float* hout2 = g.out2.base ? g.out2.base + (long long)(step * g.out2.step_mul + g.out2.step_add) * g.out2.slot_stride : nullptr;
        if (zin) {      // precomputed input term (train step): all loads issue before the first store of the loop below
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float* zr = zin + (long long)(m < g.M ? m : g.M - 1) * g.zinit.ld + n0 + l31;
                acc[0][r] += zr[0]; acc[1][r] += zr[32]; acc[2][r] += zr[64]; acc[3][r] += zr[96];
            }
        }
        if (m0 + BM <= g.M && !hout2 && !gout) {
            // Full tile, inference outputs only: all cells first, then all stores, no control flow in between.  (With a branch per
            // row the compiler's wait bookkeeping put an s_waitcnt vmcnt(0) in front of every row's cell -- stores count in
            // vmcnt too, so each of the 16 rows waited for the stores of the row before: 16 serial store round trips, 44 000 cycles
            // of epilogue in the c3 decode where the arithmetic needs 7 000.)
            float hv[16], cv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const LstmCellOut cell = lstm_cell(acc[0][r] + bi, acc[1][r] + bf_, acc[2][r] + bg, acc[3][r] + bo, cpv[r]);
                hv[r] = cell.h; cv[r] = cell.c;
            }
            float* cb = cout + (long long)(m0 + wave * 32 + 4 * lh) * g.c_out.ld + u;
            float* hb = hout + (long long)(m0 + wave * 32 + 4 * lh) * g.out.ld + u;
            // (16-byte stores from an in-quad transpose of the accumulators -- 8 store instructions per wave instead of 32 --
            // measured again in round 5, behind the round-4 epilogue: c3 271.0-271.3 ms without, 271.6-272.7 with.  Not store-issue bound.)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dm = (r & 3) + 8 * (r >> 2);
                cb[(long long)dm * g.c_out.ld] = cv[r];
                hb[(long long)dm * g.out.ld] = hv[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m < g.M) {
                    const float cprev = cpv[r];
                    float zi = acc[0][r] + bi, zf = acc[1][r] + bf_, zg = acc[2][r] + bg, zo = acc[3][r] + bo;
                    const LstmCellOut cell = lstm_cell(zi, zf, zg, zo, cprev);
                    cout[(long long)m * g.c_out.ld + u] = cell.c;
                    hout[(long long)m * g.out.ld + u] = cell.h;
                    if (hout2) hout2[(long long)m * g.out2.ld + u] = cell.h;
                    if (gout) {
                        float* gr = gout + (long long)m * g.gates_out.ld + n0 + l31;
                        gr[0] = cell.i; gr[32] = cell.f; gr[64] = cell.g; gr[96] = cell.o;
                    }
                }
            }
        }
    }
#ifdef CASV_GEMM_PROF
#ifdef CASV_GEMM_PROF_PLAIN
    if (EPI == EPI_PLAIN && KS == 1 && threadIdx.x == 0 && ptiles > 0) {
#else
    if (EPI == EPI_LSTM && KS == 1 && threadIdx.x == 0 && ptiles > 0) {
#endif
        const unsigned long long pt3 = __builtin_amdgcn_s_memtime();
        atomicAdd(&g_gemm_prof[0], pt1 - pt0); atomicAdd(&g_gemm_prof[1], pt2 - pt1); atomicAdd(&g_gemm_prof[2], (unsigned long long)ptiles);
        atomicAdd(&g_gemm_prof[3], pt3 - pt2); atomicAdd(&g_gemm_prof[4], pr2 - pr1); atomicAdd(&g_gemm_prof[5], 1ull);
        atomicAdd(&g_gemm_prof[6], pt3 - pt0);
        { unsigned long long bin = (pt3 - pt0) >> 14; atomicAdd(&g_gemm_prof[16 + (bin < 63 ? bin : 63)], 1ull); }
        atomicAdd(&g_gemm_prof[8], pa - pt0); atomicAdd(&g_gemm_prof[9], pb - pa); atomicAdd(&g_gemm_prof[10], pc - pb); atomicAdd(&g_gemm_prof[11], pt1 - pc);
        atomicAdd(&g_gemm_prof[12], pe - pt2); atomicAdd(&g_gemm_prof[13], pt3 - pe);
    }
#endif
}

template <int EPI, int KS, bool SPLIT = false, bool ACC = false>
__global__ __launch_bounds__(256 * KS, 2) void gemm_kernel(const GemmBatch batch) {
    extern __shared__ __attribute__((aligned(16))) float smem_all[];
    const GemmArgs& g = batch.g[blockIdx.y];
    const int nbn = (g.N + BN - 1) / BN;
    int bn = blockIdx.x % nbn, bm = blockIdx.x / nbn;
    if (g.xcd_rows > 0) {
        // Workgroups are dealt round-robin over the 8 XCDs (private L2s).  Give each XCD a compact block of the
        // tile grid so that an A row-panel / B column-panel is fetched into ONE L2 instead of all eight
        // (placement only changes speed, never results).
        const int xr = g.xcd_rows, xc = 8 / xr;
        const int nbm = (g.M + BM - 1) / BM;
        const int pr = nbm / xr, pc = nbn / xc;            // tiles per XCD along rows / columns (host checked divisibility)
        const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
        bm = (xcd / xc) * pr + local / pc;
        bn = (xcd % xc) * pc + local % pc;
    }
    gemm_tile<EPI, KS, SPLIT, ACC>(g, bm, bn, blockIdx.z, gridDim.z, smem_all);
}

static_assert(BM == gemm_shape::BM && BN == gemm_shape::BN && BK == gemm_shape::BK, "gemm_plan.h plans these tiles");
static_assert(GEMM_LDS_BYTES == gemm_shape::LDS_FP32 && 2 * SPLIT_BUF_FLOATS * 4 == gemm_shape::LDS_SPLIT128 && CELL_LDS_BYTES + STASH_LDS_BYTES == gemm_shape::LDS_EPILOGUE, "gemm_plan.h plans these LDS sizes");

// The switches of the launchers: the environment is read here, once, when the library is loaded; options "tile" and "split_bf16"
// of casv_set_option act on the same object (gemm_plan.h: GemmSwitches).
static GemmSwitches gemm_switches_from_env() {
    GemmSwitches s;
    auto digit = [](const char* name, int hi, int otherwise) { const char* e = getenv(name); return e && e[0] >= '0' && e[0] <= '0' + hi && !e[1] ? e[0] - '0' : otherwise; };
    auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    s.tile_mode = digit("CASV_GEMM_TILE", 2, -1);
    s.split_override = digit("CASV_SPLIT_BF16", 2, -1);
    s.tail_cut = !off("CASV_TAIL_CUT");
    s.split_tail_cut = !off("CASV_SPLIT_TAIL_CUT");
    s.tn_split = !off("CASV_TN_SPLIT");
    s.split_images = !off("CASV_SPLIT_IMAGES");
    { const char* e = getenv("CASV_DEBUG_LDS_PAD"); s.lds_pad = e ? atoi(e) : 0; }
    return s;
}
static GemmSwitches g_switches = gemm_switches_from_env();
const GemmSwitches& gemm_switches() { return g_switches; }
void set_gemm_tile_mode(int mode) { g_switches.tile_mode = mode; }
long gemm_split_epoch() { return g_switches.epoch; }
void gemm_split_bump_epoch() { ++g_switches.epoch; }
void set_gemm_split_override(int v) { v = v < -1 ? -1 : v > 2 ? 2 : v; if (v != g_switches.split_override) ++g_switches.epoch; g_switches.split_override = v; }
int gemm_split_override() { return g_switches.split_override; }

template <int EPI, int KS, bool SPLIT = false, bool ACC = false>
static void launch_one(const GemmLaunchPlan& l, hipStream_t stream) {
    static LdsAttribute attr;
    (void)gemm_dynamic_lds(attr, reinterpret_cast<const void*>(&gemm_kernel<EPI, KS, SPLIT, ACC>), l.lds_bytes);
    hipLaunchKernelGGL((gemm_kernel<EPI, KS, SPLIT, ACC>), dim3(l.grid_x, l.grid_y, l.grid_z), dim3(l.block), l.lds_bytes, stream, l.batch);
}

// Runs a plan: per launch the clears, then the kernel of its form.
static void run_launches(int epi, const GemmPlan& plan, hipStream_t stream) {
    if (!gemm_plan_takes_acc_in(plan)) {        // (a host-side bug: the callers set the field only behind this very question)
        fprintf(stderr, "cor_asv_ann_hip: a GEMM job with acc_in was planned for a launch form without it\n");
        abort();
    }
    for (int i = 0; i < plan.count; ++i) {
        const GemmLaunchPlan& l = plan.launch[i];
        for (int j = 0; j < l.batch.count; ++j) {
            if (!(l.clear_jobs >> j & 1)) continue;
            // the slot to clear is computed from the immediate step: split-K jobs never take their step from device memory
            // (the planner keeps ksplit at 1 for them)
            const GemmArgs& g = l.batch.g[j];
            gemm_clear(g.out.base + (long long)(g.step_imm * g.out.step_mul + g.out.step_add) * g.out.slot_stride, g.M, g.N, g.out.ld, stream);
        }
        const bool lstm = epi == EPI_LSTM, two = l.form == FORM_FP32_128_2WG;
        if (l.form == FORM_SKINNY_32 || l.form == FORM_SKINNY_64) run_gemm_skinny(epi, l, stream);
        else if (l.form == FORM_SPLIT_256) run_gemm_split256(epi, l, stream);
        else if (l.form == FORM_SPLIT_128) {
            bool acc = false;           // (a launch with a job that carries acc_in: the variant that reads it)
            for (int j = 0; j < l.batch.count; ++j) acc = acc || l.batch.g[j].acc_in.base;
            if (acc) { if (lstm) launch_one<EPI_LSTM, 1, true, true>(l, stream); else launch_one<EPI_PLAIN, 1, true, true>(l, stream); }
            else if (lstm) launch_one<EPI_LSTM, 1, true>(l, stream); else launch_one<EPI_PLAIN, 1, true>(l, stream);
        }
        else if (lstm) { if (two) launch_one<EPI_LSTM, 2>(l, stream); else launch_one<EPI_LSTM, 1>(l, stream); }
        else { if (two) launch_one<EPI_PLAIN, 2>(l, stream); else launch_one<EPI_PLAIN, 1>(l, stream); }
    }
}

GemmPlan run_gemm_plan(const GemmContext& ctx, int epi, const GemmBatch& b, const GemmPlan& plan, hipStream_t stream) {
    for (int i = 0; i < plan.count; ++i)
        if (plan.launch[i].form == FORM_SPLIT_256 && !gemm_split256_ready()) {
            // (the 256x256 kernels cannot get their LDS: the whole batch as 128x128 split tiles, the same bits)
            GemmContext small = ctx;
            small.arithmetic = 1;
            const GemmPlan instead = plan_gemm_launches(small, g_switches, epi, b);
            run_launches(epi, instead, stream);
            return instead;
        }
    run_launches(epi, plan, stream);
    return plan;
}

void launch_gemm_batch(const GemmContext& ctx, int epi, const GemmBatch& b, hipStream_t stream) {
    (void)run_gemm_plan(ctx, epi, b, plan_gemm_launches(ctx, g_switches, epi, b), stream);
}

void launch_gemm(const GemmContext& ctx, int epi, const GemmArgs& g, hipStream_t stream) {
    GemmBatch b;
    b.g[0] = g;
    b.count = 1;
    launch_gemm_batch(ctx, epi, b, stream);
}

}  // namespace casv
