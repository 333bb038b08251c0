// Which kernels a GEMM launch becomes: the decision as a pure function of (shapes, CU count, arithmetic, switches).
//
// plan_gemm_launches() gives the ordered, flat list of launches a batch of forward contractions turns into (gemm.hip,
// gemm_skinny.hip, gemm_split.hip run it); plan_gemm_tn() the launch of one K-major weight-gradient contraction (gemm_tn.hip,
// gemm_tn_split.hip).  Nothing here calls the device, reads the environment or keeps state: the CU count and the arithmetic come
// from the handle (GemmContext), the switches from the caller (the process-wide object of gemm.hip, or a test's own).  Needs only
// gemm_args.h and the standard library, so a plain host compiler builds it (tests/test_gemm_plan.py pins the decisions on the CPU).
#pragma once
#include "gemm_args.h"
#include <algorithm>

namespace casv {

// What the launchers need to know about their caller: the CU count of the handle's device, the arithmetic of the entry point that
// enqueues the launch (0 = the fp32-input matrix instruction's k-ordered fmaf chain, 1 / 2 = bf16x3-split
// operands on the bf16 matrix instruction -- 1: 128x128 tiles, 2: 256x256 tiles where a job fills the chip that way, else as 1; both
// give the same bits), and ordered sums (the train step's "deterministic" option, DESIGN.md section 7: while set, no launch splits
// K over workgroups -- every element is ONE k-ordered chain, nothing is added atomically, whatever the shape asks for).
struct GemmContext { int ncu; int arithmetic; int ordered; };
inline int gemm_ncu(const GemmContext& c) { return c.ncu > 0 ? c.ncu : 256; }

// The switches of the launchers: read from the environment once, when the library is loaded (gemm.hip,
// gemm_switches_from_env), into one process-wide object that casv_set_option's "tile" and "split_bf16" act on.
struct GemmSwitches {
    int tile_mode = -1;             // CASV_GEMM_TILE / option "tile": -1 by size, 0 = 128x128, 1 = 32x128, 2 = 64x128 where possible
    bool tail_cut = true;           // CASV_TAIL_CUT=0 switches the cut of a partial last round off (A/B measurements)
    bool split_tail_cut = true;     // CASV_SPLIT_TAIL_CUT=0: split-arithmetic launches keep one tile shape
    bool tn_split = true;           // CASV_TN_SPLIT=0: the K-major weight gradients stay on the fp32-input kernel
    bool split_images = true;       // CASV_SPLIT_IMAGES=0: no pre-split weight images
    int lds_pad = 0;                // CASV_DEBUG_LDS_PAD: measurement aid -- extra dynamic LDS, e.g. 16384 leaves room for ONE workgroup per CU
    // The process-wide override (option "split_bf16" / CASV_SPLIT_BF16 = 0, 1 or 2 in the environment when the library is loaded)
    // puts EVERY launch of the decode path of every handle on one arithmetic: tests and A/B measurements.
    int split_override = -1;
    // (a captured step graph bakes in the arithmetic and the addresses of the pre-split weight images: both are part of its key through
    // this counter -- decode.hip, StepRunner)
    long epoch = 0;
};

// Tile geometry and dynamic-LDS sizes of the kernels (gemm.hip, gemm_split.hip and gemm_tn_split.hip assert that theirs agree)
namespace gemm_shape {
constexpr int BM = 128, BN = 128, BK = 16;
constexpr int LDS_EPILOGUE = 128 * 128 + 256 * 6 * 8;               // cell-state image + parked row pointers behind the tile buffers
constexpr int LDS_FP32 = 2 * 2 * (128 * (BK + 4)) * 4;              // per wave group: two buffers of an A and a B tile, 80-byte rows
constexpr int LDS_SPLIT128 = 2 * 6 * (128 * 32);                    // two buffers of three bf16 planes per operand
constexpr int S2_BM = 256, S2_BN = 256, S2_BK = 16;
constexpr int LDS_SPLIT256 = 8 * 64 * 128 + 2 * 6 * (256 * 32);     // [cell state | tile buffer 0 | tile buffer 1]
constexpr int TN_BM = 128, TN_BN = 128, TN_BK = 16;
constexpr int TS_BM = 256, TS_BN = 256, TS_BK = 16;
constexpr int LDS_TN_SPLIT = 2 * 6 * (256 * 32);                    // 96 KB
}

enum GemmForm {
    FORM_FP32_128 = 0,      // 128x128 tiles, fp32-input instruction (gemm.hip)
    FORM_FP32_128_2WG,      // the same with two wave groups per workgroup: a deterministic split-K inside the workgroup (train step)
    FORM_SPLIT_128,         // 128x128 tiles, bf16x3-split operands (gemm.hip, SPLIT)
    FORM_SKINNY_32,         // 32x128 tiles (gemm_skinny.hip)
    FORM_SKINNY_64,         // 64x128 tiles (gemm_skinny.hip, two row blocks per workgroup)
    FORM_SPLIT_256,         // 256x256 tiles, bf16x3-split operands (gemm_split.hip)
    FORM_COUNT
};

// One launch: the kernel form, its grid (x = tiles of the largest job, y = jobs, z = K splits), block size and dynamic LDS, and the
// batch it is launched with -- which already carries the XCD tile order, the rows, split and epilogue of cut jobs and their offset
// pointers.  clear_jobs: bit j = job j's output is cleared first (partial sums are added atomically: start from zero).
// FORM_SPLIT_256: want_image = every job of the launch can take a pre-split weight image (static weights, K in whole tiles);
// image_jobs = how many of them, from the front, are asked for one (fetching them stays with the executor: a missing image turns
// the launch into the staging variant, same values).
struct GemmLaunchPlan {
    int form;
    int grid_x, grid_y, grid_z, block, lds_bytes;
    unsigned clear_jobs;
    int want_image, image_jobs;
    GemmBatch batch;
};
// (a batch under arithmetic 2 is at most: whole rounds as 256x256, a tail that re-qualifies, its ragged rest, and the 128x128 launch
// of what is left; the cut of a partial round makes two)
constexpr int GEMM_PLAN_MAX = 6;
struct GemmPlan {
    int count;
    GemmLaunchPlan launch[GEMM_PLAN_MAX];
};

inline int gemm_count_ktiles(const GemmArgs& g) {
    int ktiles = 0;
    for (int i = 0; i < g.nseg; ++i) ktiles += g.a[i].width / gemm_shape::BK;
    return ktiles;
}

// Tile shape and split-K factor of a launch.  Launches that would occupy at most half the CUs as 128x128 tiles (even
// after split-K) run as 32x128 tiles: 4x the workgroups, same values ...
struct GemmTiles { int blocks, sblocks, ksplit; bool skinny; int srows; bool splittable; };
inline GemmTiles gemm_choose_tiles(const GemmContext& ctx, const GemmSwitches& sw, int epi, const GemmBatch& b) {
    using namespace gemm_shape;
    GemmTiles p{0, 0, 1, false, 32, false};
    for (int j = 0; j < b.count; ++j) {
        const int nbn = (b.g[j].N + BN - 1) / BN;
        const int nb = ((b.g[j].M + BM - 1) / BM) * nbn, ns = ((b.g[j].M + 31) / 32) * nbn;
        p.blocks = nb > p.blocks ? nb : p.blocks;
        p.sblocks = ns > p.sblocks ? ns : p.sblocks;
    }
    bool splittable = epi == EPI_PLAIN;         // split-K: every job of the batch must ask for it and share the shape
    for (int j = 0; j < b.count; ++j)
        if (b.g[j].step_ptr || b.g[j].ksplit == 0 || b.g[j].ksplit == 1 || b.g[j].ksplit != b.g[0].ksplit || b.g[j].Ktot != b.g[0].Ktot ||
            b.g[j].M != b.g[0].M || b.g[j].N != b.g[0].N) splittable = false;
    if (ctx.ordered) splittable = false;
    p.splittable = splittable;
    auto choose_ksplit = [&](int grid, int want) {
        if (!splittable) return 1;
        const int ktiles = gemm_count_ktiles(b.g[0]);
        int ks = b.g[0].ksplit;
        if (ks < 0) {                           // fill the chip, keep >= 16 k-tiles per workgroup
            ks = (want + grid - 1) / grid;
            if (ks > ktiles / 16) ks = ktiles / 16;
        }
        if (ks > ktiles) ks = ktiles;
        return ks < 1 ? 1 : ks;
    };
    p.ksplit = choose_ksplit(p.blocks * b.count, 512);
    // ... and so do launches of more than one but less than two 128x128 tiles per CU: half the CUs would carry two workgroups
    // and set the pace while the others idle (the encoder's anti-diagonals of three layers at 1024 lines: 384 tiles, 168 us;
    // as 1536 tiles of 32x128: 140 us)
    const int ncu = gemm_ncu(ctx);
    const int grid = p.blocks * b.count * p.ksplit;
    p.skinny = sw.tile_mode == 1 || (sw.tile_mode < 0 && (grid <= 128 || (grid > ncu && grid < 2 * ncu)));
    if (p.skinny) p.ksplit = choose_ksplit(p.sblocks * b.count, 1024);
    // Split-K launches of few rows (the train step's per-time-step data GEMMs: 512 rows, K = 2048): 32x128 tiles with just enough
    // K splits for ONE round of workgroups.  As 128x128 tiles they needed eight splits to fill the chip, and the eight partial
    // tiles per output went through float atomics -- 16.8 MB per launch at the memory side's ~1.3 TB/s = 13 of the launch's
    // 36 us.  Measured on the train step of configs[3] (splits 2 / 3 / 4 / 6 / 8 of 32x128 tiles: 90.2 / 91.8 / 87.9 / 89.9 /
    // 94.2 ms per step; 128x128 tiles with four splits 103.2; before 94.1).
    if (sw.tile_mode < 0 && splittable && b.g[0].ksplit < 0 && b.g[0].M <= 1024) {
        p.skinny = true;
        p.ksplit = choose_ksplit(p.sblocks * b.count, 512);
    }
    // 64 x 128 tiles (gemm_skinny.hip, two row blocks per workgroup) for launches without split-K that leave at most one 128x128
    // workgroup per CU, or go as 32-row tiles, while 64-row tiles still put two on every CU: the encoder at 1024 lines -- layer 1's
    // two directions (256 tiles of 128x128) and the anti-diagonals of the layers above (384)
    // (fused-LSTM launches only: the plain-epilogue launch it would also catch, the page call's logits -- 10240 x 640 x 512 --, runs
    // 67.6 us as 32-row tiles and 75.6 us as 64-row tiles)
    if ((epi == EPI_LSTM || sw.tile_mode == 2) && !splittable && p.ksplit == 1) {
        int blocks64 = 0;
        for (int j = 0; j < b.count; ++j) blocks64 = std::max(blocks64, ((b.g[j].M + 63) / 64) * ((b.g[j].N + BN - 1) / BN));
        const bool fits = blocks64 * b.count >= 2 * ncu;
        if (sw.tile_mode == 2 || (sw.tile_mode < 0 && fits && (p.skinny || grid < 2 * ncu))) { p.skinny = true; p.srows = 64; }
    }
    return p;
}
inline bool gemm_train_launch(const GemmBatch& b) {        // (the train step's fused-LSTM launches carry side outputs the decode path never has)
    for (int j = 0; j < b.count; ++j) if (b.g[j].zinit.base || b.g[j].gates_out.base || b.g[j].out2.base) return true;
    return false;
}
inline bool gemm_splittable_launch(int epi, const GemmBatch& b) {        // (a launch whose jobs ask for split-K: never re-planned below)
    if (epi != EPI_PLAIN) return false;
    for (int j = 0; j < b.count; ++j) if (b.g[j].ksplit != 0 && b.g[j].ksplit != 1) return true;
    return false;
}

// Train step's big plain contractions (GemmArgs.ksplit = -1: the caller leaves the launch form to the launcher; M = 51 712 rows):
// a 128x128 tile grid that ends in a partial round of workgroups -- 1 616 tiles on 512 slots = 3.16 rounds -- spends the time of
// most of a round on its last few tiles (a workgroup alone on its CU still needs ~2/3 of the time two of them share).  The row
// blocks of that partial round go as a second launch of 32-row (64-row) tiles instead: four (two) times the workgroups for the same
// rows, every element contracted by the same k-ordered chain (gemm_skinny.hip: same bits, no split-K, nothing atomic).
// CASV_TAIL_CUT=0 switches it off (A/B measurements).
// true: `main` holds the whole rounds (planned like any batch), `tail` the rest, to go as tiles of `tail_rows` rows.
inline bool gemm_cut_partial_round(const GemmContext& ctx, const GemmSwitches& sw, int epi, const GemmBatch& b, const GemmTiles& plan,
                                   GemmBatch& main, GemmBatch& tail, int& tail_rows) {
    using namespace gemm_shape;
    if (!sw.tail_cut || epi != EPI_PLAIN || b.count != 1 || plan.ksplit != 1 || plan.skinny || sw.tile_mode >= 0 || ctx.arithmetic) return false;
    const GemmArgs& g = b.g[0];
    if (g.ksplit != -1 || g.step_ptr || g.nact || g.Bimg) return false;
    for (int i = 0; i < g.nseg; ++i) if (g.a[i].rows || g.a[i].skip_first || g.a[i].first_base) return false;    // rows at base + m * ld only
    const int ncu = gemm_ncu(ctx);
    const int nbm = (g.M + BM - 1) / BM, nbn = (g.N + BN - 1) / BN, slots = 2 * ncu;
    const int tiles = nbm * nbn, rounds = tiles / slots, rem = tiles % slots;
    if (rounds < 1 || rem == 0 || rem * 4 > slots * 3) return false;         // (a last round that is three quarters full is left alone)
    const int main_bm = (rounds * slots) / nbn;
    if (main_bm < 1 || main_bm >= nbm) return false;
    main.count = tail.count = 1;
    GemmArgs& gm = main.g[0]; GemmArgs& gt = tail.g[0];
    gm = g; gt = g;
    gm.M = main_bm * BM; gm.ksplit = 0;                                      // (0: one block per tile, and no second look at this function)
    gt.M = g.M - gm.M; gt.ksplit = 0;
    for (int i = 0; i < g.nseg; ++i) gt.a[i].base += (long long)gm.M * g.a[i].ld;
    gt.out.base += (long long)gm.M * g.out.ld;
    const int tail_tiles = (nbm - main_bm) * nbn;
    tail_rows = tail_tiles * 4 <= 2 * slots ? 32 : 64;
    return true;
}

// Which jobs of a launch can go as 256x256 tiles: whole tiles only, inference outputs only (no gate / second-h / precomputed-term
// side channels of the train step), K segments in whole tiles.
inline bool gemm_split256_job_ok(int epi, const GemmArgs& g) {
    using namespace gemm_shape;
    if (g.M <= 0 || g.M % S2_BM || g.N % S2_BN || g.nseg < 1) return false;
    if (g.accumulate || g.ksplit > 1 || g.zinit.base || g.gates_out.base || g.out2.base) return false;
    for (int i = 0; i < g.nseg; ++i) if (g.a[i].width % S2_BK || g.a[i].koff % 4 || g.a[i].ld % 4) return false;
    if (g.Ktot % 4) return false;
    if (epi == EPI_LSTM && !g.epi_plain && (!g.c_out.base || !g.c_in.base)) return false;
    return true;
}
inline bool gemm_split256_wants(int epi, const GemmArgs& g) {
    using namespace gemm_shape;
    return gemm_split256_job_ok(epi, g) && (g.M / S2_BM) * (g.N / S2_BN) >= 128;      // fewer tiles: the smaller tile shapes do better
}

// Split arithmetic, 256x256 tiles (gemm_split.hip: ONE workgroup per CU): a grid of more than one round of workgroups that ends in
// a partial round -- the page call's 10 240 rows x 2048 gate columns = 320 tiles on 256 CUs: the second round occupies a quarter
// of the chip for the time of a whole one -- keeps its whole rounds; the rows of the partial round (and a ragged last row block)
// go as 128x128 split tiles, which contract every element with the same instruction sequence (same bits: tests/test_gpu_split.py).
// The tail job addresses its rows through offset pointers (no kernel knows about the cut).  false: the job stays as it is.
inline bool gemm_split256_cut_rows(const GemmContext& ctx, const GemmSwitches& sw, const GemmArgs& g, GemmArgs& head, GemmArgs& tail) {
    const int ncu = gemm_ncu(ctx);
    if (!sw.split_tail_cut || g.N <= 0 || g.N % 256 || g.M < 256) return false;
    const int nbn = g.N / 256, nbm = g.M / 256, tiles = nbm * nbn;
    const int rounds = tiles / ncu, rem = tiles % ncu;
    int main_bm;
    if (rounds >= 1 && rem > 0 && rem * 4 <= ncu * 3) main_bm = (rounds * ncu) / nbn;      // (a last round that is three quarters full is left alone)
    else if (g.M % 256) main_bm = nbm;                                                      // ragged last row block only
    else return false;
    if (main_bm < 1 || (long long)main_bm * 256 >= g.M) return false;
    const int m_off = main_bm * 256;
    if (g.nact && (g.nact_group <= 0 || m_off % g.nact_group)) return false;
    head = g; tail = g;
    head.M = m_off; tail.M = g.M - m_off;
    auto shift = [&](Seg& sg) {
        if (!sg.base && !sg.first_base) return;
        if (sg.rows) sg.rows += m_off; else if (sg.base) sg.base += (long long)m_off * sg.ld;
        if (sg.first_base) sg.first_base += (long long)m_off * sg.ld;
    };
    for (int i = 0; i < g.nseg; ++i) shift(tail.a[i]);
    shift(tail.c_in);
    shift(tail.acc_in);         // (moves with its rows like every input; a plan that pairs it with a 256x256 launch is refused all the same)
    for (SlotPtr* sp : {&tail.out, &tail.c_out, &tail.zinit, &tail.gates_out, &tail.out2})
        if (sp->base) sp->base += (long long)m_off * sp->ld;
    if (g.nact) tail.nact += m_off / g.nact_group;
    return true;
}

// XCD-aware tile order of every job of a launch of tile x tile blocks: minimise (A bytes x column-splits + B bytes x row-splits)
// over the 8 = xr * xc splits.  Returns the launch's grid width, the tiles of its largest job.
inline int gemm_set_xcd_order(GemmBatch& bb, int tile) {
    int blocks = 0;
    for (int j = 0; j < bb.count; ++j)
        blocks = std::max(blocks, ((bb.g[j].M + tile - 1) / tile) * ((bb.g[j].N + tile - 1) / tile));
    for (int j = 0; j < bb.count; ++j) {
        GemmArgs& g = bb.g[j];
        const int nbm = (g.M + tile - 1) / tile, nbn = (g.N + tile - 1) / tile;
        g.xcd_rows = 0;
        if ((nbm * nbn) % 8 != 0 || nbm * nbn != blocks) continue;
        double best = 0; int best_xr = 0;
        for (int xr = 1; xr <= 8; xr *= 2) {
            const int xc = 8 / xr;
            if (nbm % xr || nbn % xc) continue;
            const double cost = (double)g.M * xc + (double)g.N * xr;     // both operands share K
            if (!best_xr || cost < best) { best = cost; best_xr = xr; }
        }
        g.xcd_rows = best_xr;
    }
    return blocks;
}

inline GemmLaunchPlan& gemm_plan_add(GemmPlan& plan, int form, int gx, int gy, int gz, int block, int lds, const GemmBatch& b) {
    GemmLaunchPlan& l = plan.launch[plan.count++];
    l.form = form; l.grid_x = gx; l.grid_y = gy; l.grid_z = gz; l.block = block; l.lds_bytes = lds;
    l.clear_jobs = 0; l.want_image = 0; l.image_jobs = 0;
    l.batch = b;
    return l;
}
inline GemmLaunchPlan& gemm_plan_add_skinny(GemmPlan& plan, const GemmBatch& b, int ksplit, int rows) {      // rows = 32 or 64 per tile
    int blocks = 0;
    for (int j = 0; j < b.count; ++j) {
        const int nb = ((b.g[j].M + rows - 1) / rows) * ((b.g[j].N + gemm_shape::BN - 1) / gemm_shape::BN);
        blocks = nb > blocks ? nb : blocks;
    }
    return gemm_plan_add(plan, rows == 64 ? FORM_SKINNY_64 : FORM_SKINNY_32, blocks, b.count, ksplit, 256, 0, b);
}

// The launches of one batch, in order.  (A loop, not a recursion: `cur` is the batch still to be decided -- the caller's, then the
// whole rounds of a cut batch or what is left behind a 256x256 launch, kept in `next`.)
inline GemmPlan plan_gemm_launches(const GemmContext& ctx, const GemmSwitches& sw, int epi, const GemmBatch& batch) {
    using namespace gemm_shape;
    GemmPlan plan;
    plan.count = 0;
    const GemmBatch* cur = &batch;
    GemmBatch next, cut_tail;
    int cut_tail_rows = 0;
    const int arithmetic = ctx.arithmetic;
    for (;;) {
        const GemmBatch& b = *cur;
        const GemmTiles tiles = gemm_choose_tiles(ctx, sw, epi, b);
        // (only the caller's batch can be cut: what follows a cut has ksplit 0, what follows a 256x256 launch a split arithmetic)
        if (cur == &batch && gemm_cut_partial_round(ctx, sw, epi, b, tiles, next, cut_tail, cut_tail_rows)) { cur = &next; continue; }
        const int blocks = tiles.blocks, ksplit = tiles.ksplit;
        bool skinny = tiles.skinny;
        // split-bf16 experiment: a launch that would go as 64- or 32-row tiles only because 128x128 tiles leave CUs idle (the
        // encoder's cells at 1024 lines: 256 / 384 tiles; the attention-query job) runs faster as 128x128 tiles on the bf16
        // instruction, one workgroup per CU, than as small tiles on the fp32-input one (c3: 190.9 -> 178 ms per batch)
        // ... and every other inference launch too, whatever tile shape was asked for: with the option on, all GEMM launches of the
        // decode path share ONE arithmetic (128x128 and 256x256 split tiles give the same bits), so that a row's result does not depend
        // on the batch it sits in -- the property the fp32-input kernels have among themselves.  (The train step's per-time-step launches
        // keep the fp32-input small tiles: its persistent recurrences, which they must equal, are fp32-input kernels.)
        if (arithmetic && skinny && ksplit == 1 && !gemm_splittable_launch(epi, b) && !gemm_train_launch(b)) skinny = false;
        unsigned clear_jobs = 0;
        for (int j = 0; j < b.count && ksplit > 1; ++j)
            if (!(b.g[j].accumulate || b.g[j].out_zeroed)) clear_jobs |= 1u << j;   // partial sums are added atomically: start from zero
        if (skinny) {
            GemmLaunchPlan& l = gemm_plan_add_skinny(plan, b, ksplit, tiles.srows);
            gemm_set_xcd_order(l.batch, BM);        // (the tile order of the 128x128 grid, as every launch of a batch gets it)
            l.clear_jobs = clear_jobs;
            break;
        }
        // wave-group split-K (train step only, GemmArgs.kgroups): worth it while the grid leaves CUs idle
        bool two = true;
        for (int j = 0; j < b.count; ++j)
            if (b.g[j].kgroups != 2 || gemm_count_ktiles(b.g[j]) / ksplit < 16) two = false;
        if (blocks * b.count * ksplit > 256) two = false;
        if (arithmetic && !two) {
            // (no room for another 256x256 launch and what follows it: the batch goes whole as 128x128 split tiles, the same bits)
            if (arithmetic >= 2 && ksplit == 1 && plan.count + 2 <= GEMM_PLAN_MAX - (cut_tail_rows ? 1 : 0)) {
                // jobs that fill the chip as 256x256 tiles go to gemm_split.hip; the rest of the batch follows as a launch of its own
                GemmBatch big{}, rest{};
                for (int j = 0; j < b.count; ++j) {
                    GemmArgs head = b.g[j], tail{};
                    // (a job whose 256x256 grid ends in a partial round of workgroups, or in a ragged row block: whole rounds here, the
                    // remaining rows as 128x128 split tiles -- the same bits -- in the launch of the rest)
                    const bool cut = gemm_split256_cut_rows(ctx, sw, b.g[j], head, tail);
                    if (gemm_split256_wants(epi, head)) {
                        big.g[big.count++] = head;
                        if (cut && rest.count < GEMM_MAX_JOBS) { rest.g[rest.count++] = tail; continue; }
                        if (cut) { big.g[big.count - 1] = b.g[j]; }      // (no room for the tail job: the job stays whole)
                        continue;
                    }
                    rest.g[rest.count] = b.g[j]; if (epi == EPI_PLAIN) rest.g[rest.count].epi_plain = 0; ++rest.count;
                }
                bool ok = big.count > 0;
                for (int j = 0; j < big.count; ++j) ok = ok && gemm_split256_job_ok(epi, big.g[j]);
                if (ok) {
                    const int blocks256 = gemm_set_xcd_order(big, S2_BM);
                    GemmLaunchPlan& l = gemm_plan_add(plan, FORM_SPLIT_256, blocks256, big.count, 1, 512, LDS_SPLIT256, big);
                    // weight images: every job of the launch must have one (static weights, K in whole tiles)
                    bool bimg = sw.split_images;
                    for (int j = 0; j < big.count && bimg; ++j) bimg = big.g[j].b_static && big.g[j].Ktot % S2_BK == 0;
                    for (int j = 0; j < big.count && bimg; ++j) {
                        for (int i = 0; i < big.g[j].nseg; ++i) if (big.g[j].a[i].koff % S2_BK) bimg = false;
                        if (bimg) ++l.image_jobs;
                    }
                    l.want_image = bimg;
                    if (!rest.count) break;
                    next = rest;
                    cur = &next;
                    continue;
                }
            }
            GemmLaunchPlan& l = gemm_plan_add(plan, FORM_SPLIT_128, blocks, b.count, ksplit, 256, LDS_SPLIT128 + LDS_EPILOGUE + sw.lds_pad, b);
            gemm_set_xcd_order(l.batch, BM);
            l.clear_jobs = clear_jobs;
            break;
        }
        GemmLaunchPlan& l = gemm_plan_add(plan, two ? FORM_FP32_128_2WG : FORM_FP32_128, blocks, b.count, ksplit, two ? 512 : 256,
                                          LDS_FP32 * (two ? 2 : 1) + LDS_EPILOGUE + sw.lds_pad, b);
        gemm_set_xcd_order(l.batch, BM);
        l.clear_jobs = clear_jobs;
        break;
    }
    if (cut_tail_rows) gemm_plan_add_skinny(plan, cut_tail, 1, cut_tail_rows);
    return plan;
}
// GemmArgs.acc_in is honoured by the 128x128 split tiles alone (one block per tile).  The field takes no part in any decision above;
// a caller that wants to set it plans its batch first and asks here whether every launch that would carry it has that form -- the
// launchers refuse a plan that fails this.
inline bool gemm_plan_takes_acc_in(const GemmPlan& p) {
    for (int i = 0; i < p.count; ++i) {
        const GemmLaunchPlan& l = p.launch[i];
        for (int j = 0; j < l.batch.count; ++j)
            if (l.batch.g[j].acc_in.base && (l.form != FORM_SPLIT_128 || l.grid_z != 1)) return false;
    }
    return true;
}
// (which tile shape a batch starts with: the profile class of a fused-LSTM launch, engine.h)
inline bool gemm_plan_is_skinny(const GemmPlan& p) { return p.count > 0 && (p.launch[0].form == FORM_SKINNY_32 || p.launch[0].form == FORM_SKINNY_64); }

// ---- K-major weight gradients (gemm_tn.hip, gemm_tn_split.hip) ----
enum TnKernel {
    TN_FP32 = 0,            // 128x128 tiles, fp32-input instruction; K shares add into C atomically
    TN_SPLIT,               // 256x256 tiles, bf16x3-split operands; the same epilogue
    TN_FP32_PART,           // ordered form: every K share stores its partial tile, a second launch adds them in share order
    TN_SPLIT_PART,
    TN_KERNEL_COUNT
};
struct TnPlan {
    int kernel;
    int shares, nonempty;   // K shares launched; shares that hold k-tiles at all (the last share may be partly filled)
    int grid, block, lds_bytes;
    int clear;              // C is cleared first (`accumulate` = 0 with a split K needs a cleared C: the caller says so -- out_zeroed -- or gets a memset)
    int reduce_grid;        // ordered form: grid of the launch that adds the shares; else 0
};
// K shares of a weight-gradient launch: `fill` shares would fill the chip; keep >= 64 k-tiles per workgroup so that the atomic
// epilogue stays a small part
inline int gemm_tn_shares(int fill, int ktiles) {
    int ks = fill;
    if (ks > ktiles / 64) ks = ktiles / 64;
    return ks < 1 ? 1 : ks;
}
// The launch of one contraction.  ordered: the train step's "deterministic" form -- K shares chosen from the shape alone (a chip of
// 256 CUs / 512 workgroup slots whatever the device has, so that the partition -- and with it every bit of the result -- follows
// from the shape), each share's partial stored, then added in share order: no float atomics.  Else under the context's arithmetic
// the split kernel where the shape has that form on this device's CUs, else the fp32-input kernel.
inline TnPlan plan_gemm_tn(const GemmContext& ctx, const GemmSwitches& sw, const TnArgs& g, bool ordered) {
    using namespace gemm_shape;
    TnPlan p{};
    const int chip = ordered ? 256 : gemm_ncu(ctx);
    bool split = ctx.arithmetic && sw.tn_split && g.M > 0 && g.N > 0 && g.M % TS_BM == 0 && g.N % TS_BN == 0 && g.K >= 64 * TS_BK &&
                 g.K % TS_BK == 0 && g.Mstore > 0 && g.Mstore <= g.M;
    int tiles = 0, ktiles = 0;
    if (split) {
        tiles = (g.M / TS_BM) * (g.N / TS_BN); ktiles = g.K / TS_BK;
        // one workgroup per CU: fill the chip
        p.shares = gemm_tn_shares(chip / tiles, ktiles);
        if (tiles * p.shares < chip / 2) split = false;      // (too few workgroups for this tile shape: the fp32-input kernel's 128x128 tiles fill the chip better)
    }
    if (!split) {
        tiles = ((g.M + TN_BM - 1) / TN_BM) * ((g.N + TN_BN - 1) / TN_BN); ktiles = (g.K + TN_BK - 1) / TN_BK;
        // fill the chip (512 workgroup slots)
        p.shares = gemm_tn_shares((512 + tiles - 1) / tiles, ktiles);
    }
    const int per = (ktiles + p.shares - 1) / p.shares;
    p.nonempty = per > 0 ? (ktiles + per - 1) / per : 1;
    p.kernel = ordered ? (split ? TN_SPLIT_PART : TN_FP32_PART) : (split ? TN_SPLIT : TN_FP32);
    p.grid = tiles * p.shares;
    p.block = split ? 512 : 256;
    p.lds_bytes = split ? LDS_TN_SPLIT : 0;
    p.clear = !ordered && p.shares > 1 && !g.accumulate && !g.out_zeroed;
    const long long mn = (long long)g.Mstore * g.N;
    p.reduce_grid = ordered ? (int)std::min<long long>((mn + 255) / 256, 2048) : 0;
    return p;
}
// floats of the ordered form's workspace: per share that holds k-tiles a partial tile [Mstore][N] and its column sums [Mstore]
inline size_t gemm_tn_plan_floats(const TnPlan& p, const TnArgs& g) { return (size_t)p.nonempty * g.Mstore * ((size_t)g.N + 1); }

}  // namespace casv
