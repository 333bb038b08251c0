// The plan of the train step's persistent launches -- the forward and backward recurrences of up to two plain layers
// (train_persist.hip, train_persist_bwd.hip), the attention cell (train_persist_top.hip) and its backward (train_persist_topb.hip) --
// as pure functions of the shape, the device's CU count, the workgroups per CU the runtime admits for the kernel (the kernel
// files ask for it, train.hip hands it in), the options and the launches the step has taken so far.  Nothing here knows the device
// or the environment: a stand-alone driver (tests/train_plan_driver.cpp) plans the case table of tests/train_form_cases.py on the CPU.
// Every number and rule of these forms is here and nowhere else; the kernel files' dispatch is generated from the width lists
// below, so a width has a plan exactly where it has a kernel.  train.hip launches what TrainStepPlan::next returns.
#pragma once
#include <algorithm>
#include <cstddef>

namespace casv {

enum TrainKind { TRAIN_REC = 0, TRAIN_REC_BWD, TRAIN_CELL, TRAIN_CELL_BWD, TRAIN_KINDS };

constexpr int TRAIN_ROW_BLOCK = 32;                 // rows of a row block: BM of train_tile.h, the four kernel files' tile
constexpr int TRAIN_LAUNCH_CAP = 16;                // persistent launches of one step: the slots of rec_cnt, the words of rec_abort
constexpr int TRAIN_MIN_CUS = 64;                   // below: no persistent launch of the train step
// per kind: the workgroups per CU the form plans for (the kernels' launch bounds; the cell kinds one: the idle waves of a part
// leave room) and the hand-off counters per row block
constexpr int TRAIN_BLOCKS_PER_CU[TRAIN_KINDS] = {2, 2, 1, 1};
constexpr int TRAIN_COUNTERS_PER_ROW_BLOCK[TRAIN_KINDS] = {2, 16, 3, 12};
// The widths NT = W / 32 that have an instantiation.  (Wider recurrences: the rows of h no longer fit a thread's registers; the
// backward kernels take whole column tiles of 128 units; the cell kinds' unit groups must divide the 32 rows of a row block.)
#define CASV_TRAIN_REC_WIDTHS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#define CASV_TRAIN_REC_BWD_WIDTHS(X) X(4) X(8) X(12) X(16)
#define CASV_TRAIN_CELL_WIDTHS(X) X(4) X(8) X(16)
#define CASV_TRAIN_CELL_BWD_WIDTHS(X) X(4) X(8) X(16)
// The attention backward's deferred sums hold a sample's T positions in LDS (train_kernels.hip: attention_deferred_*_kernel)
constexpr int ATTN_DEFER_MAX_T = 288;

// NT of a width, 0 where W is no multiple of 32: the switch value of every dispatch generated from the lists
inline int train_width_nt(int W) { return W > 0 && W % 32 == 0 ? W / 32 : 0; }
inline bool train_has_width(TrainKind kind, int nt) {
#define CASV_TRAIN_HAS(NT_) case NT_:
    switch (kind) {
        case TRAIN_REC: switch (nt) { CASV_TRAIN_REC_WIDTHS(CASV_TRAIN_HAS) return true; default: return false; }
        case TRAIN_REC_BWD: switch (nt) { CASV_TRAIN_REC_BWD_WIDTHS(CASV_TRAIN_HAS) return true; default: return false; }
        case TRAIN_CELL: switch (nt) { CASV_TRAIN_CELL_WIDTHS(CASV_TRAIN_HAS) return true; default: return false; }
        case TRAIN_CELL_BWD: switch (nt) { CASV_TRAIN_CELL_BWD_WIDTHS(CASV_TRAIN_HAS) return true; default: return false; }
        default: return false;
    }
#undef CASV_TRAIN_HAS
}

// ---- hand-off counters ----
// A launch's counters (persist_host.h's layout: 32 words per counter, then 32 words the first of which is the give-up word) ...
inline int train_row_blocks(int B) { return (B + TRAIN_ROW_BLOCK - 1) / TRAIN_ROW_BLOCK; }
inline size_t train_counter_bytes(TrainKind kind, int B) {
    return ((size_t)TRAIN_COUNTERS_PER_ROW_BLOCK[kind] * train_row_blocks(B) * 32 + 32) * sizeof(unsigned);
}
// ... and the slot of rec_cnt a launch takes: of one size whatever its kind, the largest of the four (the backward recurrence's) --
// for the addresses, the allocation and the clear.  The give-up word sits inside the slot at the end of the KIND'S OWN counters.
inline size_t train_slot_bytes(int B) {
    size_t n = 0;
    for (int k = 0; k < TRAIN_KINDS; ++k) n = std::max(n, train_counter_bytes((TrainKind)k, B));
    return n;
}

// ---- the shape rule ----
// B: the rows of the launch (a job with fewer rows, the encoder's of a candidates call, plans as B: grid and counters are B's);
// U: the steps of a cell kind (the recurrences' lengths decide nothing); jobs: the layers of a recurrence's launch.
struct TrainShape { int W, C, B, U, jobs; };
// Workgroups of the launch, all resident at once (they wait for each other), or 0: the shape has no persistent form on `ncu` CUs.
// per_cu: the runtime's workgroups per CU for the kind's kernel at this width, at most TRAIN_BLOCKS_PER_CU (0: the query failed).
inline int train_form_grid(TrainKind kind, const TrainShape& s, int ncu, int per_cu) {
    const bool cell = kind == TRAIN_CELL || kind == TRAIN_CELL_BWD;
    if (s.B < 1 || !train_has_width(kind, train_width_nt(s.W))) return 0;
    if (cell ? s.W != s.C || s.U < 1 : s.jobs < 1 || s.jobs > 2) return 0;           // (the cell: context as wide as the layer, i.e. depth >= 2)
    if ((kind == TRAIN_REC_BWD || kind == TRAIN_CELL_BWD) && s.W % 128) return 0;   // whole column tiles of 128 units
    if (kind == TRAIN_CELL_BWD && s.C > 1024) return 0;
    const int grid = (cell ? 1 : s.jobs) * train_row_blocks(s.B) * train_width_nt(s.W);
    return grid <= per_cu * ncu ? grid : 0;
}

// ---- one step ----
// What every site of a step shares: the option "persistent" (0: never), "deterministic", a back-off pending after a give-up, the CUs.
struct TrainGate { int persistent; bool deterministic, backoff; int ncu; };
inline bool train_gate_open(const TrainGate& g) { return g.persistent != 0 && !g.deterministic && !g.backoff && g.ncu >= TRAIN_MIN_CUS; }
// CASV_ATTN_DEFER (0, 1 or 3: what the cell's backward sums behind the recurrence instead of by atomics inside it) and
// CASV_TOPB_SPLIT with the serialised-dispatch rule applied (the attention backward of the samples as a launch of its own)
struct TrainSwitches { int defer; bool split; };
struct TrainSite {
    TrainKind kind; TrainShape shape;
    int per_cu;                 // train_form_grid's
    bool plain;                 // the site's own condition -- rec_bwd: every job's kr == W; cell: the outputs dense (hs_ld == W)
    // cell_bwd only: the encoder's steps, the switches, a step gave up in the two-launch form, both launches fit a CU together
    int T; TrainSwitches sw; bool split_off, rows_fit;
};
struct TrainLaunch {
    bool persistent = false;    // the site takes its persistent launch
    bool capped = false;        // it has a form but comes behind the TRAIN_LAUNCH_CAP-th launch
    int grid = 0, nt = 0;       // of the form, where the gate is open and the shape has one
    int slot = 0; size_t slot_offset = 0;   // its slot of rec_cnt
    size_t counter_bytes = 0;   // its kind's counters: the give-up word sits behind them
    int defer = 0, split_a = 0; // cell_bwd: the deferred sums (bits: 1 = d_enc, 2 = du), the two-launch form
};
// The launches of one step: asked once per site, in the step's own order.
struct TrainStepPlan {
    int launches = 0;           // taken so far (the statistic "train_persistent_launches")
    TrainLaunch next(const TrainGate& gate, const TrainSite& site) {
        TrainLaunch p;
        const TrainShape& s = site.shape;
        if (!train_gate_open(gate) || !site.plain) return p;
        p.grid = train_form_grid(site.kind, s, gate.ncu, site.per_cu);
        if (!p.grid) return p;
        p.nt = train_width_nt(s.W);
        if (launches >= TRAIN_LAUNCH_CAP) { p.capped = true; return p; }
        p.persistent = true;
        p.slot = launches++;
        p.slot_offset = train_slot_bytes(s.B) * p.slot;
        p.counter_bytes = train_counter_bytes(site.kind, s.B);
        if (site.kind == TRAIN_CELL_BWD) {
            p.defer = site.T <= ATTN_DEFER_MAX_T && s.W % 64 == 0 && s.C % 64 == 0 ? site.sw.defer : 0;
            p.split_a = site.sw.split && !site.split_off && site.rows_fit ? 1 : 0;
        }
        return p;
    }
};

// ---- the fused backward step (gemm_bwd.hip) ----
// One launch per time step for up to two jobs: workgroups of BWD_STEP_ROWS rows x BWD_STEP_COLS columns, the grid the larger
// job's.  K = 4W is shared out in whole unit groups of 32 units: the most shares, at most BWD_STEP_MAX_SHARES, that divide W / 32
// and keep the launch within BWD_STEP_MAX_BLOCKS workgroups (about two per CU and a half).  gper = unit groups per share picks the
// kernel's pipeline: 1, 2, or >= 3 (a loop of gper - 3 rounds); ksplit == 1 stores plainly, more shares meet in float atomics.
constexpr int BWD_STEP_ROWS = 32, BWD_STEP_COLS = 128;
constexpr int BWD_STEP_MAX_SHARES = 8, BWD_STEP_MAX_BLOCKS = 640;
struct BwdStepPlan { int blocks, ksplit, gper; };
inline BwdStepPlan bwd_step_plan(const int rows[2], const int N[2], int count, int W) {
    int blocks = 0;
    for (int j = 0; j < count; ++j) {
        const int nb = ((rows[j] + BWD_STEP_ROWS - 1) / BWD_STEP_ROWS) * ((N[j] + BWD_STEP_COLS - 1) / BWD_STEP_COLS);
        blocks = nb > blocks ? nb : blocks;
    }
    const int groups = W / 32;
    int ksplit = 1;
    for (int s = 2; s <= groups && s <= BWD_STEP_MAX_SHARES; ++s)
        if (groups % s == 0 && (long long)blocks * count * s <= BWD_STEP_MAX_BLOCKS) ksplit = s;
    return BwdStepPlan{blocks, ksplit, groups / ksplit};
}

}  // namespace casv
