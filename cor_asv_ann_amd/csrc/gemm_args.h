// Plain argument structs of the GEMM launchers: what a launch is described by, without any HIP type (common.h includes this; the
// launch planner gemm_plan.h needs nothing else).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace casv {

// One K-segment of a GEMM's A operand: rows of `width` floats (a multiple of 32) taken from
//   base + slot * slot_stride + row_id * ld,   slot = step * step_mul + step_add,
// where row_id = rows ? rows[m] : m.  `skip_first` drops the segment (treated as zeros) at
// step 0 -- the zero initial LSTM state of the encoder.
struct Seg {
    const float* base;
    const int* rows;
    long long slot_stride;
    int step_mul, step_add;
    int ld;
    int width;
    int skip_first;
    int koff;   // offset of this segment in the fused weight's K dimension
    const float* first_base;   // if set: at step 0 the rows come from first_base + m * ld (initial LSTM state)
};

// Output / state pointer that moves with the step the same way.
struct SlotPtr {
    float* base;
    long long slot_stride;
    int step_mul, step_add;
    int ld;
};

struct GemmArgs {
    Seg a[3];
    int nseg;
    const float* Bt;      // [N][Ktot], K contiguous (LSTM: rows in gate-interleaved order)
    const float* bias;    // [N] (same order) or nullptr
    int M, N, Ktot;
    SlotPtr out;          // PLAIN: C[M][N]; LSTM: h'[M][N/4]
    // LSTM epilogue only
    Seg c_in;             // previous cell state rows (width = units), skip_first = zero state
    SlotPtr c_out;
    SlotPtr zinit;        // LSTM: pre-activation term added to the contraction, [M][4U] interleaved (x.K + b of all steps, precomputed)
    SlotPtr gates_out;    // training: activated gates i,f,g,o, [M][4U] in the interleaved column order (or null)
    SlotPtr out2;         // training: a second copy of h (the next step's cell input rows [ctx | h]) (or null)
    const int* nact;      // beam decode: live rows per line (0 = search finished); a tile without a live row is skipped --
    int nact_group;       // rows per line                                   its rows are never read
    int epi_plain;        // job of an EPI_LSTM launch that takes the PLAIN epilogue (lets independent GEMMs of both kinds share a launch)
    int accumulate;       // PLAIN: C += A.B^T instead of C = (weight-gradient sums)
    int out_zeroed;       // PLAIN with split-K: the caller has already cleared the output (no memset per launch)
    int kgroups;          // 2 = allow the two-wave-group split-K variant (train step; changes the summation order)
    int xcd_rows;         // XCD-aware tile order: the 8 XCDs form an xcd_rows x (8/xcd_rows) grid over the tile grid (0 = off)
    int b_static;         // Bt changes only at casv_commit_weights (inference weights): the split-bf16 experiment may keep a pre-split image of it
    const void* Bimg;     // set by launch_gemm_split256: that image (gemm_split.hip), or nullptr
    Seg acc_in;           // optional (base != nullptr), 128x128 split tiles only (gemm.hip, SPLIT): the tile's accumulators start from
                          // rows of N floats in the job's column order -- row rows[m] (or m) of base + slot * slot_stride, `ld` floats
                          // apart -- instead of from zero: the fp32 accumulators another launch left behind the K segments that come
                          // first (its raw plain output), so that [x | h] in one launch and x, then h on top of it, are the same
                          // instruction sequence per element.  width / koff / skip_first / first_base are not used.
    int ksplit;           // PLAIN: 0/1 = one block per tile; n > 1 = K split over n blocks (float atomics into C);
                          // -1 = let the launcher choose (train step only: sums become order-dependent)
    // step source
    int step_imm;
    const int* step_ptr;
};

enum { EPI_PLAIN = 0, EPI_LSTM = 1 };

// Up to four independent GEMMs in one launch (blockIdx.y selects the job): the two directions of the
// bidirectional encoder layer, or the (layer, time) cells on one anti-diagonal of the stacked encoder.
constexpr int GEMM_MAX_JOBS = 4;
struct GemmBatch {
    GemmArgs g[GEMM_MAX_JOBS];
    int count;
};

// C[M][N] (+)= sum_k A[k][m] * B[k][n] for operands that lie K-major (gemm_tn.hip: weight gradients of the train step).
// lda / ldb / M / N multiples of 4, 16-byte aligned bases; rows m >= Mstore are computed but not stored (padded operand).
struct TnArgs {
    const float* A; long long lda; const float* B; long long ldb; float* C; long long ldc;
    int M, Mstore, N, K;
    int accumulate;      // C += (gradient sums) instead of C =
    int out_zeroed;      // C = with a split K: the caller has cleared C already
    float* colsum;       // optional [Mstore]: += sum_k A[k][m] (the bias gradient that goes with a weight gradient)
    int nsplit;          // set by launch_gemm_tn: K shares of the launch
    float* part;         // ordered form (launch_gemm_tn_ordered): K share z stores its partial tile at part[z][Mstore][N] ...
    float* colpart;      // ... and its column sums at colpart[z][Mstore]; a second pass adds the shares in z order
};
struct TnLaunch { int split, shares, nonempty; };   // which kernel ran (1: gemm_tn_split.hip), K shares launched, shares holding k-tiles

}  // namespace casv
