// Shared declarations of the HIP hot path (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gemm_args.h"      // Seg, SlotPtr, GemmArgs, GemmBatch, TnArgs, TnLaunch
#include "gemm_plan.h"      // GemmContext, GemmSwitches, the launch plans

namespace casv {

// tanh on the transcendental units (v_exp_f32 + v_rcp_f32): |error| <= 1.06e-7 absolute for tanh and sigmoid alike, measured on an
// MI355X against float64 over every 64th float32 with |x| <= 30 plus the branch switch and saturation ranges
// (profiles/r09_activation_error.txt; tests/test_gpu_activations.py holds it to 2e-7).  The energies
// need 11*W tanh per decoder row; libm's tanhf made this kernel VALU-bound at 5x the time.
// Value of lane (id ^ MASK) of a fully active 64-lane wave, without the LDS crossbar round trip of ds_bpermute (what
// __shfl_xor compiles to): DPP for partners inside a row of 16 lanes, the gfx950 row-swap instructions across rows.  Same
// partner, same value: butterflies built from these reduce in exactly the order of the __shfl_xor loops they replace
// (profiles/lane_xor_probe.hip checks every mask against __shfl_xor on the device).
template <int MASK> __device__ __forceinline__ int lane_xor(const int x) {
    static_assert(MASK == 1 || MASK == 2 || MASK == 4 || MASK == 8 || MASK == 16 || MASK == 32, "one bit");
    if constexpr (MASK == 1) return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true);                 // quad_perm [1,0,3,2]
    else if constexpr (MASK == 2) return __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true);            // quad_perm [2,3,0,1]
    else if constexpr (MASK == 4)                                                                      // i^7 then i^3
        return __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(x, 0x141, 0xF, 0xF, true), 0x1B, 0xF, 0xF, true);
    else if constexpr (MASK == 8) return __builtin_amdgcn_mov_dpp(x, 0x128, 0xF, 0xF, true);            // row_ror:8
    else if constexpr (MASK == 16) {
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
        return (int)((__lane_id() & 16) ? r[0] : r[1]);
    } else {
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
        return (int)((__lane_id() & 32) ? r[0] : r[1]);
    }
}
template <int MASK> __device__ __forceinline__ float lane_xor(const float x) { return __int_as_float(lane_xor<MASK>(__float_as_int(x))); }
template <int MASK> __device__ __forceinline__ double lane_xor(const double x) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)lane_xor<MASK>((int)(unsigned)b), hi = (unsigned)lane_xor<MASK>((int)(unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// butterfly over the wave, partners 32, 16, 8, 4, 2, 1 in this order: v = op(v, partner's v)
template <class T, class Op> __device__ __forceinline__ T wave_butterfly(T v, Op op) {
    v = op(v, lane_xor<32>(v)); v = op(v, lane_xor<16>(v)); v = op(v, lane_xor<8>(v));
    v = op(v, lane_xor<4>(v)); v = op(v, lane_xor<2>(v)); v = op(v, lane_xor<1>(v));
    return v;
}

// 4 x 4 transpose inside every quad of lanes: the caller's lane q (= lane & 3) holds column q of rows 0..3 in (v0, v1, v2, v3) and
// gets row q's four columns back -- two exchange stages (partner q ^ 1, then q ^ 2), each swapping the off-diagonal blocks.  A GEMM
// epilogue whose lanes hold one column of several rows stores 16 bytes per lane with it (gemm.hip, gemm_skinny.hip: plain epilogues).
typedef float QuadF4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ QuadF4 quad_transpose(float v0, float v1, float v2, float v3, const int q) {
    const bool b0 = q & 1, b1 = q & 2;
    const float y01 = lane_xor<1>(b0 ? v0 : v1), y23 = lane_xor<1>(b0 ? v2 : v3);
    if (b0) { v0 = y01; v2 = y23; } else { v1 = y01; v3 = y23; }
    const float z0 = lane_xor<2>(b1 ? v0 : v2), z1 = lane_xor<2>(b1 ? v1 : v3);
    if (b1) { v0 = z0; v1 = z1; } else { v2 = z0; v3 = z1; }
    return QuadF4{v0, v1, v2, v3};
}

#ifdef CASV_ACCURATE_ACT       // measurement aid (profiles/r04_split_bf16.txt, section 9): libm's functions in place of the exp2/rcp forms
__device__ __forceinline__ float fast_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ float fast_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
#else
__device__ __forceinline__ float fast_tanh(float x) {
    // both branches are evaluated and one is selected: a dozen straight-line instructions instead of a divergent branch per
    // call (the attention rows make 44 calls per loop iteration); the selected value is the one the branch computed
    const float ax = fabsf(x);
    const float x2 = x * x;         // odd Taylor region: avoids the cancellation of 1 - 2/(1+e^2x)
    const float small = x * (1.0f + x2 * (-0.333333333f + x2 * (0.133333333f + x2 * (-0.0539682540f + x2 * 0.0218694885f))));
    const float t = 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(ax * 2.88539008177792681472f));
    return ax < 0.25f ? small : copysignf(t, x);
}
__device__ __forceinline__ float fast_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-x * 1.44269504088896340736f));
}
#endif

// The LSTM cell on gate pre-activations (Keras gate order i, f, c~, o; recurrent_activation = sigmoid,
// seq2seq.py:268-272).  ONE definition for every GEMM variant, so that a row's result does not depend on which
// variant the launcher picked for the batch it sits in.
struct LstmCellOut { float i, f, g, o, c, h; };
__device__ __forceinline__ LstmCellOut lstm_cell(float zi, float zf, float zg, float zo, float cprev) {
    LstmCellOut r;
    r.i = fast_sigmoid(zi);
    r.f = fast_sigmoid(zf);
    r.g = fast_tanh(zg);
    r.o = fast_sigmoid(zo);
    r.c = __builtin_fmaf(r.f, cprev, r.i * r.g);
    r.h = r.o * fast_tanh(r.c);
    return r;
}
// The cell's pointwise backward (oracle/train.py lstm_backward) on what the forward pass kept: the gate activations, the cell
// state c and the one before it.  dh = dL/dh of this step, all its addends summed by the caller; dc = dL/dc carried from the
// step after.  -> the gate pre-activations' derivatives and dL/dc for the step before.  ONE definition, as for the forward cell:
// the tests that hold the fused backward paths to the per-step ones rest on every kernel evaluating this expression.
struct LstmCellBwdOut { float zi, zf, zg, zo, dc; };
__device__ __forceinline__ LstmCellBwdOut lstm_cell_bwd(float dh, float ig, float fg, float gg, float og, float c, float cp, float dc) {
    LstmCellBwdOut r;
    const float tc = tanhf(c);
    const float dov = dh * tc;
    const float dct = dh * og * (1.0f - tc * tc) + dc;
    r.zi = dct * gg * ig * (1.0f - ig);
    r.zf = dct * cp * fg * (1.0f - fg);
    r.zg = dct * ig * (1.0f - gg * gg);
    r.zo = dov * og * (1.0f - og);
    r.dc = dct * fg;
    return r;
}

// ---- GEMM launchers: the decision is the plan (gemm_plan.h), these run it.  ctx: the handle's (casv_model::gemm) ----
const GemmSwitches& gemm_switches();       // the process-wide switches (gemm.hip: read from the environment when the library is loaded)
void launch_gemm(const GemmContext& ctx, int epi, const GemmArgs& g, hipStream_t stream);
void launch_gemm_batch(const GemmContext& ctx, int epi, const GemmBatch& b, hipStream_t stream);
// the same for a plan the caller has made already (plan_gemm_launches(ctx, gemm_switches(), epi, b)); returns the plan it ran --
// the caller's, or the 128x128 one that stands in where the 256x256 kernels cannot get their LDS
GemmPlan run_gemm_plan(const GemmContext& ctx, int epi, const GemmBatch& b, const GemmPlan& plan, hipStream_t stream);
void run_gemm_skinny(int epi, const GemmLaunchPlan& l, hipStream_t stream);        // gemm_skinny.hip: FORM_SKINNY_32 / _64
void run_gemm_split256(int epi, const GemmLaunchPlan& l, hipStream_t stream);      // gemm_split.hip: FORM_SPLIT_256
bool gemm_split256_ready();                // gemm_split.hip: its kernels have their dynamic LDS on the current device
// The weight-gradient launch as the train step makes it (plan_gemm_tn): the ordered form when `ordered_ws` is given -- it needs
// gemm_tn_ordered_floats(ctx, g) floats there --, else under the context's arithmetic the split kernel where the shape has that form,
// else the fp32-input kernel.
size_t gemm_tn_ordered_floats(const GemmContext& ctx, const TnArgs& g);
TnLaunch launch_gemm_tn_any(const GemmContext& ctx, const TnArgs& g, float* ordered_ws, hipStream_t stream);
bool run_gemm_tn_split(bool part, int grid, const TnArgs& g, hipStream_t stream);   // gemm_tn_split.hip; false: the kernel cannot get its LDS
// optional vendor path for plain contractions C[M][N] (+)= A[M][K] . Bt[N][K]^T (+ bias) (vendor_gemm.hip); false = not taken
bool vendor_gemm_nt(const float* A, long long lda, long long M, int K, const float* Bt, int N, const float* bias, float* C, long long ldc,
                    int accumulate, hipStream_t stream);
void vendor_gemm_release(hipStream_t stream);         // frees the vendor path's workspace of a stream (model destruction)
// tile shape of the GEMM launches: -1 = by size (default), 0 = always 128x128, 1 = always 32x128 (same results)
void set_gemm_tile_mode(int mode);
// arithmetic of the GEMM launches (gemm.hip): 0 = fp32-input matrix instruction, 1 / 2 = bf16x3-split operands (three bf16 per fp32
// value, six products, fp32 accumulation) on the bf16 matrix instruction -- fp32-accurate sums, another summation order
void set_gemm_split_override(int v);       // process-wide: -1 none (every entry point's own choice), 0 / 1 / 2 = all launches of the decode path
int gemm_split_override();
#ifdef CASV_S2_CLOCK
void s2_clock_dump();
#endif
void gemm_split_prepare(const float* Bt, int N, int K, hipStream_t stream);    // makes the image of a weight buffer now (ahead of a graph recording)
void gemm_split_invalidate(const float* Bt);     // drops the pre-split image of a weight buffer (call where it changes or is released); nullptr: all
long gemm_split_epoch();                   // changes whenever the option or a pre-split weight image does (key of captured step graphs)
void gemm_split_bump_epoch();
// C[rows][cols] (row stride ld) = 0 on the stream: partial sums of a split K are added atomically and start from zero
inline void gemm_clear(float* c, long long rows, long long cols, long long ld, hipStream_t stream) {
    if (ld == cols) (void)hipMemsetAsync(c, 0, (size_t)rows * cols * sizeof(float), stream);
    else (void)hipMemset2DAsync(c, (size_t)ld * sizeof(float), 0, (size_t)cols * sizeof(float), rows, stream);
}
// The dynamic-LDS size of a kernel function: the attribute belongs to the (function, device) pair -- a second model on another
// device needs its own --, so every function keeps one of these.  false: the runtime refused.
struct LdsAttribute { bool set[64] = {false}; };
inline bool gemm_dynamic_lds(LdsAttribute& a, const void* fn, int bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && a.set[dev]) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (dev >= 0 && dev < 64) a.set[dev] = true;
    return true;
}

// ---- small kernels (decode_kernels.hip) ----
struct AttnArgs {
    const float* wq;        // [R][W]  h_d . W_a + b_UW
    const int* wq_rows;     // optional [R]: row r's query is row wq_rows[r] of `wq` (beam search: the query of the parent expansion, computed once per expansion)
    const float* u;         // [B][T][W]
    const float* enc;       // [B][T][C]
    const float* va;        // [W]
    const float* bv;        // [1]
    const float* a_base;    // alignment store [(S+1)*R][T]
    const int* prev;        // [R] global row id of the parent expansion
    const int* line;        // [R] or nullptr (then line = r / rows_per_line)
    int rows_per_line;
    float* ctx;             // [R][C] (row stride ctx_ld if set)
    long long ctx_ld;       // 0 = C; train step: the context goes straight into the cell's input rows [ctx | h]
    const float* ctx_mask; long long ctx_mask_ld;   // optional per-row keep-mask of the context (train step: dropout on the cell input)
    int R, T, W, C, window;
    int step_imm; const int* step_ptr;   // output slot = step + 1
    double* apos;           // [R] sum_s a'[s]*s
    int* amax1;             // [R] max(a') == 1.0
    const int* nrows;       // optional device row count (rows >= *nrows are skipped)
    const int* nact;        // optional live rows per line: row r is skipped unless r % nact_group < nact[r / nact_group]
    int nact_group;
    long long u_line, u_time, enc_line, enc_time;   // element strides of u / enc by line and by position
    int* win_out;           // optional [R]: window of this step, s_lo | cnt << 16 (train step backward)
    int* win_store;         // optional [(S+1)*R]: the same per output slot (decode: sparse form of the alignment store)
};
void launch_attention(const AttnArgs& a, hipStream_t stream);

struct SoftmaxArgs {
    const float* logits;    // [R][V]
    float* p_base;          // score store [(S+1)*R][V], output slot = step + 1
    int R, V;
    int step_imm; const int* step_ptr;
    // greedy bookkeeping (mode < 0: none)
    int mode;               // 0: argmax over 1..V-1; 1: argmax over all V with index-0 NaN write-back
    int* out_idx;           // [R][S]
    float* out_prob;        // [R][S]
    int S;
    int* nan_flag;          // set when a row is all NaN (numpy would raise)
    const int* nact;        // optional live rows per line: row r is skipped unless r % nact_group < nact[r / nact_group]
    int nact_group;
};
void launch_softmax(const SoftmaxArgs& a, hipStream_t stream);
// lm_predict's probabilities for casv_decoder_step_lm: softmax_kernel's arithmetic on the LM logits; rows whose LM context is NaN
// (row_kernels.h, lm_context_nan: the window `win` of the step, -1 = empty, and the query wq of the row) are NaN
struct LmSoftmaxArgs {
    const float* logits;    // [R][Vp]
    float* probs;           // [R][Vp]
    const float* wq;        // [R][W]
    const float* va; const float* bv;
    const int* win;         // [R]
    int R, V, W;
};
void launch_lm_softmax(const LmSoftmaxArgs& a, hipStream_t stream);
// The sampling pick of a step (sample_kernels.hip): in place of the softmax and the greedy pick, a draw
// from every row's logits and the one-hot row of what was drawn as the next step's input.
struct SampleArgs {
    const float* logits;    // [R][Vp]
    float* feedback;        // row r of the output slot: feedback + (step + 1) * fb_slot + r * Vp (the score store: fb_slot = R * Vp)
    long long fb_slot;
    int R, V;
    int step_imm; const int* step_ptr;      // the step: counter word of the draw, output slot and column
    int rows_per_line;      // row r draws sample r % rows_per_line of line r / rows_per_line ...
    const long long* stream;    // ... whose stream id is stream[line], or (nullptr) the line's number
    const int* sample;      // optional [R]: the sample number of every row instead
    const float* u;         // optional [R]: the uniform of every row instead of the generator's (test support)
    unsigned long long seed;
    float temperature; int top_k;
    int* out_idx;           // [R][S], column step * out_col
    float* out_logp;        // log-probability of the draw under the model (all V entries, temperature 1)
    float* out_logq;        // ... under the proposal (the candidates at this temperature)
    int S, out_col;
    int* nan_flag;          // set when a row is invalid
    float top_p;            // launch_sample_cut only: the nucleus of the cut (top_k, top_p); 1 = none
};
void launch_sample(const SampleArgs& a, hipStream_t stream);
// The same pick under a cut (top_k <= 4095, top_p): sample_cut_kernel, which sorts every row's keys in LDS (DESIGN.md section 4.8,
// items 11 to 13).  A row takes Vp floats and P keys of 8 bytes, P = V rounded up to a power of two, so the rows (= waves) of a
// workgroup follow from V: as many as SAMPLE_CUT_LDS holds, at most 4 -- and at most `rows_max` where that is positive (a test
// switch: the results do not depend on it).
constexpr int SAMPLE_CUT_LDS = 160 * 1024;
constexpr int SAMPLE_CUT_MAX_K = 4095;
inline int sample_cut_sort_size(int V) { int P = 2; while (P < V) P <<= 1; return P; }
inline int sample_cut_row_bytes(int V) { return ((V + 31) & ~31) * 4 + sample_cut_sort_size(V) * 8; }
inline int sample_cut_rows_per_workgroup(int V, int rows_max) {
    const int fit = std::min(4, SAMPLE_CUT_LDS / sample_cut_row_bytes(V));
    return std::max(1, rows_max > 0 ? std::min(fit, rows_max) : fit);
}
// false: the runtime refused the kernels' dynamic LDS (nothing may be launched then); callers ask before they enqueue anything
bool sample_cut_ready();
// returns the rows per workgroup it launched with
int launch_sample_cut(const SampleArgs& a, int rows_max, hipStream_t stream);
// dst row line * rows_per_line + n (n < rows_per_line) = src row line, `width` floats each, rows packed: the encoder's final
// states under every sample row of a line
void launch_spread_rows(const float* src, float* dst, int lines, int rows_per_line, int width, hipStream_t stream);

// The vote over N candidates per source (consensus_kernels.hip).  sym [B][N][L] arbitrary int32 symbols
// compared for equality only, len [B][N] in -1 .. L (-1: a padding candidate), weight [B][N] or nullptr (all 1.0);
// dist [B][N][N], risk [B][N], pick [B].
// The costed calls (casv_edit_costs): key [B][N][L] beside sym -- never nullptr there: a call without keys
// passes sym itself, under which keys are equal exactly where symbols are -- and the costs; key == nullptr takes the plain kernels,
// which read of `costs` only the risk kernel's unit = 1.
struct EditCosts { int gap, sub, near, unit; };
struct ConsensusArgs {
    const int* sym; const int* len; const double* weight;
    int* dist; double* risk; int* pick;
    int B, N, L, mode;
    const int* key; EditCosts costs;
};
constexpr int CONSENSUS_MAX_N = 256, CONSENSUS_MAX_L = 8192;
constexpr int CONSENSUS_COSTED_MAX_L = 2048, EDIT_COST_MAX = 255;
// nullptr, or what is wrong with a cost set: 1 <= gap, 0 <= near <= sub, 1 <= unit, all at most 255
inline const char* edit_costs_refused(const EditCosts& c) {
    if (c.gap < 1 || c.gap > EDIT_COST_MAX) return "gap outside 1..255";
    if (c.sub < 0 || c.sub > EDIT_COST_MAX) return "sub outside 0..255";
    if (c.near < 0 || c.near > c.sub) return "near outside 0..sub";
    if (c.unit < 1 || c.unit > EDIT_COST_MAX) return "unit outside 1..255";
    return nullptr;
}
// a wave's LDS at the longest pair: one string's symbols, and per column the other's symbol and one DP row's entry, with
// CONSENSUS_GUARD columns in front and behind for the lanes that stand outside the matrix (consensus_pair)
constexpr int CONSENSUS_GUARD = 64;
inline int consensus_lds_bytes(int max_len) { return (3 * max_len + 4 * CONSENSUS_GUARD) * 4; }
// the costed form's: per column {symbol, DP entry, key, unused} with the guards on both sides -- 34 KiB at CONSENSUS_COSTED_MAX_L
// (the row string stays in registers)
inline int consensus_costed_lds_bytes(int max_len) { return (max_len + 2 * CONSENSUS_GUARD) * 16; }
// sources a launch takes side by side (the blocks of a pair loop over the rest): at most 2^20 blocks in all
inline int consensus_grid_z(int B, int N) { return std::max(1, std::min(std::min(B, 65535), (1 << 20) / (N * N))); }
// false: the runtime refused consensus_dist_kernel's dynamic LDS at the longest strings (nothing may be launched then)
bool consensus_ready();
// max_len: the longest live candidate of the call (the LDS a wave gets)
void launch_consensus_dist(const ConsensusArgs& a, int max_len, hipStream_t stream);
void launch_consensus_risk(const ConsensusArgs& a, hipStream_t stream);

// The confusion network voted from N candidates per source (consensus_kernels.hip).  sym, len as above,
// pivot [B] in -1 .. N-1 (-1: the source is skipped); where [B][N][L]: per candidate symbol the pivot symbol it stands against
// (>= 0) or -1 - slot of its insertion, CASV_ALIGN_NONE beyond a length; ins / start [B][stride]: per slot 0 .. len[pivot] the
// most symbols a candidate inserts there and the slot's first column; ncol [B].  dir: the direction words of the sources
// b0 .. b1-1 of one round, [b - b0][N][rows][wpr] of {diagonal holds, pivot-against-gap holds}, bit k & 31 of word k >> 5 for
// candidate symbol k, one row per pivot symbol.
struct AlignArgs {
    const int* sym; const int* len; const int* pivot;
    int* where; int* ins; int* start; int* ncol;
    uint2* dir;
    unsigned long long* stamps;     // nullptr, or two sums over the waves of s_memtime clocks: [0] in the fill, [1] in the walk
    int B, N, L, stride, rows, wpr, b0, b1;
    const int* key; EditCosts costs;   // as in ConsensusArgs: nullptr takes the plain kernel
};
// src / mass [B][C][N], best [B][C] (include/cor_asv_ann_hip.h, casv_consensus_vote)
struct VoteArgs {
    const int* sym; const int* len; const int* pivot; const int* where; const int* ins; const int* start; const int* ncol;
    const double* weight;
    int* src; double* mass; int* best;
    int B, N, L, stride, C;
};
constexpr int CONSENSUS_ALIGN_MAX_L = 2048;
constexpr int CASV_ALIGN_NONE_VALUE = INT32_MIN;
// the direction words of one round of casv_consensus_align (at least one source's, whatever the budget)
constexpr size_t CONSENSUS_ALIGN_BUDGET = (size_t)256 << 20;
// bytes of one pair's direction words: `rows` pivot symbols by `cols` candidate symbols
inline int consensus_align_wpr(int cols) { return (cols + 31) >> 5; }
inline size_t consensus_align_pair_bytes(int rows, int cols) { return (size_t)rows * consensus_align_wpr(cols) * sizeof(uint2); }
void launch_consensus_align(const AlignArgs& a, int max_len, hipStream_t stream);
void launch_consensus_layout(const AlignArgs& a, hipStream_t stream);
void launch_consensus_vote(const VoteArgs& a, hipStream_t stream);

void launch_embed_sparse(const float* E, const int* idx, const float* val, float* x0,
                         int rows, int A, int V, int W, hipStream_t stream);
// one-alternative input idx [B][T] -> out [T][B]: the character of (line, position), V where there is none (encoder.hip: rows of
// layer 1's per-character table, in the order step t reads them)
void launch_char_rows(const int* idx, int* out, int B, int T, int V, hipStream_t stream);
// the table's own input, as launch_embed_sparse reads it: idx[v] = v with val[v] = 1 for v < V, idx[V] = -1 (no character)
void launch_table_input(int* idx, float* val, int V, hipStream_t stream);
void launch_advance_step(int* step_ptr, hipStream_t stream);
// elementwise helpers of the optional topologies (seq2seq.py:284-301): dst[i] += src[i]; dst[i] = tanh(src[i]) (n floats, 16-byte aligned)
void launch_add_inplace(float* dst, const float* src, long long n, hipStream_t stream);
void launch_tanh(const float* src, float* dst, long long n, hipStream_t stream);
// test support (casv_debug_activation): which 0 = fast_tanh, 1 = fast_sigmoid on n floats; 2 = lstm_cell on n rows of 5 floats
// (z_i, z_f, z_g, z_o, c_prev) -> n rows of 2 (c, h)
void launch_debug_activation(int which, const float* in, float* out, long long n, hipStream_t stream);
// deep_bidirectional_encoder's "cross sum" (seq2seq.py:246-259, as computed): dst[2k] = dst[2k+1] = src[2k] + src[2k+1] (n floats, n even)
void launch_cross_sum(const float* src, float* dst, long long n, hipStream_t stream);
// Source of the result records of one decode call (pack_records_kernel): row j * row_mul of idx / prob [rows][S];
// beam: len / score per row (len == 0: no finished hypothesis -> the input line src_idx [B][T][A], slot 0);
// batched greedy: len == nullptr, the line ends at its first `eos`, empty input lines (src_idx / src_val) give empty records.
struct RecordSrc {
    const int* idx; const float* prob; const int* len; const double* score;
    const int* src_idx; const float* src_val;
    int B, S, T, A, row_mul, eos;
};
void launch_pack_records(const RecordSrc& r, int* rec, hipStream_t stream);
void launch_scatter_rows(const float* src, int src_ld, float* dst, int dst_ld, int rows, int width,
                         int dst_row_mul, hipStream_t stream);
// Small fills and row copies batched into one launch (decode_kernels.hip): op = fill `n` 4-byte words at dst with `fill`
// (src == nullptr), or copy rows: word w < width of source row r (stride src_ld) -> destination row r * row_mul (stride dst_ld),
// n = rows * width.
struct SmallOp { void* dst; const void* src; long long n; long long src_ld, dst_ld; int width, row_mul; unsigned fill; };
constexpr int SMALL_OPS_MAX = 28;
static_assert(SMALL_OPS_MAX >= 10 + 2 * 8 + 2, "the greedy decode's set-up launch takes 10 + 2 * depth operations (depth <= 8) and the encoder's 1 + depth");
struct SmallOps {
    SmallOp op[SMALL_OPS_MAX]; int count;
    int dropped;            // operations that did not fit (sticky): launch_small_ops then launches NOTHING and says so
    bool fill(void* dst, size_t bytes, unsigned word = 0u) {
        if (count >= SMALL_OPS_MAX || (bytes & 3)) { ++dropped; return false; }
        op[count++] = SmallOp{dst, nullptr, (long long)(bytes / 4), 0, 0, 1, 1, word}; return true;
    }
    bool rows(const float* src, long long src_ld, float* dst, long long dst_ld, int nrows, int width, int row_mul) {
        if (count >= SMALL_OPS_MAX) { ++dropped; return false; }
        op[count++] = SmallOp{dst, src, (long long)nrows * width, src_ld, dst_ld, width, row_mul, 0u}; return true;
    }
};
bool launch_small_ops(const SmallOps& ops, hipStream_t stream);    // false: an operation had been dropped (nothing launched)

// ---- beam search (beam_kernels.hip) ----
struct BeamParams {
    int N, width_in, width_out, max_results;
    double threshold_in, rejection, cost0;
    int q_stage;   // set by launch_beam_step: entries of the old queue staged in LDS
    int sort_cap;  // set by launch_beam_step: new keys sorted in LDS at once
    int pop_cap;   // set by launch_beam_step: entries at the head of the merged queue kept in LDS for the pop loop
    int eos;       // vocabulary index of the end-of-line character
};

// What phase A of the beam step finds out about one expansion row (beam_kernels.hip)
struct RowRec { int count, beampos, rej, srcpos, nan, rejlate; };

struct BeamState {
    // per line
    int B, T, V, S, R;          // R = B*N
    int node_cap, q_cap, f_cap;
    // node pool [B][node_cap]
    int* n_parent; int* n_chr; float* n_prob; double* n_cum; int* n_len; int* n_exp;
    int* n_k; int* n_rejpos; double* n_pos; int* n_is1;
    int* n_count;               // [B]
    // per expansion row [(S+1)*R]
    short* created;             // [..][beam_width_in + 1] vocabulary indices of the children, in creation order
    // queue: two buffers [2][B][q_cap] of (key, node id) sorted best-first (step parity selects the live one);
    // q_n[0..B) = entries, q_n[B..2B) = offset of the first entry after the last pop
    double* q_key; int* q_id; int* q_n;
    // scratch for steps that create more keys than the LDS sorts at once: [B][2][g_cap]
    double* g_key; int* g_id; int g_cap;
    // finals
    double* f_key; int* f_id; int* f_n; int* f_total;
    // current beam
    int* beam_node;             // [R]
    int* nact;                  // [B] active rows of the current step
    int* line_done;             // [B]
    int* line_steps;            // [B]
    int* active_lines;          // [0] lines still searching, [1] statistic: most new keys of any line in any step
    // step io
    int* prev;                  // [R]
    float* p_in;                // [R][V]
    const float* p_base;        // score store
    const float* logits;        // [R][Vp] of this step: the kernel turns them into the step's row of the score store itself
                                // (the arithmetic of softmax_kernel); nullptr: a softmax launch has done that already
    const double* apos; const int* amax1;
    const int* src_rej;         // [B][T]
    const int* step_ptr;        // step number in device memory (graph replay), or nullptr: step_imm
    int step_imm;
    // wide beams (N >= 64): phase A as its own grid -- per row its record and the list of its children in creation order
    RowRec* rowrec;             // [R] or nullptr (then the per-line kernel does phase A itself)
    short* cand_idx; float* cand_val;   // [R][min(beam_width_in, V) + 1]
    // lm_predict (lm_logits == nullptr: off): a child's cost is -log of the LM's probability of its index.
    // lm_logits [R][Vp] of this step; the NaN rule of the LM's context (row_kernels.h, lm_context_nan) reads the query store
    // [(S+1)*R][W] at the parent expansion prev[r], v_a, b_v and the window store [(S+1)*R]; wide beams: cand_lm [R][CMAX] = the
    // LM probability of every child beam_expand_kernel chose
    const float* lm_logits; const float* lm_q; const float* lm_va; const float* lm_bv; const int* lm_win; int W;
    float* cand_lm;
};
void launch_beam_init(const BeamState& s, const BeamParams& p, hipStream_t stream);
void launch_beam_step(const BeamState& s, const BeamParams& p, hipStream_t stream);
#ifdef CASV_GEMM_PROF
void gemm_prof_dump();               // diagnostic build: in-kernel cycle stamps of the 128x128 LSTM GEMM (gemm.hip)
void skinny_prof_dump();             // ... and of the 64x128 LSTM launches (gemm_skinny.hip)
#endif
#ifdef CASV_BEAM_PROF
void beam_prof_dump(int steps);      // diagnostic build: phase times of the beam step kernel (beam_kernels.hip)
#endif
struct BeamOut {
    int* idx; float* prob; int* len; double* score; int* rejpos; float* align; int* n_found; int* n_steps;
    const float* a_base;
};
void launch_beam_extract(const BeamState& s, const BeamParams& p, const BeamOut& o, hipStream_t stream);
// Window form of the alignments: (lo, K weights) per result row and step; lo = -1 marks an all-NaN row.
struct SparseAlignOut { int* lo; float* w; int K; const int* win_store; };
void launch_beam_extract_sparse(const BeamState& s, const BeamParams& p, const BeamOut& o, const SparseAlignOut& sp, hipStream_t stream);
void launch_greedy_extract_sparse(const float* a_base, const int* win_store, int B, int S, int T, const SparseAlignOut& sp, hipStream_t stream);

// ---- persistent small-batch decoder (persist.hip) ----
struct PersistLayer {
    const float* w;        // [W/16 unit groups][4 gates][16 units][Kt], K of every 16-tile in MFMA-group order
    const float* bias;     // [W/16][4][16]
    int Kt;
};
struct PersistArgs {
    int R, D, W, V, Vp, C, T, S, mode;
    int lda;                               // row stride of the staged activation rows in LDS: widest K of any task + 4
    PersistLayer layer[8];
    const float* wa; const float* bUW;     // attention query weights [W][W] (packed K order), bias
    const float* e;                        // tied output projection [Vp][W] (packed K order; rows >= V are zero)
    float* h[8]; float* c[8];              // state stores [(S+1)*R][W], slot s+1 = outputs of step s
    float* ctx;                            // [(S+1)*R][C]
    float* wq;                             // [(S+1)*R][W]
    float* logits;                         // [(S+1)*R][Vp]
    AttnArgs att;                          // u, enc, v_a, b_v, alignment store, window store (wq / ctx are set per step)
    int* out_idx; float* out_prob; int* nan_flag;
    unsigned* counters;                    // persist_counter_bytes(); zeroed ahead of the launch
    int g_lstm, g_att, g_plain;            // workgroups per role
    unsigned long long* prof;              // diagnostic build only (CASV_PERSIST_PROF): 32 tick sums, see persist.hip
};
// persistent encoder: x0 [B][T][W] embedded input, H1 [B][T][2W] layer-1 outputs (fw | bw), Hn[n-2] [B][T][W] outputs of layer
// n >= 2, cfin [(D+1)][B][W] final cell states (slot 0: backward direction of layer 1, slot n-1: layer n, slot D: forward)
struct PersistEncArgs {
    int B, T, D, W, lda;
    PersistLayer l1[2];            // forward, backward
    PersistLayer ln[7];            // layers 2..D
    const float* x0; float* H1; float* Hn[7]; float* cfin;
    unsigned* counters;            // persist_enc_counter_bytes(); zeroed ahead of the launch
    unsigned long long* prof;      // diagnostic build only (CASV_PERSIST_PROF): tick sums of workgroup 0, see persist.hip
};
size_t persist_enc_counter_bytes(int B, int D);
// workgroups per CU the runtime admits for the persistent kernels at a given dynamic-LDS size (capped at 2; 0: none)
int persist_encode_blocks_per_cu(size_t lds_bytes);
int persist_decode_blocks_per_cu(size_t lds_bytes);
int persist_enc_max_tiles();                       // tiles of one phase a workgroup of the encoder may own
int launch_persist_encode(const PersistEncArgs& pa, int grid, hipStream_t stream);
// persistent encoder in the split arithmetic (persist_split.hip): the same buffers; rows in blocks of 32, units in groups of 32;
// PersistLayer.w = the per-step launches' weights [4W][Kt] (gate-interleaved rows, K in natural order), .bias = theirs [4W]
struct PersistSplitEncArgs {
    int B, T, D, W;
    PersistLayer l1[2];            // forward, backward
    PersistLayer ln[7];            // layers 2..D
    const float* x0; float* H1; float* Hn[7]; float* cfin;
    unsigned* counters;            // persist_split_enc_counter_bytes(); zeroed ahead of the launch
    int inject;                    // test support: workgroup 0 leaves without handing on (the launch gives up and is redone per step)
};
size_t persist_split_enc_counter_bytes(int B, int D);
int persist_split_encode_blocks_per_cu();          // workgroups per CU the runtime admits (capped at 2; 0: none)
int persist_split_enc_max_tiles();                 // tiles of one phase a workgroup may own
int launch_persist_split_encode(const PersistSplitEncArgs& pa, int grid, hipStream_t stream);
size_t persist_counter_bytes(int R, int D);
size_t persist_lds_bytes(const PersistArgs& pa);
int launch_persist_decode(const PersistArgs& pa, hipStream_t stream);   // -1: the staged rows do not fit the LDS

}  // namespace casv
