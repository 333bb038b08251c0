// The attention cell's forward recurrence of the train step (seq2seq.py:343-349, attention.py:526-575, teacher-forced) as
// ONE launch.  train.hip walks it with four launches per time step -- attention query GEMM, attention rows, cell input rows,
// LSTM step GEMM: ~62 us of kernels and four launch boundaries, 102 times.  Here (row block of 32) x (unit group of 32)
// workgroups, one per CU, stay resident and all play the same three parts in every step, handing rows to the other 15 workgroups
// of their row block through memory (handoff.h):
//   H  behind h(t-1) of the row block: its 32 rows, all W/32 stages at once into registers, are contracted with the unit
//      group's recurrent weight panel (the h columns of Wr: 128 gate rows) AND, riding on the same A stages, with 32 rows of W_a:
//      the workgroup's 32 columns of the attention query h.W_a + b (every wave a k quarter of each stage, summed through LDS);
//   A  behind the row block's query: two of the row block's rows per workgroup, one wave each -- attention_row (row_kernels.h),
//      the per-step kernel's code; the context goes, masked, straight into the cell's input rows;
//   C  behind the row block's context: its 32 rows are contracted with the ctx columns of Wr on top of H's accumulators, then
//      the cell (x.Wx + b precomputed; cell state in registers for the whole sequence); h(t) goes out twice: time-major for the
//      loss and into the next step's input rows.
// H and C are the staged tile of train_tile.h (the pipeline is described there), once each per step on the same accumulators: H
// the rider variant at column C of the weight rows, with two LDS images of 32 + 128 + 32 rows, C the plain variant at column 0.
// The sums: gate pre-activations run over [h | ctx] (the per-step launch: [ctx | h]) and the query's k quarters meet in LDS
// (per-step: two split-K shares), so the results agree with the per-step path to fp32 rounding, not bit for bit.
#include "common.h"
#include "handoff.h"
#include "persist_host.h"
#include "row_kernels.h"
#include "train_kernels.h"
#include "train_tile.h"

namespace casv {

using namespace tile;

template <int NT>        // W / 32 = C / 32: unit groups per row block; stages per K half
__global__ __launch_bounds__(256, 1) void train_attention_cell_kernel(const TopRecArgs ra) {
    __shared__ __attribute__((aligned(16))) float s_stage[2 * Tile<QN>::STAGE];      // A, Wr and W_a rows: 54 KB; the epilogues' exchanges reuse it
    __shared__ int s_ok;
    Tile<QN> tl(s_stage);
    float (*s_gate)[16][64] = reinterpret_cast<float (*)[16][64]>(s_stage);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    constexpr int W = NT * 32, C = W, KR = C + W;
    const int B = ra.B, U = ra.U;
    const int nrb = (B + BM - 1) / BM;
    const int ug = blockIdx.x % NT, rb = blockIdx.x / NT;
    const int m0 = rb * BM, n0 = ug * BN;
    unsigned* const cnt_h = ra.counters + (long long)(rb * 3 + 0) * 32;
    unsigned* const cnt_q = ra.counters + (long long)(rb * 3 + 1) * 32;
    unsigned* const cnt_c = ra.counters + (long long)(rb * 3 + 2) * 32;
    unsigned* const abort_w = ra.counters + (long long)nrb * 3 * 32;

    const int srow = tid >> 3, sk = 4 * (tid & 7);
    int mrow = m0 + srow; mrow = mrow < B ? mrow : B - 1;
    // weight rows staged by this thread: gate rows n0 + srow + 32 i of Wr [4W][KR], query row ug * 32 + srow of W_a^T [W][W]
    const float* bp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bp[i] = ra.Wr + (long long)(n0 + srow + 32 * i) * KR + sk;
    const float* qp = ra.WaT + (long long)(ug * QN + srow) * W + sk;
    f32x16& acc = tl.acc;
    f32x16& accq = tl.accq;

    // cell state of this lane's four (row, unit) elements: rows m0 + q + 8 wave + 4 lh, unit ug * 32 + l31
    const int u = ug * 32 + l31;
    float cst[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int m = m0 + q + 8 * wave + 4 * lh; m = m < B ? m : B - 1;
        cst[q] = ra.c0 ? ra.c0[(long long)m * W + u] : 0.0f;
    }
    const float qbias = ra.bUW ? ra.bUW[ug * QN + l31] : 0.0f;

    // Part A's rows.  A wave keeps its row for the whole sequence, so what the row can do ahead of its query it does (as in the
    // persistent decoder, persist.hip): the NEXT step's window is carried over from the weights just normalised (att_window_next:
    // the sum att_window reads back from memory, from registers), and the <= 11 rows of u and of the encoder outputs that window
    // attends are requested while the workgroup waits for the query.  At 16 unit groups a workgroup has two rows and four waves:
    // two waves share a row, each the tanh terms of half its columns -- wave 1 continues the per-lane sums of wave 0 in the
    // per-step kernel's order (column j = lane, then lane + 64), so the bits are attention_row's.
    constexpr int RPW = BM / NT;                                  // rows of the row block per workgroup
    constexpr int WPR = RPW == 2 ? 2 : 1;                          // waves per row
    constexpr bool FAST_A = RPW * WPR == 4 && W / 4 == 64 * WPR;   // 16 unit groups: 2 rows x 2 waves, 128 float4 columns; 8: 4 rows x 1 wave, 64
    const int a_i = WPR == 2 ? (wave & 1) : wave, a_half = WPR == 2 ? (wave >> 1) : 0;
    const int a_r = m0 + ug * RPW + a_i;
    const bool a_live = FAST_A && a_r < B;
    const int a_rc = a_r < B ? a_r : B - 1;
    AttWin a_w{0, 0};
    const float* a_ub = nullptr; const float* a_eb = nullptr;
    if constexpr (FAST_A) {
        const AttnArgs& a0 = ra.att;
        a_w = att_window(a0, a_rc, 0, lane);
        const int ln = a0.line ? a0.line[a_rc] : a_rc / a0.rows_per_line;
        a_ub = a0.u + (long long)ln * a0.u_line;
        a_eb = a0.enc + (long long)ln * a0.enc_line;
    }

    for (int t = 0; t < U; ++t) {
        float* const rec = ra.RecIn + (long long)t * B * KR;            // the cell's input rows of this step: [ctx | h(t-1)]
        // x.Wx + b of this step's elements
        float zpre[4][4];
        tl.load_zpre(zpre, ra.Z + (long long)t * B * (4 * W), 4 * W, m0, B, n0);
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[r] = 0.0f; accq[r] = 0.0f; }

        // =========== H: h(t-1) . [Wr_h | W_a] -- the h columns of Wr start at C; the query rows ride along ===========
        {
            const float* arow = rec + (long long)mrow * KR + C + sk;
            BStage g0, g1;
            tl.request<NT, RIDER, C>(g0, g1, bp, qp);
            if (t > 0) {
                if (!wait_deps(Dep{cnt_h, (unsigned)(NT * t)}, Dep{nullptr, 0}, Dep{nullptr, 0}, abort_w, &s_ok)) return;
            }
            f32x4 areg[NT];
            load_a(areg, arow);
            wait_a(areg);
            tl.start<RIDER>(g0, g1, areg[0]);
            tl.chain<NT, RIDER, C>(g1, g0, areg, bp, qp);
        }
        // the query columns: four k quarters -> LDS -> wave w sums rows 4 w .. 4 w + 3 of the accumulator layout; + bias
#pragma unroll
        for (int r = 0; r < 16; ++r) s_gate[wave][r][lane] = accq[r];
        __syncthreads();
        {
            float* wq = ra.WQ + (long long)t * B * W + ug * QN + l31;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rr = 4 * wave + q;                           // accumulator row index: matrix row (rr & 3) + 8 (rr >> 2) + 4 lh
                const float v = ((s_gate[0][rr][lane] + s_gate[1][rr][lane]) + (s_gate[2][rr][lane] + s_gate[3][rr][lane])) + qbias;
                const int m = m0 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
                if (m < B) store_sc1(wq + (long long)m * W, v);
            }
        }
        publish(cnt_q);

        // =========== A: attention rows m0 + RPW ug ... ===========
        float4 uu[MAXWIN], xx[MAXWIN];
        if constexpr (FAST_A) {         // the window's rows: on their way while the workgroup waits for the row block's query
            const int Ta = ra.att.T;
#pragma unroll
            for (int i = 0; i < MAXWIN; ++i) {
                int sr = a_w.s_lo + i; sr = sr < Ta ? sr : Ta - 1; sr = sr < 0 ? 0 : sr;
                uu[i] = reinterpret_cast<const float4*>(a_ub + (long long)sr * ra.att.u_time)[lane + 64 * a_half];
                xx[i] = reinterpret_cast<const float4*>(a_eb + (long long)sr * ra.att.enc_time)[lane + 64 * a_half];
            }
        }
        if (!wait_deps(Dep{cnt_q, (unsigned)(NT * (t + 1))}, Dep{nullptr, 0}, Dep{nullptr, 0}, abort_w, &s_ok)) return;
        if constexpr (FAST_A) {
            AttnArgs a = ra.att;
            a.wq = ra.WQ + (long long)t * B * W;
            a.ctx = rec; a.ctx_ld = KR;
            a.step_imm = t; a.step_ptr = nullptr;
            a.win_out = ra.WIN + (long long)t * B;
            float e[MAXWIN];
#pragma unroll
            for (int i = 0; i < MAXWIN; ++i) e[i] = 0.0f;
            if constexpr (WPR == 1) {
                if (a_live) {
                    att_energy_sums<true, MAXWIN>(a, a_r, lane, a_w, [&](int sr) { return RegRows{uu, sr - a_w.s_lo}; }, [](int) { return true; }, e);
                    att_normalise(a, a_r, t, lane, a_w, e);
                    att_context<true, MAXWIN>(a, a_r, lane, a_w, [&](int sr) { return RegRows{xx, sr - a_w.s_lo}; }, e);
                }
            } else {
                float (*s_part)[MAXWIN][64] = reinterpret_cast<float (*)[MAXWIN][64]>(s_stage);      // [row][position][lane]: wave 0's sums
                float* s_sum = s_stage + RPW * MAXWIN * 64;                                           // [row][MAXWIN + 1]: the row's sums
                const int j = lane + 64 * a_half;
                const float4 q = load_sc1(a.wq + (long long)a_rc * W + 4 * j);
                const float4 v = reinterpret_cast<const float4*>(a.va)[j];
                float p[MAXWIN];
                if (a_half == 0) {
#pragma unroll
                    for (int i = 0; i < MAXWIN; ++i) {
                        p[i] = 0.0f;
                        p[i] += fast_tanh(q.x + uu[i].x) * v.x;
                        p[i] += fast_tanh(q.y + uu[i].y) * v.y;
                        p[i] += fast_tanh(q.z + uu[i].z) * v.z;
                        p[i] += fast_tanh(q.w + uu[i].w) * v.w;
                        s_part[a_i][i][lane] = p[i];
                    }
                } else {        // the tanh values first: they do not wait for wave 0
#pragma unroll
                    for (int i = 0; i < MAXWIN; ++i) {
                        uu[i].x = fast_tanh(q.x + uu[i].x); uu[i].y = fast_tanh(q.y + uu[i].y);
                        uu[i].z = fast_tanh(q.z + uu[i].z); uu[i].w = fast_tanh(q.w + uu[i].w);
                    }
                }
                __syncthreads();
                if (a_half == 1) {
#pragma unroll
                    for (int i = 0; i < MAXWIN; ++i) {
                        p[i] = s_part[a_i][i][lane];
                        p[i] += uu[i].x * v.x;
                        p[i] += uu[i].y * v.y;
                        p[i] += uu[i].z * v.z;
                        p[i] += uu[i].w * v.w;
                        p[i] = wave_sum(p[i]);
                    }
                    if (lane == 0) {
#pragma unroll
                        for (int i = 0; i < MAXWIN; ++i) s_sum[a_i * (MAXWIN + 1) + i] = p[i];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < MAXWIN; ++i) e[i] = s_sum[a_i * (MAXWIN + 1) + i];
                if (a_live) {
                    att_normalise(a, a_r, t, lane, a_w, e, a_half == 1);
                    AttnArgs a2 = a;                        // this wave's half of the context columns
                    a2.C = C / 2; a2.ctx = a.ctx + a_half * (C / 2);
                    if (a.ctx_mask) a2.ctx_mask = a.ctx_mask + a_half * (C / 2);
                    att_context<true, MAXWIN>(a2, a_r, lane, a_w, [&](int sr) { return RegRows{xx, sr - a_w.s_lo}; }, e);
                }
            }
            publish(cnt_c);
            a_w = att_window_next(ra.att, a_w, e, lane);
        } else {
            for (int i = wave; i < RPW; i += 4) {
                const int r = m0 + ug * RPW + i;
                if (r < B) {
                    AttnArgs a = ra.att;
                    a.wq = ra.WQ + (long long)t * B * W;
                    a.ctx = rec; a.ctx_ld = KR;
                    a.step_imm = t; a.step_ptr = nullptr;
                    a.win_out = ra.WIN + (long long)t * B;
                    attention_row<true, 6>(a, r, t, lane);
                }
            }
            publish(cnt_c);
        }

        // =========== C: ctx(t) . Wr_c on top, then the cell ===========
        {
            const float* arow = rec + (long long)mrow * KR + sk;
            BStage g0, g1;
            tl.request<NT, PLAIN>(g0, g1, bp);
            if (!wait_deps(Dep{cnt_c, (unsigned)(NT * (t + 1))}, Dep{nullptr, 0}, Dep{nullptr, 0}, abort_w, &s_ok)) return;
            f32x4 areg[NT];
            load_a(areg, arow);
            wait_a(areg);
            tl.start<PLAIN>(g0, g1, areg[0]);
            tl.chain<NT, PLAIN>(g1, g0, areg, bp);
        }
        {
            float z[4][4];
            tl.exchange_gates(z);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 4; ++c) z[q][c] += zpre[q][c];
            float* cout = ra.Cs + (long long)t * B * W;
            float* hout = ra.hs + (long long)t * B * W;
            float* gout = ra.Gt + (long long)t * B * (4 * W);
            float* hnext = t + 1 < U ? ra.RecIn + (long long)(t + 1) * B * KR + C : nullptr;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int m = m0 + q + 8 * wave + 4 * lh;
                if (m < B) {
                    const LstmCellOut cell = lstm_cell(z[q][0] + 0.f, z[q][1] + 0.f, z[q][2] + 0.f, z[q][3] + 0.f, cst[q]);
                    cst[q] = cell.c;
                    cout[(long long)m * W + u] = cell.c;
                    hout[(long long)m * W + u] = cell.h;
                    if (hnext) store_sc1(hnext + (long long)m * KR + u, cell.h);
                    float* gr = gout + (long long)m * (4 * W) + n0 + l31;
                    gr[0] = cell.i; gr[32] = cell.f; gr[64] = cell.g; gr[96] = cell.o;
                }
            }
        }
        publish(cnt_h);
    }
}

// The instantiation of a width, from train_plan.h's list (nullptr: the width has none, and no plan)
typedef void (*TopKernel)(const TopRecArgs);
static TopKernel top_kernel(int W) {
    switch (train_width_nt(W)) {
#define CASV_TOP_CASE(NT_) case NT_: return train_attention_cell_kernel<NT_>;
        CASV_TRAIN_CELL_WIDTHS(CASV_TOP_CASE)
#undef CASV_TOP_CASE
        default: return nullptr;
    }
}
int train_attention_cell_blocks_per_cu(int W) {
    const TopKernel k = top_kernel(W);
    return k ? persist_blocks_per_cu(k, 0, TRAIN_BLOCKS_PER_CU[TRAIN_CELL]) : 0;
}
void launch_train_attention_cell(const TopRecArgs& ra, int grid, hipStream_t stream) {
    if (const TopKernel k = top_kernel(ra.W)) hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, stream, ra);
}

}  // namespace casv
