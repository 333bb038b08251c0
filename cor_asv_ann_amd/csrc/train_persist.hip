// The forward recurrences of the train step (keras LSTM over time, seq2seq.py:268-272,293-298,363-367) as ONE launch per
// pair of layers instead of one launch per time step.
//
// train.hip walks encoder layer n and decoder layer n-1 in lockstep: per step one gemm_skinny launch of 2 x 256 workgroups,
// each contracting a 32 x 128 tile of h(t-1).Wr^T over K = W and finishing the cell.  A launch lasts ~30 us of which the
// matrix pipes need ~15; the rest is launch gap, the first round trip to the L2 and the tail.  Here the same workgroups stay
// resident for the whole sequence: workgroup (layer, row block, unit group) owns 32 rows x 32 units, keeps their cell state in
// registers, and hands h(t) to the 16 workgroups of its row block through memory (handoff.h: sc1 stores + drain + one counter
// per row block; sc1 loads behind the poll).  The weights of a unit group (128 rows of Wr) are read by 2 x 16 workgroups; the
// mapping puts a unit group's workgroups on ONE XCD, whose L2 then holds 2 groups x 2 layers x 256 KB.
//
// What a workgroup does per step: the staged tile of train_tile.h (the pipeline is described there), plain variant, once -- the
// first three weight stages and the step's x.Wx + b values requested BEFORE it polls (they do not depend on h), all W/32 stages of
// its 32 rows of h(t-1) behind the poll -- then gemm_skinny.hip's cell epilogue.  The tile walks the stages through the LDS image
// and the MFMA sequence of gemm_skinny.hip's K loop: results are those of the per-step launches bit for bit (tested).
//
// The two jobs of a launch may differ in rows (casv_score_candidates: encoder layer n on the Be sources beside decoder layer n - 1
// on Be * N candidates).  The grid, the (layer, row block, unit group) mapping and the counters are those of RecArgs.B, the larger
// count; a job with RecJob.rows < B uses its own rows for strides, clamps and guards, and its workgroups beyond them leave at once.
// Nothing here waits for the whole grid -- hand-offs are per (job, row block) -- so the idle workgroups are harmless.
#include "common.h"
#include "handoff.h"
#include "persist_host.h"
#include "train_kernels.h"
#include "train_tile.h"

namespace casv {

using namespace tile;

template <int NT>        // W / 32: K stages per step
__global__ __launch_bounds__(256, 2) void train_recurrence_kernel(const RecArgs ra) {
    __shared__ __attribute__((aligned(16))) float s_stage[2 * Tile<>::STAGE];
    __shared__ int s_ok;
    Tile<> tl(s_stage);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    constexpr int W = NT * 32;
    const int B = ra.B;
    const int nrb = (B + BM - 1) / BM;
    // consecutive workgroups go to consecutive XCDs: unit group fastest, so that XCD x sees unit groups x, x + 8, ...
    const int ug = blockIdx.x % NT, rest = blockIdx.x / NT;
    const int rb = rest % nrb, jb = rest / nrb;
    const RecJob& job = ra.job[jb];
    const int m0 = rb * BM, n0 = ug * BN;
    unsigned* const counter = ra.counters + (long long)(jb * nrb + rb) * 32;
    unsigned* const abort_w = ra.counters + (long long)2 * nrb * 32;
    const int len = job.len;
    // the job's own rows: its strides [len][R][..], row clamps and store guards; the mapping and the counters above are ra.B's alone
    const int R = job.rows ? job.rows : B;
    if (m0 >= R) return;        // (a row block beyond the smaller job's rows: nobody waits for it -- the hand-offs are per (job, row block))

    const int srow = tid >> 3, sk = 4 * (tid & 7);
    int mrow = m0 + srow; mrow = mrow < R ? mrow : R - 1;
    const float* bp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bp[i] = job.Wr + (long long)(n0 + srow + 32 * i) * W + sk;
    f32x16& acc = tl.acc;

    // cell state of this lane's four (row, unit) elements: rows m0 + q + 8 wave + 4 lh, unit ug * 32 + l31
    const int u = ug * 32 + l31;
    const float omask_u = job.omask ? job.omask[u] : 1.0f;
    float cst[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int m = m0 + q + 8 * wave + 4 * lh; m = m < R ? m : R - 1;
        cst[q] = job.c0 ? job.c0[(long long)m * W + u] : 0.0f;
    }

    for (int k = 0; k < len; ++k) {
        if (ra.fault && blockIdx.x == 0 && k == 1) return;      // (test: a workgroup that never hands on -- its peers must give up)
        const int t = job.reverse ? len - 1 - k : k, tp = job.reverse ? t + 1 : t - 1;
        const float* arow = k == 0 ? (job.h0 ? job.h0 + (long long)mrow * W + sk : nullptr)
                                   : job.hs + ((long long)tp * R + mrow) * job.hs_ld + sk;
        // x.Wx + b of this step's elements
        float zpre[4][4];
        tl.load_zpre(zpre, job.Z + (long long)t * R * (4 * W), 4 * W, m0, R, n0);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        if (arow) {         // (uniform: a zero initial state contributes nothing -- the per-step path skips the segment too)
            BStage g0, g1;
            tl.request<NT, PLAIN>(g0, g1, bp);
            if (k > 0) {
                if (!wait_deps(Dep{counter, (unsigned)(k * NT)}, Dep{nullptr, 0}, Dep{nullptr, 0}, abort_w, &s_ok)) return;
            }
            f32x4 areg[NT];
            load_a(areg, arow);
            wait_a(areg);
            tl.start<PLAIN>(g0, g1, areg[0]);
            tl.chain<NT, PLAIN>(g1, g0, areg, bp);
        } else if (k > 0) {
            return;          // (never: only the first step can lack its input)
        }

        // ---- cell epilogue (gemm_skinny.hip) ----
        float z[4][4];
        tl.exchange_gates(z);
#pragma unroll
        for (int q = 0; q < 4; ++q) { z[q][0] += zpre[q][0]; z[q][1] += zpre[q][1]; z[q][2] += zpre[q][2]; z[q][3] += zpre[q][3]; }
        float* cout = job.Cs + (long long)t * R * W;
        float* hout = job.hs + (long long)t * R * job.hs_ld;
        float* gout = job.Gt + (long long)t * R * (4 * W);
        float* mout = job.om ? job.om + (long long)t * R * job.om_ld : nullptr;        // the outputs once more, masked: the next layer's input
        // (the layer's dL/dh accumulator of the backward pass, cleared here 16 bytes per thread and step instead of by a fill of the
        // whole buffer in front of the backward pass: these stores cost nothing beside the epilogue's own)
        if (job.zero && m0 + srow < R)
            *reinterpret_cast<f32x4*>(job.zero + ((long long)t * R + m0 + srow) * W + ug * 32 + sk) = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = m0 + q + 8 * wave + 4 * lh;
            if (m < R) {
                const LstmCellOut cell = lstm_cell(z[q][0] + 0.f, z[q][1] + 0.f, z[q][2] + 0.f, z[q][3] + 0.f, cst[q]);
                cst[q] = cell.c;
                cout[(long long)m * W + u] = cell.c;
                __hip_atomic_store(hout + (long long)m * job.hs_ld + u, cell.h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (mout) mout[(long long)m * job.om_ld + u] = cell.h * omask_u;
                float* gr = gout + (long long)m * (4 * W) + n0 + l31;
                gr[0] = cell.i; gr[32] = cell.f; gr[64] = cell.g; gr[96] = cell.o;
            }
        }
        publish(counter);        // drain + barrier (also: the gate exchange is read before the next step's stage lands on it)
    }
}

// The instantiation of a width, from train_plan.h's list (nullptr: the width has none, and no plan)
typedef void (*RecKernel)(const RecArgs);
static RecKernel rec_kernel(int W) {
    switch (train_width_nt(W)) {
#define CASV_REC_CASE(NT_) case NT_: return train_recurrence_kernel<NT_>;
        CASV_TRAIN_REC_WIDTHS(CASV_REC_CASE)
#undef CASV_REC_CASE
        default: return nullptr;
    }
}
int train_recurrence_blocks_per_cu(int W) {
    const RecKernel k = rec_kernel(W);
    return k ? persist_blocks_per_cu(k, 0, TRAIN_BLOCKS_PER_CU[TRAIN_REC]) : 0;
}
void launch_train_recurrence(const RecArgs& ra, int grid, hipStream_t stream) {
    if (const RecKernel k = rec_kernel(ra.W)) hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, stream, ra);
}

}  // namespace casv
