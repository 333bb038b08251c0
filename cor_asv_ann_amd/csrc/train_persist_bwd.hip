// The backward recurrences of the train step (keras' LSTM gradient through time, oracle/train.py lstm_backward) as ONE launch
// per pair of layers -- the mirror of train_persist.hip.
//
// A backward time step is: the cells' pointwise backward (gate derivatives dZ(t) from dL/dh(t) = dOut(t) + dRec(t+1) and the
// running dL/dc), then the data GEMM dRec(t) = dZ(t) . Wr that carries the gradient one step further.  As launches that is
// ~33 us per step (gemm_bwd.hip: one fused launch), 407 times per train step for the plain layers.  Here 2 x 16 x 16 workgroups
// stay resident and play BOTH parts in every step:
//   P  workgroup (layer, row block, unit group) owns the cells of 32 rows x 32 units: their dL/dc lives in its registers for
//      the whole sequence; it waits for the four K shares of dRec(t+1) of its column tile, computes dZ(t) and hands it on;
//   G  the same workgroup as (layer, row block, column tile, K share) contracts dZ(t) of its 32 rows over its quarter of the gate
//      axis (= W columns: as many stages as the forward step) with its 128 x W panel of Wr^T, and adds the partial tile to
//      dRec(t) with float atomics (four shares per element, as the per-step launches do).
// Hand-offs as in handoff.h (write-through stores / memory-side atomics, drain, one counter per (row block, quarter) and per
// (row block, column tile)); everything a step needs that does not depend on the step before -- gate activations, cell states,
// dOut -- is requested together with the dZ rows of the step before it, so that P itself waits for one 16-byte load.
// G is the staged tile of train_tile.h, plain variant, once per step (the pipeline is described there); P's inputs are its
// CellBwdIn and its arithmetic lstm_cell_bwd (common.h).
// Weight panels: slot s = (column tile, K share) of every row block and both layers sits on XCD s % 8, whose L2 holds them.
#include "common.h"
#include "handoff.h"
#include "persist_host.h"
#include "train_kernels.h"
#include "train_tile.h"

namespace casv {

using namespace tile;

template <int NT>        // W / 32: unit groups = slots per (layer, row block); K stages per step
__global__ __launch_bounds__(256, 2) void train_recurrence_bwd_kernel(const RecBwdArgs ra) {
    __shared__ __attribute__((aligned(16))) float s_stage[2 * Tile<>::STAGE];
    __shared__ int s_ok;
    Tile<> tl(s_stage);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    constexpr int W = NT * 32;
    constexpr long long K = 4LL * W;
    const int B = ra.B;
    const int nrb = (B + BM - 1) / BM;
    const int slot = blockIdx.x % NT, rest = blockIdx.x / NT;
    const int rb = rest % nrb, jb = rest / nrb;
    const RecBwdJob& job = ra.job[jb];
    const int len = job.len;
    const int m0 = rb * BM;
    // counters of this (layer, row block): four "dZ quarter ready" lines, then up to four "dRec column tile ready" lines
    unsigned* const cbase = ra.counters + (long long)(jb * nrb + rb) * 8 * 32;
    unsigned* const abort_w = ra.counters + (long long)2 * nrb * 8 * 32;
    // P: unit group ug of the row block;  G: column tile ct, K share ks
    const int ug = slot, ct = slot >> 2, ks = slot & 3;
    unsigned* const z_mine = cbase + (ug / (NT / 4)) * 32;          // the quarter my dZ columns belong to
    unsigned* const z_need = cbase + ks * 32;
    unsigned* const r_mine = cbase + (4 + ct) * 32;
    unsigned* const r_need = cbase + (4 + (ug >> 2)) * 32;         // the column tile (128 units) my cells' dL/dh sits in

    const int srow = tid >> 3, su = 4 * (tid & 7);
    const bool row_ok = m0 + srow < B;
    const int mrow = row_ok ? m0 + srow : B - 1;
    const int u0 = ug * 32 + su;                                    // this thread's four cells: row mrow, units u0 .. u0 + 3

    // ---- G: operands ----
    const float* bp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bp[i] = job.WrT + (long long)(ct * BN + srow + 32 * i) * K + (long long)ks * W + su;
    f32x16& acc = tl.acc;

    // ---- P: state and the inputs of the first step ----
    const bool a_on = job.dOut != nullptr, cfin_on = job.dc_fin != nullptr;
    f32x4 dc, mk;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        dc[e] = cfin_on ? job.dc_fin[(long long)mrow * W + u0 + e] : 0.0f;
        mk[e] = job.mask ? job.mask[u0 + e] : 1.0f;
    }
    auto time_of = [&](int k) { return job.reverse ? len - 1 - k : k; };
    // (an absent input is read from a row that exists and not used)
    auto load_pin = [&](CellBwdIn& in, int k) {
        const int t = time_of(k);
        const float* xg = job.Gt + ((long long)t * B + mrow) * K + ug * 128 + su;
        const float* xc = job.Cs + ((long long)t * B + mrow) * W + u0;
        const float* xa = a_on ? job.dOut + ((long long)t * B + mrow) * job.ld_out + u0 : xc;
        const float* xp = k > 0 ? job.Cs + ((long long)time_of(k - 1) * B + mrow) * W + u0 : (job.c0 ? job.c0 + (long long)mrow * W + u0 : xc);
        in.request(xa, xg, xc, xp);
    };
    CellBwdIn in;
    load_pin(in, len - 1);
    in.wait();

    for (int i = 0; i < len; ++i) {
        const int k = len - 1 - i, t = time_of(k);
        // =========== P: dZ(t) of my cells ===========
        f32x4 bv;
        if (i > 0) {
            if (!wait_deps(Dep{r_need, 4u * (unsigned)i}, Dep{nullptr, 0}, Dep{nullptr, 0}, abort_w, &s_ok)) return;
            const float* xb = job.dRec + ((long long)time_of(k + 1) * B + mrow) * W + u0;
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(bv) : "v"(xb));
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(bv));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[e] = job.dh_fin ? job.dh_fin[(long long)mrow * W + u0 + e] : 0.0f;
        }
        {
            const bool cp_on = k > 0 || job.c0 != nullptr;
            f32x4 zi, zf, zg, zo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {         // dh summed as lstm_bwd_kernel does (train_kernels.hip)
                float dh = 0.f;
                if (a_on) dh += in.a[e] * mk[e];
                if (i > 0 || job.dh_fin) dh += bv[e];
                const LstmCellBwdOut d = lstm_cell_bwd(dh, in.gi[e], in.gf[e], in.gg[e], in.go[e], in.cell[e], cp_on ? in.cp[e] : 0.0f, dc[e]);
                zi[e] = d.zi; zf[e] = d.zf; zg[e] = d.zg; zo[e] = d.zo; dc[e] = d.dc;
            }
            if (row_ok) {
                float* z = job.dZ + ((long long)t * B + mrow) * K + ug * 128 + su;
                asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(z), "v"(zi) : "memory");
                asm volatile("global_store_dwordx4 %0, %1, off offset:128 sc1" :: "v"(z), "v"(zf) : "memory");
                asm volatile("global_store_dwordx4 %0, %1, off offset:256 sc1" :: "v"(z), "v"(zg) : "memory");
                asm volatile("global_store_dwordx4 %0, %1, off offset:384 sc1" :: "v"(z), "v"(zo) : "memory");
            }
        }
        publish(z_mine);

        // =========== G: my share of dRec(t) ===========
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        {
            BStage g0, g1;
            tl.request<NT, PLAIN>(g0, g1, bp);
            if (!wait_deps(Dep{z_need, (unsigned)((NT / 4) * (i + 1))}, Dep{nullptr, 0}, Dep{nullptr, 0}, abort_w, &s_ok)) return;
            const float* arow = job.dZ + ((long long)t * B + mrow) * K + (long long)ks * W + su;
            f32x4 areg[NT];
            load_a(areg, arow);
            // ... and what the next step's cells need that does not depend on this step (none left after the last)
            load_pin(in, k > 0 ? k - 1 : 0);
            wait_a(areg);
            in.wait();
            tl.start<PLAIN>(g0, g1, areg[0]);
            tl.chain<NT, PLAIN>(g1, g0, areg, bp);
        }
        {
            float* out = job.dRec + (long long)t * B * W + ct * BN + wave * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m < B) atomicAdd(out + (long long)m * W, acc[r]);
            }
        }
        publish(r_mine);
    }
    // dL/dc of the layer's initial state
    if (row_ok) *reinterpret_cast<f32x4*>(job.dc_out + (long long)mrow * W + u0) = dc;
}

// The instantiation of a width, from train_plan.h's list (nullptr: the width has none, and no plan)
typedef void (*RecBwdKernel)(const RecBwdArgs);
static RecBwdKernel recb_kernel(int W) {
    switch (train_width_nt(W)) {
#define CASV_RECB_CASE(NT_) case NT_: return train_recurrence_bwd_kernel<NT_>;
        CASV_TRAIN_REC_BWD_WIDTHS(CASV_RECB_CASE)
#undef CASV_RECB_CASE
        default: return nullptr;
    }
}
int train_recurrence_bwd_blocks_per_cu(int W) {
    const RecBwdKernel k = recb_kernel(W);
    return k ? persist_blocks_per_cu(k, 0, TRAIN_BLOCKS_PER_CU[TRAIN_REC_BWD]) : 0;
}
void launch_train_recurrence_bwd(const RecBwdArgs& ra, int grid, hipStream_t stream) {
    if (const RecBwdKernel k = recb_kernel(ra.W)) hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, stream, ra);
}

}  // namespace casv
