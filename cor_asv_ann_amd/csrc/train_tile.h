// The staged tile of the train step's persistent kernels (train_persist*.hip), device code only: a workgroup of 256 threads
// contracts BM = 32 rows of A, handed over by other workgroups a moment ago, with BN = 128 rows of a weight panel B over
// NT = W/32 stages of K2 = 32 columns, on 16 v_mfma_f32_32x32x2_f32 per wave and stage (wave w: B rows 32 w .. 32 w + 31).
//
// The pipeline.  Nothing the weights need depends on the hand-off, so request() runs AHEAD of the caller's wait_deps: stage 0 of
// B is requested, waited for and stored to LDS buffer 0, stages 1 and 2 leave for the two register sets g1 and g0.  BEHIND the
// wait load_a() requests all NT stages of the thread's A row at once (16 bytes per thread and stage, sc1: the lines were written
// by other XCDs and miss every cache -- one memory round trip per step, not one per stage).  wait_a() and start() wait for
// everything, put stage 0 of A beside stage 0 of B and meet at a barrier.  chain() then walks the stages: at stage J, stage J + 1
// goes from registers into the LDS buffer whose readers passed the last barrier, stage J + 3 of B leaves for the register set
// just emptied, stage J is contracted, barrier.  The two register sets swap at every level of the recursion.  The wait in front
// of the store is counted: the loads of stage J + 2, the younger ones, stay in flight.
//
// The loads are `asm` statements, hidden from the compiler's own wait bookkeeping (it would drain the queue at the first use),
// with the stage's offset in the instruction: no address registers per stage.  THE RULE that goes with them: between such a load
// and the wait that names its destination "+v", nothing may touch that register -- the compiler believes the value is there as
// soon as the statement has `executed`.  Every wait here names exactly the registers it releases; check_asm_loads.py holds the
// listings of the four files to the rule.
//
// Variants, all parameters of the one chain:
//   PLAIN   four B registers per stage, counted wait 4;
//   RIDER   QN = 32 more B rows behind the BN (LDS rows BM + BN ...; Tile<QN>), loaded from the row qp into the stage's q register,
//           counted wait 5; every wave also contracts its k quarter of the stage with those rows into accq (the quarters meet in
//           LDS later);
//   QUERY   the q register alone, counted wait 1, its 32 rows in place of the first 32 B rows, contracted by k quarters into acc.
// The weights come as this thread's row pointers: bp[i] row srow + 32 i of the BN, qp row srow of the QN, both at column sk.
// B0 is the column at which the panel starts in the rows bp (the attention cell's h half: C), added to the stage's offset.  They
// are plain pointers, not a struct: held in one, the compiler forms their addresses differently and the listings move.
#pragma once
#include "common.h"
#include "train_plan.h"

namespace casv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace tile {

constexpr int BM = 32, BN = 128;
constexpr int QN = 32;                       // rows of W_a that ride along (RIDER) or stand alone (QUERY): a workgroup's query columns
constexpr int K2 = 32, LD = K2 + 4;          // a stage's columns; row stride of its LDS image in floats
static_assert(BM == TRAIN_ROW_BLOCK, "train_plan.h plans for this row block");

enum Variant { PLAIN, RIDER, QUERY };
constexpr int stage_loads(int v) { return v == PLAIN ? 4 : v == RIDER ? 5 : 1; }      // hidden loads per thread and B stage

struct BStage { f32x4 b[4], q; };            // one B stage in flight

#define CASV_TILE_LD16 "global_load_dwordx4 %0, %1, off offset:%2"
template <int V, int KT, int B0>
__device__ __forceinline__ void load_b(BStage& g, const float* const (&bp)[4], const float* qp) {
    if constexpr (V != QUERY) {
        asm volatile(CASV_TILE_LD16 : "=v"(g.b[0]) : "v"(bp[0]), "n"((B0 + KT * K2) * 4));
        asm volatile(CASV_TILE_LD16 : "=v"(g.b[1]) : "v"(bp[1]), "n"((B0 + KT * K2) * 4));
        asm volatile(CASV_TILE_LD16 : "=v"(g.b[2]) : "v"(bp[2]), "n"((B0 + KT * K2) * 4));
        asm volatile(CASV_TILE_LD16 : "=v"(g.b[3]) : "v"(bp[3]), "n"((B0 + KT * K2) * 4));
    }
    if constexpr (V != PLAIN) asm volatile(CASV_TILE_LD16 : "=v"(g.q) : "v"(qp), "n"(KT * K2 * 4));
}
// all but the youngest N hidden loads have arrived: the stage's registers may be touched
template <int V, int N>
__device__ __forceinline__ void wait_b(BStage& g) {
    if constexpr (V == PLAIN) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(g.b[0]), "+v"(g.b[1]), "+v"(g.b[2]), "+v"(g.b[3]) : "n"(N));
    if constexpr (V == RIDER) asm volatile("s_waitcnt vmcnt(%5)" : "+v"(g.b[0]), "+v"(g.b[1]), "+v"(g.b[2]), "+v"(g.b[3]), "+v"(g.q) : "n"(N));
    if constexpr (V == QUERY) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(g.q) : "n"(N));
}
// nothing is in flight any more: both stages' registers may be touched
template <int V>
__device__ __forceinline__ void wait_b(BStage& g0, BStage& g1) {
    if constexpr (V == PLAIN) asm volatile("s_waitcnt vmcnt(0)" : "+v"(g0.b[0]), "+v"(g0.b[1]), "+v"(g0.b[2]), "+v"(g0.b[3]),
                                                                   "+v"(g1.b[0]), "+v"(g1.b[1]), "+v"(g1.b[2]), "+v"(g1.b[3]));
    if constexpr (V == RIDER) asm volatile("s_waitcnt vmcnt(0)" : "+v"(g0.b[0]), "+v"(g0.b[1]), "+v"(g0.b[2]), "+v"(g0.b[3]), "+v"(g0.q),
                                                                   "+v"(g1.b[0]), "+v"(g1.b[1]), "+v"(g1.b[2]), "+v"(g1.b[3]), "+v"(g1.q));
    if constexpr (V == QUERY) asm volatile("s_waitcnt vmcnt(0)" : "+v"(g0.q), "+v"(g1.q));
}
// the A row of this thread, every stage at once, in the order 0 .. NT - 1
template <int NT, int J = 0>
__device__ __forceinline__ void load_a(f32x4 (&areg)[NT], const float* arow) {
    if constexpr (J < NT) {
        asm volatile(CASV_TILE_LD16 " sc1" : "=v"(areg[J]) : "v"(arow), "n"(J * K2 * 4));
        load_a<NT, J + 1>(areg, arow);
    }
}
#undef CASV_TILE_LD16
template <int NT>
__device__ __forceinline__ void wait_a(f32x4 (&areg)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) asm volatile("s_waitcnt vmcnt(0)" : "+v"(areg[j]));
}

template <int QROWS = 0>        // B rows of a stage behind the BN: the rider's 32
struct Tile {
    static constexpr int STAGE = (BM + BN + QROWS) * LD;       // floats of a stage's LDS image; the tile has two
    float* const s;
    const int wave = threadIdx.x >> 6, l31 = threadIdx.x & 31, lh = (threadIdx.x & 63) >> 5;
    const int srow = threadIdx.x >> 3, sk = 4 * (threadIdx.x & 7);      // staging: this thread's row and first of 4 columns
    const int a_off = l31 * LD + 4 * lh, b_off = (BM + wave * 32 + l31) * LD + 4 * lh;
    f32x16 acc, accq;

    __device__ __forceinline__ explicit Tile(float* lds) : s(lds) {}

    __device__ __forceinline__ void store_a(const f32x4& a, int buf) const {
        *reinterpret_cast<f32x4*>(s + buf * STAGE + srow * LD + sk) = a;
    }
    template <int V>
    __device__ __forceinline__ void store_b(const BStage& g, int buf) const {
        float* sb = s + buf * STAGE + (BM + srow) * LD + sk;
        if constexpr (V != QUERY) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(sb + 32 * i * LD) = g.b[i];
        }
        if constexpr (V != PLAIN) *reinterpret_cast<f32x4*>(sb + (V == RIDER ? BN : 0) * LD) = g.q;
    }
    template <int V>
    __device__ __forceinline__ void compute(int buf) {
        const float* base = s + buf * STAGE;
        f32x4 fa[4], fb[4];
        if constexpr (V != QUERY) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                fa[q] = *reinterpret_cast<const f32x4*>(base + a_off + 8 * q);
                fb[q] = *reinterpret_cast<const f32x4*>(base + b_off + 8 * q);
            }
        }
        if constexpr (V != PLAIN) {       // this wave's k quarter of the stage against the 32 q rows
            f32x16& sum = V == RIDER ? accq : acc;
            const int q_off = (BM + (V == RIDER ? BN : 0) + l31) * LD + 4 * lh;
            const f32x4 faq = *reinterpret_cast<const f32x4*>(base + a_off + 8 * wave);
            const f32x4 fq = *reinterpret_cast<const f32x4*>(base + q_off + 8 * wave);
#pragma unroll
            for (int i = 0; i < 4; ++i) sum = __builtin_amdgcn_mfma_f32_32x32x2f32(faq[i], fq[i], sum, 0, 0, 0);
        }
        if constexpr (V != QUERY) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][i], fb[q][i], acc, 0, 0, 0);
        }
    }

    // ahead of the hand-off wait: stage 0 of B into LDS, stages 1 and 2 in flight
    template <int NT, int V, int B0 = 0>
    __device__ __forceinline__ void request(BStage& g0, BStage& g1, const float* const (&bp)[4], const float* qp = nullptr) const {
        load_b<V, 0, B0>(g0, bp, qp);
        wait_b<V, 0>(g0);
        store_b<V>(g0, 0);
        if constexpr (NT > 1) load_b<V, 1, B0>(g1, bp, qp);
        if constexpr (NT > 2) load_b<V, 2, B0>(g0, bp, qp);
    }
    // everything requested so far has arrived (the caller has waited for what it requested itself): stage 0 is complete
    template <int V>
    __device__ __forceinline__ void start(BStage& g0, BStage& g1, const f32x4& a0) const {
        wait_b<V>(g0, g1);
        store_a(a0, 0);
        __syncthreads();
    }
    // stages J .. NT - 1; ga holds stage J + 1 (or is on its way), gb stage J + 2.  Called as chain(g1, g0, ...).
    template <int NT, int V, int B0 = 0, int J = 0>
    __device__ __forceinline__ void chain(BStage& ga, BStage& gb, const f32x4 (&areg)[NT], const float* const (&bp)[4], const float* qp = nullptr) {
        if constexpr (J < NT) {
            if constexpr (J + 1 < NT) {
                if constexpr (J >= 2) wait_b<V, (J + 2 < NT ? stage_loads(V) : 0)>(ga);
                store_a(areg[J + 1], (J + 1) & 1);
                store_b<V>(ga, (J + 1) & 1);
            }
            if constexpr (J + 3 < NT) load_b<V, J + 3, B0>(ga, bp, qp);
            compute<V>(J & 1);
            __syncthreads();
            chain<NT, V, B0, J + 1>(gb, ga, areg, bp, qp);
        }
    }

    // x.Wx + b of this lane's four rows m0 + q + 8 wave + 4 lh (clamped to the last of R) x four gates, from a step's Z [R][ldz]
    // at the lane's unit of the group that starts at column n0
    __device__ __forceinline__ void load_zpre(float (&zpre)[4][4], const float* z_step, int ldz, int m0, int R, int n0) const {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = m0 + q + 8 * wave + 4 * lh;
            const float* zr = z_step + (long long)(m < R ? m : R - 1) * ldz + n0 + l31;
            zpre[q][0] = zr[0]; zpre[q][1] = zr[32]; zpre[q][2] = zr[64]; zpre[q][3] = zr[96];
        }
    }
    // The gate exchange: wave c holds gate c of all 32 rows in acc; afterwards z[q][c] is gate c of this lane's row q (as above).
    // The image lies over the stages: the chain's last barrier is before it, the caller's publish between it and the next stage.
    __device__ __forceinline__ void exchange_gates(float (&z)[4][4]) const {
        float (*s_gate)[16][64] = reinterpret_cast<float (*)[16][64]>(s);
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int r = 0; r < 16; ++r) s_gate[wave][r][lane] = acc[r];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 4; ++c) z[q][c] = s_gate[c][4 * wave + q][lane];
    }
};

// The seven 16-byte inputs of a thread's four backward cells (row r, units u0 .. u0 + 3), requested one step ahead with the A
// stages of the step before: the addend of dL/dh, the four gate activations, the cell state and the one before it.
struct CellBwdIn {
    f32x4 a, gi, gf, gg, go, cell, cp;
    // xg: the row's gates of unit group u0 / 32 at u0 % 32 (i, f, g, o 32 floats apart)
    __device__ __forceinline__ void request(const float* xa, const float* xg, const float* xc, const float* xp) {
#define CASV_TILE_LD16(DST, PTR, OFF) asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(DST) : "v"(PTR), "n"(OFF))
        CASV_TILE_LD16(a, xa, 0);
        CASV_TILE_LD16(gi, xg, 0); CASV_TILE_LD16(gf, xg, 128); CASV_TILE_LD16(gg, xg, 256); CASV_TILE_LD16(go, xg, 384);
        CASV_TILE_LD16(cell, xc, 0); CASV_TILE_LD16(cp, xp, 0);
#undef CASV_TILE_LD16
    }
    __device__ __forceinline__ void wait() {
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(gi), "+v"(gf), "+v"(gg), "+v"(go), "+v"(cell), "+v"(cp));
    }
};

}  // namespace tile
}  // namespace casv
