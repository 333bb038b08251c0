// Persistent encoder in the SPLIT arithmetic: the whole encoder recurrence of a small batch as ONE launch,
// for the entry points whose GEMMs contract bf16x3-split operands on v_mfma_f32_32x32x16_bf16 (the beam search).  Structure and
// hand-offs are those of persist_encode_kernel (persist.hip, whose module comment describes the protocol): phase A walks the two
// directions of layer 1 step by step, phase B the layers 2..D along anti-diagonals; cell state stays inside its workgroup; every buffer
// that crosses workgroups is indexed by the time step; producers store write-through + drain + barrier + one counter add, one
// lane polls (bounded in time, abort word), barrier, loads that go past the L2.
//
// What differs is the tile, and it follows from the numbers: the outputs must be, bit for bit, those of the per-step launches
// (gemm.hip, gemm_tile<EPI_LSTM, 1, SPLIT>; gemm_split.hip gives the same bits).  There an output element is ONE fp32 accumulator of
// v_mfma_f32_32x32x16_bf16 over K tiles of 16 in the order [x | h], six products per tile in the order a1.b1, a0.b2, a0.b1, a2.b0,
// a1.b0, a0.b0 (a = activation planes, b = weight planes, plane 0 the leading bf16).  How the instruction sums its 16 products is
// not a documented chain, so this kernel issues the same instruction with the same operand roles in the same order:
//   tile = 32 lines x 32 units x 4 gates, wave g = gate g (the weights' packed order [unit/32][i,f,c,o][unit%32] is a 128-column
//   block of the per-step tile), one 32x32 accumulator per wave over the full K; the four gates of a (line, unit) meet in LDS, then
//   lstm_cell (common.h) as everywhere.
// Operands are split by the arithmetic of gemm.hip's split4 (round to nearest, remainders exact).  The 32 activation rows as three
// bf16 planes over the full K do not fit a CU's LDS (288 KB at width 512), so they pass through LDS in chunks of PS_CT K tiles,
// double-buffered: chunk c + 1 is requested from memory before the products of chunk c issue and split + stored behind them, one
// barrier per chunk.  A tile plane lies in LDS as gemm.hip's (32-byte rows, the 16-byte halves swapped where bit 4 of the row is
// set: ds_read_b128 without conflicts).  Weights stay fp32 in memory (4 bytes per value from the L2 instead of 6 for a pre-split
// image; a lane's 8 k of a tile are 32 contiguous bytes) and are split in registers between the products, PS_RING tiles ahead --
// requested ahead of the dependency wait, they depend on nothing.
#include "common.h"
#include "row_kernels.h"
#include "handoff.h"
#include "persist_host.h"

namespace casv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int PS_CT = 8;                                  // K tiles (16 k each) per staged chunk
constexpr int PS_RING = 4;                                // weight tiles in flight per lane (slot = tile % PS_RING: PS_CT is a multiple)
constexpr int PS_PLANE_BYTES = 32 * 32;                   // one bf16 plane of a tile: 32 rows x 16 k
constexpr int PS_TILE_BYTES = 3 * PS_PLANE_BYTES;
constexpr int PS_BUF_BYTES = PS_CT * PS_TILE_BYTES;
constexpr int PS_LDS_BYTES = 2 * PS_BUF_BYTES;            // 48 KB; the gate exchange (4 x 32 x 32 floats) reuses buffer 0
constexpr int PS_MAXT = 4;                                // tiles of one phase a workgroup may own
static_assert(4 * 32 * 32 * 4 <= PS_BUF_BYTES, "the gate exchange lives in one chunk buffer");
static_assert(PS_CT % PS_RING == 0, "a tile's ring slot is a compile-time constant of its place in the chunk");

// x = x0 + x1 + x2 in bf16, four values at a time: gemm.hip's split4, operation for operation
__device__ __forceinline__ void ps_split4(const f32x4 x, u32x2& p0, u32x2& p1, u32x2& p2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const f32x2 v = {x[2 * h], x[2 * h + 1]};
        const unsigned q0 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
        const f32x2 r1 = v - f32x2{__uint_as_float(q0 << 16), __uint_as_float(q0 & 0xffff0000u)};
        const unsigned q1 = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
        const f32x2 r2 = r1 - f32x2{__uint_as_float(q1 << 16), __uint_as_float(q1 & 0xffff0000u)};
        p0[h] = q0; p1[h] = q1; p2[h] = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
    }
}

__global__ __launch_bounds__(256, 2) void persist_split_encode_kernel(const PersistSplitEncArgs pa) {
    extern __shared__ __attribute__((aligned(16))) char s_buf[];       // two chunk buffers
    __shared__ float s_bias[128];                                       // the tile's bias values [gate][unit]
    // cell state of the tiles this workgroup owns in the running phase, [tile][element][thread]: as registers the tile loop would
    // have to be unrolled PS_MAXT times around the whole cell
    __shared__ float s_creg[PS_MAXT][4][256];
    __shared__ int s_ok;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int B = pa.B, T = pa.T, D = pa.D, W = pa.W;
    const int NRB = (B + 31) / 32, NUG = W / 32, NT = NRB * NUG;
    const int NCNT = D + 1;                                        // counters per row block: fw, bw, layers 2..D
    unsigned* const abort_w = pa.counters + (long long)NRB * NCNT * 32;
    auto counter = [&](int rb, int kind) { return pa.counters + ((long long)rb * NCNT + kind) * 32; };
    const int g = blockIdx.x, G = gridDim.x;
    // test support (option "persistent" = 3 of a fault-injection process): this workgroup leaves without handing on -- its peers'
    // bounded waits elapse, the abort word is set, the launch drains and the host redoes the pass per step
    if (pa.inject && g == 0) return;
    // staging: thread = 16 bytes (chunk column sj: tile sj >> 2, floats 4 (sj & 3) ..) of the rows sr + 8 i
    const int sj = tid & 31, sr = tid >> 5, stl = sj >> 2, skc = sj & 3;
    const int st_off = stl * PS_TILE_BYTES + sr * 32 + (skc & 1) * 8;          // + row-dependent half, below
    const int fr_off = l31 * 32 + (((lh ^ (l31 >> 4)) & 1) * 16);
    float* const s_gate = reinterpret_cast<float*>(s_buf);                      // [gate][row][unit]
    const int eu = tid & 31, er = tid >> 5;                                     // cell epilogue: unit eu of rows er + 8 i

    // One cell: tile (rb, ug) at one time step.  x rows: xbase + row * xld (width kx; x_handoff: written inside this launch);
    // h rows of the previous step: hprev + row * hld.  Output h -> hout + row * hld (+ unit).  creg: the cell state of this thread's
    // four (row, unit) elements (creg[256 i], written and read by this thread only).
    auto cell = [&](const PersistLayer& L, const int kx, const float* xbase, const long long xld, const bool x_handoff, const float* hprev,
                    float* hout, const long long hld, const int rb, const int ug, const bool first, float* creg, unsigned* done,
                    const Dep dx, const Dep dh, const Dep d3) {
        const int c0 = kx / 16;
        const int nt = first ? c0 : L.Kt / 16;                      // zero initial state: the recurrent segment is skipped
        const int nch = (nt + PS_CT - 1) / PS_CT;
        // this lane's weight row (gate `wave`, unit l31 of the group), its 8 k of every tile
        const float* b = L.w + ((long long)((ug * 4 + wave) * 32 + l31)) * L.Kt + 8 * lh;
        f32x4 ring[PS_RING][2];
#pragma unroll
        for (int q = 0; q < PS_RING; ++q) {
            const int kt = q < nt ? q : nt - 1;
            ring[q][0] = *reinterpret_cast<const f32x4*>(b + (long long)kt * 16);
            ring[q][1] = *reinterpret_cast<const f32x4*>(b + (long long)kt * 16 + 4);
        }
        wait_deps(dx, dh, d3, abort_w, &s_ok);
        float bias_v = 0.0f;
        if (tid < 128) bias_v = L.bias[(long long)ug * 128 + tid];
        const float* xr[4]; const float* hr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int row = rb * 32 + sr + 8 * i; row = row < B ? row : B - 1;       // (a ragged last block computes padding rows and stores none)
            xr[i] = xbase + (long long)row * xld + 4 * skc;
            hr[i] = first ? xr[i] : hprev + (long long)row * hld + 4 * skc;
        }
        f32x4 gt[4];
        auto load_chunk = [&](const int ch) {
            int kt = ch * PS_CT + stl; kt = kt < nt ? kt : nt - 1;
            const bool inx = kt < c0;
            const int ko = (inx ? kt : kt - c0) * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* p = (inx ? xr[i] : hr[i]) + ko;
                if (inx && !x_handoff) gt[i] = *reinterpret_cast<const f32x4*>(p);
                else { const float4 v = load_sc1(p); gt[i] = f32x4{v.x, v.y, v.z, v.w}; }
            }
        };
        auto store_chunk = [&](const int buf) {
            char* base = s_buf + buf * PS_BUF_BYTES + st_off;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = sr + 8 * i;
                char* d = base + 8 * i * 32 + ((((skc >> 1) ^ (r >> 4)) & 1) * 16);
                u32x2 p0, p1, p2;
                ps_split4(gt[i], p0, p1, p2);
                *reinterpret_cast<u32x2*>(d) = p0;
                *reinterpret_cast<u32x2*>(d + PS_PLANE_BYTES) = p1;
                *reinterpret_cast<u32x2*>(d + 2 * PS_PLANE_BYTES) = p2;
            }
        };
        load_chunk(0);
        if (tid < 128) s_bias[tid] = bias_v;
        store_chunk(0);
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        // one K tile: the six products in the order of the per-step kernels
        auto tile = [&](const char* buf, const int tl, const int kt) {
            const char* ta = buf + tl * PS_TILE_BYTES + fr_off;
            const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ta);
            const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ta + PS_PLANE_BYTES);
            const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(ta + 2 * PS_PLANE_BYTES);
            u32x2 l0, l1, l2, h0, h1, h2;
            ps_split4(ring[tl % PS_RING][0], l0, l1, l2);
            ps_split4(ring[tl % PS_RING][1], h0, h1, h2);
            const bf16x8 b0 = __builtin_bit_cast(bf16x8, u32x4{l0[0], l0[1], h0[0], h0[1]});
            const bf16x8 b1 = __builtin_bit_cast(bf16x8, u32x4{l1[0], l1[1], h1[0], h1[1]});
            const bf16x8 b2 = __builtin_bit_cast(bf16x8, u32x4{l2[0], l2[1], h2[0], h2[1]});
            const int nx = kt + PS_RING < nt ? kt + PS_RING : nt - 1;          // past the end: a valid, unused re-load
            ring[tl % PS_RING][0] = *reinterpret_cast<const f32x4*>(b + (long long)nx * 16);
            ring[tl % PS_RING][1] = *reinterpret_cast<const f32x4*>(b + (long long)nx * 16 + 4);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);
        };
        for (int ch = 0; ch < nch; ++ch) {
            const bool more = ch + 1 < nch;
            if (more) load_chunk(ch + 1);
            const char* buf = s_buf + (ch & 1) * PS_BUF_BYTES;
            const int kt0 = ch * PS_CT;
            if (kt0 + PS_CT <= nt) {
#pragma unroll
                for (int tl = 0; tl < PS_CT; ++tl) tile(buf, tl, kt0 + tl);
            } else {
#pragma unroll
                for (int tl = 0; tl < PS_CT; ++tl)
                    if (kt0 + tl < nt) tile(buf, tl, kt0 + tl);
            }
            // (buffer (ch + 1) & 1 was last read for chunk ch - 1: every wave has passed the barrier behind it)
            if (more) store_chunk((ch + 1) & 1);
            __syncthreads();
        }
        // gate `wave` of (row = (r & 3) + 8 (r >> 2) + 4 lh, unit = l31) -> LDS (buffer 0: every fragment read lies behind the last barrier)
#pragma unroll
        for (int r = 0; r < 16; ++r) s_gate[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + l31] = acc[r];
        __syncthreads();
        const float bi = s_bias[eu], bf_ = s_bias[32 + eu], bg = s_bias[64 + eu], bo = s_bias[96 + eu];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = er + 8 * i, row = rb * 32 + r;
            const float zi = s_gate[(0 * 32 + r) * 32 + eu] + bi, zf = s_gate[(1 * 32 + r) * 32 + eu] + bf_;
            const float zg = s_gate[(2 * 32 + r) * 32 + eu] + bg, zo = s_gate[(3 * 32 + r) * 32 + eu] + bo;
            const LstmCellOut c = lstm_cell(zi, zf, zg, zo, first ? 0.0f : creg[256 * i]);
            creg[256 * i] = c.c;
            if (row < B) store_sc1(hout + (long long)row * hld + ug * 32 + eu, c.h);
        }
        publish(done);          // (its barrier also keeps the next cell's staging stores behind these reads of the gates)
    };
    auto store_cfin = [&](const int slot, const int rb, const int ug, const float* creg) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = rb * 32 + er + 8 * i;
            if (row < B) pa.cfin[(long long)slot * B * W + (long long)row * W + ug * 32 + eu] = creg[256 * i];
        }
    };

    // ---- phase A: layer 1, forward and backward
    {
        const long long hld = (long long)T * 2 * W, xld = (long long)T * W;
        for (int st = 0; st < T; ++st) {
            for (int i = 0; i < PS_MAXT; ++i) {
                const int tile_id = g + i * G;
                if (tile_id >= 2 * NT) break;
                const int dir = tile_id / NT, rb = (tile_id % NT) / NUG, ug = tile_id % NUG;
                const int t = dir == 0 ? st : T - 1 - st, tp = dir == 0 ? t - 1 : t + 1;
                float* H = pa.H1 + dir * W;
                const Dep dh = st > 0 ? Dep{counter(rb, dir), (unsigned)(st * NUG)} : Dep{nullptr, 0};
                cell(pa.l1[dir], W, pa.x0 + (long long)t * W, xld, false, H + (long long)tp * 2 * W, H + (long long)t * 2 * W, hld, rb, ug,
                     st == 0, &s_creg[i][0][tid], counter(rb, dir), Dep{nullptr, 0}, dh, Dep{nullptr, 0});
                if (st == T - 1) store_cfin(dir == 0 ? D : 0, rb, ug, &s_creg[i][0][tid]);            // final cell state of this direction
            }
        }
    }
    // ---- phase B: layers 2..D along anti-diagonals
    if (D >= 2) {
        for (int k = 0; k < T + D - 2; ++k) {
            for (int i = 0; i < PS_MAXT; ++i) {
                const int tile_id = g + i * G;
                if (tile_id >= (D - 1) * NT) break;
                const int n = 2 + tile_id / NT, rb = (tile_id % NT) / NUG, ug = tile_id % NUG;
                const int t = k - (n - 2);
                if (t < 0 || t >= T) continue;
                const int win = n == 2 ? 2 * W : W;
                const float* xin = n == 2 ? pa.H1 : pa.Hn[n - 3];
                float* H = pa.Hn[n - 2];
                const long long xld = (long long)T * win, hld = (long long)T * W;
                Dep dx;
                const Dep dh = t > 0 ? Dep{counter(rb, n), (unsigned)(t * NUG)} : Dep{nullptr, 0};
                if (n == 2) dx = Dep{counter(rb, 1), (unsigned)((T - t) * NUG)};       // backward output of time t (the forward one came earlier)
                else dx = Dep{counter(rb, n - 1), (unsigned)((t + 1) * NUG)};
                const Dep dfw = n == 2 ? Dep{counter(rb, 0), (unsigned)((t + 1) * NUG)} : Dep{nullptr, 0};
                cell(pa.ln[n - 2], win, xin + (long long)t * win, xld, true, H + (long long)(t - 1) * W, H + (long long)t * W, hld, rb, ug,
                     t == 0, &s_creg[i][0][tid], counter(rb, n), dx, dh, dfw);
                if (t == T - 1) store_cfin(n - 1, rb, ug, &s_creg[i][0][tid]);
            }
        }
    }
}

int persist_split_encode_blocks_per_cu() { return persist_blocks_per_cu(persist_split_encode_kernel, PS_LDS_BYTES, 2); }
int persist_split_enc_max_tiles() { return PS_MAXT; }

size_t persist_split_enc_counter_bytes(int B, int D) { return persist_counters_bytes((size_t)((B + 31) / 32) * (D + 1)); }

int launch_persist_split_encode(const PersistSplitEncArgs& pa, int grid, hipStream_t stream) {
    if (grid < 1 || pa.W % 32 || pa.D < 1 || pa.D > 8) return -1;
    hipLaunchKernelGGL(persist_split_encode_kernel, dim3(grid), dim3(256), PS_LDS_BYTES, stream, pa);
    return 0;
}

}  // namespace casv
