// The vote over N candidate lines per source: consensus_dist_kernel fills every source's matrix of unit-cost
// Levenshtein distances between its candidates, consensus_risk_kernel turns a matrix into each candidate's expected distance to the
// others and picks the smallest.  The distances are integers; the risks are float64 sums in a fixed order without contraction,
// so every output is a function of the source's candidates, lengths and weights alone, whatever B, N, L and the launch shape.
#include "common.h"
#include "sample_row.h"

namespace casv {

// v of lane l - 1 (lane 0: 0): a DPP move over the whole wave (wave_shr:1), no LDS crossbar as __shfl_up's ds_bpermute
__device__ __forceinline__ int lane_below(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }

// D[la][lb] of the strings a (la >= 1 symbols) and b (lb >= 1), both in global memory, by one 64-lane wave on its own LDS
// (consensus_lds_bytes): both strings are staged once, beside b's symbols lies one DP row.
//   The rows are taken in strips of 64: lane l owns row r = 64 * strip + l + 1 and walks it left to right, one anti-diagonal of the
// strip per step -- at step t it stands in column c = t - l + 1.  Of the three cells it reads, D[r][c-1] is its own last result,
// D[r-1][c] is what the lane below it computed one step earlier (one cross-lane move), and D[r-1][c-1] is what that move
// delivered the step before.  Lane 0 reads its upper row from LDS: row 0 (D[0][c] = c) in the first strip, then what lane 63
// of the strip before left there.  Lane 63 overwrites an entry 63 steps after lane 0 has read it, so one row serves both.
//   LDS: col[k] = {b[k], D[64 * strip][k + 1]} for column k + 1, one 8-byte read per lane and step at col[t - l], fetched one step
// ahead (what it holds depends on t and the lane alone, so the read is off the chain cur -> cur).  CONSENSUS_GUARD entries in front
// of col[0] and behind col[lb - 1] take the reads of the lanes that stand outside the matrix; such a lane (a row beyond la, a
// column outside 1 .. lb) throws the value away, keeps its registers and stores nothing.  Nothing beyond la / lb symbols is loaded.
__device__ __forceinline__ int consensus_pair(const int* __restrict__ ga, int la, const int* __restrict__ gb, int lb, int* lds, int lane) {
    int2* col = reinterpret_cast<int2*>(lds) + CONSENSUS_GUARD;
    int* sa = lds + 2 * (lb + 2 * CONSENSUS_GUARD);
    wave_lds_handover();                         // (the pair before this one has read its last LDS word)
    for (int k = lane; k < la; k += 64) sa[k] = ga[k];
    for (int k = lane; k < lb; k += 64) col[k] = make_int2(gb[k], k + 1);
    wave_lds_handover();
    const int strips = (la + 63) >> 6;
    int cur = 0;
    for (int s = 0; s < strips; ++s) {
        const int rows = min(64, la - s * 64);   // rows of this strip: only the last one may be short
        const int r = s * 64 + lane + 1;
        const bool row = lane < rows;
        const int ca = row ? sa[r - 1] : 0;
        int diag = r - 1;                        // D[r-1][0]
        cur = r;                                 // D[r][0]
        const int steps = lb + rows - 1;
        const int2* p = col - lane;              // col[t - lane] of step t = 0
        int2 next = *p;
        for (int t = 0; t < steps; ++t) {
            const int k = t - lane;              // column k + 1
            const bool on = row && (unsigned)k < (unsigned)lb;
            const int2 now = next;
            next = *++p;                         // (lane 0 reads col[t + 1] here; lane 63 writes col[t - 63] below)
            const int below = lane_below(cur);   // (by all lanes: a lane that is switched off is not read)
            const int up = lane == 0 ? now.y : below;
            const int best = min(min(up, cur) + 1, diag + (ca != now.x ? 1 : 0));
            if (on) { cur = best; diag = up; }
            if (on && lane == 63) col[k].y = best;
        }
        wave_lds_handover();                     // lane 63's row -> lane 0 of the next strip
    }
    return __shfl(cur, (la - 1) & 63);           // the lane of row la stands in column lb
}

// Grid (N, N, consensus_grid_z(B, N)), 64 threads: the block (j, i) with i <= j owns the pair of every source b = z, z + gridDim.z, ...
__global__ __launch_bounds__(64) void consensus_dist_kernel(ConsensusArgs a) {
    extern __shared__ __align__(16) int consensus_lds[];
    const int i = blockIdx.y, j = blockIdx.x, lane = threadIdx.x, N = a.N;
    if (i > j) return;
    for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
        const int* len = a.len + (long long)b * N;
        const int li = len[i], lj = len[j];
        int d;
        if (li < 0 || lj < 0) d = -1;            // a padding row or column
        else if (i == j) d = 0;
        else if (li == 0 || lj == 0) d = max(li, lj);
        else {
            const int* si = a.sym + ((long long)b * N + i) * a.L;
            const int* sj = a.sym + ((long long)b * N + j) * a.L;
            // (the distance is symmetric: the rows go to the string that makes fewer steps of it)
            const bool rows_i = ((li + 63) >> 6) * (lj + 63) <= ((lj + 63) >> 6) * (li + 63);
            d = consensus_pair(rows_i ? si : sj, rows_i ? li : lj, rows_i ? sj : si, rows_i ? lj : li, consensus_lds, lane);
        }
        if (lane == 0) {
            int* D = a.dist + (long long)b * N * N;
            D[i * N + j] = d;
            D[j * N + i] = d;
        }
    }
}

// One workgroup of 256 threads per source (b = blockIdx.x, + gridDim.x, ...); thread c < N owns candidate c.  risk[c] = the sum
// over the live candidates k in ascending order of w[k] * d (mode 0) or w[k] * (d / max(len[c], len[k], 1)) (mode 1),
// d = (double)D[c][k], one rounding per operation; then thread 0 takes the first live candidate of the smallest risk.
__global__ __launch_bounds__(256) void consensus_risk_kernel(ConsensusArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_risk[CONSENSUS_MAX_N];
    __shared__ int s_len[CONSENSUS_MAX_N];
    const int c = threadIdx.x, N = a.N;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int* len = a.len + (long long)b * N;
        const int* D = a.dist + (long long)b * N * N;
        const double* w = a.weight ? a.weight + (long long)b * N : nullptr;
        if (c < N) s_len[c] = len[c];
        __syncthreads();
        if (c < N) {
            const int lc = s_len[c];
            double risk = __builtin_inf();
            if (lc >= 0) {
                risk = 0.0;
                for (int k = 0; k < N; ++k) {
                    const int lk = s_len[k];
                    if (lk < 0) continue;
                    double d = (double)D[k * N + c];         // (= D[c][k]: the kernel above wrote both; this one is coalesced)
                    if (a.mode == 1) d = d / (double)max(max(lc, lk), 1);
                    const double term = (w ? w[k] : 1.0) * d;
                    risk = risk + term;
                }
            }
            s_risk[c] = risk;
            a.risk[(long long)b * N + c] = risk;
        }
        __syncthreads();
        if (c == 0) {
            int pick = -1;
            double best = 0.0;
            for (int k = 0; k < N; ++k)
                if (s_len[k] >= 0 && (pick < 0 || s_risk[k] < best)) { pick = k; best = s_risk[k]; }
            a.pick[b] = pick;
        }
        __syncthreads();                                     // (thread 0 has read the lengths and risks of this source)
    }
}

static LdsAttribute consensus_attr;
bool consensus_ready() {
    return gemm_dynamic_lds(consensus_attr, reinterpret_cast<const void*>(&consensus_dist_kernel), consensus_lds_bytes(CONSENSUS_MAX_L));
}

void launch_consensus_dist(const ConsensusArgs& a, int max_len, hipStream_t stream) {
    hipLaunchKernelGGL(consensus_dist_kernel, dim3(a.N, a.N, consensus_grid_z(a.B, a.N)), dim3(64), (size_t)consensus_lds_bytes(max_len), stream, a);
}

void launch_consensus_risk(const ConsensusArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(consensus_risk_kernel, dim3(std::min(a.B, 65535)), dim3(256), 0, stream, a);
}

}  // namespace casv
