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
//   The costed form (include/cor_asv_ann_hip.h, casv_edit_costs) is the same sweep with gap for the 1 of an
// insertion or deletion and c(x, y) for the substitution.  Its column entry is {b[k], D, key of b[k], unused}: 16 bytes, still one
// aligned LDS read per lane and step (ds_read_b128; a 12-byte entry would need two, as a b96 read wants 16-byte alignment); a's
// symbols and keys do not pass through LDS -- a lane loads those of its own row from global memory, coalesced, once per strip.
template <bool COSTED> struct PairForm { using Entry = int2; };
template <> struct PairForm<true> { using Entry = int4; };
__device__ __forceinline__ int2 pair_entry(int2*, int sym, int d, int) { return make_int2(sym, d); }
__device__ __forceinline__ int4 pair_entry(int4*, int sym, int d, int key) { return make_int4(sym, d, key, 0); }
// c(x, y) of the costed form: 0 for equal symbols whatever the keys, else near for equal keys, else sub
__device__ __forceinline__ int edit_cost(int x, int kx, const int4& y, const EditCosts& ec) { return x == y.x ? 0 : (kx == y.z ? ec.near : ec.sub); }

template <bool COSTED>
__device__ __forceinline__ int consensus_pair(const int* __restrict__ ga, const int* __restrict__ gka, int la, const int* __restrict__ gb,
                                              const int* __restrict__ gkb, int lb, int* lds, int lane, const EditCosts& ec) {
    using Entry = typename PairForm<COSTED>::Entry;
    Entry* col = reinterpret_cast<Entry*>(lds) + CONSENSUS_GUARD;
    int* sa = lds + 2 * (lb + 2 * CONSENSUS_GUARD);      // (the plain form only)
    const int gap = COSTED ? ec.gap : 1;
    wave_lds_handover();                         // (the pair before this one has read its last LDS word)
    if constexpr (!COSTED)
        for (int k = lane; k < la; k += 64) sa[k] = ga[k];
    for (int k = lane; k < lb; k += 64) col[k] = pair_entry(col, gb[k], (k + 1) * gap, COSTED ? gkb[k] : 0);
    wave_lds_handover();
    const int strips = (la + 63) >> 6;
    int cur = 0;
    for (int s = 0; s < strips; ++s) {
        const int rows = min(64, la - s * 64);   // rows of this strip: only the last one may be short
        const int r = s * 64 + lane + 1;
        const bool row = lane < rows;
        int ca, ka = 0;
        if constexpr (COSTED) { ca = row ? ga[r - 1] : 0; ka = row ? gka[r - 1] : 0; }
        else ca = row ? sa[r - 1] : 0;
        int diag = (r - 1) * gap;                // D[r-1][0]
        cur = r * gap;                           // D[r][0]
        const int steps = lb + rows - 1;
        const Entry* p = col - lane;             // col[t - lane] of step t = 0
        Entry next = *p;
        for (int t = 0; t < steps; ++t) {
            const int k = t - lane;              // column k + 1
            const bool on = row && (unsigned)k < (unsigned)lb;
            const Entry now = next;
            next = *++p;                         // (lane 0 reads col[t + 1] here; lane 63 writes col[t - 63] below)
            const int below = lane_below(cur);   // (by all lanes: a lane that is switched off is not read)
            const int up = lane == 0 ? now.y : below;
            int c;
            if constexpr (COSTED) c = edit_cost(ca, ka, now, ec);
            else c = ca != now.x ? 1 : 0;
            const int best = min(min(up, cur) + gap, diag + c);
            if (on) { cur = best; diag = up; }
            if (on && lane == 63) col[k].y = best;
        }
        wave_lds_handover();                     // lane 63's row -> lane 0 of the next strip
    }
    return __shfl(cur, (la - 1) & 63);           // the lane of row la stands in column lb
}

// Grid (N, N, consensus_grid_z(B, N)), 64 threads: the block (j, i) with i <= j owns the pair of every source b = z, z + gridDim.z, ...
template <bool COSTED>
__device__ __forceinline__ void consensus_dist_body(const ConsensusArgs& a, int* lds) {
    const int i = blockIdx.y, j = blockIdx.x, lane = threadIdx.x, N = a.N;
    if (i > j) return;
    for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
        const int* len = a.len + (long long)b * N;
        const int li = len[i], lj = len[j];
        int d;
        if (li < 0 || lj < 0) d = -1;            // a padding row or column
        else if (i == j) d = 0;
        else if (li == 0 || lj == 0) d = max(li, lj) * (COSTED ? a.costs.gap : 1);
        else {
            const long long at_i = ((long long)b * N + i) * a.L, at_j = ((long long)b * N + j) * a.L;
            const int* si = a.sym + at_i;
            const int* sj = a.sym + at_j;
            const int* ki = COSTED ? a.key + at_i : nullptr;
            const int* kj = COSTED ? a.key + at_j : nullptr;
            // (the distance is symmetric: the rows go to the string that makes fewer steps of it)
            const bool rows_i = ((li + 63) >> 6) * (lj + 63) <= ((lj + 63) >> 6) * (li + 63);
            d = consensus_pair<COSTED>(rows_i ? si : sj, rows_i ? ki : kj, rows_i ? li : lj, rows_i ? sj : si, rows_i ? kj : ki, rows_i ? lj : li,
                                       lds, lane, a.costs);
        }
        if (lane == 0) {
            int* D = a.dist + (long long)b * N * N;
            D[i * N + j] = d;
            D[j * N + i] = d;
        }
    }
}

__global__ __launch_bounds__(64) void consensus_dist_kernel(ConsensusArgs a) {
    extern __shared__ __align__(16) int consensus_lds[];
    consensus_dist_body<false>(a, consensus_lds);
}

// The costed form (casv_consensus_costed): a.key and a.costs are read, the LDS is consensus_costed_lds_bytes
__global__ __launch_bounds__(64) void consensus_dist_costed_kernel(ConsensusArgs a) {
    extern __shared__ __align__(16) int consensus_lds[];
    consensus_dist_body<true>(a, consensus_lds);
}

// One workgroup of 256 threads per source (b = blockIdx.x, + gridDim.x, ...); thread c < N owns candidate c.  risk[c] = the sum
// over the live candidates k in ascending order of w[k] * d (mode 0) or w[k] * (d / (unit * max(len[c], len[k], 1))) (mode 1),
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
                    if (a.mode == 1) d = d / (double)(a.costs.unit * max(max(lc, lk), 1));     // (unit = 1 in the plain call: the same double)
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

// ---------------------------------------------------------------------------------------------------------------------------------
// The confusion network: every candidate aligned to its source's pivot, the columns, the vote per column.

// consensus_pair's sweep with the pivot p (lp >= 1 symbols) as rows and the candidate c (lc >= 1) as columns, keeping the path: per
// cell (i, j), i, j >= 1, two bits -- "diagonal holds", D[i][j] == D[i-1][j-1] + (p[i-1] != c[j-1]), and "pivot-against-gap holds",
// D[i][j] == D[i-1][j] + 1.  A lane collects the bits of its row in two registers, bit (j - 1) & 31 each, and stores them as one
// 8-byte word {diagonal, gap} per 32 columns (and at the row's end) to dir[(i - 1) * wpr + ((j - 1) >> 5)]: every word the walk can
// read is written, whole, by one vector store.
//   The costed form as in consensus_pair: the bits are "D[i][j] == D[i-1][j-1] + c(p[i-1], c[j-1])" and "D[i][j] == D[i-1][j] + gap".
template <bool COSTED>
__device__ __forceinline__ void consensus_align_fill(const int* __restrict__ gp, const int* __restrict__ gkp, int lp, const int* __restrict__ gc,
                                                     const int* __restrict__ gkc, int lc, int* lds, int lane, uint2* dir, int wpr,
                                                     const EditCosts& ec) {
    using Entry = typename PairForm<COSTED>::Entry;
    Entry* col = reinterpret_cast<Entry*>(lds) + CONSENSUS_GUARD;
    int* sa = lds + 2 * (lc + 2 * CONSENSUS_GUARD);      // (the plain form only)
    const int gap = COSTED ? ec.gap : 1;
    wave_lds_handover();                         // (the pair before this one has read its last LDS word)
    if constexpr (!COSTED)
        for (int k = lane; k < lp; k += 64) sa[k] = gp[k];
    for (int k = lane; k < lc; k += 64) col[k] = pair_entry(col, gc[k], (k + 1) * gap, COSTED ? gkc[k] : 0);
    wave_lds_handover();
    const int strips = (lp + 63) >> 6;
    for (int s = 0; s < strips; ++s) {
        const int rows = min(64, lp - s * 64);
        const int r = s * 64 + lane + 1;
        const bool row = lane < rows;
        int ca, ka = 0;
        if constexpr (COSTED) { ca = row ? gp[r - 1] : 0; ka = row ? gkp[r - 1] : 0; }
        else ca = row ? sa[r - 1] : 0;
        uint2* words = dir + (size_t)(row ? r - 1 : 0) * wpr;
        int diag = (r - 1) * gap, cur = r * gap;
        unsigned wd = 0, wu = 0;
        const int steps = lc + rows - 1;
        const Entry* p = col - lane;
        Entry next = *p;
        for (int t = 0; t < steps; ++t) {
            const int k = t - lane;              // column k + 1
            const bool on = row && (unsigned)k < (unsigned)lc;
            const Entry now = next;
            next = *++p;
            const int below = lane_below(cur);
            const int up = lane == 0 ? now.y : below;
            int c;
            if constexpr (COSTED) c = edit_cost(ca, ka, now, ec);
            else c = ca != now.x ? 1 : 0;
            const int sub = diag + c;
            const int best = min(min(up, cur) + gap, sub);
            if (on) {
                const unsigned bit = 1u << (k & 31);
                if (best == sub) wd |= bit;
                if (best == up + gap) wu |= bit;
                cur = best; diag = up;
                if ((k & 31) == 31 || k == lc - 1) { words[k >> 5] = make_uint2(wd, wu); wd = 0; wu = 0; }
            }
            if (on && lane == 63) col[k].y = best;
        }
        wave_lds_handover();                     // lane 63's row -> lane 0 of the next strip
    }
}

// The walk of DESIGN.md section 4.10 from (lp, lc) to (0, 0) by one lane: where[j] per candidate symbol, and per slot the length of
// the run of insertions there (a slot's insertions are consecutive steps: once i has gone down it does not come back) as a maximum
// over the source's candidates.  lp + lc dependent steps; a direction word is read again only when the row or the word changes.
__device__ __forceinline__ void consensus_align_walk(const uint2* dir, int wpr, int lp, int lc, int* where, int* ins) {
    int i = lp, j = lc, run = 0, have_row = -1, have_word = -1;
    uint2 w = make_uint2(0u, 0u);
    while (j > 0) {
        if (i == 0) { where[j - 1] = -1; ++run; --j; continue; }           // (in front of the pivot's first symbol: slot 0)
        const int word = (j - 1) >> 5;
        if (have_row != i || have_word != word) { w = dir[(size_t)(i - 1) * wpr + word]; have_row = i; have_word = word; }
        const unsigned bit = 1u << ((j - 1) & 31);
        if ((w.x | w.y) & bit) {
            if (run) { atomicMax(ins + i, run); run = 0; }
            if (w.x & bit) { where[j - 1] = i - 1; --j; }
            --i;
        } else { where[j - 1] = -1 - i; ++run; --j; }
    }
    if (run) atomicMax(ins + i, run);
}

// Grid (N, sources side by side), 64 threads: the wave of block (c, y) owns candidate c of the sources b = b0 + y, + gridDim.y, ...
// below b1 -- its row of `where` whole (CASV_ALIGN_NONE beyond the length, the identity for the pivot itself), and for a live
// candidate other than the pivot the fill into the pair's own direction words, then the walk.
template <bool COSTED>
__device__ __forceinline__ void consensus_align_body(const AlignArgs& a, int* consensus_lds) {
    const int c = blockIdx.x, lane = threadIdx.x, N = a.N;
    for (int b = a.b0 + blockIdx.y; b < a.b1; b += gridDim.y) {
        const int piv = a.pivot[b];
        const int lc = a.len[(long long)b * N + c];
        int* where = a.where + ((long long)b * N + c) * a.L;
        const bool live = piv >= 0 && lc >= 0;
        for (int j = (live ? lc : 0) + lane; j < a.L; j += 64) where[j] = CASV_ALIGN_NONE_VALUE;
        if (!live) continue;
        if (c == piv) {
            for (int j = lane; j < lc; j += 64) where[j] = j;
            continue;
        }
        const int lp = a.len[(long long)b * N + piv];
        uint2* dir = a.dir + ((size_t)(b - a.b0) * N + c) * ((size_t)a.rows * a.wpr);
        const long long t0 = a.stamps ? clock64() : 0;
        if (lp > 0 && lc > 0) {
            const long long at_p = ((long long)b * N + piv) * a.L, at_c = ((long long)b * N + c) * a.L;
            consensus_align_fill<COSTED>(a.sym + at_p, COSTED ? a.key + at_p : nullptr, lp, a.sym + at_c, COSTED ? a.key + at_c : nullptr, lc,
                                         consensus_lds, lane, dir, a.wpr, a.costs);
            __threadfence();                     // the lanes' direction words -> lane 0's reads
            __builtin_amdgcn_wave_barrier();
        }
        const long long t1 = a.stamps ? clock64() : 0;
        if (lane == 0) consensus_align_walk(dir, a.wpr, lp, lc, where, a.ins + (long long)b * a.stride);
        if (a.stamps && lane == 0) {
            atomicAdd(a.stamps, (unsigned long long)(t1 - t0));
            atomicAdd(a.stamps + 1, (unsigned long long)(clock64() - t1));
        }
    }
}

__global__ __launch_bounds__(64) void consensus_align_kernel(AlignArgs a) {
    extern __shared__ __align__(16) int consensus_lds[];
    consensus_align_body<false>(a, consensus_lds);
}

// The costed form (casv_consensus_align_costed): a.key and a.costs are read, the LDS is consensus_costed_lds_bytes
__global__ __launch_bounds__(64) void consensus_align_costed_kernel(AlignArgs a) {
    extern __shared__ __align__(16) int consensus_lds[];
    consensus_align_body<true>(a, consensus_lds);
}

// One wave per source (b = blockIdx.x, + gridDim.x, ...): start[g] = g + ins[0] + ... + ins[g-1], the first column of slot g
// (its insertion columns, then at start[g] + ins[g] the column of pivot symbol g), and ncol = len[pivot] + the sum of all ins.
__global__ __launch_bounds__(64) void consensus_layout_kernel(AlignArgs a) {
    const int lane = threadIdx.x;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int piv = a.pivot[b];
        if (piv < 0) { if (lane == 0) a.ncol[b] = 0; continue; }
        const int lp = a.len[(long long)b * a.N + piv];
        const int* ins = a.ins + (long long)b * a.stride;
        int* start = a.start + (long long)b * a.stride;
        const int n = lp + 1, chunk = (n + 63) >> 6;
        const int lo = min(n, lane * chunk), hi = min(n, lo + chunk);
        int sum = 0;
        for (int g = lo; g < hi; ++g) sum += ins[g];
        int incl = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        int run = incl - sum;
        for (int g = lo; g < hi; ++g) { start[g] = g + run; run += ins[g]; }
        if (lane == 63) a.ncol[b] = lp + incl;
    }
}

// One workgroup of 256 threads per source (b = blockIdx.x, + gridDim.x, ...).  First all threads preset src (-1 live, -2 padding
// or beyond ncol); then thread c < N owns candidate c and puts its symbols where `where` and the layout send
// them, the k-th symbol of a slot in order of j into the slot's k-th column.  Then each of the four waves takes every fourth
// column: the class of candidate c is "gap", or its symbol; c represents its class when no k < c is in it, and then
// mass[c] = the sum of w[k] over the members k in ascending order from +0.0, float64, one rounding per addition; -1.0 otherwise.
// best = the representative of the largest mass, the lowest index among equals.
__global__ __launch_bounds__(256) void consensus_vote_kernel(VoteArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_w[CONSENSUS_MAX_N];
    __shared__ int s_sym[4][CONSENSUS_MAX_N];
    __shared__ int s_cls[4][CONSENSUS_MAX_N];     // 0 a gap, 1 a symbol, 2 no vote (padding, or no column)
    __shared__ int s_fill[CONSENSUS_MAX_N];       // what a candidate's entry of a column holds before its symbols go in: -1 live, -2 padding
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, N = a.N, C = a.C;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int piv = a.pivot[b], ncol = a.ncol[b];
        int* src = a.src + (long long)b * C * N;
        double* mass = a.mass + (long long)b * C * N;
        if (t < N) {
            s_fill[t] = (piv >= 0 && a.len[(long long)b * N + t] >= 0) ? -1 : -2;
            s_w[t] = a.weight ? a.weight[(long long)b * N + t] : 1.0;
        }
        __syncthreads();
        for (long long at = t; at < (long long)C * N; at += 256) src[at] = at < (long long)ncol * N ? s_fill[at % N] : -2;
        __syncthreads();                         // (the presets are in place before a candidate's symbols go over them)
        if (t < N) {
            const int lc = a.len[(long long)b * N + t];
            const bool live = s_fill[t] == -1;
            if (live) {
                const int* where = a.where + ((long long)b * N + t) * a.L;
                const int* start = a.start + (long long)b * a.stride;
                const int* ins = a.ins + (long long)b * a.stride;
                const int lp = a.len[(long long)b * N + piv];
                int prev = CASV_ALIGN_NONE_VALUE, k = 0;
                for (int j = 0; j < lc; ++j) {
                    const int v = where[j];
                    const int g = v >= 0 ? v : -1 - v;       // (the slot: 0 .. lp, below lp for a symbol against the pivot's)
                    if ((unsigned)g > (unsigned)lp - (v >= 0 ? 1u : 0u) || (v >= 0 && lp == 0)) continue;
                    k = (v < 0 && v == prev) ? k + 1 : 0;
                    const int col = start[g] + (v >= 0 ? ins[g] : k);
                    prev = v;
                    if ((unsigned)col < (unsigned)ncol) src[(long long)col * N + t] = j;
                }
            }
        }
        __syncthreads();
        for (int col = wv; col < C; col += 4) {
            if (col >= ncol) {                   // (no column of this source: nobody votes)
                for (int c = lane; c < N; c += 64) mass[(long long)col * N + c] = -1.0;
                if (lane == 0) a.best[(long long)b * C + col] = -1;
                continue;
            }
            for (int c = lane; c < N; c += 64) {
                const int s = src[(long long)col * N + c];
                s_cls[wv][c] = s >= 0 ? 1 : (s == -1 ? 0 : 2);
                s_sym[wv][c] = s >= 0 ? a.sym[((long long)b * N + c) * a.L + s] : 0;
            }
            wave_lds_handover();
            double top = -1.0;
            int top_c = INT32_MAX;
            for (int c = lane; c < N; c += 64) {
                const int cls = s_cls[wv][c], sy = s_sym[wv][c];
                double m = -1.0;
                if (cls != 2) {
                    bool first = true;
                    for (int k = 0; k < c && first; ++k) first = !(s_cls[wv][k] == cls && s_sym[wv][k] == sy);
                    if (first) {
                        m = 0.0;
                        for (int k = c; k < N; ++k)
                            if (s_cls[wv][k] == cls && s_sym[wv][k] == sy) m = m + s_w[k];
                    }
                }
                mass[(long long)col * N + c] = m;
                if (m > top) { top = m; top_c = c; }             // (ascending c: the lower index stays among equals)
            }
            for (int d = 32; d; d >>= 1) {
                const double om = __shfl_xor(top, d);
                const int oc = __shfl_xor(top_c, d);
                if (om > top || (om == top && oc < top_c)) { top = om; top_c = oc; }
            }
            if (lane == 0) a.best[(long long)b * C + col] = top_c == INT32_MAX ? -1 : top_c;
            wave_lds_handover();                 // (the next column overwrites the wave's LDS)
        }
        __syncthreads();                         // (every wave has read this source's weights)
    }
}

static LdsAttribute consensus_attr;
bool consensus_ready() {
    return gemm_dynamic_lds(consensus_attr, reinterpret_cast<const void*>(&consensus_dist_kernel), consensus_lds_bytes(CONSENSUS_MAX_L));
}

void launch_consensus_dist(const ConsensusArgs& a, int max_len, hipStream_t stream) {
    const dim3 grid(a.N, a.N, consensus_grid_z(a.B, a.N));
    if (a.key) hipLaunchKernelGGL(consensus_dist_costed_kernel, grid, dim3(64), (size_t)consensus_costed_lds_bytes(max_len), stream, a);
    else hipLaunchKernelGGL(consensus_dist_kernel, grid, dim3(64), (size_t)consensus_lds_bytes(max_len), stream, a);
}

void launch_consensus_risk(const ConsensusArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(consensus_risk_kernel, dim3(std::min(a.B, 65535)), dim3(256), 0, stream, a);
}

// max_len: the longest live candidate of the call (at most CONSENSUS_ALIGN_MAX_L: within the LDS every kernel may have unasked)
void launch_consensus_align(const AlignArgs& a, int max_len, hipStream_t stream) {
    const dim3 grid(a.N, std::min(a.b1 - a.b0, 65535));
    if (a.key) hipLaunchKernelGGL(consensus_align_costed_kernel, grid, dim3(64), (size_t)consensus_costed_lds_bytes(max_len), stream, a);
    else hipLaunchKernelGGL(consensus_align_kernel, grid, dim3(64), (size_t)consensus_lds_bytes(max_len), stream, a);
}

void launch_consensus_layout(const AlignArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(consensus_layout_kernel, dim3(std::min(a.B, 65535)), dim3(64), 0, stream, a);
}

void launch_consensus_vote(const VoteArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(consensus_vote_kernel, dim3(std::min(a.B, 65535)), dim3(256), 0, stream, a);
}

}  // namespace casv
