// The row code of the sampling pick, shared by sample_kernel (sample_kernels.hip: the decode path) and sched_mix_kernel
// (sched_kernels.hip: scheduled sampling inside the train step): the counter-based generator, the row's staging pass and the
// ordered draw.  One 64-lane wave owns one row; the row lies in the wave's own Vp floats of LDS.
#pragma once
#include "common.h"
#include "alt_order.h"
#include "row_kernels.h"
#include <math.h>

namespace casv {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32x32 -> 64
// multiplications on the counter (c0, c1, c2, c3), the key (k0, k1) bumped by the Weyl constants between rounds.
struct Philox4 { unsigned o0, o1, o2, o3; };
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    return Philox4{c0, c1, c2, c3};
}
// The first output word is all the decode path's draw needs.
__device__ __forceinline__ unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    return philox4x32_10(c0, c1, c2, c3, k0, k1).o0;
}
// a generator word as a uniform in [0, 1): its upper 24 bits
__device__ __forceinline__ float philox_uniform(unsigned o) { return (float)(o >> 8) * 0x1p-24f; }

// Pass 1 of a row: x[0 .. V) into the wave's LDS row s (every lane the entries v = lane, lane + 64, ...); the maximum m over all
// V, m_C over the candidates' range 1 .. V-1, and whether the row can be drawn from: no NaN, m_C finite.  The same in every lane.
struct SampleRowStats { float m, mc; bool valid; };
__device__ __forceinline__ SampleRowStats sample_row_stage(const float* __restrict__ x, float* s, int V, int lane) {
    float m = -INFINITY, mc = -INFINITY;
    int nan = 0;
    for (int v = lane; v < V; v += 64) {
        const float xv = x[v];
        s[v] = xv; nan |= xv != xv; m = fmaxf(m, xv);       // (fmaxf passes a NaN by)
        if (v >= 1) mc = fmaxf(mc, xv);
    }
    m = wave_butterfly(m, [](float p, float q) { return fmaxf(p, q); });
    mc = wave_butterfly(mc, [](float p, float q) { return fmaxf(p, q); });
    nan = wave_butterfly(nan, [](int p, int q) { return p | q; });
    return SampleRowStats{m, mc, !nan && mc > -INFINITY && mc < INFINITY};
}

// Pass 3 of a valid row staged in s (sample_kernels.hip numbers the passes): the bound of the top_k candidates, by top_k rounds of
// the wave-wide maximum over the keys strictly below the previous winner's.  The candidates are the indices >= 1 whose key is no
// smaller than the bound; 0 = all of them.
__device__ __forceinline__ unsigned long long sample_row_bound(const float* s, int V, int lane, int top_k) {
    unsigned long long kth = 0ull;
    if (top_k > 0 && top_k < V - 1) {
        unsigned long long prev = ~0ull;
        for (int j = 0; j < top_k; ++j) {
            unsigned long long top = 0ull;
            for (int v = lane < 1 ? 64 : lane; v < V; v += 64) {
                const unsigned long long key = alt_key(s[v], v);
                if (key < prev && key > top) top = key;
            }
            prev = wave_max_key(top);           // (top_k < V - 1: every round finds one)
        }
        kth = prev;
    }
    return kth;
}

// LDS entries written by one lane of the wave and read by another: a wavefront fence, no workgroup barrier
__device__ __forceinline__ void wave_lds_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Passes 4 and 5 under the bound kth: the weights w = expf((x - m_C) / temperature) of the candidates over the row in LDS, the
// ordered float64 prefix sum and the pick for the uniform u.  *Z: the total.
__device__ __forceinline__ int sample_row_draw_under(float* s, int V, int lane, unsigned long long kth, float temperature, float mc, float u,
                                                     double* Zout) {
    for (int v = lane; v < V; v += 64) {
        const float xv = s[v];
        s[v] = (v >= 1 && alt_key(xv, v) >= kth) ? expf((xv - mc) / temperature) : 0.f;
    }
    wave_lds_handover();
    const int chunk = (V + 63) >> 6;
    const int lo = lane * chunk, hi = min(V, lo + chunk);
    double c = 0.0;
    int last = -1;
    for (int v = lo; v < hi; ++v) { const float w = s[v]; c += (double)w; if (w > 0.f) last = v; }
    double off = 0.0, Z = 0.0;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        const double cj = __shfl(c, j, 64);
        if (j < lane) off += cj;
        Z += cj;
    }
    *Zout = Z;
    const double target = (double)u * Z;
    const unsigned long long holders = __ballot(off + c > target);
    if (holders) {
        const int holder = __ffsll((long long)holders) - 1;
        int mine = last;
        if (lane == holder) {
            double run = 0.0;
            for (int v = lo; v < hi; ++v) {
                const float w = s[v];
                if (w > 0.f) { run += (double)w; if (off + run > target) { mine = v; break; } }
            }
        }
        return __shfl(mine, holder, 64);
    }
    return wave_butterfly(last, [](int p, int q) { return max(p, q); });
}

// Passes 3 to 5 of the pick without a nucleus and with top_k <= 64 (sample_kernel, sched_mix_kernel)
__device__ __forceinline__ int sample_row_draw(float* s, int V, int lane, int top_k, float temperature, float mc, float u, double* Zout) {
    return sample_row_draw_under(s, V, lane, sample_row_bound(s, V, lane, top_k), temperature, mc, u, Zout);
}

// Pass 3 under a cut (top_k, top_p) (sample_cut_kernel, sched_mix_cut_kernel): the bound from
// the row's keys SORTED by the wave in its own P entries of LDS, P = the power of two >= V (sample_cut_sort_size).
//   a. keys[v] = alt_key of the candidates 1 .. V-1, 0 at index 0 and at the padding V .. P-1 (below every key of a valid row); a
//      bitonic network, descending: log2(P) (log2(P) + 1) / 2 stages, every lane the pairs p = lane, lane + 64, ... of the P / 2 of
//      a stage, a handover between stages.  Place j of the sorted keys is rank j; top_k > 0 keeps n = min(top_k, V - 1) places.
//   b. top_p < 1: lane l owns the places [l * ceil(V / 64), (l + 1) * ceil(V / 64)) below n, their weights summed in ascending
//      order in float64, the lanes' offsets by one sequential pass over the lanes -- pass 5's scan on places instead of indices;
//      the nucleus ends at the first place j with P_j >= (double)top_p * Z_s, which exists (P_{n-1} = Z_s, the same additions)
//      and has a positive weight (a P_j that first reaches a positive target has just grown).
// Returns the key of the last place kept, 0 where all V - 1 candidates are.  LDS banking: the 8-byte keys of a stage with
// distance >= 32 are read by consecutive lanes at consecutive entries (conflict-free for ds_read_b64: a half-wave covers one 256-byte
// bank row); below that a half-wave's 32 lower (or upper) entries spread over 64 entries = two bank rows, a 2-way conflict.  The
// rank-order scan of (b) strides the lanes by ceil(V / 64) entries like pass 5: the same known conflict.
__device__ __forceinline__ unsigned long long sample_row_cut_bound(const float* s, unsigned long long* keys, int V, int P, int lane, int top_k,
                                                                   float top_p, float temperature, float mc) {
    for (int v = lane; v < P; v += 64) keys[v] = (v >= 1 && v < V) ? alt_key(s[v], v) : 0ull;
    wave_lds_handover();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = lane; p < (P >> 1); p += 64) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), o = i | j;       // (i < o < P: p < P / 2, j <= P / 2)
                const unsigned long long ki = keys[i], ko = keys[o];
                if ((i & k) == 0 ? ki < ko : ki > ko) { keys[i] = ko; keys[o] = ki; }
            }
            wave_lds_handover();
        }
    const int nc = V - 1;
    int n = top_k > 0 && top_k < nc ? top_k : nc;
    if (top_p < 1.f) {
        const int chunk = (V + 63) >> 6;
        const int lo = min(n, lane * chunk), hi = min(n, lo + chunk);
        double c = 0.0;
        for (int j = lo; j < hi; ++j) c += (double)expf((s[0xffffffffu - (unsigned)keys[j]] - mc) / temperature);
        double off = 0.0, Z = 0.0;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const double cj = __shfl(c, j, 64);
            if (j < lane) off += cj;
            Z += cj;
        }
        const double target = (double)top_p * Z;
        const unsigned long long holders = __ballot(off + c >= target);
        const int holder = holders ? __ffsll((long long)holders) - 1 : 63;
        int mine = n - 1;
        if (holders && lane == holder) {
            double run = 0.0;
            for (int j = lo; j < hi; ++j) {
                run += (double)expf((s[0xffffffffu - (unsigned)keys[j]] - mc) / temperature);
                if (off + run >= target) { mine = j; break; }
            }
        }
        n = __shfl(mine, holder, 64) + 1;
    }
    return n < nc ? keys[n - 1] : 0ull;
}

}  // namespace casv
