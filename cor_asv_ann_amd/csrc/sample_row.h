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

// Passes 3 to 5 of a valid row staged in s (sample_kernels.hip numbers them): the top_k bound, the weights w = expf((x - m_C) /
// temperature) of the candidates over the row in LDS, the ordered float64 prefix sum and the pick for the uniform u.  *Z: the total.
// Passes 4 -> 5 hand LDS entries from lane to lane inside the wave: a wavefront fence, no workgroup barrier.
__device__ __forceinline__ int sample_row_draw(float* s, int V, int lane, int top_k, float temperature, float mc, float u, double* Zout) {
    unsigned long long kth = 0ull;              // the candidates: indices >= 1 whose key is no smaller
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
    for (int v = lane; v < V; v += 64) {
        const float xv = s[v];
        s[v] = (v >= 1 && alt_key(xv, v) >= kth) ? expf((xv - mc) / temperature) : 0.f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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

}  // namespace casv
