// The sampling pick of a decoder step: a draw from every row's logits in place of the softmax and the
// greedy pick, and the one-hot row of what was drawn as the next step's input.  One 64-lane wave owns one row, as in
// decode_kernels.hip; every sum has a fixed order, the uniform is a function of (seed, stream, sample, step), so a row's result
// depends neither on the batch it sits in nor on the launch shape.
#include "common.h"
#include "alt_order.h"
#include "row_kernels.h"
#include <algorithm>
#include <math.h>

namespace casv {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds of two 32x32 -> 64
// multiplications on the counter (c0, c1, c2, c3), the key (k0, k1) bumped by the Weyl constants between rounds.  The first output
// word is all the draw needs.
__device__ __forceinline__ unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    return c0;
}

// Passes of a row, all but the fourth over v = lane, lane + 64, ... (every lane reads back the LDS entries it wrote itself):
//   1. the row into the wave's own Vp floats of LDS; NaN test, the maximum m over all V and m_C over the candidates' range 1 .. V-1
//   2. sum of expf(x - m) over all V: with m the statistics of score_rows_kernel (train_kernels.hip), formed by the same loops, so
//      logp has the bits of the scoring head's for the drawn index as target
//   3. top_k > 0: top_k rounds of the wave-wide maximum over the keys (alt_order.h) strictly below the previous winner's; the last
//      winner's key bounds the candidates
//   4. the weights w = expf((x - m_C) / temperature) of the candidates, 0 elsewhere, over the row in LDS
//   5. lane l owns the CONTIGUOUS indices [l * ceil(V / 64), (l + 1) * ceil(V / 64)): their weights summed in ascending order in
//      float64 (c_l); the lanes' offsets off_l = ((c_0 + c_1) + ...) + c_{l-1} and the total Z = off_63 + c_63 by one sequential pass
//      over the lanes in ascending order; the first lane with off_l + c_l > u * Z walks its indices again, and the pick is the first
//      with off_l + (w_first + ... + w_v) > u * Z.  No lane (a caller's u >= 1): the last index with w > 0.
// Passes 4 -> 5 hand LDS entries from lane to lane inside the wave: a wavefront fence, no workgroup barrier.
__global__ __launch_bounds__(256) void sample_kernel(const SampleArgs a) {
    extern __shared__ float sample_rows[];          // [4][Vp]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.R) return;
    const int step = a.step_ptr ? *a.step_ptr : a.step_imm;
    const int V = a.V, Vp = (V + 31) & ~31;
    const float* x = a.logits + (long long)r * Vp;
    float* s = sample_rows + wave * Vp;
    float* fb = a.feedback + (long long)(step + 1) * a.fb_slot + (long long)r * Vp;
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
    const bool valid = !nan && mc > -INFINITY && mc < INFINITY;          // (the same in every lane)
    int pick = 1;
    float lp = __builtin_nanf(""), lq = __builtin_nanf("");
    if (valid) {
        float sum = 0.f;
        for (int v = lane; v < V; v += 64) sum += expf(s[v] - m);
        sum = wave_sum(sum);
        unsigned long long kth = 0ull;              // the candidates: indices >= 1 whose key is no smaller
        if (a.top_k > 0 && a.top_k < V - 1) {
            unsigned long long prev = ~0ull;
            for (int j = 0; j < a.top_k; ++j) {
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
            s[v] = (v >= 1 && alt_key(xv, v) >= kth) ? expf((xv - mc) / a.temperature) : 0.f;
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
        float u;
        if (a.u) u = a.u[r];
        else {
            const int line = r / a.rows_per_line;
            const unsigned long long id = a.stream ? (unsigned long long)a.stream[line] : (unsigned long long)line;
            const unsigned n = (unsigned)(a.sample ? a.sample[r] : r % a.rows_per_line);
            const unsigned o0 = philox4x32_10_word0((unsigned)id, (unsigned)(id >> 32), n, (unsigned)step, (unsigned)a.seed, (unsigned)(a.seed >> 32));
            u = (float)(o0 >> 8) * 0x1p-24f;
        }
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
            pick = __shfl(mine, holder, 64);
        } else {
            pick = wave_butterfly(last, [](int p, int q) { return max(p, q); });
        }
        const float xp = x[pick];
        lp = m < INFINITY ? (xp - m) - logf(sum) : __builtin_nanf("");
        lq = (float)((double)((xp - mc) / a.temperature) - log(Z));
    }
    // the next step's input: exactly one-hot over all Vp columns (an invalid row: all zero)
    for (int v = lane * 4; v < Vp; v += 256) {
        const int hot = valid ? pick - v : -1;
        *reinterpret_cast<float4*>(fb + v) = make_float4(hot == 0 ? 1.f : 0.f, hot == 1 ? 1.f : 0.f, hot == 2 ? 1.f : 0.f, hot == 3 ? 1.f : 0.f);
    }
    if (lane == 0) {
        if (!valid && a.nan_flag) atomicOr(a.nan_flag, 1);
        const long long o = (long long)r * a.S + (long long)step * a.out_col;
        a.out_idx[o] = pick; a.out_logp[o] = lp; a.out_logq[o] = lq;
    }
}

void launch_sample(const SampleArgs& a, hipStream_t stream) {
    const int Vp = (a.V + 31) & ~31;
    hipLaunchKernelGGL(sample_kernel, dim3((a.R + 3) / 4), dim3(256), (size_t)4 * Vp * sizeof(float), stream, a);
}

__global__ void spread_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n, int rows_per_line, int width) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / width; const int w = (int)(i - row * width);
        dst[i] = src[(row / rows_per_line) * width + w];
    }
}
void launch_spread_rows(const float* src, float* dst, int lines, int rows_per_line, int width, hipStream_t stream) {
    const long long n = (long long)lines * rows_per_line * width;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
    if (n > 0) hipLaunchKernelGGL(spread_rows_kernel, dim3(blocks), dim3(256), 0, stream, src, dst, n, rows_per_line, width);
}

}  // namespace casv
