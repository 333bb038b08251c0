// The sampling pick of a decoder step: a draw from every row's logits in place of the softmax and the
// greedy pick, and the one-hot row of what was drawn as the next step's input.  One 64-lane wave owns one row, as in
// decode_kernels.hip; every sum has a fixed order, the uniform is a function of (seed, stream, sample, step), so a row's result
// depends neither on the batch it sits in nor on the launch shape.
#include "common.h"
#include "alt_order.h"
#include "sample_row.h"
#include <algorithm>
#include <math.h>

namespace casv {

// Passes of a row (1 and 3 to 5: sample_row.h, shared with sched_mix_kernel), all but the fourth over v = lane, lane + 64, ... (every lane reads back the LDS entries it wrote itself):
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
// The row r of a launch on its wave's LDS: s = the row's Vp floats; CUT: keys = its P sort entries, the bound from the cut.
template <bool CUT> __device__ __forceinline__ void sample_row(const SampleArgs& a, int r, int lane, float* s, unsigned long long* keys, int P) {
    const int step = a.step_ptr ? *a.step_ptr : a.step_imm;
    const int V = a.V, Vp = (V + 31) & ~31;
    const float* x = a.logits + (long long)r * Vp;
    float* fb = a.feedback + (long long)(step + 1) * a.fb_slot + (long long)r * Vp;
    const SampleRowStats rs = sample_row_stage(x, s, V, lane);
    const float m = rs.m, mc = rs.mc;
    const bool valid = rs.valid;          // (the same in every lane)
    int pick = 1;
    float lp = __builtin_nanf(""), lq = __builtin_nanf("");
    if (valid) {
        float sum = 0.f;
        for (int v = lane; v < V; v += 64) sum += expf(s[v] - m);
        sum = wave_sum(sum);
        float u;
        if (a.u) u = a.u[r];
        else {
            const int line = r / a.rows_per_line;
            const unsigned long long id = a.stream ? (unsigned long long)a.stream[line] : (unsigned long long)line;
            const unsigned n = (unsigned)(a.sample ? a.sample[r] : r % a.rows_per_line);
            u = philox_uniform(philox4x32_10_word0((unsigned)id, (unsigned)(id >> 32), n, (unsigned)step, (unsigned)a.seed, (unsigned)(a.seed >> 32)));
        }
        double Z;
        if constexpr (CUT)
            pick = sample_row_draw_under(s, V, lane, sample_row_cut_bound(s, keys, V, P, lane, a.top_k, a.top_p, a.temperature, mc), a.temperature, mc, u, &Z);
        else
            pick = sample_row_draw(s, V, lane, a.top_k, a.temperature, mc, u, &Z);
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

__global__ __launch_bounds__(256) void sample_kernel(const SampleArgs a) {
    extern __shared__ float sample_rows[];          // [4][Vp]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.R) return;
    sample_row<false>(a, r, lane, sample_rows + wave * ((a.V + 31) & ~31), nullptr, 0);
}

void launch_sample(const SampleArgs& a, hipStream_t stream) {
    const int Vp = (a.V + 31) & ~31;
    hipLaunchKernelGGL(sample_kernel, dim3((a.R + 3) / 4), dim3(256), (size_t)4 * Vp * sizeof(float), stream, a);
}

// The same under a cut (sample_row.h, sample_row_cut_bound): blockDim.x / 64 rows per workgroup (common.h,
// sample_cut_rows_per_workgroup), the rows' sort entries [rows][P] in front of their floats [rows][Vp].
__global__ __launch_bounds__(256) void sample_cut_kernel(const SampleArgs a, int P) {
    extern __shared__ unsigned long long sample_cut_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rows = blockDim.x >> 6;
    const int r = blockIdx.x * rows + wave;
    if (r >= a.R) return;
    float* floats = reinterpret_cast<float*>(sample_cut_lds + (size_t)rows * P);
    sample_row<true>(a, r, lane, floats + wave * ((a.V + 31) & ~31), sample_cut_lds + (size_t)wave * P, P);
}

static LdsAttribute sample_cut_attr;
bool sample_cut_ready() { return gemm_dynamic_lds(sample_cut_attr, reinterpret_cast<const void*>(&sample_cut_kernel), SAMPLE_CUT_LDS); }

int launch_sample_cut(const SampleArgs& a, int rows_max, hipStream_t stream) {
    const int rows = sample_cut_rows_per_workgroup(a.V, rows_max);
    if (!sample_cut_ready()) return 0;
    hipLaunchKernelGGL(sample_cut_kernel, dim3((a.R + rows - 1) / rows), dim3(64 * rows), (size_t)rows * sample_cut_row_bytes(a.V), stream, a,
                       sample_cut_sort_size(a.V));
    return rows;
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
