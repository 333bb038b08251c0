// Scheduled sampling inside the train step: the mix of a pass.  One 64-lane wave owns one decoder position
// (b, u): its coin, and where the coin is true and the position eligible, a pick from the logits row of position (u - 1, b) -- the
// greedy one by the keys of alt_order.h, or sample_kernel's draw by its own row code (sample_row.h).  A position's result is a
// function of (seed, step_id, b, u, the row) only: neither the batch it sits in, nor the launch shape, nor the pass enters.
#include "train_kernels.h"
#include "sample_row.h"

namespace casv {

// Position q of a launch on its wave's LDS: s = the row's Vp floats; CUT: keys = its P sort entries, the draw under the cut.
template <bool CUT> __device__ __forceinline__ void sched_mix_position(const SchedMixArgs& a, long long q, int lane, float* s, unsigned long long* keys,
                                                                       int P) {
    int b, u;
    long long row;
    if (a.row_b) { b = a.row_b[q]; u = a.row_u[q]; row = q; }                     // (the rows form: casv_debug_sched_rows)
    else { b = (int)(q / a.U); u = (int)(q - (long long)b * a.U); row = (long long)(u - 1) * a.B + b; }
    const int gold = a.gold[q];
    int mix = gold;
    if (u >= 1 && gold >= 0) {                      // (b, u, gold: the same in every lane)
        const Philox4 o = philox4x32_10((unsigned)a.step_id, (unsigned)(a.step_id >> 32), (unsigned)b, (unsigned)u,
                                        (unsigned)a.seed, (unsigned)(a.seed >> 32));
        if (philox_uniform(o.o0) < a.ratio) {
            const int V = a.V;
            const SampleRowStats rs = sample_row_stage(a.logits + row * a.Vp, s, V, lane);      // (columns [V, Vp) are not read)
            if (rs.valid && a.pick == 0) {
                // the largest key over v = 1 .. V-1: x descending, the two zeros equal, the lower index first
                unsigned long long top = 0ull;
                for (int v = lane < 1 ? 64 : lane; v < V; v += 64) {
                    const unsigned long long key = alt_key(s[v], v);
                    if (key > top) top = key;
                }
                top = wave_max_key(top);
                mix = (int)(0xffffffffu - (unsigned)top);
            } else if (rs.valid) {
                double Z;
                if constexpr (CUT)
                    mix = sample_row_draw_under(s, V, lane, sample_row_cut_bound(s, keys, V, P, lane, a.top_k, a.top_p, a.temperature, rs.mc),
                                                a.temperature, rs.mc, philox_uniform(o.o1), &Z);
                else
                    mix = sample_row_draw(s, V, lane, 0, a.temperature, rs.mc, philox_uniform(o.o1), &Z);
            }
        }
    }
    if (lane == 0) {
        a.out[q] = mix;
        if (a.d_in) a.d_in[q] = mix;
    }
}

__global__ __launch_bounds__(256) void sched_mix_kernel(const SchedMixArgs a) {
    extern __shared__ float sched_rows[];           // [4][Vp]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * 4 + wave;
    if (q >= a.R) return;
    sched_mix_position<false>(a, q, lane, sched_rows + wave * a.Vp, nullptr, 0);
}

// The mix with the sampled pick under a cut (top_k, top_p): sample_cut_kernel's LDS layout and rows per workgroup.
__global__ __launch_bounds__(256) void sched_mix_cut_kernel(const SchedMixArgs a, int P) {
    extern __shared__ unsigned long long sched_cut_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rows = blockDim.x >> 6;
    const long long q = (long long)blockIdx.x * rows + wave;
    if (q >= a.R) return;
    float* floats = reinterpret_cast<float*>(sched_cut_lds + (size_t)rows * P);
    sched_mix_position<true>(a, q, lane, floats + wave * a.Vp, sched_cut_lds + (size_t)wave * P, P);
}

static LdsAttribute sched_cut_attr;
bool sched_mix_cut_ready() { return gemm_dynamic_lds(sched_cut_attr, reinterpret_cast<const void*>(&sched_mix_cut_kernel), SAMPLE_CUT_LDS); }

void launch_sched_mix(const SchedMixArgs& a, hipStream_t stream) {
    if (a.R < 1) return;
    if (a.pick == 1 && (a.top_k != 0 || a.top_p != 1.f)) {          // (callers have asked sched_mix_cut_ready())
        const int rows = sample_cut_rows_per_workgroup(a.V, 0);
        if (!sched_mix_cut_ready()) return;
        hipLaunchKernelGGL(sched_mix_cut_kernel, dim3((unsigned)((a.R + rows - 1) / rows)), dim3(64 * rows), (size_t)rows * sample_cut_row_bytes(a.V),
                           stream, a, sample_cut_sort_size(a.V));
        return;
    }
    hipLaunchKernelGGL(sched_mix_kernel, dim3((unsigned)((a.R + 3) / 4)), dim3(256), (size_t)4 * a.Vp * sizeof(float), stream, a);
}

}  // namespace casv
